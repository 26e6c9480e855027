#!/usr/bin/env python3
"""What the symbol counts of an encode plan's items (aws_huffman_amd_encode_plan_symbol_counts, huffman_amd_plan_counts.h)
cost on uniform bytes resident in device memory, next to their floor, and what the fourth body costs the three older bodies
of count_kernel.  Prints one JSON document (and writes it to the path given, by default profiles/plan_counts_mi355x.json).

One process, device events, medians of `--launches` launches behind `--warmup` launches that are thrown away.  Every step
runs under an alarm of `--step-seconds` whose default action ends the process: the script ends at the first failure.

  plan_counts : 1 GiB as ONE item, 65 536 items of 16 KiB, 1 Mi items of 16 .. 80 bytes, and a strided batch with gaps (16 KiB
                of every 20 KiB of the GiB): the call against aws_huffman_amd_symbol_counts over the same bytes -- the same
                read with no item records: the floor -- with the ratio to it; where the items tile their range the two arrays
                must be equal.  For the 1 Mi short items also aws_huffman_amd_encode_plan_block_index (64 symbols a block) of
                the same batch: a count slower than that points to idle lanes.
  gate        : the three older bodies -- aws_huffman_amd_symbol_counts, aws_huffman_amd_block_index at 64 and 16 384 symbols a
                block over 1 GiB, aws_huffman_amd_encode_plan_block_index on the three shapes -- through
                batch_index_rate.py's own functions.  With --gate-only nothing else runs, so that the same numbers can be
                taken from the parent commit's build (--lib) on the same box, in turn, one process each:

                    plan_counts_rate.py parent_first.json --gate-only --lib parent.so
                    plan_counts_rate.py this.json
                    plan_counts_rate.py parent_second.json --gate-only --lib parent.so
                    plan_counts_rate.py --merge this.json parent_first.json parent_second.json

                --merge writes the parent's two runs and the verdict into the document: a body passes where this build's
                median is no more than the slower parent run plus the larger of the parent runs' own spread and 3 %.

usage: plan_counts_rate.py [out.json] [--launches N] [--warmup N] [--shrink N] [--lib path] [--gate-only]
       plan_counts_rate.py --merge this.json parent_first.json parent_second.json [out.json]"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import harness  # noqa: E402
import index_api as ia  # noqa: E402
import packed_api as pa  # noqa: E402
from batch_index_rate import measure_batch, measure_single, ratio  # noqa: E402
from block_index_rate import Steps, timed_events  # noqa: E402

GiB = 1 << 30
DEFAULT_OUT = os.path.join(REPO, "profiles", "plan_counts_mi355x.json")
SHAPES = ("one_item", "items_of_16_KiB", "items_of_16_to_80_bytes")
GATE_KEYS = [("single", k) for k in ("count", "index_64", "index_16384")] + \
            [(s, k) for s in SHAPES for k in ("batch_index_64", "batch_index_16384")]


def shapes(n, shrink):
    many = 65_536 // shrink
    size = n // many
    small = np.random.default_rng(11).integers(16, 81, (1 << 20) // shrink).astype(np.int64)
    return {"one_item": (np.asarray([0]), np.asarray([n])),
            "items_of_16_KiB": (np.arange(many, dtype=np.int64) * size, np.full(many, size, np.int64)),
            "items_of_16_to_80_bytes": (np.concatenate([[0], np.cumsum(small)])[:-1], small)}


def device_counts(eng, d_counts):
    return eng.download(d_counts, 256 * 8).view(np.uint64).copy()


def measure_plan_counts(pk, lib, eng, d_in, plan, n_bytes, span, tiles, label, args, step):
    """The call over `plan`, whose items hold n_bytes of the `span` bytes at d_in, against the range count of as many bytes."""
    step("%s: plan counts" % label)
    d_counts = eng.alloc(256 * 8)
    eng.fill(d_counts, 0, 256 * 8)
    count_range = lambda size: lib.aws_huffman_amd_symbol_counts(-1, d_in, size, d_counts, eng.stream)
    row = {"items": eng.encode_stats(plan)["items"], "bytes": int(n_bytes), "span_bytes": int(span),
           "count": timed_events(eng, lambda: count_range(n_bytes), args.launches, args.warmup),
           "plan_counts": timed_events(eng, lambda: pk.plan_counts(eng, plan, d_in, d_counts, eng.stream), args.launches, args.warmup)}
    ratio(row, "plan_counts", "count")
    if tiles:  # the same bytes: the same 256 sums
        eng.fill(d_counts, 0, 256 * 8)
        assert count_range(span) == 0
        theirs = device_counts(eng, d_counts)
        eng.fill(d_counts, 0, 256 * 8)
        assert pk.plan_counts(eng, plan, d_in, d_counts, eng.stream) == (0, 0)
        assert np.array_equal(device_counts(eng, d_counts), theirs) and int(theirs.sum()) == n_bytes, label
    else:
        eng.fill(d_counts, 0, 256 * 8)
        assert pk.plan_counts(eng, plan, d_in, d_counts, eng.stream) == (0, 0)
        assert int(device_counts(eng, d_counts).sum()) == n_bytes, label
    eng.free(d_counts)
    return row


def measure(lib, eng, d_in, n, args, step):
    import batch_index_api as bi
    import plan_counts_api as pk
    pk.bind(lib)
    out = {}
    for label, (offsets, lengths) in shapes(n, args.shrink).items():
        step("%s: plan" % label)
        plan, d_items = pa.plan_from_records(eng, offsets, lengths)
        span = int(offsets[-1] + lengths[-1])
        row = measure_plan_counts(pk, lib, eng, d_in, plan, int(np.sum(lengths)), span, True, label, args, step)
        if label == "items_of_16_to_80_bytes":
            blocks = int(np.sum((lengths + 63) // 64))
            a = bi.Arrays(eng, len(lengths), blocks + 1)
            row["batch_index_64"] = timed_events(
                eng, lambda: bi.plan_block_index(eng, plan, d_in, 64, a.d_dir, a.d_index, blocks + 1, a.d_status, eng.stream),
                args.launches, args.warmup)
            ratio(row, "plan_counts", "batch_index_64")
            a.close()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        eng.free(d_items)
        print(label, json.dumps(row), flush=True)
        out[label] = row
    label = "strided_16_KiB_of_every_20_KiB"
    step("%s: plan" % label)
    count = n // (20 << 10)
    plan = eng.plan_strided(True, count=count, in_offset=0, in_stride=20 << 10, in_len=16 << 10, out_offset=0, out_stride=0,
                            out_capacity=0, first_bit=0, eos_padding=0xFF)
    out[label] = measure_plan_counts(pk, lib, eng, d_in, plan, count * (16 << 10), (count - 1) * (20 << 10) + (16 << 10), False,
                                     label, args, step)
    out[label]["note"] = "count: aws_huffman_amd_symbol_counts over as many contiguous bytes as the items hold"
    lib.aws_huffman_amd_encode_plan_destroy(plan)
    print(label, json.dumps(out[label]), flush=True)
    return out


def measure_gate(lib, eng, d_in, n, args, step):
    import batch_index_api as bi
    bi.bind(lib)
    out = {"single": measure_single(lib, eng, d_in, n, args, step)}
    for label, (offsets, lengths) in shapes(n, args.shrink).items():
        out[label] = measure_batch(bi, lib, eng, d_in, offsets, lengths, label.replace("_", " "), args, step)
    return out


def merge(paths, out_path):
    this, first, second = (json.load(open(p)) for p in paths)
    rows, ok = {}, True
    for section, key in GATE_KEYS:
        a, b, mine = (d["gate"][section][key]["median_ms"] for d in (first, second, this))
        slower, spread = max(a, b), abs(a - b)
        margin = max(spread, 0.03 * slower)
        passed = mine <= slower + margin
        ok = ok and passed
        rows["%s.%s" % (section, key)] = {"parent_first_ms": a, "this_ms": mine, "parent_second_ms": b,
                                          "allowed_ms": round(slower + margin, 4), "passes": passed}
    this["gate_against_parent"] = {
        "rule": "this build between two runs of the parent commit's build (--gate-only --lib) on one box, one process each: a "
                "body passes where its median is at most the slower parent run plus the larger of the parent runs' spread and 3 %",
        "rows": rows, "passes": ok}
    text = json.dumps(this, indent=1)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=DEFAULT_OUT)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--shrink", type=int, default=1, help="every size divided by this (a rehearsal)")
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--gate-only", action="store_true")
    ap.add_argument("--merge", nargs=3, metavar=("THIS", "PARENT_FIRST", "PARENT_SECOND"))
    args = ap.parse_args()
    if args.merge:
        sys.exit(merge(args.merge, args.out))
    assert args.warmup >= 15 or args.shrink > 1, "the clocks settle over about 13 launches"
    lib = ia.bind(harness.load_product(args.lib))
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: nothing is measured without one"
    patterns, lens = harness.load_table()
    coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    eng = harness.Engine(lib, coder)
    n = GiB // args.shrink
    step = Steps(args.step_seconds)
    d_in = eng.alloc(n + 64)
    eng.fill_splitmix64(d_in, n, 41)
    out = {"bytes": n, "launches": args.launches, "warmup": args.warmup, "library": args.lib or "the tree's own",
           "tool": "profiles/tools/plan_counts_rate.py (one MI355X, one process, device events)"}
    if not args.gate_only:
        out["plan_counts"] = measure(lib, eng, d_in, n, args, step)
    out["gate"] = measure_gate(lib, eng, d_in, n, args, step)
    step.done()
    eng.free(d_in)
    eng.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out != "-":
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
