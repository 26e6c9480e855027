#!/usr/bin/env python3
"""What a packed encode launch that makes the batch's block index (aws_huffman_amd_encode_plan_launch_packed_indexed,
huffman_amd_packed_index.h) costs on uniform bytes resident in device memory, next to the two calls it replaces.  Prints one
JSON document (and writes it to the path given, by default profiles/packed_indexed_mi355x.json).

One process, device events, medians of `--launches` launches behind `--warmup` launches that are thrown away.  Every step
runs under an alarm of `--step-seconds` whose default action ends the process: the script ends at the first failure.

The shapes are batch_index_rate.py's -- 1 GiB as one item, 65 536 items of 16 KiB, 1 Mi items of 16 .. 80 bytes -- at 16 384
and 64 symbols a block, with the test coder.  Per shape and block size:
  a_indexed            the new call
  b_index_then_packed  aws_huffman_amd_encode_plan_block_index followed by aws_huffman_amd_encode_plan_launch_packed, the same
                       arguments: what a sender did before
  index_alone, packed_alone, length_only_alone
                       the index call, the packed launch, and a plain length_only launch: where the difference comes from
Before anything is timed, a's offsets, total and status are compared with b's.

The yardstick for `a` is `b` ON THE PARENT COMMIT'S BUILD, run before and after on the same box (--lib, which skips `a`:
that build has no such call), never this build's own b.  --parent-runs before.json after.json puts those two documents
beside this run's and says per shape whether a is below both.

The three runs are three processes, the parent's last: --from-run this.json measures nothing and puts the documents together.

usage: packed_indexed_rate.py [out.json] [--launches N] [--warmup N] [--shrink N] [--lib path]
                              [--from-run this.json] [--parent-runs before.json after.json] [--also name=path.json ...]"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_index_api as bi  # noqa: E402
import harness  # noqa: E402
import packed_api as pa  # noqa: E402
from block_index_rate import Steps, timed_events  # noqa: E402

GiB = 1 << 30
BLOCKS = (16_384, 64)
SHAPES = ("one_item", "items_of_16_KiB", "items_of_16_to_80_bytes")


def measure(lib, eng, has_new, d_in, d_out, cap, offsets, lengths, label, args, step):
    n_items = len(lengths)
    step("%s: plan" % label)
    plan, d_items = pa.plan_from_records(eng, offsets, lengths)
    d_off, d_off_b = eng.alloc(8 * (n_items + 1)), eng.alloc(8 * (n_items + 1))
    row = {"items": n_items, "bytes": int(np.sum(lengths))}
    length_only = lambda: lib.aws_huffman_amd_encode_plan_launch(plan, d_in, d_out, True, eng.stream)
    packed = lambda: pa.launch_packed(eng, plan, d_in, d_out, cap, d_off_b, 1, eng.stream)
    row["length_only_alone"] = timed_events(eng, length_only, args.launches, args.warmup)
    row["packed_alone"] = timed_events(eng, packed, args.launches, args.warmup)
    for B in BLOCKS:
        step("%s: %d symbols a block" % (label, B))
        blocks = int(np.sum((np.asarray(lengths, dtype=np.int64) + B - 1) // B))
        a = bi.Arrays(eng, n_items, blocks + 1)
        index = lambda: bi.plan_block_index(eng, plan, d_in, B, a.d_dir, a.d_index, blocks + 1, a.d_status, eng.stream)
        both = lambda: (index(), packed())
        assert both() == ((0, 0), (0, 0))
        eng.sync()
        assert int(eng.download(a.d_status, 4).view(np.uint32)[0]) == bi.INDEX_OK
        want = (pa.packed_size(eng, plan), bi.index_size(eng, plan), int(pa.download_u64(eng, a.d_index + 8 * blocks, 1)[0]))
        assert want[0][:2] == (0, 0) and want[0][2] <= cap, want
        sub = {"blocks": blocks, "encoded_bytes": int(want[0][2]),
               "index_alone": timed_events(eng, index, args.launches, args.warmup),
               "b_index_then_packed": timed_events(eng, both, args.launches, args.warmup)}
        if has_new:
            import packed_index_api as pi
            new = lambda: pi.launch_indexed(eng, plan, d_in, d_out, cap, d_off, 1, B, a.d_dir, a.d_index, blocks + 1, a.d_status,
                                            eng.stream)
            a.refill()
            assert new() == (0, 0)
            eng.sync()
            assert int(eng.download(a.d_status, 4).view(np.uint32)[0]) == bi.INDEX_OK
            got = (pa.packed_size(eng, plan), bi.index_size(eng, plan), int(pa.download_u64(eng, a.d_index + 8 * blocks, 1)[0]))
            assert got == want, (got, want)
            assert np.array_equal(pa.download_u64(eng, d_off, n_items + 1), pa.download_u64(eng, d_off_b, n_items + 1))
            sub["a_indexed"] = timed_events(eng, new, args.launches, args.warmup)
            if sub["b_index_then_packed"]["median_ms"]:  # (0 under the emulator build, whose events measure nothing: a rehearsal)
                sub["a_indexed"]["over_this_builds_b"] = round(sub["a_indexed"]["median_ms"] / sub["b_index_then_packed"]["median_ms"], 3)
        row["block_%d" % B] = sub
        a.close()
    lib.aws_huffman_amd_encode_plan_destroy(plan)
    for d in (d_items, d_off, d_off_b):
        eng.free(d)
    print(label, json.dumps(row), flush=True)
    return row


def verdicts(out, parents):
    """Per shape and block size: a's median against b's of both parent runs."""
    table = {}
    for shape in SHAPES:
        for B in BLOCKS:
            key = "block_%d" % B
            a = out[shape][key]["a_indexed"]["median_ms"]
            bs = [p[shape][key]["b_index_then_packed"]["median_ms"] for p in parents]
            table["%s/%d" % (shape, B)] = {"a_ms": a, "parent_b_ms": bs, "a_below_both": bool(a < min(bs)),
                                           "saved_ms_against_the_faster_parent_run": round(min(bs) - a, 4)}
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(REPO, "profiles", "packed_indexed_mi355x.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--shrink", type=int, default=1, help="every size divided by this (a rehearsal)")
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--parent-runs", nargs=2, default=None, help="two documents of this tool made with --lib <the parent's build>")
    ap.add_argument("--also", nargs="*", default=[], help="name=path.json: further documents recorded beside this one as they are")
    ap.add_argument("--from-run", default=None, help="this build's document of an earlier process: nothing is measured")
    args = ap.parse_args()
    if args.from_run:
        finish(json.load(open(args.from_run)), args)
        return
    assert args.warmup >= 15 or args.shrink > 1, "the clocks settle over about 13 launches"
    lib = pa.bind(bi.bind(harness.load_product(args.lib)))
    has_new = hasattr(lib, "aws_huffman_amd_encode_plan_launch_packed_indexed")
    assert has_new or args.lib, "the tree's own build must have the call"
    if has_new:
        import packed_index_api as pi
        pi.bind(lib)
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: nothing is measured without one"
    patterns, lens = harness.load_table()
    coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    eng = harness.Engine(lib, coder)
    n = GiB // args.shrink
    step = Steps(args.step_seconds)
    cap = 2 * n + 64
    d_in, d_out = eng.alloc(n + 64), eng.alloc(cap)
    eng.fill_splitmix64(d_in, n, 41)
    out = {"bytes": n, "launches": args.launches, "warmup": args.warmup, "library": args.lib or "the tree's own",
           "tool": "profiles/tools/packed_indexed_rate.py (one MI355X, one process, device events)"}
    out["one_item"] = measure(lib, eng, has_new, d_in, d_out, cap, np.asarray([0]), np.asarray([n]), "one item", args, step)
    many = 65_536 // args.shrink
    size = n // many
    out["items_of_16_KiB"] = measure(lib, eng, has_new, d_in, d_out, cap, np.arange(many, dtype=np.int64) * size,
                                     np.full(many, size, np.int64), "items of 16 KiB", args, step)
    small = np.random.default_rng(11).integers(16, 81, (1 << 20) // args.shrink).astype(np.int64)
    at = np.concatenate([[0], np.cumsum(small)])[:-1]
    out["items_of_16_to_80_bytes"] = measure(lib, eng, has_new, d_in, d_out, cap, at, small, "items of 16 to 80 bytes", args, step)
    step.done()
    eng.free(d_in)
    eng.free(d_out)
    eng.close()
    finish(out, args)


def finish(out, args):
    if args.parent_runs:
        parents = [json.load(open(p)) for p in args.parent_runs]
        out["parent_runs_before_and_after"] = parents
        out["a_against_the_parents_b"] = verdicts(out, parents)
    for spec in args.also:
        name, path = spec.split("=", 1)
        out[name] = json.load(open(path))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out != "-":
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
