#!/usr/bin/env python3
"""What the ONE call for an indexed packed batch with stored items (aws_huffman_amd_encode_plan_launch_packed_stored_indexed,
huffman_amd_stored_index.h) costs under the test coder, next to the two calls it replaces
(aws_huffman_amd_encode_plan_block_index, then aws_huffman_amd_encode_plan_launch_packed_stored), and what ranges of such a
batch cost its receiver.  Prints one JSON document (and writes it to the path given, by default
profiles/stored_index_mi355x.json).

One process, device events, medians of `--launches` launches behind `--warmup` launches that are thrown away.  Every step
runs under an alarm of `--step-seconds` whose default action ends the process: the script ends at the first failure.

  shapes   : 1 GiB as ONE item, 65 536 items of 16 KiB, 1 Mi items of 16 .. 80 bytes
  contents : uniform bytes (everything stored), lowercase text (nothing stored), every second item stored (the one-item
             shape has no second item: left out)
  blocks   : 16 384 and 64 symbols
  rows     : pair (the two calls, one behind the other on one stream), one_call
  ranges   : a random 1 % of the blocks of the 65 536-item batch, every second item stored: the reset (host clock: it waits
             for the planner's totals) and the plain launch, through the calls that take the flags; and the same ranges over
             the all-coded batch through aws_huffman_amd_decode_plan_reset_item_block_ranges, for reference
  --pair-only --lib parent.so : the pair rows and the all-coded ranges alone, from the parent commit's build on the same
             box, in turn:

      stored_index_rate.py parent_first.json --pair-only --lib parent.so
      stored_index_rate.py this.json
      stored_index_rate.py parent_second.json --pair-only --lib parent.so
      stored_index_rate.py --merge this.json parent_first.json parent_second.json

  --merge : the rule, written before the run: the one call is below the FASTER of the parent's two runs of the pair, on
            every row

usage: stored_index_rate.py [out.json] [--launches N] [--warmup N] [--shrink N] [--lib path] [--pair-only]"""
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
import packed_decode_api as pda  # noqa: E402
import stored_api as sa  # noqa: E402
from block_index_rate import Steps, timed_events, timed_host  # noqa: E402
from stored_rate import SHAPES, content, shapes  # noqa: E402

GiB = 1 << 30
DEFAULT_OUT = os.path.join(REPO, "profiles", "stored_index_mi355x.json")
CONTENTS = ("everything_stored", "nothing_stored", "every_second_stored")
BLOCKS = (16384, 64)


def measure(lib, eng, n, args, step, si):
    d_in = eng.alloc(n + 64)
    room = n + n // 2 + 4096
    d_out = eng.alloc(room)
    out = {}
    for label, (offsets, lengths) in shapes(n, args.shrink).items():
        count, span = len(lengths), int(offsets[-1] + lengths[-1])
        d_off, d_flags = eng.alloc(8 * (count + 1)), eng.alloc(count + 8)
        plan, d_items = pa.plan_from_records(eng, offsets, lengths)
        out[label] = {}
        for kind in CONTENTS:
            if kind == "every_second_stored" and count == 1:
                continue
            step("%s, %s: upload" % (label, kind))
            eng.upload(d_in, content(kind, span, lengths))
            for B in BLOCKS:
                entries = int(((lengths + B - 1) // B).sum()) + 1
                d_dir, d_index, d_status = eng.alloc(16 * (count + 1)), eng.alloc(8 * entries), eng.alloc(8)
                row = {"items": count, "bytes": span, "block_symbols": B, "index_entries": entries}

                def pair():
                    assert bi.plan_block_index(eng, plan, d_in, B, d_dir, d_index, entries, d_status, eng.stream) == (0, 0)
                    assert sa.launch_stored(eng, plan, d_in, d_out, room, d_off, d_flags, 1, eng.stream) == (0, 0)

                def one_call():
                    assert si.launch(eng, plan, d_in, d_out, room, d_off, d_flags, 1, B, d_dir, d_index, entries, d_status,
                                     eng.stream) == (0, 0)

                step("%s, %s, B %d: pair" % (label, kind, B))
                pair()
                row["output_bytes"] = pa.packed_size(eng, plan)[2]
                row["stored_items"], row["stored_bytes"] = sa.stored_size(eng, plan)[2:]
                row["pair"] = timed_events(eng, pair, args.launches, args.warmup)
                if not args.pair_only:
                    step("%s, %s, B %d: one call" % (label, kind, B))
                    one_call()
                    assert pa.packed_size(eng, plan)[2] == row["output_bytes"] and sa.stored_size(eng, plan)[2] == row["stored_items"], row
                    row["one_call"] = timed_events(eng, one_call, args.launches, args.warmup)
                    row["saved_ms"] = round(row["pair"]["median_ms"] - row["one_call"]["median_ms"], 4)
                print(label, kind, json.dumps(row), flush=True)
                out[label]["%s_B%d" % (kind, B)] = row
                for p in (d_dir, d_index, d_status):
                    eng.free(p)
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        for p in (d_items, d_off, d_flags):
            eng.free(p)
    eng.free(d_in)
    eng.free(d_out)
    return out


def measure_ranges(lib, eng, n, args, step, si):
    """A random 1 % of the blocks of the 65 536-item batch, one range a block."""
    offsets, lengths = shapes(n, args.shrink)["items_of_16_KiB"]
    count, span, B = len(lengths), int(offsets[-1] + lengths[-1]), 1024
    d_in, room = eng.alloc(span + 64), span + span // 2 + 4096
    d_out, d_back = eng.alloc(room), eng.alloc(span + 64)
    d_off, d_flags = eng.alloc(8 * (count + 1)), eng.alloc(count + 8)
    entries = int(((lengths + B - 1) // B).sum()) + 1
    d_dir, d_index, d_status = eng.alloc(16 * (count + 1)), eng.alloc(8 * entries), eng.alloc(8)
    plan, d_items = pa.plan_from_records(eng, offsets, lengths)
    dplan = eng.empty_decode_plan()
    rng = np.random.default_rng(23)
    per_item = int(lengths[0]) // B
    picked = rng.choice(count * per_item, max(1, count * per_item // 100), replace=False)
    ranges = np.zeros((picked.size, 4), np.uint64)
    ranges[:, 0], ranges[:, 1], ranges[:, 2] = picked // per_item, picked % per_item, 1
    ranges[:, 3] = np.arange(picked.size, dtype=np.uint64) * B
    d_ranges = pda.upload_u64(eng, ranges.reshape(-1))
    out = {"items": count, "block_symbols": B, "ranges": int(picked.size)}
    for kind in ("nothing_stored",) if args.pair_only else ("nothing_stored", "every_second_stored"):
        step("ranges, %s: the batch" % kind)
        eng.upload(d_in, content(kind, span, lengths))
        assert bi.plan_block_index(eng, plan, d_in, B, d_dir, d_index, entries, d_status, eng.stream) == (0, 0)
        assert sa.launch_stored(eng, plan, d_in, d_out, room, d_off, d_flags, 1, eng.stream) == (0, 0)
        total = pa.packed_size(eng, plan)[2]
        flags = None if kind == "nothing_stored" else d_flags
        if kind == "nothing_stored":  # (a text item whose code ties with its length is stored: this batch goes without flags)
            assert pa.launch_packed(eng, plan, d_in, d_out, room, d_off, 1, eng.stream) == (0, 0)
            total = pa.packed_size(eng, plan)[2]

        def reset():
            if args.pair_only or flags is None:
                rc = lib.aws_huffman_amd_decode_plan_reset_item_block_ranges(
                    dplan, d_dir, d_index, entries, count, B, d_off, None, 0, total, d_ranges, picked.size, None)
            else:
                rc = lib.aws_huffman_amd_decode_plan_reset_stored_item_block_ranges(
                    dplan, d_dir, d_index, entries, count, B, d_off, None, flags, 0, total, d_ranges, picked.size, None)
            assert rc == 0, lib.aws_last_error()

        step("ranges, %s: reset and launch" % kind)
        row = {"reset_host": timed_host(eng, reset, args.launches, args.warmup)}
        row["launch"] = timed_events(eng, lambda: eng.decode_launch(dplan, d_out, d_back), args.launches, args.warmup)
        print("ranges", kind, json.dumps(row), flush=True)
        out[kind] = row
    lib.aws_huffman_amd_decode_plan_destroy(dplan)
    lib.aws_huffman_amd_encode_plan_destroy(plan)
    for p in (d_in, d_out, d_back, d_off, d_flags, d_dir, d_index, d_status, d_items, d_ranges):
        eng.free(p)
    return out


def merge(paths, out_path):
    this, first, second = (json.load(open(p)) for p in paths)
    rows, ok = {}, True
    for shape in SHAPES:
        for key, mine in this["rows"][shape].items():
            a, b = (d["rows"][shape][key]["pair"]["median_ms"] for d in (first, second))
            passed = mine["one_call"]["median_ms"] < min(a, b)
            ok = ok and passed
            rows["%s/%s" % (shape, key)] = {"parent_pair_first_ms": a, "this_one_call_ms": mine["one_call"]["median_ms"],
                                            "parent_pair_second_ms": b, "this_pair_ms": mine["pair"]["median_ms"],
                                            "saved_against_the_faster_ms": round(min(a, b) - mine["one_call"]["median_ms"], 4),
                                            "passes": passed}
    this["one_call_against_parent_pair"] = {
        "rule": "written before the run: the one call is below the faster of the parent commit's two runs of the pair "
                "(block_index + launch_packed_stored), on every row; two runs of the parent's build on one box around this one",
        "rows": rows, "passes": ok}
    this["ranges"]["parent_all_coded"] = [d["ranges"]["nothing_stored"] for d in (first, second)]
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
    ap.add_argument("--pair-only", action="store_true")
    ap.add_argument("--merge", nargs=3, metavar=("THIS", "PARENT_FIRST", "PARENT_SECOND"))
    args = ap.parse_args()
    if args.merge:
        sys.exit(merge(args.merge, args.out))
    assert args.warmup >= 15 or args.shrink > 1, "the clocks settle over about 13 launches"
    lib = harness.load_product(args.lib)
    si = None
    if args.pair_only:
        sa.bind(lib)
        bi.bind(lib)
    else:
        import stored_index_api as si
        si.bind(lib)
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: nothing is measured without one"
    patterns, lens = harness.load_table()
    eng = harness.Engine(lib, lib.aws_huffman_amd_table_coder_new(patterns, lens))
    n = GiB // args.shrink
    step = Steps(args.step_seconds)
    out = {"bytes": n, "launches": args.launches, "warmup": args.warmup, "library": args.lib or "the tree's own",
           "tool": "profiles/tools/stored_index_rate.py (one MI355X, one process, device events)",
           "rows": measure(lib, eng, n, args, step, si), "ranges": measure_ranges(lib, eng, n, args, step, si)}
    step.done()
    eng.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out != "-":
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
