#!/usr/bin/env python3
"""What a packed launch (aws_huffman_amd_encode_plan_launch_packed) costs next to what a caller had before it, on three
batches: 65 536 x 16 KiB, 65 536 x 2 KiB, a million items of 16-80 bytes (splitmix64 seed 5 bytes, made on the device).
Prints one JSON document (and writes it to the path given).

Per batch, three ways to the same dense output, timed side by side in one process (one after the other in every step,
host clock from the first call to the end of the stream's work; the steps before the clocks have settled are thrown
away):
  a  packed    : the packed launch, then a wait for the stream
  b  composite : what a caller has without it -- length_only launch, aws_huffman_amd_encode_plan_encoded_lengths, a
                 prefix sum on the host, aws_huffman_amd_encode_plan_reset with the new offsets, launch, wait
  c  two_plain : a length_only launch and a plain launch of the same plan (sparse output), then the wait: a - c is what
                 the offset kernels cost
and the length_only launch alone (the share of `a` that is the length pass).  Every figure is the median over the steps
of a run; a batch is measured in `runs` runs and the spread between their medians is recorded beside them.
Also: the bytes the documented 2x output slots allocate against the packed total.

--baseline-only measures `b` alone and touches no symbol of huffman_amd_packed.h: with --lib it runs against a build
of the commit before the packed launch existed, on the same machine.
usage: packed_rate.py [out.json] [--steps N] [--warmup N] [--runs N] [--baseline-only] [--lib path/to/lib.so] [--shrink N]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
import harness  # noqa: E402

ITEM = np.dtype([("in_offset", "<u8"), ("in_len", "<u8"), ("out_offset", "<u8"), ("out_capacity", "<u8"),
                 ("pattern", "<u4"), ("num_bits", "u1"), ("pad0", "u1", 3), ("eos_padding", "u1"), ("pad1", "u1", 7)])
ITEM_P = C.POINTER(harness.AmdEncodeItem)


def shapes(shrink):
    rng = np.random.default_rng(5)
    short = rng.integers(16, 81, 1_000_000 // shrink).astype(np.uint64)
    return [("65536x16KiB", np.full(65536 // shrink, 16384, np.uint64)), ("65536x2KiB", np.full(65536 // shrink, 2048, np.uint64)),
            ("1Mx16-80B", short)]


def records(in_lens, out_offsets, out_caps):
    recs = np.zeros(in_lens.size, ITEM)
    recs["in_len"] = in_lens
    recs["in_offset"] = np.concatenate([[0], np.cumsum(in_lens)[:-1]])
    recs["out_offset"], recs["out_capacity"], recs["eos_padding"] = out_offsets, out_caps, 0xFF
    return recs


def new_plan(eng, recs):
    plan = C.c_void_p()
    assert eng.lib.aws_huffman_amd_encode_plan_new(C.byref(plan), eng.h, recs.ctypes.data_as(ITEM_P), recs.size) == 0
    return plan


def measure(eng, name, in_lens, args, pa):
    lib = eng.lib
    n = int(in_lens.size)
    in_bytes = int(in_lens.sum())
    slots = 2 * in_lens  # the documented batch: every buffer a slot of twice its size
    slot_offs = np.concatenate([[0], np.cumsum(slots)[:-1]]).astype(np.uint64)
    sparse_bytes = int(slots.sum())
    d_in, d_out = eng.alloc(in_bytes + 64), eng.alloc(sparse_bytes + 64)
    eng.fill_splitmix64(d_in, in_bytes, 5)
    recs_b = records(in_lens, slot_offs, slots)
    plan_b = new_plan(eng, recs_b)
    lengths = np.zeros(n, np.uint64)
    lengths_p = lengths.ctypes.data_as(C.POINTER(C.c_uint64))

    def composite():
        assert lib.aws_huffman_amd_encode_plan_launch(plan_b, d_in, d_out, True, None) == 0
        assert lib.aws_huffman_amd_encode_plan_encoded_lengths(plan_b, lengths_p, None) == 0
        recs_b["out_capacity"] = lengths
        recs_b["out_offset"][0] = 0
        np.cumsum(lengths[:-1], out=recs_b["out_offset"][1:])
        assert lib.aws_huffman_amd_encode_plan_reset(plan_b, recs_b.ctypes.data_as(ITEM_P), n) == 0
        assert lib.aws_huffman_amd_encode_plan_launch(plan_b, d_in, d_out, False, None) == 0
        eng.sync()

    ways = {"b_composite": composite}
    if pa is not None:
        plan_a = new_plan(eng, records(in_lens, slot_offs, slots))
        d_off = eng.alloc(8 * (n + 1))

        def packed():
            assert lib.aws_huffman_amd_encode_plan_launch_packed(plan_a, d_in, d_out, sparse_bytes, d_off, 1, None) == 0
            eng.sync()

        def two_plain():
            assert lib.aws_huffman_amd_encode_plan_launch(plan_a, d_in, d_out, True, None) == 0
            assert lib.aws_huffman_amd_encode_plan_launch(plan_a, d_in, d_out, False, None) == 0
            eng.sync()

        def length_only():
            assert lib.aws_huffman_amd_encode_plan_launch(plan_a, d_in, d_out, True, None) == 0
            eng.sync()

        ways = {"a_packed": packed, "b_composite": composite, "c_two_plain": two_plain, "length_only": length_only}

    runs = {k: [] for k in ways}
    for _ in range(args.runs):
        times = {k: [] for k in ways}
        for step in range(args.warmup + args.steps):
            for k, fn in ways.items():
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                if step >= args.warmup:
                    times[k].append((t1 - t0) * 1e3)
        for k in ways:
            runs[k].append(statistics.median(times[k]))
    row = {"items": n, "input_bytes": in_bytes, "sparse_output_bytes_2x_slots": sparse_bytes}
    for k in ways:
        row[k] = {"median_ms": round(statistics.median(runs[k]), 4), "run_medians_ms": [round(x, 4) for x in runs[k]],
                  "spread_ms": round(max(runs[k]) - min(runs[k]), 4)}
    # the composite's own result: the dense total (and, with the packed launch, the same bytes from both)
    composite()
    total_b = int(lengths.sum())
    row["total_bytes"] = total_b
    row["sparse_over_dense"] = round(sparse_bytes / total_b, 3)
    if pa is not None:
        dense_b = eng.download(d_out, total_b)
        eng.fill(d_out, 0, total_b)
        packed()
        rc, _, total_a, longest = pa.packed_size(eng, plan_a)
        assert rc == 0 and total_a == total_b, (total_a, total_b)
        assert np.array_equal(eng.download(d_out, total_a), dense_b), "the packed launch and the composite differ"
        assert np.array_equal(pa.download_u64(eng, d_off, n + 1)[:-1], recs_b["out_offset"].astype(np.int64))
        a, b, c, lo = (row[k]["median_ms"] for k in ("a_packed", "b_composite", "c_two_plain", "length_only"))
        spread = max(row["a_packed"]["spread_ms"], row["b_composite"]["spread_ms"])
        row["longest_item_bytes"] = int(longest)
        row["offset_kernels_ms_a_minus_c"] = round(a - c, 4)
        row["length_pass_share_of_a"] = round(lo / a, 3)
        row["b_over_a"] = round(b / a, 2)
        row["a_below_b_by_more_than_the_spread"] = bool(b - a > spread)
        lib.aws_huffman_amd_encode_plan_destroy(plan_a)
        eng.free(d_off)
    lib.aws_huffman_amd_encode_plan_destroy(plan_b)
    eng.free(d_in)
    eng.free(d_out)
    print(name, json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="-")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=15)  # (the clocks settle in about 13 steps)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--shrink", type=int, default=1)  # (a quick look: so many times fewer items; not the measurement)
    args = ap.parse_args()
    lib = harness.load_product(args.lib)
    lib.aws_huffman_amd_encode_plan_reset.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_reset.argtypes = [C.c_void_p, ITEM_P, C.c_size_t]
    pa = None
    if not args.baseline_only:
        import packed_api as pa

        pa.bind(lib)
    patterns, lens = harness.load_table()
    coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    eng = harness.Engine(lib, coder)
    out = {"steps": args.steps, "warmup": args.warmup, "runs": args.runs, "baseline_only": bool(args.baseline_only), "shrink": args.shrink,
           "library": os.path.relpath(args.lib or harness.PRODUCT_SO, REPO), "clock": "host, first call to stream idle, ms",
           "shapes": {}}
    for name, in_lens in shapes(args.shrink):
        out["shapes"][name] = measure(eng, name, in_lens, args, pa)
    eng.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out != "-":
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
