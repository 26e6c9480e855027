#!/usr/bin/env python3
"""What a packed decode launch (aws_huffman_amd_decode_plan_launch_packed) costs next to what a receiver had before it, on
three batches: BASELINE configs[3] (65 536 x 16 KiB of splitmix64 seed 5), a million items of 16-80 bytes of printable
text, and the 1 GiB stream as one item.  The encoded input is made on the device by a plain encode launch.
Prints one JSON document (and writes it to the path given).

Per batch, three ways to the decoded symbols, timed side by side in one process (one after the other in every step, host
clock from the first call to the end of the stream's work; the steps before the clocks have settled are thrown away):
  a  packed     : the packed launch into exactly the total, then a wait for the stream
  b  worst_case : what a receiver has without it -- a plain launch into slots of ceil(8 * in_len / min_bits) symbols
                  each, then aws_huffman_amd_decode_plan_results (the only way to learn a decoded length)
  c  exact      : a plain launch of a plan with the exact capacities at the packed offsets, then the wait: the floor --
                  a is c plus the offset kernels and, for items short enough for a thread or a wave, a second walk
Every figure is the median over the steps of a run; a batch is measured in `runs` runs and the spread between their
medians is recorded beside them.  Also: the symbols b's slots allocate against the packed total.

--baseline-only measures `b` alone and touches no symbol of huffman_amd_packed.h: with --lib it runs against a build of
the commit before the packed decode existed, on the same machine.
usage: packed_decode_rate.py [out.json] [--steps N] [--warmup N] [--runs N] [--baseline-only] [--lib path/to/lib.so] [--shrink N]"""
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

ENC_ITEM = np.dtype([("in_offset", "<u8"), ("in_len", "<u8"), ("out_offset", "<u8"), ("out_capacity", "<u8"),
                     ("pattern", "<u4"), ("num_bits", "u1"), ("pad0", "u1", 3), ("eos_padding", "u1"), ("pad1", "u1", 7)])
ENC_RESULT = np.dtype([("rc", "<i4"), ("error", "<i4"), ("consumed", "<u8"), ("produced", "<u8"), ("pattern", "<u4"),
                       ("num_bits", "u1"), ("pad", "u1", 3)])
DEC_ITEM = np.dtype([("in_offset", "<u8"), ("in_len", "<u8"), ("first_bit", "<u4"), ("pad", "<u4"), ("out_offset", "<u8"),
                     ("out_capacity", "<u8")])
DEC_RESULT = np.dtype([("rc", "<i4"), ("error", "<i4"), ("produced", "<u8"), ("bits_consumed", "<u8")])
assert DEC_ITEM.itemsize == C.sizeof(harness.AmdDecodeItem) and ENC_ITEM.itemsize == C.sizeof(harness.AmdEncodeItem)


def shapes(shrink):
    rng = np.random.default_rng(5)
    short = rng.integers(16, 81, 1_000_000 // shrink).astype(np.uint64)
    return [("65536x16KiB", np.full(65536 // shrink, 16384, np.uint64), False), ("1Mx16-80B", short, True),
            ("1x1GiB", np.asarray([(1 << 30) // shrink], np.uint64), False)]


def starts(lens):
    return np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)


def encoded_input(eng, in_lens, printable):
    """The items encoded by a plain launch into slots of twice their size: (device buffer, offsets, lengths)."""
    lib = eng.lib
    n, in_bytes = int(in_lens.size), int(in_lens.sum())
    slots = 2 * in_lens + 8
    recs = np.zeros(n, ENC_ITEM)
    recs["in_len"], recs["in_offset"], recs["out_offset"], recs["out_capacity"], recs["eos_padding"] = in_lens, starts(in_lens), starts(slots), slots, 0xFF
    d_in, d_enc = eng.alloc(in_bytes + 64), eng.alloc(int(slots.sum()) + 64)
    if printable:
        step = 64 << 20
        for off in range(0, in_bytes, step):
            size = min(step, in_bytes - off)
            eng.upload(d_in, harness.printable_map(harness.splitmix64_bytes(9 + off // step, size)), offset=off)
    else:
        eng.fill_splitmix64(d_in, in_bytes, 5)
    plan = C.c_void_p()
    assert lib.aws_huffman_amd_encode_plan_new(C.byref(plan), eng.h, recs.ctypes.data_as(C.POINTER(harness.AmdEncodeItem)), n) == 0
    assert lib.aws_huffman_amd_encode_plan_launch(plan, d_in, d_enc, False, None) == 0
    res = np.zeros(n, ENC_RESULT)
    assert lib.aws_huffman_amd_encode_plan_results(plan, res.ctypes.data_as(C.POINTER(harness.AmdEncodeResult)), None) == 0
    assert np.all(res["rc"] == 0)
    lib.aws_huffman_amd_encode_plan_destroy(plan)
    eng.free(d_in)
    return d_enc, recs["out_offset"].copy(), res["produced"].copy()


def new_plan(eng, in_offs, in_lens, out_offs, out_caps):
    recs = np.zeros(in_lens.size, DEC_ITEM)
    recs["in_offset"], recs["in_len"], recs["out_offset"], recs["out_capacity"] = in_offs, in_lens, out_offs, out_caps
    plan = C.c_void_p()
    assert eng.lib.aws_huffman_amd_decode_plan_new(C.byref(plan), eng.h, recs.ctypes.data_as(C.POINTER(harness.AmdDecodeItem)), recs.size) == 0
    return plan


def measure(eng, name, in_lens, printable, args, pd, min_bits):
    lib = eng.lib
    n = int(in_lens.size)
    d_enc, enc_offs, enc_lens = encoded_input(eng, in_lens, printable)
    worst = (8 * enc_lens + min_bits - 1) // min_bits
    worst_total = int(worst.sum())
    d_out = eng.alloc(worst_total + 64)
    plan_b = new_plan(eng, enc_offs, enc_lens, starts(worst), worst)
    results = np.zeros(n, DEC_RESULT)
    results_p = results.ctypes.data_as(C.POINTER(harness.AmdDecodeResult))

    def worst_case():
        assert lib.aws_huffman_amd_decode_plan_launch(plan_b, d_enc, d_out, None) == 0
        assert lib.aws_huffman_amd_decode_plan_results(plan_b, results_p, None) == 0

    ways = {"b_worst_case": worst_case}
    worst_case()
    assert np.all(results["rc"] == 0)
    symbols = results["produced"].copy()
    total = int(symbols.sum())
    if pd is not None:
        plan_a = new_plan(eng, enc_offs, enc_lens, np.zeros(n, np.uint64), np.zeros(n, np.uint64))
        plan_c = new_plan(eng, enc_offs, enc_lens, starts(symbols), symbols)
        d_off = eng.alloc(8 * (n + 1))

        def packed():
            assert lib.aws_huffman_amd_decode_plan_launch_packed(plan_a, d_enc, d_out, total, d_off, 1, None) == 0
            eng.sync()

        def exact():
            assert lib.aws_huffman_amd_decode_plan_launch(plan_c, d_enc, d_out, None) == 0
            eng.sync()

        ways = {"a_packed": packed, "b_worst_case": worst_case, "c_exact": exact}

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
    row = {"items": n, "encoded_bytes": int(enc_lens.sum()), "worst_case_symbols": worst_total, "total_symbols": total,
           "worst_case_over_total": round(worst_total / total, 3)}
    for k in ways:
        row[k] = {"median_ms": round(statistics.median(runs[k]), 4), "run_medians_ms": [round(x, 4) for x in runs[k]],
                  "spread_ms": round(max(runs[k]) - min(runs[k]), 4)}
    if pd is not None:
        # the three ways leave the same symbols: the exact launch's dense output against the packed launch's
        exact()
        dense_c = eng.download(d_out, min(total, 256 << 20))
        eng.fill(d_out, 0, min(total, 256 << 20))
        packed()
        rc, _, total_a, longest = pd.packed_size(eng, plan_a)
        assert rc == 0 and total_a == total, (total_a, total)
        assert np.array_equal(eng.download(d_out, dense_c.size), dense_c), "the packed launch and the exact one differ"
        a, b, c = (row[k]["median_ms"] for k in ("a_packed", "b_worst_case", "c_exact"))
        row["longest_item_symbols"] = int(longest)
        row["a_minus_c_ms"] = round(a - c, 4)
        row["a_over_c"] = round(a / c, 3)
        row["b_over_a"] = round(b / a, 3)
        lib.aws_huffman_amd_decode_plan_destroy(plan_a)
        lib.aws_huffman_amd_decode_plan_destroy(plan_c)
        eng.free(d_off)
    lib.aws_huffman_amd_decode_plan_destroy(plan_b)
    eng.free(d_enc)
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
    ap.add_argument("--only", default=None)           # (one batch by name: the kernel trace of the 1 GiB item)
    args = ap.parse_args()
    lib = harness.load_product(args.lib)
    pd = None
    if not args.baseline_only:
        import packed_decode_api as pd

        pd.bind(lib)
    patterns, lens = harness.load_table()
    min_bits = min(int(l) for l in lens if l)
    coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    eng = harness.Engine(lib, coder)
    out = {"steps": args.steps, "warmup": args.warmup, "runs": args.runs, "baseline_only": bool(args.baseline_only), "shrink": args.shrink,
           "library": os.path.relpath(args.lib or harness.PRODUCT_SO, REPO), "clock": "host, first call to stream idle, ms",
           "shapes": {}}
    for name, in_lens, printable in shapes(args.shrink):
        if args.only in (None, name):
            out["shapes"][name] = measure(eng, name, in_lens, printable, args, pd, min_bits)
    eng.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out != "-":
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
