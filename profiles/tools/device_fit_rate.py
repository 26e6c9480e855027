#!/usr/bin/env python3
"""What a coder fitted on the device costs (huffman_amd_fit.h), on 1 GiB of printable bytes that is resident on the GPU
and laid out as 65 536 items of 16 KiB.  In one process, device events on one stream, the median of `steps` steps behind
`warmup` unrecorded ones, in `runs` runs whose medians' spread is recorded:
  a  fit        : aws_huffman_amd_engine_fit_counts alone (one kernel)
  b  chain      : clear the counts, aws_huffman_amd_symbol_counts, fit, aws_huffman_amd_encode_plan_launch_packed
  c  host route : what the chain replaces, with the interfaces that existed before it -- count, copy the counts back (the
                  wait), aws_huffman_amd_code_lengths_from_counts, aws_huffman_amd_table_coder_from_lengths,
                  aws_huffman_amd_engine_new, a new plan, the packed launch.  Events around it on the same stream, and the
                  host's clock from the first call to the stream idle.  (Freeing that engine, plan and coder afterwards is
                  outside both clocks.)
The three take turns inside every step.  (c) is the yardstick: no earlier number exists for this step.
Both roads' output is compared once, byte for byte.
--only-chain N: N chains and nothing else, for a kernel trace (rocprofv3 --kernel-trace --stats -- python this --only-chain 20).
usage: device_fit_rate.py [out.json] [--steps N] [--warmup N] [--runs N] [--mib N] [--only-chain N]"""
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
import build_api as ba  # noqa: E402
import fit_api as fa  # noqa: E402
import harness  # noqa: E402
import packed_api as pa  # noqa: E402

ITEM_P = C.POINTER(harness.AmdEncodeItem)
ITEM_BYTES = 16384


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="-")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)  # (the clocks settle in about 13 steps)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--only-chain", type=int, default=0)
    args = ap.parse_args()
    lib = fa.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no GPU: nothing to measure"
    hip = fa.Hip()
    n_bytes = args.mib << 20
    n = n_bytes // ITEM_BYTES
    capacity = n_bytes * 12 // 8 + n
    eng = fa.FittedEngine(lib, 4, 12)
    st = C.c_void_p(eng.stream)
    d_in, d_out, d_off = eng.alloc(n_bytes), eng.alloc(capacity), eng.alloc(8 * (n + 1))
    # printable bytes, resident: 64 MiB made on the host, repeated on the device
    piece = harness.printable_map(harness.splitmix64_bytes(4, min(n_bytes, 64 << 20)))
    for at in range(0, n_bytes, piece.size):
        eng.upload(d_in, piece[:min(piece.size, n_bytes - at)], offset=at)
    recs = np.zeros(n, pa.ITEM_DTYPE)
    recs["in_len"], recs["eos_padding"] = ITEM_BYTES, 0xFF
    recs["in_offset"] = np.arange(n, dtype=np.uint64) * ITEM_BYTES
    plan = C.c_void_p()
    assert lib.aws_huffman_amd_encode_plan_new(C.byref(plan), eng.h, recs.ctypes.data_as(ITEM_P), n) == 0
    ev = eng.new_events(2)

    def timed(enqueue):
        assert lib.aws_huffman_amd_event_record(eng.h, ev[0], st) == 0
        enqueue()
        assert lib.aws_huffman_amd_event_record(eng.h, ev[1], st) == 0
        eng.sync()
        return eng.elapsed_ms(ev[0], ev[1])

    def fit():
        assert eng.fit_counts_async(None, st) == (0, 0)

    def chain():
        fa.enqueue_chain(hip, eng, plan, d_in, n_bytes, d_out, capacity, d_off, st)

    if args.only_chain:
        for _ in range(args.only_chain):
            chain()
        eng.sync()
        print(json.dumps({"chains": args.only_chain, "status": eng.status()}))
        return

    counts = np.zeros(256, np.uint64)
    left = []  # what a step of the host route leaves to free: outside the clocks

    def host_route():
        hip.memset_async(eng.d_counts, 0, 256 * 8, st)
        assert lib.aws_huffman_amd_symbol_counts(-1, d_in, n_bytes, eng.d_counts, st) == 0
        assert lib.aws_huffman_amd_copy_to_host(eng.h, counts.ctypes.data, eng.d_counts, 256 * 8) == 0
        rc, _, lengths = ba.lengths_from_counts(lib, counts, 4, 12, ba.CODE_EVERY_SYMBOL)
        assert rc == 0
        coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*lengths))
        other = harness.Engine(lib, coder)
        p = C.c_void_p()
        assert lib.aws_huffman_amd_encode_plan_new(C.byref(p), other.h, recs.ctypes.data_as(ITEM_P), n) == 0
        assert lib.aws_huffman_amd_encode_plan_launch_packed(p, d_in, d_out, capacity, d_off, 1, st) == 0
        left.append((other, p, coder))

    def free_left():
        for other, p, coder in left:
            lib.aws_huffman_amd_encode_plan_destroy(p)
            other.close()
            lib.aws_huffman_amd_table_coder_destroy(coder)
        del left[:]

    # the two roads make the same bytes
    chain()
    eng.sync()
    assert eng.status() == fa.FIT_OK
    total = int(pa.download_u64(eng, d_off, n + 1)[-1])
    dense = eng.download(d_out, total)
    eng.fill(d_out, 0, total)
    host_route()
    eng.sync()
    assert int(pa.download_u64(eng, d_off, n + 1)[-1]) == total and np.array_equal(eng.download(d_out, total), dense)
    free_left()
    del dense

    names = ("a_fit", "b_chain", "c_host_route", "c_host_route_wall")
    runs = {k: [] for k in names}
    for _ in range(args.runs):
        times = {k: [] for k in names}
        for step in range(args.warmup + args.steps):
            a = timed(fit)
            b = timed(chain)
            t0 = time.perf_counter()
            c = timed(host_route)
            wall = (time.perf_counter() - t0) * 1e3
            free_left()
            if step >= args.warmup:
                for k, v in zip(names, (a, b, c, wall)):
                    times[k].append(v)
        for k in names:
            runs[k].append(statistics.median(times[k]))
    out = {"bytes": n_bytes, "items": n, "item_bytes": ITEM_BYTES, "data": "printable", "bounds": [4, 12], "encoded_bytes": total,
           "steps": args.steps, "warmup": args.warmup, "runs": args.runs,
           "clock": "device events on one stream, ms (c_host_route_wall: the host's clock, first call to stream idle)"}
    for k in names:
        out[k] = {"median_ms": round(statistics.median(runs[k]), 4), "run_medians_ms": [round(x, 4) for x in runs[k]],
                  "spread_ms": round(max(runs[k]) - min(runs[k]), 4)}
    out["c_over_b"] = round(out["c_host_route"]["median_ms"] / out["b_chain"]["median_ms"], 2)
    out["c_wall_over_b"] = round(out["c_host_route_wall"]["median_ms"] / out["b_chain"]["median_ms"], 2)
    out["note"] = "c is the yardstick: what a caller had before the fit on the device; no earlier number exists for this step"
    text = json.dumps(out, indent=1)
    print(text)
    if args.out != "-":
        with open(args.out, "w") as f:
            f.write(text + "\n")
    lib.aws_huffman_amd_encode_plan_destroy(plan)
    for d in (d_in, d_out, d_off):
        eng.free(d)
    eng.close()


if __name__ == "__main__":
    main()
