#!/usr/bin/env python3
"""Rate of the symbol-count kernel (aws_huffman_amd_symbol_counts) on 1 GiB of five inputs, and what a coder fitted to
printable text buys against the test coder.  Prints one JSON document (and writes it to the path given).

  count     : per input, the median of >= 20 launches between device events, in ms and TB/s of bytes read
  build     : host time of code_lengths_from_counts + table_coder_from_lengths + engine_new
  printable : bits per symbol of the fitted [4, 12] coder against the entropy, and encode / decode GiB/s through plans
              of one 1 GiB item, the fitted coder next to the test coder on the same data

Kernel durations come from a separate rocprofv3 --kernel-trace --stats run of this script.
usage: count_rate.py [out.json] [launches]"""
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
import harness  # noqa: E402

GiB = 1 << 30
LAUNCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 30


def timed(eng, fn, launches=LAUNCHES, warmup=3):
    for _ in range(warmup):
        fn()
    eng.sync()
    ev = eng.new_events(2)
    times = []
    for _ in range(launches):
        eng.record(ev[0])
        fn()
        eng.record(ev[1])
        eng.sync()
        times.append(eng.elapsed_ms(ev[0], ev[1]))
    for e in ev:
        eng.lib.aws_huffman_amd_event_destroy(eng.h, e)
    return statistics.median(times), min(times)


def main():
    lib = ba.bind(harness.load_product())
    patterns, lens = harness.load_table()
    test_coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    eng = harness.Engine(lib, test_coder)
    n = GiB
    d_in = eng.alloc(n + 64)
    d_counts = eng.alloc(256 * 8)
    raw = harness.splitmix64_bytes(41, n)
    shapes = {
        "uniform": (raw, 0),
        "printable": (harness.printable_map(raw), 0),
        "one_byte": (np.full(n, 0x41, np.uint8), 0),
        "two_symbols": (np.where(raw & 1, 0x41, 0x61).astype(np.uint8), 0),
        "uniform_offset5": (raw, 5),
    }
    out = {"bytes": n, "launches": LAUNCHES, "count": {}}
    printable_counts = None
    for name, (data, off) in shapes.items():
        eng.upload(d_in, data, offset=off)
        eng.fill(d_counts, 0, 256 * 8)

        def launch():
            assert lib.aws_huffman_amd_symbol_counts(-1, d_in + off, n, d_counts, eng.stream) == 0

        med, best = timed(eng, launch)
        eng.fill(d_counts, 0, 256 * 8)
        launch()
        counts = eng.download(d_counts, 256 * 8).view(np.uint64).copy()
        assert np.array_equal(counts, ba.bincount(data)), name
        out["count"][name] = {"median_ms": round(med, 4), "min_ms": round(best, 4), "TB_per_s": round(n / med / 1e9, 3)}
        if name == "printable":
            printable_counts = counts
        print(name, out["count"][name], flush=True)

    # the host half: lengths, coder, engine
    t0 = time.perf_counter()
    num_bits = ba.U8x256()
    assert lib.aws_huffman_amd_code_lengths_from_counts(ba.U64x256(*[int(c) for c in printable_counts]), 4, 12,
                                                        ba.CODE_EVERY_SYMBOL, num_bits) == 0
    t1 = time.perf_counter()
    fitted = lib.aws_huffman_amd_table_coder_from_lengths(num_bits)
    t2 = time.perf_counter()
    feng = harness.Engine(lib, fitted)
    t3 = time.perf_counter()
    out["build_ms"] = {"code_lengths": round((t1 - t0) * 1e3, 4), "coder": round((t2 - t1) * 1e3, 4),
                       "engine_new": round((t3 - t2) * 1e3, 3)}

    # printable text through both coders
    data = shapes["printable"][0]
    p = printable_counts.astype(np.float64) / n
    entropy = float(-(p[p > 0] * np.log2(p[p > 0])).sum())
    lengths = list(num_bits)
    fitted_bits = float(sum(int(c) * l for c, l in zip(printable_counts, lengths))) / n
    test_bits = float(sum(int(c) * l for c, l in zip(printable_counts, list(lens)))) / n
    rows = {"entropy_bits_per_symbol": round(entropy, 4)}
    for label, e, bits in (("fitted_4_12", feng, fitted_bits), ("test_coder", eng, test_bits)):
        cap = int(n * bits / 8) + 64
        din, dout, dback = e.alloc(n), e.alloc(cap), e.alloc(n)
        e.upload(din, data)
        plan = e.encode_plan([{"in_offset": 0, "in_len": n, "out_offset": 0, "out_capacity": cap}])
        enc_med, _ = timed(e, lambda: e.encode_launch(plan, din, dout), launches=20)
        (rc, _, _, produced, _, _), = e.encode_results(plan, 1)
        assert rc == 0
        dplan = e.decode_plan([{"in_offset": 0, "in_len": produced, "out_offset": 0, "out_capacity": n}])
        dec_med, _ = timed(e, lambda: e.decode_launch(dplan, dout, dback), launches=20)
        (rc, _, dproduced, _), = e.decode_results(dplan, 1)
        assert rc == 0 and dproduced == n
        assert np.array_equal(e.download(dback, 1 << 20), data[: 1 << 20])
        rows[label] = {"bits_per_symbol": round(bits, 4), "encoded_bytes": int(produced),
                       "one_pass": bool(lib.aws_huffman_amd_engine_encodes_in_one_pass(e.h)),
                       "max_code_bits": int(lib.aws_huffman_amd_engine_max_code_bits(e.h)),
                       "encode_ms": round(enc_med, 4), "encode_GiB_per_s": round(1e3 / enc_med, 1),
                       "decode_ms": round(dec_med, 4), "decode_GiB_per_s": round(1e3 / dec_med, 1)}
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        lib.aws_huffman_amd_decode_plan_destroy(dplan)
        for q in (din, dout, dback):
            e.free(q)
    out["printable_text"] = rows
    feng.close()
    eng.free(d_in)
    eng.free(d_counts)
    eng.close()
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1 and sys.argv[1] != "-":
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
