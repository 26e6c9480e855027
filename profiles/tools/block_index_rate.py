#!/usr/bin/env python3
"""What the block index (aws_huffman_amd_block_index) costs next to the symbol-count kernel, and what a decode of ranges
(aws_huffman_amd_decode_plan_reset_block_ranges) costs next to the decode of the whole stream, on 1 GiB resident in device
memory.  Prints one JSON document (and writes it to the path given).

One process, device events (host clock where a call itself waits), medians of `--launches` launches behind `--warmup`
launches that are thrown away (the clocks settle over about 13 steps).  Every step runs under an alarm of
`--step-seconds` whose default action ends the process: the script ends at the first failure.

  index   : uniform and printable bytes; aws_huffman_amd_symbol_counts and aws_huffman_amd_block_index at 64, 512 and
            16 384 symbols a block on the same buffer (the whole call: block bits + scan), their ratio, and the call with
            the buffer one byte off a 16-byte boundary.  The first 4 MiB of every index are checked against numpy.
  ranges  : the uniform stream encoded by a plain launch, indexed at 16 384 symbols a block: a random 1 % of its blocks and
            all of its blocks as range plans (reset + launch on the host's clock, launch alone between events), and the
            whole stream as one item -- the only way to those symbols without an index.

--trace runs a handful of launches of each step and times nothing: for `rocprofv3 --kernel-trace --output-format csv`,
whose per-dispatch durations --merge-trace then adds to the JSON (the block-bits pass alone beside the count; the scan's two
kernels separately).
usage: block_index_rate.py [out.json] [--launches N] [--warmup N] [--shrink N] [--lib path] [--trace]
       block_index_rate.py out.json --merge-trace kernel_trace.csv"""
import argparse
import csv
import ctypes as C
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
import harness  # noqa: E402
import index_api as ia  # noqa: E402

GiB = 1 << 30
BLOCKS = (64, 512, 16_384)
TRACE_LAUNCHES = 5


class Steps:
    """Each step under an alarm of its own (SIGALRM's default action: the process ends, also inside a driver call)."""

    def __init__(self, seconds):
        self.seconds = seconds
        signal.signal(signal.SIGALRM, signal.SIG_DFL)

    def __call__(self, label):
        signal.alarm(self.seconds)
        print("step:", label, flush=True)

    def done(self):
        signal.alarm(0)


def timed_events(eng, fn, launches, warmup):
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
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4)}


def timed_host(eng, fn, launches, warmup):
    """fn and the wait for the stream, on the host's clock."""
    times = []
    for k in range(warmup + launches):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        eng.sync()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4)}


def fill(eng, d_in, n, shape):
    if shape == "uniform":
        eng.fill_splitmix64(d_in, n, 41)
        return
    step = 64 << 20
    for off in range(0, n, step):
        size = min(step, n - off)
        eng.upload(d_in, harness.printable_map(harness.splitmix64_bytes(9 + off // step, size)), offset=off)


def measure_index(lib, eng, code_lens, n, args, step):
    out = {}
    d_in, d_counts = eng.alloc(n + 64), eng.alloc(256 * 8)
    d_index, d_status = eng.alloc(8 * (n // 64 + 2)), eng.alloc(4)
    for shape in ("uniform", "printable"):
        step("index: %s" % shape)
        fill(eng, d_in, n, shape)
        eng.fill(d_counts, 0, 256 * 8)
        row = {"count": timed_events(eng, lambda: lib.aws_huffman_amd_symbol_counts(-1, d_in, n, d_counts, eng.stream),
                                     args.launches, args.warmup)}
        head = eng.download(d_in, min(n, 4 << 20) + 1)
        for B in BLOCKS:
            for off in (0, 1):
                call = lambda: ia.block_index(eng, d_in + off, n - off, B, d_index, d_status, eng.stream)
                key = "index_%d" % B + ("_off1" if off else "")
                row[key] = timed_events(eng, call, args.launches, args.warmup)
                if row["count"]["median_ms"]:  # (0 under the emulator build, whose events measure nothing: a rehearsal)
                    row[key]["over_count"] = round(row[key]["median_ms"] / row["count"]["median_ms"], 3)
                # (the prefix of the index is the prefix's index: the first 4 MiB against numpy)
                part = head[off:off + min(n - off, 4 << 20) // B * B]
                want = ia.expected_index(code_lens, part, B)
                got = ia.pa.download_u64(eng, d_index, want.size)
                assert np.array_equal(got, want), (shape, B, off)
                assert int(eng.download(d_status, 4).view(np.uint32)[0]) == ia.INDEX_OK
        out[shape] = row
        print(shape, json.dumps(row), flush=True)
    for d in (d_in, d_counts, d_index, d_status):
        eng.free(d)
    return out


def measure_ranges(lib, eng, n, args, step):
    B = 16_384
    nb = ia.n_blocks_of(n, B)
    step("ranges: encode and index")
    d_in = eng.alloc(n + 64)
    fill(eng, d_in, n, "uniform")
    cap = n * 2 + 64
    d_enc, d_out = eng.alloc(cap), eng.alloc(n + 64)
    plan = eng.encode_plan([{"in_offset": 0, "in_len": n, "out_offset": 0, "out_capacity": cap}])
    eng.encode_launch(plan, d_in, d_enc)
    (rc, _, consumed, produced, _, _), = eng.encode_results(plan, 1)
    assert rc == 0 and consumed == n
    lib.aws_huffman_amd_encode_plan_destroy(plan)
    d_index = eng.alloc(8 * (nb + 1))
    assert ia.block_index(eng, d_in, n, B, d_index, None) == (0, 0)
    eng.sync()
    total_bits = int(ia.pa.download_u64(eng, d_index, nb + 1)[-1])
    assert (total_bits + 7) // 8 == produced, (total_bits, produced)
    rng = np.random.default_rng(7)
    picked = rng.permutation(nb)[:max(nb // 100, 1)]
    out = {"block_symbols": B, "blocks": nb, "encoded_bytes": int(produced)}
    dplan = eng.empty_decode_plan()
    for label, blocks in (("one_percent_of_blocks", picked), ("all_blocks", np.arange(nb))):
        step("ranges: %s" % label)
        arr = (ia.BlockRange * blocks.size)(*[ia.BlockRange(int(b), 1, i * B) for i, b in enumerate(blocks)])
        d_ranges = eng.alloc(C.sizeof(arr))
        eng.upload(d_ranges, np.frombuffer(arr, dtype=np.uint8))
        reset = lambda: ia.reset_block_ranges(eng, dplan, d_index, n, B, 0, produced, d_ranges, blocks.size)
        launch = lambda: lib.aws_huffman_amd_decode_plan_launch(dplan, d_enc, d_out, None)
        assert reset() == (0, 0)
        row = {"ranges": int(blocks.size), "symbols": int(min(blocks.size * B, n)),
               "reset_and_launch_host": timed_host(eng, lambda: (reset(), launch()), args.launches, args.warmup),
               "launch_alone": timed_events(eng, launch, args.launches, args.warmup)}
        res = ia.pda.results_array(eng, dplan, blocks.size)
        sizes = np.minimum((blocks + 1) * B, n) - blocks * B
        assert np.array_equal(res["produced"].astype(np.int64), sizes)
        for i in (0, blocks.size // 2, blocks.size - 1):  # three of the ranges against the symbols they came from
            want = eng.download(d_in, int(sizes[i]), offset=int(blocks[i]) * B)
            assert np.array_equal(eng.download(d_out, int(sizes[i]), offset=i * B), want), (label, i)
        out[label] = row
        print(label, json.dumps(row), flush=True)
        eng.free(d_ranges)
    lib.aws_huffman_amd_decode_plan_destroy(dplan)
    step("ranges: the whole stream as one item")
    whole = eng.decode_plan([{"in_offset": 0, "in_len": int(produced), "out_offset": 0, "out_capacity": n}])
    out["whole_stream_one_item"] = {"launch_alone": timed_events(eng, lambda: eng.decode_launch(whole, d_enc, d_out),
                                                                 args.launches, args.warmup)}
    (rc, _, got, _), = eng.decode_results(whole, 1)
    assert rc == 0 and got == n
    lib.aws_huffman_amd_decode_plan_destroy(whole)
    print("whole", json.dumps(out["whole_stream_one_item"]), flush=True)
    for d in (d_in, d_enc, d_out, d_index):
        eng.free(d)
    return out


def trace(lib, eng, n, step):
    """count_kernel, then the index at each block size, TRACE_LAUNCHES launches each, in this order (--merge-trace relies on it)."""
    step("trace")
    d_in, d_counts = eng.alloc(n + 64), eng.alloc(256 * 8)
    d_index, d_status = eng.alloc(8 * (n // 64 + 2)), eng.alloc(4)
    fill(eng, d_in, n, "uniform")
    eng.fill(d_counts, 0, 256 * 8)
    for _ in range(TRACE_LAUNCHES):
        assert lib.aws_huffman_amd_symbol_counts(-1, d_in, n, d_counts, eng.stream) == 0
    for B in BLOCKS:
        for _ in range(TRACE_LAUNCHES):
            assert ia.block_index(eng, d_in, n, B, d_index, d_status, eng.stream) == (0, 0)
    eng.sync()


def merge_trace(json_path, csv_path):
    """Per step and block size, the median duration of its dispatches in a --trace run.  The block-bits pass is a body of
    count_kernel and the scan is the two pack kernels, so the dispatches are told apart by their order: TRACE_LAUNCHES
    counts, then TRACE_LAUNCHES index calls for each block size."""
    rows = list(csv.DictReader(open(csv_path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        for name in ("count_kernel", "pack_tile_sums_kernel", "pack_offsets_kernel"):
            if name in r["Kernel_Name"]:
                by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    doc = json.load(open(json_path))
    med = lambda v: round(statistics.median(v), 4)
    groups = TRACE_LAUNCHES * len(BLOCKS)
    assert len(by["count_kernel"]) == TRACE_LAUNCHES + groups, len(by["count_kernel"])
    out = {"count": med(by["count_kernel"][:TRACE_LAUNCHES])}
    steps = {"block_bits": by["count_kernel"][TRACE_LAUNCHES:], "scan_tile_sums": by["pack_tile_sums_kernel"],
             "scan_offsets": by["pack_offsets_kernel"]}
    for name, got in steps.items():
        assert len(got) == groups, (name, len(got))
        for k, B in enumerate(BLOCKS):
            out["%s_%d" % (name, B)] = med(got[k * TRACE_LAUNCHES:(k + 1) * TRACE_LAUNCHES])
    for B in BLOCKS:
        out["block_bits_over_count_%d" % B] = round(out["block_bits_%d" % B] / out["count"], 3)
    doc["kernel_trace_ms"] = out
    with open(json_path, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="-")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--shrink", type=int, default=1, help="1 GiB / this (a rehearsal)")
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--merge-trace", default=None)
    args = ap.parse_args()
    if args.merge_trace:
        return merge_trace(args.out, args.merge_trace)
    assert args.warmup >= 15 or args.shrink > 1, "the clocks settle over about 13 launches"
    lib = ia.bind(harness.load_product(args.lib))
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: nothing is measured without one"
    patterns, lens = harness.load_table()
    coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    eng = harness.Engine(lib, coder)
    code_lens = np.asarray(list(lens), dtype=np.int64)
    n = GiB // args.shrink
    step = Steps(args.step_seconds)
    if args.trace:
        trace(lib, eng, n, step)
        step.done()
        eng.close()
        return
    out = {"bytes": n, "launches": args.launches, "warmup": args.warmup,
           "tool": "profiles/tools/block_index_rate.py (one MI355X, one process, device events)"}
    out["index"] = measure_index(lib, eng, code_lens, n, args, step)
    out["ranges"] = measure_ranges(lib, eng, n, args, step)
    step.done()
    eng.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out != "-":
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
