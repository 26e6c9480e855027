#!/usr/bin/env python3
"""What it costs to find where a symbol of an indexed stream starts (aws_huffman_amd_locate_symbols) on either of its two
roads, and what a read of random symbol ranges costs through aws_huffman_amd_decode_plan_reset_symbol_ranges next to the
route that existed before it: aws_huffman_amd_decode_plan_reset_block_ranges over each range's covering blocks.  One stream
of 1 GiB of uniform bytes under the test coder, resident in device memory, indexed at 64, 512 and 16 384 symbols a block.
Prints one JSON document (and writes it to the path given).

Method: one process on one MI355X.  A step is timed between two device events on the engine's stream where nothing in it
waits on the host (locate, a plan's launch), and on the host's clock from the call to the end of a stream synchronize where
the call itself waits (a reset brings a few totals back).  Every figure is the median of `--launches` runs behind `--warmup`
runs that are thrown away (the clocks settle over about 13 steps); the minimum is kept beside it.  Both routes
are measured in the same run on the same stream, positions and ranges (seeded), so their ratio is free of box-to-box
spread.  Every step runs under an alarm of `--step-seconds` whose default action ends the process: the script ends at the
first failure.  What is timed is also checked: located bits against numpy over the block's own symbols for 64 positions (and
the two roads against each other for all of them), decoded ranges against the symbols they came from for three ranges a
plan.

  locate : 65 536 random positions; the lane-a-position road alone (limit above the block) and the workgroup-a-position
           road alone (limit 1), per block size.  "crossover": see DESIGN.md, "Symbols of an indexed stream".
  ranges : 65 536 random ranges of 100 and of 4 096 symbols per block size: reset, launch, and both, for symbol ranges and
           for block ranges over the covering blocks; the output bytes each route reserves; the ratios.

usage: symbol_ranges_rate.py [out.json] [--launches N] [--warmup N] [--shrink N] [--positions N] [--lib path]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import harness  # noqa: E402
import index_api as ia  # noqa: E402
import ranges_api as ra  # noqa: E402
from block_index_rate import Steps, fill, timed_events, timed_host  # noqa: E402

GiB = 1 << 30
BLOCKS = (64, 512, 16_384)
COUNT = 65_536
RANGE_SYMBOLS = (100, 4_096)


def upload_records(eng, kind, rows):
    arr = (kind * len(rows))(*[kind(*r) for r in rows])
    d = eng.alloc(C.sizeof(arr))
    eng.upload(d, np.frombuffer(arr, dtype=np.uint8))
    return d


def measure_locate(lib, eng, code_lens, s, B, args, step):
    step("locate: blocks of %d" % B)
    pos = np.random.default_rng(11).integers(0, s["n"], COUNT).astype(np.uint64)
    d_pos, d_bits, d_status = ia.pda.upload_u64(eng, pos), eng.alloc(8 * COUNT), eng.alloc(4)
    call = lambda: ra.locate_call(eng, s["d_enc"], s["produced"], s["d_index"][B], s["n"], B, d_pos, COUNT, d_bits, d_status, eng.stream)
    row, seen = {}, []
    for road, limit in (("lone_lane", B + 1), ("cooperative", 1), ("built_in_rule", 0)):
        with ra.lone_symbols(lib, limit):
            assert call() == (0, 0)
            row[road] = timed_events(eng, call, args.launches, args.warmup)
        seen.append(ia.pa.download_u64(eng, d_bits, COUNT).astype(np.uint64))
        assert int(eng.download(d_status, 4).view(np.uint32)[0]) == ra.LOCATE_OK
    assert np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], seen[2]), "the roads disagree"
    index = ia.pa.download_u64(eng, s["d_index"][B], s["n"] // B + 1)
    for i in range(0, COUNT, COUNT // 64):
        p = int(pos[i])
        b = p // B
        syms = eng.download(s["d_in"], p - b * B, offset=b * B)
        assert int(seen[0][i]) == int(index[b]) + int(code_lens[syms].sum()), (B, p)
    if row["lone_lane"]["median_ms"]:
        row["cooperative_over_lone_lane"] = round(row["cooperative"]["median_ms"] / row["lone_lane"]["median_ms"], 3)
    for d in (d_pos, d_bits, d_status):
        eng.free(d)
    print("locate", B, json.dumps(row), flush=True)
    return row


def measure_ranges(lib, eng, s, B, symbols, args, step):
    step("ranges: %d symbols, blocks of %d" % (symbols, B))
    n = s["n"]
    firsts = np.random.default_rng(13).integers(0, n - symbols, COUNT)
    cover_first = firsts // B
    cover_count = (firsts + symbols - 1) // B - cover_first + 1
    cover_room = int(cover_count.max()) * B
    sym_rows = [(int(f), symbols, i * symbols) for i, f in enumerate(firsts)]
    blk_rows = [(int(b), int(c), i * cover_room) for i, (b, c) in enumerate(zip(cover_first, cover_count))]
    d_sym, d_blk = upload_records(eng, ra.SymbolRange, sym_rows), upload_records(eng, ia.BlockRange, blk_rows)
    reserved = {"symbol_ranges": COUNT * symbols, "block_ranges": COUNT * cover_room}
    d_out = eng.alloc(max(reserved.values()) + 64)
    plan = eng.empty_decode_plan()
    resets = {
        "symbol_ranges": lambda: ra.reset_symbol_ranges(eng, plan, s["d_enc"], s["d_index"][B], n, B, 0, s["produced"], d_sym, COUNT),
        "block_ranges": lambda: ia.reset_block_ranges(eng, plan, s["d_index"][B], n, B, 0, s["produced"], d_blk, COUNT)}
    launch = lambda: lib.aws_huffman_amd_decode_plan_launch(plan, s["d_enc"], d_out, None)
    row = {"ranges": COUNT, "symbols_a_range": symbols}
    for route, reset in resets.items():
        assert reset() == (0, 0), route
        stats = eng.decode_stats(plan)
        part = {"output_bytes_reserved": reserved[route],
                "symbols_decoded": int(COUNT * symbols if route == "symbol_ranges" else np.minimum((cover_first + cover_count) * B, n).sum() - (cover_first * B).sum()),
                "by_thread": stats["by_thread"], "by_wave": stats["by_wave"], "by_pieces": stats["by_pieces"],
                "reset_host": timed_host(eng, reset, args.launches, args.warmup),
                "launch": timed_events(eng, launch, args.launches, args.warmup),
                "reset_and_launch_host": timed_host(eng, lambda: (reset(), launch()), args.launches, args.warmup)}
        res = ia.pda.results_array(eng, plan, COUNT)
        assert np.all(res["produced"] == (symbols if route == "symbol_ranges" else np.minimum((cover_first + cover_count) * B, n) - cover_first * B))
        for i in (0, COUNT // 2, COUNT - 1):  # three of the ranges against the symbols they came from
            want = eng.download(s["d_in"], symbols, offset=int(firsts[i]))
            at = i * symbols if route == "symbol_ranges" else i * cover_room + int(firsts[i] - cover_first[i] * B)
            assert np.array_equal(eng.download(d_out, symbols, offset=at), want), (route, i)
        row[route] = part
    for key in ("reset_host", "launch", "reset_and_launch_host"):
        if row["symbol_ranges"][key]["median_ms"]:
            row["block_over_symbol_" + key] = round(row["block_ranges"][key]["median_ms"] / row["symbol_ranges"][key]["median_ms"], 3)
    row["block_over_symbol_output_bytes"] = round(reserved["block_ranges"] / reserved["symbol_ranges"], 2)
    lib.aws_huffman_amd_decode_plan_destroy(plan)
    for d in (d_sym, d_blk, d_out):
        eng.free(d)
    print("ranges", B, symbols, json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="-")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--shrink", type=int, default=1, help="1 GiB / this (a rehearsal)")
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--positions", type=int, default=COUNT, help="positions and ranges a step (a rehearsal: fewer)")
    args = ap.parse_args()
    globals()["COUNT"] = args.positions
    assert args.warmup >= 15 or args.shrink > 1, "the clocks settle over about 13 launches"
    lib = ra.bind(harness.load_product(args.lib))
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: nothing is measured without one"
    patterns, lens = harness.load_table()
    coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    eng = harness.Engine(lib, coder)
    code_lens = np.asarray(list(lens), dtype=np.int64)
    n = GiB // args.shrink
    step = Steps(args.step_seconds)
    step("encode and index")
    d_in = eng.alloc(n + 64)
    fill(eng, d_in, n, "uniform")
    cap = n * 2 + 64
    d_enc = eng.alloc(cap)
    plan = eng.encode_plan([{"in_offset": 0, "in_len": n, "out_offset": 0, "out_capacity": cap}])
    eng.encode_launch(plan, d_in, d_enc)
    (rc, _, consumed, produced, _, _), = eng.encode_results(plan, 1)
    assert rc == 0 and consumed == n
    lib.aws_huffman_amd_encode_plan_destroy(plan)
    s = {"n": n, "d_in": d_in, "d_enc": d_enc, "produced": int(produced), "d_index": {}}
    for B in BLOCKS:
        s["d_index"][B] = eng.alloc(8 * (ia.n_blocks_of(n, B) + 1))
        assert ia.block_index(eng, d_in, n, B, s["d_index"][B], None) == (0, 0)
    eng.sync()
    out = {"bytes": n, "encoded_bytes": int(produced), "positions": COUNT, "launches": args.launches, "warmup": args.warmup,
           "tool": "profiles/tools/symbol_ranges_rate.py (one MI355X, one process, device events; host clock where a call waits)",
           "locate": {}, "ranges": {}}
    for B in BLOCKS:
        out["locate"][str(B)] = measure_locate(lib, eng, code_lens, s, B, args, step)
    for B in BLOCKS:
        for symbols in RANGE_SYMBOLS:
            out["ranges"]["%d_symbols_blocks_of_%d" % (symbols, B)] = measure_ranges(lib, eng, s, B, symbols, args, step)
    step.done()
    eng.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out != "-":
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
