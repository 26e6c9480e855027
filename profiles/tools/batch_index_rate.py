#!/usr/bin/env python3
"""What one block index over the items of a batch (aws_huffman_amd_encode_plan_block_index, huffman_amd_batch_index.h) costs
on uniform bytes resident in device memory, next to its yardsticks.  Prints one JSON document (and writes it to the path
given, by default profiles/batch_index_mi355x.json).

One process, device events (host clock where a call itself waits), medians of `--launches` launches behind `--warmup`
launches that are thrown away.  Every step runs under an alarm of `--step-seconds` whose default action ends the process:
the script ends at the first failure.

  single   : aws_huffman_amd_symbol_counts and aws_huffman_amd_block_index (64 and 16 384 symbols a block) over 1 GiB: the
             two older bodies of count_kernel.  With --single-only nothing else runs, so that the same numbers can be taken
             from the parent commit's build (--lib) on the same box, in turn.
  one_item : the 1 GiB as ONE item of a plan: the batch call against aws_huffman_amd_block_index of the same bytes; the last
             entry of both indexes must agree.
  batches  : 65 536 items of 16 KiB, and 1 Mi items of 16 .. 80 bytes, at 64 and 16 384 symbols a block: the batch call
             against aws_huffman_amd_symbol_counts over the same bytes (which reads them once: the floor) and against
             aws_huffman_amd_block_index over the same bytes taken as one stream.
  ranges   : the 65 536 items encoded by a packed launch and indexed at 512 symbols a block: a random 1 % of all blocks as
             item block ranges (reset + launch on the host's clock, the launch alone between events) against the whole
             batch decoded by aws_huffman_amd_decode_plan_launch_packed.

usage: batch_index_rate.py [out.json] [--launches N] [--warmup N] [--shrink N] [--lib path] [--single-only]"""
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
import packed_decode_api as pda  # noqa: E402
from block_index_rate import Steps, timed_events, timed_host  # noqa: E402

GiB = 1 << 30
BLOCKS = (64, 16_384)


def ratio(row, key, over):
    if row[over]["median_ms"]:  # (0 under the emulator build, whose events measure nothing: a rehearsal)
        row[key]["over_" + over] = round(row[key]["median_ms"] / row[over]["median_ms"], 3)


def measure_single(lib, eng, d_in, n, args, step):
    step("single: counts and the single-stream index")
    d_counts, d_index, d_status = eng.alloc(256 * 8), eng.alloc(8 * (n // 64 + 2)), eng.alloc(4)
    eng.fill(d_counts, 0, 256 * 8)
    row = {"count": timed_events(eng, lambda: lib.aws_huffman_amd_symbol_counts(-1, d_in, n, d_counts, eng.stream),
                                 args.launches, args.warmup)}
    for B in BLOCKS:
        row["index_%d" % B] = timed_events(eng, lambda: ia.block_index(eng, d_in, n, B, d_index, d_status, eng.stream),
                                           args.launches, args.warmup)
    for d in (d_counts, d_index, d_status):
        eng.free(d)
    print("single", json.dumps(row), flush=True)
    return row


def measure_batch(bi, lib, eng, d_in, offsets, lengths, label, args, step):
    """The batch call over these items, the counts and the single-stream call over the bytes they span."""
    n_items = len(lengths)
    span = int(offsets[-1] + lengths[-1])
    step("%s: plan" % label)
    plan, d_items = pa.plan_from_records(eng, offsets, lengths)
    d_counts = eng.alloc(256 * 8)
    eng.fill(d_counts, 0, 256 * 8)
    row = {"items": n_items, "bytes": int(np.sum(lengths)), "span_bytes": span,
           "count": timed_events(eng, lambda: lib.aws_huffman_amd_symbol_counts(-1, d_in, span, d_counts, eng.stream),
                                 args.launches, args.warmup)}
    for B in BLOCKS:
        step("%s: %d symbols a block" % (label, B))
        blocks = int(np.sum((np.asarray(lengths, dtype=np.int64) + B - 1) // B))
        a = bi.Arrays(eng, n_items, blocks + 1)
        d_one = eng.alloc(8 * (span // B + 2))
        call = lambda: bi.plan_block_index(eng, plan, d_in, B, a.d_dir, a.d_index, blocks + 1, a.d_status, eng.stream)
        assert call() == (0, 0)
        eng.sync()
        assert int(eng.download(a.d_status, 4).view(np.uint32)[0]) == bi.INDEX_OK
        assert bi.index_size(eng, plan) == (0, 0, blocks + 1)
        key = "batch_index_%d" % B
        row[key] = timed_events(eng, call, args.launches, args.warmup)
        row[key]["blocks"] = blocks
        one = "one_stream_index_%d" % B
        row[one] = timed_events(eng, lambda: ia.block_index(eng, d_in, span, B, d_one, None, eng.stream), args.launches, args.warmup)
        ratio(row, key, "count")
        ratio(row, key, one)
        if n_items == 1:  # the same bytes, the same blocks: the same last entry
            assert int(pa.download_u64(eng, a.d_index + 8 * blocks, 1)[0]) == int(pa.download_u64(eng, d_one + 8 * blocks, 1)[0])
        a.close()
        eng.free(d_one)
    lib.aws_huffman_amd_encode_plan_destroy(plan)
    eng.free(d_items)
    eng.free(d_counts)
    print(label, json.dumps(row), flush=True)
    return row


def measure_ranges(bi, lib, eng, d_in, offsets, lengths, args, step):
    B = 512
    n_items = len(lengths)
    step("ranges: index and packed encode")
    plan, d_items = pa.plan_from_records(eng, offsets, lengths)
    per_item = (np.asarray(lengths, dtype=np.int64) + B - 1) // B
    first = np.concatenate([[0], np.cumsum(per_item)])
    blocks = int(first[-1])
    a = bi.Arrays(eng, n_items, blocks + 1)
    assert bi.plan_block_index(eng, plan, d_in, B, a.d_dir, a.d_index, blocks + 1, a.d_status) == (0, 0)
    cap = int(np.sum(lengths)) * 2 + 64
    d_enc, d_off = eng.alloc(cap), eng.alloc(8 * (n_items + 1))
    assert pa.launch_packed(eng, plan, d_in, d_enc, cap, d_off, 1) == (0, 0)
    rc, err, total, _ = pa.packed_size(eng, plan)
    assert (rc, err) == (0, 0) and total <= cap
    lib.aws_huffman_amd_encode_plan_destroy(plan)
    eng.free(d_items)
    rng = np.random.default_rng(7)
    picked = np.sort(rng.permutation(blocks)[:max(blocks // 100, 1)])
    item = np.searchsorted(first, picked, side="right") - 1
    recs = np.zeros((picked.size, 4), np.uint64)
    recs[:, 0], recs[:, 1], recs[:, 2], recs[:, 3] = item, picked - first[item], 1, np.arange(picked.size) * B
    d_ranges = pda.upload_u64(eng, recs.reshape(-1))
    symbols = int(np.sum(lengths))
    d_out, d_sym = eng.alloc(symbols + 64), eng.alloc(8 * (n_items + 1))
    dplan = eng.empty_decode_plan()
    step("ranges: one percent of the blocks")
    reset = lambda: lib.aws_huffman_amd_decode_plan_reset_item_block_ranges(dplan, a.d_dir, a.d_index, blocks + 1, n_items, B, d_off, None,
                                                                            0, total, d_ranges, picked.size, None)
    launch = lambda: lib.aws_huffman_amd_decode_plan_launch(dplan, d_enc, d_out, None)
    assert reset() == 0
    row = {"block_symbols": B, "items": n_items, "blocks": blocks, "ranges": int(picked.size), "encoded_bytes": int(total),
           "one_percent_reset_and_launch_host": timed_host(eng, lambda: (reset(), launch()), args.launches, args.warmup),
           "one_percent_launch_alone": timed_events(eng, launch, args.launches, args.warmup)}
    res = pda.results_array(eng, dplan, picked.size)
    sizes = np.minimum((picked - first[item] + 1) * B, np.asarray(lengths)[item]) - (picked - first[item]) * B
    assert np.array_equal(res["produced"].astype(np.int64), sizes)
    for i in (0, picked.size // 2, picked.size - 1):  # three of the ranges against the symbols they came from
        src = int(offsets[item[i]]) + int(picked[i] - first[item[i]]) * B
        assert np.array_equal(eng.download(d_out, int(sizes[i]), offset=i * B), eng.download(d_in, int(sizes[i]), offset=src)), i
    step("ranges: the whole batch by a packed launch")
    whole_reset = lambda: pda.reset_packed_input(eng, dplan, d_off, None, n_items)
    whole = lambda: pda.launch_packed(eng, dplan, d_enc, d_out, symbols, d_sym, 1)
    assert whole_reset() == (0, 0)
    row["whole_batch_reset_and_launch_host"] = timed_host(eng, lambda: (whole_reset(), whole()), args.launches, args.warmup)
    row["whole_batch_launch_alone"] = timed_events(eng, whole, args.launches, args.warmup)
    assert pda.packed_size(eng, dplan)[:3] == (0, 0, symbols)
    lib.aws_huffman_amd_decode_plan_destroy(dplan)
    a.close()
    for d in (d_enc, d_off, d_ranges, d_out, d_sym):
        eng.free(d)
    print("ranges", json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(REPO, "profiles", "batch_index_mi355x.json"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--shrink", type=int, default=1, help="every size divided by this (a rehearsal)")
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--single-only", action="store_true")
    args = ap.parse_args()
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
           "tool": "profiles/tools/batch_index_rate.py (one MI355X, one process, device events)"}
    out["single"] = measure_single(lib, eng, d_in, n, args, step)
    if not args.single_only:
        import batch_index_api as bi
        bi.bind(lib)
        out["one_item"] = measure_batch(bi, lib, eng, d_in, np.asarray([0]), np.asarray([n]), "one item", args, step)
        many = 65_536 // args.shrink
        size = n // many
        out["items_of_16_KiB"] = measure_batch(bi, lib, eng, d_in, np.arange(many, dtype=np.int64) * size,
                                               np.full(many, size, np.int64), "items of 16 KiB", args, step)
        small = np.random.default_rng(11).integers(16, 81, (1 << 20) // args.shrink).astype(np.int64)
        at = np.concatenate([[0], np.cumsum(small)])[:-1]
        out["items_of_16_to_80_bytes"] = measure_batch(bi, lib, eng, d_in, at, small, "items of 16 to 80 bytes", args, step)
        out["ranges"] = measure_ranges(bi, lib, eng, d_in, np.arange(many, dtype=np.int64) * size, np.full(many, size, np.int64),
                                       args, step)
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
