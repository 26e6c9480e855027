#!/usr/bin/env python3
"""What the byte planes of differences in runs (aws_huffman_amd_plane_delta_split / _merge, huffman_amd_planes_delta.h) cost
on 1 GiB resident in device memory, beside the plain split and merge of the same build.  Prints one JSON document and writes
it to the path given (by default profiles/planes_delta_mi355x.json).

Device events, medians of `--launches` launches behind `--warmup` launches that are thrown away, one process a table.  Every
step runs under an alarm of `--step-seconds` whose default action ends the process: the script ends at the first failure.

  --table rates : element sizes 2, 4 and 8; runs of 16, 1024 and 2048; uniform bytes and a rising ramp (16 Mi values,
                  repeated).  The plain calls and the copy do not depend on the run: they are taken once for an element
                  size and content, in the same process, and stand in each of its three rows.  Per row:
                    memcpy                hipMemcpyAsync device to device of the same bytes: one read and one write a byte
                    split, merge          the plain calls without counts; counted_split with them
                    split_delta, counted_split_delta, merge_delta   the calls over differences
                  THE RULE, written before the run: a pass of its own for the differences could not do less than one more
                  read and write of every byte, so  split_delta < split + memcpy,  counted_split_delta < counted_split +
                  memcpy  and  merge_delta < merge + memcpy  on every row.  The ratios to the plain calls are reported;
                  nothing was predicted for them.

  --compare     : planes_rate.py's, for the plain roads of this build against two runs of the parent's (see there).
  --merge       : the table, and with --gates name=compared.json ... the compared roads, and with --headline text the
                  bench's, as one document.

usage: planes_delta_rate.py [out.json] --table rates [--launches N] [--warmup N] [--shrink N] [--lib path]
       planes_delta_rate.py [out.json] --merge rates.json [--gates name=compared.json ...] [--headline TEXT]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_api as fa  # noqa: E402
import harness  # noqa: E402
import planes_api as pl  # noqa: E402
import planes_delta_api as pd  # noqa: E402
from block_index_rate import Steps, timed_events  # noqa: E402
from planes_rate import compare  # noqa: E402

GiB = 1 << 30
DEFAULT_OUT = os.path.join(REPO, "profiles", "planes_delta_mi355x.json")
CHUNK_VALUES = 1 << 24
BODIES = {"split_delta": "planes_split_run<E, COUNT, true> (planes.hpp), an arm of the fifth body of count_kernel",
          "merge_delta": "planes_merge_run<E, true> (planes.hpp), an arm of pass 4 of unpack_records_kernel"}
RULES = (("split_delta", "split"), ("counted_split_delta", "counted_split"), ("merge_delta", "merge"))


def fill(eng, d_in, n_bytes, e, content):
    if content == "uniform":
        eng.fill_splitmix64(d_in, n_bytes, 43)
        return
    chunk = (np.arange(CHUNK_VALUES, dtype=np.uint64) * np.uint64(3) + np.uint64(1000)).astype(pd.DTYPE[e]).view(np.uint8)
    for at in range(0, n_bytes, chunk.size):
        eng.upload(d_in, chunk[:min(chunk.size, n_bytes - at)], offset=at)


def table_rates(lib, eng, hip, n_bytes, args, step):
    out, ok = {}, True
    d_in, d_planes, d_out, d_counts = eng.alloc(n_bytes), eng.alloc(n_bytes), eng.alloc(n_bytes), eng.alloc(256 * 8 * 8)
    stream = C.c_void_p(eng.stream)
    timed = lambda fn: timed_events(eng, fn, args.launches, args.warmup)
    for e in (2, 4, 8):
        n = n_bytes // e
        for content in ("uniform", "ramp"):
            step("E %d, %s: plain" % (e, content))
            fill(eng, d_in, n_bytes, e, content)
            eng.fill(d_counts, 0, 256 * 8 * 8)
            plain = {"memcpy": timed(lambda: hip.call("hipMemcpyAsync", d_out, d_in, n_bytes, 3, stream)),
                     "split": timed(lambda: pl.split(eng, d_in, n, e, d_planes, n, None, stream)),
                     "counted_split": timed(lambda: pl.split(eng, d_in, n, e, d_planes, n, d_counts, stream)),
                     "merge": timed(lambda: pl.merge(eng, d_planes, n, n, e, d_out, stream))}
            for r in (16, 1024, 2048):
                label = "E %d, R %d, %s" % (e, r, content)
                step(label)
                row = dict(plain)
                row["split_delta"] = timed(lambda: pd.split_delta(eng, d_in, n, e, r, d_planes, n, None, stream))
                row["counted_split_delta"] = timed(lambda: pd.split_delta(eng, d_in, n, e, r, d_planes, n, d_counts, stream))
                row["merge_delta"] = timed(lambda: pd.merge_delta(eng, d_planes, n, n, e, r, d_out, stream))
                row["passes"] = True
                for mine, theirs in RULES:
                    row["%s_over_%s" % (mine, theirs)] = round(row[mine]["median_ms"] / row[theirs]["median_ms"], 3)
                    row["%s_plus_memcpy_ms" % theirs] = round(row[theirs]["median_ms"] + row["memcpy"]["median_ms"], 4)
                    row["passes"] = row["passes"] and row[mine]["median_ms"] < row["%s_plus_memcpy_ms" % theirs]
                ok = ok and row["passes"]
                # the same launches, checked on samples: the merge of the split is the input, the counts sum to the elements
                eng.fill(d_counts, 0, 256 * 8 * 8)
                assert pd.split_delta(eng, d_in, n, e, r, d_planes, n, d_counts, stream) == (0, 0)
                assert pd.merge_delta(eng, d_planes, n, n, e, r, d_out, stream) == (0, 0)
                eng.sync()
                for at in (0, n_bytes // 2 + 4096, n_bytes - (1 << 20)):
                    assert np.array_equal(eng.download(d_in, 1 << 20, offset=at), eng.download(d_out, 1 << 20, offset=at)), label
                counts = eng.download(d_counts, 256 * 8 * e).view(np.uint64).reshape(e, 256)
                assert np.all(counts.sum(axis=1) == n), label
                print(label, json.dumps(row), flush=True)
                out[label] = row
    for d in (d_in, d_planes, d_out, d_counts):
        eng.free(d)
    return {"rows": out,
            "rule": "split_delta < split + memcpy, counted_split_delta < counted_split + memcpy, merge_delta < merge + memcpy "
                    "on every row (written before the run)",
            "passes_on_every_row": ok, "rows_that_miss": [k for k, v in out.items() if not v["passes"]]}


def merge(path, out_path, gates, headline):
    rates = json.load(open(path))
    doc = {k: rates[k] for k in ("bytes", "launches", "warmup", "tool")}
    doc["bodies"] = BODIES
    doc["rates"] = rates["rates"]
    if gates:
        doc["plain_roads_against_the_parent"] = {name: json.load(open(p)) for name, p in (g.split("=", 1) for g in gates)}
    if headline:
        doc["headline"] = headline
    text = json.dumps(doc, indent=1)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=DEFAULT_OUT)
    ap.add_argument("--table", choices=("rates",))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--shrink", type=int, default=1, help="every size divided by this (a rehearsal)")
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--merge", metavar="RATES")
    ap.add_argument("--gates", nargs="*", default=[], help="name=compared.json: documents of --compare, recorded by --merge")
    ap.add_argument("--headline", default=None)
    ap.add_argument("--compare", nargs=3, metavar=("THIS", "PARENT_FIRST", "PARENT_SECOND"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare, args.out))
    if args.merge:
        sys.exit(merge(args.merge, args.out, args.gates, args.headline))
    assert args.table, "one process a table: --table rates"
    assert args.warmup >= 15 or args.shrink > 1, "the clocks settle over about 13 launches"
    lib = pd.bind(harness.load_product(args.lib))
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: nothing is measured without one"
    patterns, lens = harness.load_table()
    coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    eng = harness.Engine(lib, coder)
    hip = fa.Hip()
    hip.hip.hipMemcpyAsync.restype = C.c_int
    hip.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    n_bytes = GiB // args.shrink
    step = Steps(args.step_seconds)
    out = {"bytes": n_bytes, "launches": args.launches, "warmup": args.warmup,
           "tool": "profiles/tools/planes_delta_rate.py (one MI355X, one process a table, device events)"}
    out[args.table] = table_rates(lib, eng, hip, n_bytes, args, step)
    step.done()
    eng.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out != "-":
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
