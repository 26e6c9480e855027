#!/usr/bin/env python3
"""What the byte planes of multi-byte elements (aws_huffman_amd_planes_split / _merge, huffman_amd_planes.h) cost on 1 GiB
resident in device memory.  Prints one JSON document and writes it to the path given (by default
profiles/planes_mi355x.json; with --table the table alone, to be put together with --merge).

Device events, medians of `--launches` launches behind `--warmup` launches that are thrown away, one process a table.  Every
step runs under an alarm of `--step-seconds` whose default action ends the process: the script ends at the first failure.

  --table rates : element sizes 2, 4 and 8; uniform bytes, N(0, 1) in that element type (bf16 for 2 bytes; 16 Mi values,
                  repeated) and one repeated element (the worst case of the histograms' fewer copies).  Per row:
                    memcpy         hipMemcpyAsync device to device of the same bytes: one read and one write a byte, the floor
                    split, merge   the two calls without counts, and their ratio to memcpy
                    counted_split  the split with the counts of every plane
                    count_planes   aws_huffman_amd_symbol_counts over the planes' bytes
                  THE RULE, written before the run: counted_split < split + count_planes on every row -- the composition it
                  replaces, taken in the same process.  A row that fails says the fusion does not earn its place for that
                  element size.
  --table chain : f32 of N(0, 1), 1 GiB: clear, counted split, four fits and four packed stored launches (items of 4 KiB) on
                  one stream -- the time, and the packed bytes as a share of the GiB -- beside a fit and ONE packed stored
                  launch over the interleaved bytes.  Reported, not gated.

  --compare     : the roads that share a host kernel with the new bodies.  THIS, PARENT_FIRST and PARENT_SECOND are documents
                  of one of the other rate tools (plan_counts_rate.py, stored_rate.py, packed_rate.py, packed_indexed_rate.py,
                  packed_decode_rate.py), made in that order on one box, one process each, the parent's with --lib <the parent
                  commit's build>.  Every median both builds have is a row; a row passes where this build's is at most the
                  slower parent run plus 3 % plus 0.01 ms.
  --merge       : the two tables, and with --gates name=compared.json ... the compared roads, as one document.

usage: planes_rate.py [out.json] --table rates|chain [--launches N] [--warmup N] [--shrink N] [--lib path]
       planes_rate.py out.json --compare THIS PARENT_FIRST PARENT_SECOND
       planes_rate.py [out.json] --merge rates.json chain.json [--gates name=compared.json ...]"""
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
import packed_api as pa  # noqa: E402
import planes_api as pl  # noqa: E402
import stored_api as sa  # noqa: E402
from block_index_rate import Steps, timed_events  # noqa: E402

GiB = 1 << 30
DEFAULT_OUT = os.path.join(REPO, "profiles", "planes_mi355x.json")
CHUNK_VALUES = 1 << 24
ITEM = 4096
BODIES = {"split": "planes_split (planes.hpp), the fifth body of count_kernel (count_kernels.hip)",
          "merge": "planes_merge (planes.hpp), a body of unpack_records_kernel (pack_kernels.hip)"}


def normal_chunk(e, seed=7):
    """CHUNK_VALUES samples of N(0, 1) as elements of e bytes: bf16 (the top 16 bits of the f32), f32, f64."""
    x = np.random.default_rng(seed).standard_normal(CHUNK_VALUES)
    if e == 2:
        return (x.astype("<f4").view("<u4") >> 16).astype("<u2").view(np.uint8)
    return x.astype("<f4" if e == 4 else "<f8").view(np.uint8)


def fill(eng, d_in, n_bytes, e, content):
    if content == "uniform":
        eng.fill_splitmix64(d_in, n_bytes, 41)
        return
    chunk = normal_chunk(e) if content == "normal" else np.tile(np.arange(0x31, 0x31 + e, dtype=np.uint8), CHUNK_VALUES)
    for at in range(0, n_bytes, chunk.size):
        eng.upload(d_in, chunk[:min(chunk.size, n_bytes - at)], offset=at)


def ratio(row, a, b):
    row["%s_over_%s" % (a, b)] = round(row[a]["median_ms"] / row[b]["median_ms"], 3)


def table_rates(lib, eng, hip, n_bytes, args, step):
    out, ok = {}, True
    d_in, d_planes, d_out, d_counts = eng.alloc(n_bytes), eng.alloc(n_bytes), eng.alloc(n_bytes), eng.alloc(256 * 8 * 8)
    stream = C.c_void_p(eng.stream)
    timed = lambda fn: timed_events(eng, fn, args.launches, args.warmup)
    for e in (2, 4, 8):
        n = n_bytes // e
        for content in ("uniform", "normal", "one element"):
            label = "E %d, %s" % (e, content)
            step(label)
            fill(eng, d_in, n_bytes, e, content)
            eng.fill(d_counts, 0, 256 * 8 * 8)
            row = {"memcpy": timed(lambda: hip.call("hipMemcpyAsync", d_out, d_in, n_bytes, 3, stream)),
                   "split": timed(lambda: pl.split(eng, d_in, n, e, d_planes, n, None, stream)),
                   "merge": timed(lambda: pl.merge(eng, d_planes, n, n, e, d_out, stream)),
                   "counted_split": timed(lambda: pl.split(eng, d_in, n, e, d_planes, n, d_counts, stream)),
                   "count_planes": timed(lambda: lib.aws_huffman_amd_symbol_counts(-1, d_planes, n_bytes, d_counts, stream))}
            for k in ("split", "merge", "counted_split"):
                ratio(row, k, "memcpy")
            row["split_plus_count_planes_ms"] = round(row["split"]["median_ms"] + row["count_planes"]["median_ms"], 4)
            row["fusion_passes"] = row["counted_split"]["median_ms"] < row["split_plus_count_planes_ms"]
            ok = ok and row["fusion_passes"]
            # the same launches, checked on a sample: the merge of the split is the input, the counts sum to the bytes
            eng.fill(d_counts, 0, 256 * 8 * 8)
            assert pl.split(eng, d_in, n, e, d_planes, n, d_counts, stream) == (0, 0)
            assert pl.merge(eng, d_planes, n, n, e, d_out, stream) == (0, 0)
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
            "rule": "counted_split < split + count_planes on every row (written before the run); memcpy is the floor of split and merge",
            "fusion_passes_on_every_row": ok}


def table_chain(lib, eng, hip, n_bytes, args, step):
    e, n = 4, n_bytes // 4
    items = n // ITEM
    d_in, d_planes, d_counts = eng.alloc(n_bytes), eng.alloc(n_bytes), eng.alloc(256 * 8 * e)
    stream = C.c_void_p(eng.stream)
    step("chain: data")
    fill(eng, d_in, n_bytes, e, "normal")
    step("chain: plans")
    planes = []
    for p in range(e):
        fe = fa.FittedEngine(lib, 4, 12)
        plan = fe.plan_strided(True, count=items, in_offset=0, in_stride=ITEM, in_len=ITEM, out_offset=0, out_stride=0,
                               out_capacity=0, first_bit=0, eos_padding=0xFF)
        planes.append((fe, plan, sa.Buffers(fe, items, n, d_planes + p * n)))

    def chain():
        hip.memset_async(d_counts, 0, 256 * 8 * e, stream)
        assert pl.split(eng, d_in, n, e, d_planes, n, d_counts, stream) == (0, 0)
        for p, (fe, plan, bufs) in enumerate(planes):
            assert fe.fit_counts_async(d_counts + 256 * 8 * p, stream) == (0, 0)
            assert sa.launch_stored(fe, plan, bufs.d_in, bufs.d_out, n, bufs.d_off, bufs.d_flags, 1, stream) == (0, 0)

    step("chain: by planes")
    row = {"by_planes": timed_events(eng, chain, args.launches, args.warmup)}
    eng.sync()
    sizes = [pa.packed_size(fe, plan)[2] for fe, plan, _ in planes]
    stored = [sa.stored_size(fe, plan)[2] for fe, plan, _ in planes]
    row["by_planes"].update({"packed_bytes_of_each_plane": sizes, "stored_items_of_each_plane": stored, "items_a_plane": items,
                             "packed_share_of_the_input": round(sum(sizes) / n_bytes, 4)})
    for fe, plan, bufs in planes:
        bufs.close()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        fe.close()
    eng.free(d_planes)
    step("chain: interleaved")
    fe = fa.FittedEngine(lib, 4, 12)
    all_items = n_bytes // ITEM
    plan = fe.plan_strided(True, count=all_items, in_offset=0, in_stride=ITEM, in_len=ITEM, out_offset=0, out_stride=0,
                           out_capacity=0, first_bit=0, eos_padding=0xFF)
    bufs = sa.Buffers(fe, all_items, n_bytes, d_in)

    def interleaved():
        hip.memset_async(d_counts, 0, 256 * 8, stream)
        assert lib.aws_huffman_amd_symbol_counts(-1, d_in, n_bytes, d_counts, stream) == 0
        assert fe.fit_counts_async(d_counts, stream) == (0, 0)
        assert sa.launch_stored(fe, plan, d_in, bufs.d_out, n_bytes, bufs.d_off, bufs.d_flags, 1, stream) == (0, 0)

    row["interleaved"] = timed_events(eng, interleaved, args.launches, args.warmup)
    eng.sync()
    row["interleaved"].update({"packed_share_of_the_input": round(pa.packed_size(fe, plan)[2] / n_bytes, 4),
                               "stored_items": sa.stored_size(fe, plan)[2], "items": all_items})
    bufs.close()
    lib.aws_huffman_amd_encode_plan_destroy(plan)
    fe.close()
    for d in (d_in, d_counts):
        eng.free(d)
    row["note"] = ("f32 of N(0, 1), items of 4 KiB; by_planes: clear, counted split, four fits, four packed stored launches; "
                   "interleaved: clear, count, fit, one packed stored launch over the same bytes.  Reported, not gated")
    print("chain", json.dumps(row), flush=True)
    return row


def medians(doc, prefix=""):
    """{path: median_ms} of every timed entry of a rate tool's document."""
    out = {}
    for k, v in doc.items():
        if isinstance(v, dict):
            if "median_ms" in v:
                out[prefix + k] = v["median_ms"]
            else:
                out.update(medians(v, prefix + k + "."))
    return out


def compare(paths, out_path):
    mine, first, second = (medians(json.load(open(p))) for p in paths)
    rows, ok = {}, True
    for k in sorted(mine):
        if k in first and k in second:
            allowed = round(max(first[k], second[k]) * 1.03 + 0.01, 4)
            rows[k] = {"parent_first_ms": first[k], "this_ms": mine[k], "parent_second_ms": second[k], "allowed_ms": allowed,
                       "passes": mine[k] <= allowed}
            ok = ok and rows[k]["passes"]
    doc = {"rule": "each row inside the slower parent run plus 3 % plus 0.01 ms", "rows": rows, "passes": ok}
    print(json.dumps({k: v for k, v in rows.items() if not v["passes"]}, indent=1), "passes" if ok else "FAILS", len(rows), "rows")
    with open(out_path, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    return 0 if ok else 1


def merge(paths, out_path, gates):
    rates, chain = (json.load(open(p)) for p in paths)
    doc = {k: rates[k] for k in ("bytes", "launches", "warmup", "tool")}
    doc["bodies"] = BODIES
    doc["rates"] = rates["rates"]
    doc["chain"] = chain["chain"]
    if gates:
        doc["roads_that_share_a_host_kernel"] = {name: json.load(open(path)) for name, path in (g.split("=", 1) for g in gates)}
    text = json.dumps(doc, indent=1)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=DEFAULT_OUT)
    ap.add_argument("--table", choices=("rates", "chain"))
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--shrink", type=int, default=1, help="every size divided by this (a rehearsal)")
    ap.add_argument("--step-seconds", type=int, default=240)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--merge", nargs=2, metavar=("RATES", "CHAIN"))
    ap.add_argument("--gates", nargs="*", default=[], help="name=compared.json: documents of --compare, recorded by --merge")
    ap.add_argument("--compare", nargs=3, metavar=("THIS", "PARENT_FIRST", "PARENT_SECOND"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare, args.out))
    if args.merge:
        sys.exit(merge(args.merge, args.out, args.gates))
    assert args.table, "one process a table: --table rates or --table chain"
    assert args.warmup >= 15 or args.shrink > 1, "the clocks settle over about 13 launches"
    lib = pl.bind(harness.load_product(args.lib))
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
           "tool": "profiles/tools/planes_rate.py (one MI355X, one process a table, device events)"}
    out[args.table] = (table_rates if args.table == "rates" else table_chain)(lib, eng, hip, n_bytes, args, step)
    step.done()
    eng.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out != "-":
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
