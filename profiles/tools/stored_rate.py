#!/usr/bin/env python3
"""What a packed launch that stores items raw (aws_huffman_amd_encode_plan_launch_packed_stored, huffman_amd_stored.h) costs
under the test coder, next to a plain packed launch of the same batch and to a device-to-device copy of the same bytes.
Prints one JSON document (and writes it to the path given, by default profiles/stored_mi355x.json).

One process, device events, medians of `--launches` launches behind `--warmup` launches that are thrown away.  Every step
runs under an alarm of `--step-seconds` whose default action ends the process: the script ends at the first failure.

  shapes   : 1 GiB as ONE item, 65 536 items of 16 KiB, 1 Mi items of 16 .. 80 bytes
  contents : nothing stored (lowercase text), everything stored (uniform bytes), every second item stored (the one-item
             shape has no second item: left out)
  rows     : packed (aws_huffman_amd_encode_plan_launch_packed), stored, the output sizes of both, the stored counts, and for
             the everything-stored batches hipMemcpyAsync device to device of as many bytes
  --packed-only --lib parent.so : the packed rows alone, from the parent commit's build on the same box, in turn:

      stored_rate.py parent_first.json --packed-only --lib parent.so
      stored_rate.py this.json
      stored_rate.py parent_second.json --packed-only --lib parent.so
      stored_rate.py --merge this.json parent_first.json parent_second.json

  --merge : the stored launch with nothing stored passes where its median is at most the slower parent packed run plus 3 %
            plus 0.01 ms
  --once SHAPE : (behind --once-warm N such pairs) ONE stored launch of the everything-stored batch of that shape (--content: of another) and one hipMemcpyAsync
            of as many bytes, for rocprofv3 --kernel-trace --stats (the copy alone is the launch's LAST dispatch of unpack_records_kernel,
            which hosts it, in the kernel trace)

usage: stored_rate.py [out.json] [--launches N] [--warmup N] [--shrink N] [--lib path] [--packed-only] [--once SHAPE]"""
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
import packed_api as pa  # noqa: E402
from block_index_rate import Steps, timed_events  # noqa: E402

GiB = 1 << 30
DEFAULT_OUT = os.path.join(REPO, "profiles", "stored_mi355x.json")
SHAPES = ("one_item", "items_of_16_KiB", "items_of_16_to_80_bytes")
CONTENTS = ("nothing_stored", "everything_stored", "every_second_stored")
ALPHABET = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ", dtype=np.uint8)


def shapes(n, shrink):
    many = 65_536 // shrink
    size = n // many
    small = np.random.default_rng(11).integers(16, 81, (1 << 20) // shrink).astype(np.int64)
    return {"one_item": (np.asarray([0]), np.asarray([n])),
            "items_of_16_KiB": (np.arange(many, dtype=np.int64) * size, np.full(many, size, np.int64)),
            "items_of_16_to_80_bytes": (np.concatenate([[0], np.cumsum(small)])[:-1], small)}


def content(kind, n, lengths):
    """n bytes: lowercase text, uniform bytes, or the two in turn by item."""
    rng = np.random.default_rng(7)
    text = lambda: ALPHABET[rng.integers(0, ALPHABET.size, n, dtype=np.uint8)]
    if kind == "nothing_stored":
        return text()
    if kind == "everything_stored":
        return rng.integers(0, 256, n, dtype=np.uint8)
    uniform = np.repeat(np.arange(len(lengths)) % 2 == 1, lengths)
    host = text()
    host[:uniform.size][uniform] = rng.integers(0, 256, int(uniform.sum()), dtype=np.uint8)
    return host


def hip_runtime():
    hip = pa.HipGraphs().hip
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return hip


def measure(lib, eng, n, args, step, sa):
    hip = hip_runtime()
    d_in = eng.alloc(n + 64)
    room = n + n // 2 + 4096
    d_out = eng.alloc(room)
    out = {}
    for label, (offsets, lengths) in shapes(n, args.shrink).items():
        if args.once and label != args.once:
            continue
        count, span = len(lengths), int(offsets[-1] + lengths[-1])
        d_off, d_flags = eng.alloc(8 * (count + 1)), eng.alloc(count + 8)
        plan, d_items = pa.plan_from_records(eng, offsets, lengths)
        out[label] = {}
        for kind in CONTENTS:
            if (kind == "every_second_stored" and count == 1) or (args.once and kind != args.content):
                continue
            step("%s, %s: upload" % (label, kind))
            eng.upload(d_in, content(kind, span, lengths))
            row = {"items": count, "bytes": span}
            packed = lambda: pa.launch_packed(eng, plan, d_in, d_out, room, d_off, 1, eng.stream)
            stored = lambda: sa.launch_stored(eng, plan, d_in, d_out, room, d_off, d_flags, 1, eng.stream)
            copy = lambda: hip.hipMemcpyAsync(d_out, d_in, span, 3, eng.stream)  # (hipMemcpyDeviceToDevice)
            if args.once:
                for _ in range(args.once_warm):  # (the trace's LAST dispatches are the ones to read)
                    assert stored() == (0, 0) and copy() == 0
                assert stored() == (0, 0) and copy() == 0
                eng.sync()
                row["stored_size"] = sa.stored_size(eng, plan)[2:]
                out[label][kind] = row
                continue
            step("%s, %s: packed" % (label, kind))
            assert packed() == (0, 0)
            row["packed_output_bytes"] = pa.packed_size(eng, plan)[2]
            row["packed"] = timed_events(eng, packed, args.launches, args.warmup)
            if not args.packed_only:
                step("%s, %s: stored" % (label, kind))
                assert stored() == (0, 0)
                row["stored_output_bytes"] = pa.packed_size(eng, plan)[2]
                row["stored_items"], row["stored_bytes"] = sa.stored_size(eng, plan)[2:]
                row["stored"] = timed_events(eng, stored, args.launches, args.warmup)
                row["stored_over_packed"] = round(row["stored"]["median_ms"] / row["packed"]["median_ms"], 3)
                if kind == "everything_stored":
                    assert row["stored_items"] == count and row["stored_output_bytes"] == span, row
                    row["memcpy_d2d"] = timed_events(eng, copy, args.launches, args.warmup)
                if kind == "nothing_stored":
                    # (a text item whose code comes to exactly its length is stored: a tie changes no size)
                    assert row["stored_items"] * 1000 <= count and row["stored_output_bytes"] == row["packed_output_bytes"], row
            print(label, kind, json.dumps(row), flush=True)
            out[label][kind] = row
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        for p in (d_items, d_off, d_flags):
            eng.free(p)
    eng.free(d_in)
    eng.free(d_out)
    return out


def merge(paths, out_path):
    this, first, second = (json.load(open(p)) for p in paths)
    rows, ok = {}, True
    for shape in SHAPES:
        a, b = (d["rows"][shape]["nothing_stored"]["packed"]["median_ms"] for d in (first, second))
        mine = this["rows"][shape]["nothing_stored"]["stored"]["median_ms"]
        allowed = max(a, b) * 1.03 + 0.01
        passed = mine <= allowed
        ok = ok and passed
        rows[shape] = {"parent_packed_first_ms": a, "this_stored_ms": mine, "parent_packed_second_ms": b,
                       "allowed_ms": round(allowed, 4), "passes": passed}
        for kind in CONTENTS:
            if kind in this["rows"][shape]:
                this["rows"][shape][kind]["parent_packed_ms"] = [d["rows"][shape][kind]["packed"]["median_ms"] for d in (first, second)]
    this["nothing_stored_against_parent_packed"] = {
        "rule": "the stored launch of a batch in which nothing is stored against the parent commit's packed launch of the same "
                "batch, two runs of the parent's build on one box around this one: at most the slower plus 3 % plus 0.01 ms",
        "rows": rows, "passes": ok}
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
    ap.add_argument("--packed-only", action="store_true")
    ap.add_argument("--once", choices=SHAPES, default=None)
    ap.add_argument("--once-warm", type=int, default=0, help="launches in front of the --once launch, so that the clocks have settled")
    ap.add_argument("--content", choices=CONTENTS, default="everything_stored", help="of the --once launch")
    ap.add_argument("--merge", nargs=3, metavar=("THIS", "PARENT_FIRST", "PARENT_SECOND"))
    args = ap.parse_args()
    if args.merge:
        sys.exit(merge(args.merge, args.out))
    assert args.warmup >= 15 or args.shrink > 1 or args.once, "the clocks settle over about 13 launches"
    lib = harness.load_product(args.lib)
    sa = None
    if args.packed_only:
        pa.bind(lib)
    else:
        import stored_api as sa
        sa.bind(lib)
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: nothing is measured without one"
    patterns, lens = harness.load_table()
    eng = harness.Engine(lib, lib.aws_huffman_amd_table_coder_new(patterns, lens))
    n = GiB // args.shrink
    step = Steps(args.step_seconds)
    out = {"bytes": n, "launches": args.launches, "warmup": args.warmup, "library": args.lib or "the tree's own",
           "tool": "profiles/tools/stored_rate.py (one MI355X, one process, device events)",
           "rows": measure(lib, eng, n, args, step, sa)}
    step.done()
    eng.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out != "-" and not args.once:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
