#!/usr/bin/env python3
"""ONE packed decode launch of the 1 GiB stream as one item, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/tools/packed_decode_once.py
The stream is encoded by a plain launch, the decode plan is made from the offsets [0, encoded length] in device memory
(aws_huffman_amd_decode_plan_reset_packed_input), and the packed launch decodes into room for the worst case.  The trace's
kernel statistics show every dec_sync* kernel once: the encoded bytes are walked once, the offsets are made between the
scan and the emit stage.  Prints what the launch reported.  --shrink N: a stream N times shorter."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, "tests"))
import harness  # noqa: E402
import packed_api as pa  # noqa: E402
import packed_decode_api as pd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shrink", type=int, default=1)
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    lib = pd.bind(harness.load_product(args.lib))
    patterns, lens = harness.load_table()
    min_bits = min(int(l) for l in lens if l)
    eng = harness.Engine(lib, lib.aws_huffman_amd_table_coder_new(patterns, lens))
    n = (1 << 30) // args.shrink
    d_in, d_enc = eng.alloc(n), eng.alloc(2 * n + 64)
    eng.fill_splitmix64(d_in, n, 5)
    eplan = eng.encode_plan([dict(in_offset=0, in_len=n, out_offset=0, out_capacity=2 * n + 64)])
    eng.encode_launch(eplan, d_in, d_enc)
    rc, err, consumed, e = eng.encode_results(eplan, 1)[0][:4]
    assert (rc, err, consumed) == (0, 0, n)
    room = e * 8 // min_bits + 8
    d_out, d_off, d_enc_off = eng.alloc(room), eng.alloc(16), pd.upload_u64(eng, [0, e])
    plan = eng.empty_decode_plan()
    assert pd.reset_packed_input(eng, plan, d_enc_off, None, 1) == (0, 0)
    assert pd.launch_packed(eng, plan, d_enc, d_out, room, d_off, 1) == (0, 0)
    rc, err, total, longest = pd.packed_size(eng, plan)
    assert (rc, err) == (0, 0) and total >= n
    print(json.dumps({"symbols_in": n, "encoded_bytes": e, "offsets": [int(x) for x in pa.download_u64(eng, d_off, 2)],
                      "total_symbols": total, "record": eng.decode_results(plan, 1)[0]}))
    eng.close()


if __name__ == "__main__":
    main()
