"""ctypes face of include/aws/compression/huffman_amd_stored_index.h (indexed packed batches with items stored raw: the
sender's one launch, the receiver's ranges and locate with the sender's flags) and what its tests share.  Used by
tests/test_emulated_stored_index.py (emulator build) and tests/test_gpu_stored_index.py (MI355X): every run_* scenario below
is called by both, at the same sizes.

Every expectation comes from the oracle, numpy and the definition helpers of the headers in front: stored_api.Sent (flags,
lengths, offsets, output and records of a stored launch), batch_index_api.expected (directory and index),
packed_api.expected_offsets, ranges_api.symbol_bits.  The bytes of a stored range are the blob's.  Nothing here asks the
library what it should have done."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import batch_index_api as bi
import build_api as ba
import fit_api as fa
import harness
import index_api as ia
import packed_api as pa
import packed_decode_api as pda
import packed_index_api as pi
import parity_cases as pc
import plan_counts_api as pk
import ranges_api as ra
import stored_api as sa

INDEX_OK, INDEX_TOO_SMALL = bi.INDEX_OK, bi.INDEX_TOO_SMALL
INVALID, UNSUPPORTED, STATE = bi.INVALID, bi.UNSUPPORTED, bi.STATE
EE, MARKER, FLAG_GUARD = bi.EE, pa.MARKER, sa.FLAG_GUARD
SEG = pa.SEG
HEADER = os.path.join(harness.REPO, "include", "aws", "compression", "huffman_amd_stored_index.h")
NAMES = ["aws_huffman_amd_encode_plan_launch_packed_stored_indexed", "aws_huffman_amd_decode_plan_reset_stored_item_block_ranges",
         "aws_huffman_amd_decode_plan_reset_stored_item_symbol_ranges", "aws_huffman_amd_locate_stored_item_symbols"]


def bind(lib):
    """Declares the four entry points of huffman_amd_stored_index.h (and those of the headers in front of it) on a loaded
    library.  The symbols are looked up here: on a build without them every test fails."""
    sa.bind(lib)
    pi.bind(lib)
    V, U, S = C.c_void_p, C.c_uint64, C.c_size_t
    lib.aws_huffman_amd_encode_plan_launch_packed_stored_indexed.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_launch_packed_stored_indexed.argtypes = [V, V, V, U, V, V, C.c_uint32, U, V, V, U, V, V]
    lib.aws_huffman_amd_decode_plan_reset_stored_item_block_ranges.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_reset_stored_item_block_ranges.argtypes = [V, V, V, U, U, U, V, V, V, U, U, V, S, V]
    lib.aws_huffman_amd_decode_plan_reset_stored_item_symbol_ranges.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_reset_stored_item_symbol_ranges.argtypes = [V, V, V, V, U, U, U, V, V, V, U, U, V, S, V]
    lib.aws_huffman_amd_locate_stored_item_symbols.restype = C.c_int
    lib.aws_huffman_amd_locate_stored_item_symbols.argtypes = [V, V, U, V, V, U, U, U, V, V, V, V, V, S, V, V, V]
    return lib


def launch(eng, plan, d_in, d_out, capacity, d_off, d_flags, align, B, d_dir, d_index, index_capacity, d_status, stream=None):
    """(rc, error) of the enqueue."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_encode_plan_launch_packed_stored_indexed(
        plan, d_in, d_out, int(capacity), d_off, d_flags, int(align), int(B), d_dir, d_index, int(index_capacity), d_status, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


# ----------------------------------------------------------------------------- what the one call must leave
def check_too_small(eng, plan, sent, bufs, label=""):
    """What is in `bufs` behind a call whose index did not fit: every offset 0, every flag 0, no output byte, every record
    the oracle's for no room, both sizes nothing."""
    n = len(sent.blobs)
    assert not pa.download_u64(eng, bufs.d_off, n + 1).any(), label
    flags = eng.download(bufs.d_flags, n + 8)
    assert not flags[:n].any() and np.all(flags[n:] == FLAG_GUARD), label
    assert np.all(eng.download(bufs.d_out, bufs.size) == MARKER), label
    res = eng.encode_results(plan, n)
    for i, blob in enumerate(sent.blobs):
        rec, _ = pa.oracle_item(sent.oracle, sent.ocoder, blob, sent.overflows[i], sent.eoss[i], 0)
        assert res[i] == rec, (label, i, res[i], rec)
    assert pa.packed_size(eng, plan) == (0, 0, 0, 0), label
    assert sa.stored_size(eng, plan) == (0, 0, 0, 0), label


def check_call(sc, eng, plan, d_in, sent, code_lens, B, cap=None, index_capacity=None, slack=0, label="", stream=None):
    """One call of `plan` against both definitions: the stored launch's (stored_api.check_sent: offsets, flags, every output
    byte, every record, both sizes) and the index call's (directory, index, status, guard words, the size).  cap None:
    exactly the total.  An index_capacity that is too small expects the header's answer.  Returns the index as expected."""
    n = len(sent.blobs)
    want_dir, want_index = bi.expected(code_lens, sent.blobs, B)
    bi.pin_to_oracle(sent.oracle, sent.ocoder, sent.blobs, want_dir, want_index)
    entries = want_index.size
    icap = entries + slack if index_capacity is None else int(index_capacity)
    fits = icap >= entries
    cap = sent.total if cap is None else int(cap)
    bufs = sa.Buffers(eng, n, max(sent.total, cap) + 64, d_in)
    a = bi.Arrays(eng, n, icap)
    try:
        bufs.refill()
        assert launch(eng, plan, d_in, bufs.d_out, cap, bufs.d_off, bufs.d_flags, sent.align, B, a.d_dir, a.d_index, icap, a.d_status,
                      stream) == (0, 0), label
        if fits:
            sa.check_sent(eng, plan, sent, bufs, cap, label, launch=False)
        else:
            check_too_small(eng, plan, sent, bufs, label)
        pi.check_arrays(a, want_dir, want_index, INDEX_OK if fits else INDEX_TOO_SMALL, label)
        assert bi.index_size(eng, plan) == (0, 0, entries), label
    finally:
        a.close()
        bufs.close()
    return want_dir, want_index


def run_calls(sc, eng, plan, d_in, blobs, overflows, eoss, aligns, blocks=(64, 512), caps_of=None, label="", code_lens=None,
              ocoder=None):
    """The call at every alignment and block size, at exactly the total and at every capacity caps_of(sent) names."""
    code_lens = sc.lens if code_lens is None else code_lens
    sents = []
    for align in aligns:
        sent = sa.Sent(sc.oracle, ocoder or sc.w.ocoder, blobs, code_lens, overflows, eoss, align)
        for B in blocks:
            for cap in [sent.total] + (caps_of(sent) if caps_of else []):
                check_call(sc, eng, plan, d_in, sent, code_lens, B, cap=cap, label="%s, align %d, B %d, capacity %d" % (label, align, B, cap))
        sents.append(sent)
    return sents


def two_calls_leave(eng, plan, d_in, n, size, cap, align, B, icap):
    """What aws_huffman_amd_encode_plan_block_index then aws_huffman_amd_encode_plan_launch_packed_stored leave."""
    bufs, a = sa.Buffers(eng, n, size, d_in), bi.Arrays(eng, n, icap)
    try:
        bufs.refill()
        assert bi.plan_block_index(eng, plan, d_in, B, a.d_dir, a.d_index, icap, a.d_status) == (0, 0)
        assert sa.launch_stored(eng, plan, d_in, bufs.d_out, cap, bufs.d_off, bufs.d_flags, align) == (0, 0)
        return snapshot(eng, plan, bufs, a, n)
    finally:
        a.close()
        bufs.close()


def one_call_leaves(eng, plan, d_in, n, size, cap, align, B, icap):
    bufs, a = sa.Buffers(eng, n, size, d_in), bi.Arrays(eng, n, icap)
    try:
        bufs.refill()
        assert launch(eng, plan, d_in, bufs.d_out, cap, bufs.d_off, bufs.d_flags, align, B, a.d_dir, a.d_index, icap, a.d_status) == (0, 0)
        return snapshot(eng, plan, bufs, a, n)
    finally:
        a.close()
        bufs.close()


def snapshot(eng, plan, bufs, a, n):
    eng.sync()
    d, x, status = a.read()
    return (eng.download(bufs.d_out, bufs.size), pa.download_u64(eng, bufs.d_off, n + 1), eng.download(bufs.d_flags, n + 8), d, x,
            status, eng.encode_results(plan, n), pa.packed_size(eng, plan), sa.stored_size(eng, plan), bi.index_size(eng, plan))


def same(mine, theirs, label=""):
    for k, (x, y) in enumerate(zip(mine, theirs)):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (label, k)


# ----------------------------------------------------------------------------- 1: composition
def mixed_plan(sc, fill, rng):
    """(plan, d_items, d_in, blobs, overflows, eoss, close) of stored_api.run_mixed's batch for this fill."""
    eng = sc.eng
    if fill == "strided":
        in_len, stride, count = 2 * SEG + 77, 2 * SEG + 200, 9
        blobs = [sa.words(rng, in_len) if i % 2 else pc.inputs(rng, in_len, "uniform") for i in range(count)]
        host = pc.inputs(rng, 3 + count * stride + 64, "uniform")
        for i, b in enumerate(blobs):
            host[3 + i * stride:3 + i * stride + in_len] = b
        d_in = eng.alloc(host.size)
        eng.upload(d_in, host)
        make = lambda: (eng.plan_strided(True, count=count, in_offset=3, in_stride=stride, in_len=in_len, out_offset=0, out_stride=0,
                                         out_capacity=0, first_bit=0, eos_padding=0xFF), None)
        return make, d_in, blobs, [(0, 0)] * count, [0xFF] * count, lambda: eng.free(d_in)
    blobs = sa.mixed_blobs(rng)
    b = pa.Batch(eng, blobs, rng)
    make = (lambda: (eng.encode_plan(b.items), None)) if fill == "host" else (lambda: eng.encode_plan_from_device_items(b.items))
    return make, b.d_in, blobs, b.overflows, b.eoss, b.close


def run_mixed(sc, fill):
    """Lowercase words and uniform bytes at every edge length, under the test coder: host, strided or device items; block
    sizes 64 and 512, align 1 and 16, against the definitions.  On a second plan of the same items, against what the two
    existing calls leave."""
    eng = sc.eng
    rng = np.random.default_rng(1501)
    make, d_in, blobs, overflows, eoss, close = mixed_plan(sc, fill, rng)
    plan, d_items = make()
    other, d_other = make()
    n = len(blobs)
    try:
        sents = run_calls(sc, eng, plan, d_in, blobs, overflows, eoss, (1, 16), label="mixed/" + fill)
        sent = sents[0]
        some = int((sent.n > 0).sum())
        assert 4 * int(sent.stored.sum()) >= some and 4 * int(((sent.n > 0) & ~sent.stored).sum()) >= some, (fill, sent.counts, some)
        for sent, B in ((sents[0], 64), (sents[1], 512)):
            icap = bi.expected(sc.lens, blobs, B)[1].size + 3
            theirs = two_calls_leave(eng, other, d_in, n, sent.total + 64, sent.total, sent.align, B, icap)
            mine = one_call_leaves(eng, plan, d_in, n, sent.total + 64, sent.total, sent.align, B, icap)
            same(mine, theirs, "mixed/%s, B %d" % (fill, B))
            assert mine[5] == INDEX_OK and mine[8][2] > 0
    finally:
        for p in (plan, other):
            sc.lib.aws_huffman_amd_encode_plan_destroy(p)
        for d in (d_items, d_other):
            if d:
                eng.free(d)
        close()


# ----------------------------------------------------------------------------- 2: ties
def run_ties(sc):
    """len_i == in_len_i is stored: every non-empty item under a coder of 256 eight-bit codes, and items of the test coder's
    own eight-bit symbols."""
    lib = sc.lib
    rng = np.random.default_rng(1503)
    sizes = [0, 1, 17, 700, 5_000, SEG, 2 * SEG + 9, 64]
    coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*([8] * 256)))
    assert coder
    eng = harness.Engine(lib, coder)
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    b = pa.Batch(eng, blobs, rng)
    plan = eng.encode_plan(b.items)
    try:
        ocoder = fa.oracle_coder(sc.oracle, ba.coder_rows(coder))
        sents = run_calls(sc, eng, plan, b.d_in, blobs, b.overflows, b.eoss, (1, 16), label="len8",
                          code_lens=np.full(256, 8, np.int64), ocoder=ocoder)
        assert np.array_equal(sents[0].stored, sents[0].n > 0) and np.array_equal(sents[0].coded, sents[0].n)
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        eng.close()
        lib.aws_huffman_amd_table_coder_destroy(coder)
    eight = np.flatnonzero(sc.lens == 8).astype(np.uint8)
    assert eight.size == 10
    eng = sc.eng
    blobs = [eight[rng.integers(0, eight.size, n)] for n in sizes] + [sa.words(rng, 300)]
    b = pa.Batch(eng, blobs, rng)
    plan = eng.encode_plan(b.items)
    try:
        sents = run_calls(sc, eng, plan, b.d_in, blobs, b.overflows, b.eoss, (1, 16), label="eight-bit symbols")
        assert np.array_equal(sents[0].stored[:-1], sents[0].n[:-1] > 0) and not sents[0].stored[-1]
        assert np.array_equal(sents[0].coded[:-1], sents[0].n[:-1])
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 3: never stored
def run_never_stored(sc):
    """Items with carried overflow bits, every second one, of ten-bit symbols, and empty items: the carried bits count in the
    length and not in the index."""
    eng = sc.eng
    rng = np.random.default_rng(1509)
    sizes = [40, 0, 700, 5_000, 0, SEG + 1, 90, 3, 2_000, 0, 33, 129]
    blobs = [pc.inputs(rng, n, "long") for n in sizes]  # (ten bits a symbol: every one of them would be stored)
    overflows = pa.carried(rng, len(blobs), every=2)
    b = pa.Batch(eng, blobs, rng, overflows=overflows)
    plan = eng.encode_plan(b.items)
    try:
        sents = run_calls(sc, eng, plan, b.d_in, blobs, b.overflows, b.eoss, (1, 16), label="never")
        for i, (blob, ov) in enumerate(zip(blobs, overflows)):
            assert bool(sents[0].stored[i]) == (blob.size > 0 and ov[1] == 0), i
        assert sents[0].stored.any() and (~sents[0].stored & (sents[0].n > 0)).any()
        bare = pa.encoded_lengths(sc.lens, blobs, [0] * len(blobs))
        assert np.any(bare != sents[0].coded)  # (the two definitions differ on this batch: the check can tell them apart)
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 4: capacity clipping
def run_capacity_clipping(sc, aligns=(1, 16)):
    """stored_api.run_capacity_clipping's sizes: the edge inside a stored item, at its first byte, around its last, and inside
    a coded item that stored ones follow."""
    eng = sc.eng
    rng = np.random.default_rng(1513)
    kinds = ["w", "u", "u", "w", "u", "w", "u", "u", "w", "u", "u"]
    sizes = [40, 700, 0, 5_000, 2 * SEG + 500, 300, 90, SEG + 1, 3 * SEG, 17, 4097]
    blobs = [sa.words(rng, n) if k == "w" else pc.inputs(rng, n, "uniform") for k, n in zip(kinds, sizes)]
    b = pa.Batch(eng, blobs, rng)
    plan = eng.encode_plan(b.items)

    def caps_of(sent):
        caps = [0, sent.total - 1, sent.total + 5]
        for i in range(len(blobs)):
            off, n = int(sent.offsets[i]), int(sent.lens[i])
            if sent.stored[i]:
                caps += [off, off + 1, off + n // 2, off + n - 1, off + n, off + n + 1]
            elif n:
                caps += [off + n // 2]
        return sorted(set(c for c in caps if 0 <= c))

    try:
        sents = run_calls(sc, eng, plan, b.d_in, blobs, b.overflows, b.eoss, aligns, blocks=(512,), caps_of=caps_of, label="clip")
        s = sents[0].stored
        assert s[1] and s[4] and s[6] and s[7] and s[9] and s[10] and not (s[0] or s[3] or s[5] or s[8]), s
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 5: scan boundaries
def run_scan_boundaries(sc, tile, counts):
    """The offset scan in tiles of a few items (packed_api.SCAN_TILES), stored and coded items mixed, every item in the index's
    tiles and by the index's rule.  The stored items' bytes and records whole (numpy), a sample of the coded ones (the
    oracle), every offset, flag, directory record and index entry."""
    eng = sc.eng
    rng = np.random.default_rng(1517 + tile)
    most = max(counts)
    sizes = rng.integers(1, 40, most)
    blobs = [sa.words(rng, int(n)) if i % 3 else pc.inputs(rng, int(n), "uniform") for i, n in enumerate(sizes)]
    b = pa.Batch(eng, blobs, None, overflows=pa.carried(rng, most, every=5))
    B = 64
    try:
        with pa.pack_tile_items(sc.lib, tile):
            for k, n in enumerate(counts):
                plan = eng.encode_plan(b.items[:n])
                want_dir, want_index = bi.expected(sc.lens, blobs[:n], B)
                try:
                    # (every item in the index's tiles where the batch is small: a workgroup an item; the rule elsewhere)
                    for align, limit in ((1, bi.ALL_TILES if n <= 1000 else 0), (16, 0)) if k == 0 else ((1, 0),):
                        sent = sa.Sent(sc.oracle, sc.w.ocoder, blobs[:n], sc.lens, b.overflows[:n], b.eoss[:n], align)
                        assert sent.stored.any() and not sent.stored.all()
                        bufs, a = sa.Buffers(eng, n, sent.total + 64, b.d_in), bi.Arrays(eng, n, want_index.size)
                        try:
                            bufs.refill()
                            with bi.wave_bytes(sc.lib, limit):
                                assert launch(eng, plan, b.d_in, bufs.d_out, sent.total, bufs.d_off, bufs.d_flags, align, B, a.d_dir,
                                              a.d_index, a.capacity, a.d_status) == (0, 0)
                            label = "tile %d, %d items, align %d" % (tile, n, align)
                            assert np.array_equal(pa.download_u64(eng, bufs.d_off, n + 1), sent.offsets), label
                            flags = eng.download(bufs.d_flags, n + 8)
                            assert np.array_equal(flags[:n], sent.stored.astype(np.uint8)) and np.all(flags[n:] == FLAG_GUARD), label
                            assert pa.packed_size(eng, plan) == (0, 0, sent.total, int(sent.reserved.max())), label
                            assert sa.stored_size(eng, plan) == (0, 0) + sent.counts, label
                            pi.check_arrays(a, want_dir, want_index, INDEX_OK, label)
                            got = eng.download(bufs.d_out, bufs.size)
                            res = pa.results_array(eng, plan, n)
                            want = np.concatenate(blobs[:n])
                            lens = sent.n
                            at = np.repeat(sent.offsets[:-1] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
                            mask = np.repeat(sent.stored, lens)
                            assert np.array_equal(got[at[mask]], want[mask]), label
                            st = sent.stored
                            assert np.all(res["rc"][st] == 0) and np.array_equal(res["produced"][st].astype(np.int64), lens[st]), label
                            assert np.array_equal(res["consumed"][st].astype(np.int64), lens[st]) and np.all(res["num_bits"][st] == 0)
                            for i in list(range(0, n, 97)) + [n - 1]:
                                if not st[i]:
                                    room = int(sent.reserved[i])
                                    rec, data = pa.oracle_item(sc.oracle, sc.w.ocoder, blobs[i], b.overflows[i], b.eoss[i], room)
                                    off = int(sent.offsets[i])
                                    assert np.array_equal(got[off:off + room], data), (label, i)
                                    assert (res["rc"][i], res["error"][i], res["consumed"][i], res["produced"][i]) == rec[:4], (label, i)
                            edges = np.zeros(bufs.size + 1, np.int64)
                            np.add.at(edges, sent.offsets[:-1], 1)
                            np.add.at(edges, sent.offsets[:-1] + sent.lens, -1)
                            owned = np.cumsum(edges)[:-1] > 0
                            assert np.all(got[~owned] == MARKER) and not owned[sent.total:].any(), label
                        finally:
                            a.close()
                            bufs.close()
                finally:
                    sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
    finally:
        pi.restore_switches(sc.lib)
        b.close()


# ----------------------------------------------------------------------------- 6: an index that does not fit
def run_index_too_small(sc):
    """One entry short and a single entry, offsets, flags and output full of markers in front: the status says so, the
    directory is whole, no index word, every offset 0, every flag 0, no output byte, every record the oracle's for no room,
    both sizes nothing.  Then the same plan with enough room, nothing reset in between."""
    eng = sc.eng
    rng = np.random.default_rng(1523)
    sizes = [700, 40, 0, 5_000, 300, SEG + 1, 17, 4097, 90]
    blobs = [sa.words(rng, n) if i % 2 else pc.inputs(rng, n, "uniform") for i, n in enumerate(sizes)]
    b = pa.Batch(eng, blobs, rng, overflows=pa.carried(rng, len(blobs), every=4))
    plan = eng.encode_plan(b.items)
    B = 64
    try:
        sent = sa.Sent(sc.oracle, sc.w.ocoder, blobs, sc.lens, b.overflows, b.eoss, 16)
        assert sent.stored.sum() >= 3
        entries = bi.expected(sc.lens, blobs, B)[1].size
        for icap in (entries - 1, 1):
            check_call(sc, eng, plan, b.d_in, sent, sc.lens, B, cap=100_000, index_capacity=icap, label="index capacity %d" % icap)
        check_call(sc, eng, plan, b.d_in, sent, sc.lens, B, label="behind the short ones")
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 7: other states
def run_other_states(sc):
    """The argument refusals (nothing is written), aws_huffman_amd_decode_plan_from_encode refused behind the call, a later
    plain packed launch as ever, a plan without items."""
    eng, lib = sc.eng, sc.lib
    rng = np.random.default_rng(1531)
    blobs = [pc.inputs(rng, 300, "uniform"), sa.words(rng, 5_000), pc.inputs(rng, 20_000, "uniform"), sa.words(rng, 40)]
    n, B = len(blobs), 64
    b = pa.Batch(eng, blobs, rng, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    none = eng.empty_encode_plan()
    dplan = eng.empty_decode_plan()
    sent = sa.Sent(sc.oracle, sc.w.ocoder, blobs, sc.lens, b.overflows, b.eoss, 1)
    bufs = sa.Buffers(eng, n, sent.total + 64, b.d_in)
    a = bi.Arrays(eng, n, 500)
    try:
        bufs.refill()
        call = lambda **kw: launch(
            eng, kw.get("plan", plan), kw.get("d_in", b.d_in), kw.get("d_out", bufs.d_out), kw.get("cap", sent.total),
            kw.get("d_off", bufs.d_off), kw.get("d_flags", bufs.d_flags), kw.get("align", 1), kw.get("B", B), kw.get("d_dir", a.d_dir),
            kw.get("d_index", a.d_index), kw.get("capacity", 500), kw.get("d_status", a.d_status))
        assert call(plan=None) == INVALID
        assert call(d_flags=None) == INVALID
        assert call(d_index=None) == INVALID
        assert call(capacity=0) == INVALID
        assert call(d_index=None, capacity=0) == INVALID    # the index call's size query is not this call's
        for bad in (0, 3, 24, 8192):
            assert call(align=bad) == INVALID, bad
        for bad in (0, 63, 96, 1 << 25):
            assert call(B=bad) == INVALID, bad
        assert call(d_off=None) == INVALID
        assert call(d_off=bufs.d_off + 4) == INVALID
        assert call(d_out=None) == INVALID                  # no output with a capacity
        assert call(d_dir=None) == INVALID
        assert call(d_index=a.d_index + 4) == INVALID
        assert call(d_status=a.d_status + 2) == INVALID
        assert call(d_in=None) == INVALID
        assert sa.stored_size(eng, plan)[:2] == INVALID and bi.index_size(eng, plan)[:2] == INVALID  # (no call was made yet)
        eng.sync()
        d, x, status = a.read()
        assert np.all(d.view(np.uint64) == EE) and np.all(x == EE) and status == 0xEEEEEEEE
        assert np.all(eng.download(bufs.d_out, bufs.size) == MARKER) and np.all(eng.download(bufs.d_off, 8 * (n + 1)) == 0xEE)
        assert np.all(eng.download(bufs.d_flags, n + 8) == FLAG_GUARD)
        # the call, then aws_huffman_amd_decode_plan_from_encode behind it
        check_call(sc, eng, plan, b.d_in, sent, sc.lens, B, label="states")
        assert list(sent.stored) == [True, False, True, False]
        assert sa.from_encode(eng, dplan, plan) == sa.INVALID_STATE
        # a later plain packed launch of the same plan clears the state and behaves as before
        pa.check_launch(sc.oracle, sc.w.ocoder, eng, plan, b.d_in, blobs, sc.lens, b.overflows, b.eoss, 1, label="packed again")
        assert sa.stored_size(eng, plan)[:2] == INVALID
        assert sa.from_encode(eng, dplan, plan) == (0, 0)
        check_call(sc, eng, plan, b.d_in, sent, sc.lens, 512, label="states, once more")
        # a plan without items
        a0 = bi.Arrays(eng, 0, 1)
        try:
            bufs.refill()
            assert launch(eng, none, None, None, 0, bufs.d_off, bufs.d_flags, 1, B, a0.d_dir, a0.d_index, 1, a0.d_status) == (0, 0)
            eng.sync()
            d, x, status = a0.read()
            assert status == INDEX_OK and d.tolist() == [[0, 0]] and x[0] == 0
            off = eng.download(bufs.d_off, 16).view(np.uint64)
            assert off[0] == 0 and off[1] == EE
            assert np.all(eng.download(bufs.d_flags, n + 8) == FLAG_GUARD) and np.all(eng.download(bufs.d_out, bufs.size) == MARKER)
            assert pa.packed_size(eng, none) == (0, 0, 0, 0) and sa.stored_size(eng, none) == (0, 0, 0, 0)
            assert bi.index_size(eng, none) == (0, 0, 1)
        finally:
            a0.close()
    finally:
        a.close()
        bufs.close()
        lib.aws_huffman_amd_decode_plan_destroy(dplan)
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        lib.aws_huffman_amd_encode_plan_destroy(none)
        b.close()


def run_fitted(sc, memset_async):
    """count -> fit -> the call on one stream, nothing waited for in between, over stored_api.run_fitted's data: the fitted
    code is the host's for the data's counts, the three binary items are exactly the stored ones, and the index is the
    definition's under the fitted lengths."""
    lib = sc.lib
    rng = np.random.default_rng(1423)
    sizes = [3_000, 40_000, 700, 20_000, 90, SEG + 5, 5_000, 300, 2_000, 60_000]
    binary = {2, 5, 8}
    blobs = [pc.inputs(rng, n, "uniform") if i in binary else harness.printable_map(rng.integers(0, 256, n, dtype=np.uint8))
             for i, n in enumerate(sizes)]
    n, B = len(blobs), 512
    eng = fa.FittedEngine(lib, 4, 12)
    b = pa.Batch(eng, blobs, None, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    capacity = 2 * sum(sizes)
    bufs = sa.Buffers(eng, n, capacity + 64, b.d_in)
    a = bi.Arrays(eng, n, sum(ia.n_blocks_of(s, B) for s in sizes) + 1)
    stream = C.c_void_p(eng.stream)
    try:
        bufs.refill()
        assert launch(eng, plan, b.d_in, bufs.d_out, capacity, bufs.d_off, bufs.d_flags, 1, B, a.d_dir, a.d_index, a.capacity,
                      a.d_status) == STATE  # (never fitted)
        eng.fill(eng.d_status, 0xEE, 4)
        memset_async(eng, eng.d_counts, 256 * 8, stream)
        assert pk.plan_counts(eng, plan, b.d_in, eng.d_counts, stream) == (0, 0)
        assert eng.fit_counts_async(None, stream) == (0, 0)
        assert launch(eng, plan, b.d_in, bufs.d_out, capacity, bufs.d_off, bufs.d_flags, 1, B, a.d_dir, a.d_index, a.capacity,
                      a.d_status, stream) == (0, 0)
        assert lib.aws_huffman_amd_stream_synchronize(eng.h, stream) == 0
        assert eng.status() == fa.FIT_OK
        lengths = fa.host_lengths(lib, ba.bincount(np.concatenate(blobs)), eng.lo, eng.hi)
        assert eng.bits() == lengths
        ocoder = fa.oracle_coder(sc.oracle, fa.host_rows(lib, lengths))
        code_lens = np.asarray(lengths, dtype=np.int64)
        sent = sa.Sent(sc.oracle, ocoder, blobs, code_lens, b.overflows, b.eoss, 1)
        assert set(np.flatnonzero(sent.stored)) == binary, (np.flatnonzero(sent.stored), sent.coded, sent.n)
        sa.check_sent(eng, plan, sent, bufs, capacity, "fitted", launch=False)
        want_dir, want_index = bi.expected(code_lens, blobs, B)
        pi.check_arrays(a, want_dir, want_index, INDEX_OK, "fitted")
    finally:
        a.close()
        bufs.close()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        eng.close()


def run_replayed(sc, graphs):
    """The call captured in a graph behind a first, uncaptured one (which allocates), and replayed into fresh markers."""
    eng = sc.eng
    rng = np.random.default_rng(1543)
    blobs = sa.round_trip_blobs(rng)
    n, B = len(blobs), 512
    b = pa.Batch(eng, blobs, rng, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    sent = sa.Sent(sc.oracle, sc.w.ocoder, blobs, sc.lens, b.overflows, b.eoss, 16)
    want_dir, want_index = bi.expected(sc.lens, blobs, B)
    bufs, a = sa.Buffers(eng, n, sent.total + 64, b.d_in), bi.Arrays(eng, n, want_index.size)
    stream = C.c_void_p(eng.stream)
    enqueue = lambda: launch(eng, plan, b.d_in, bufs.d_out, sent.total, bufs.d_off, bufs.d_flags, 16, B, a.d_dir, a.d_index, a.capacity,
                             a.d_status, stream)
    g = None
    try:
        bufs.refill()
        assert enqueue() == (0, 0)
        graphs.call("hipStreamSynchronize", stream)
        answers = []
        g = graphs.capture(stream, lambda: answers.append(enqueue()))
        assert answers == [(0, 0)]
        bufs.refill()
        a.refill()
        eng.sync()
        graphs.call("hipGraphLaunch", g, stream)
        graphs.call("hipStreamSynchronize", stream)
        sa.check_sent(eng, plan, sent, bufs, sent.total, "replayed", launch=False)
        pi.check_arrays(a, want_dir, want_index, INDEX_OK, "replayed")
    finally:
        if g:
            graphs.call("hipGraphExecDestroy", g)
        a.close()
        bufs.close()
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- the receiver
WAVE, TILE_BYTES = 4096, 16384  # HUFK_STORED_WAVE_BYTES, HUFK_STORED_TILE_BYTES: the copy's limits
COPY_LENGTHS = [WAVE - 1, WAVE, WAVE + 1, TILE_BYTES - 1, TILE_BYTES, TILE_BYTES + 1, 2 * TILE_BYTES + 1]


class StoredPackedBatch(bi.PackedBatch):
    """A batch as its receiver has it, all of it made by the device with ONE call of
    aws_huffman_amd_encode_plan_launch_packed_stored_indexed and checked against the definition before anything is built on
    it: the packed buffer (`enc_offset` bytes into a larger one), its offsets, its flags, the directory and the index."""

    def __init__(self, sc, eng, code_lens, ocoder, blobs, B, align=1, enc_offset=0):
        self.sc, self.eng, self.ocoder, self.B, self.enc_offset = sc, eng, ocoder, B, enc_offset
        self.code_lens = np.asarray(code_lens, dtype=np.int64)
        self.blobs, self.n = blobs, len(blobs)
        n = self.n
        b = pa.Batch(eng, blobs, None, eoss=[0xFF] * n)
        plan = eng.encode_plan(b.items)
        self.owned = []
        try:
            sent = sa.Sent(sc.oracle, ocoder, blobs, self.code_lens, b.overflows, b.eoss, align)
            self.stored, self.enc_lens, self.offsets, self.total = sent.stored, sent.lens, sent.offsets, sent.total
            self.dir, self.index = bi.expected(self.code_lens, blobs, B)
            self.entries = self.index.size
            self.size = enc_offset + self.total
            a = bi.Arrays(eng, n, self.entries)
            self.d_enc, self.d_off, self.d_flags = eng.alloc(self.size + 64), eng.alloc(8 * (n + 1)), eng.alloc(n + 8)
            self.owned += [a.d_dir, a.d_index, a.d_status, self.d_enc, self.d_off, self.d_flags]
            eng.fill(self.d_enc, 0x5A, self.size + 64)
            eng.fill(self.d_flags, FLAG_GUARD, n + 8)
            assert launch(eng, plan, b.d_in, self.d_enc + enc_offset, self.total, self.d_off, self.d_flags, align, B, a.d_dir, a.d_index,
                          self.entries, a.d_status) == (0, 0)
            eng.sync()
            d, x, status = a.read()
            assert status == INDEX_OK and np.array_equal(d, self.dir) and np.array_equal(x.astype(np.int64), self.index)
            self.d_dir, self.d_index = a.d_dir, a.d_index
            assert np.array_equal(pa.download_u64(eng, self.d_off, n + 1), self.offsets)
            assert np.array_equal(eng.download(self.d_flags, n), self.stored.astype(np.uint8))
            self.enc_host = eng.download(self.d_enc, self.size + 64)
            for i in np.flatnonzero(self.stored):
                at = enc_offset + int(self.offsets[i])
                assert np.array_equal(self.enc_host[at:at + blobs[i].size], blobs[i]), i
            self.d_lens = pda.upload_u64(eng, self.enc_lens)
            self.owned.append(self.d_lens)
            self.encs = {}
        finally:
            sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
            b.close()

    def reset(self, plan, ranges, **kw):
        """aws_huffman_amd_decode_plan_reset_stored_item_block_ranges: (rc, error); any argument can be replaced by name."""
        eng = self.eng
        flat = np.asarray([v & ((1 << 64) - 1) for r in ranges for v in r], dtype=np.uint64)
        d_ranges = self.upload(flat) if "d_ranges" not in kw else kw["d_ranges"]
        eng.lib.aws_reset_error()
        rc = eng.lib.aws_huffman_amd_decode_plan_reset_stored_item_block_ranges(
            kw.get("plan", plan), kw.get("d_dir", self.d_dir), kw.get("d_index", self.d_index), kw.get("entries", self.entries),
            kw.get("items", self.n), kw.get("B", self.B), kw.get("d_off", self.d_off), kw.get("d_lens", None),
            kw.get("d_flags", self.d_flags), kw.get("enc_offset", self.enc_offset), kw.get("enc_length", self.total), d_ranges,
            len(ranges), None)
        return rc, eng.lib.aws_last_error() if rc else 0

    def reset_symbols(self, plan, ranges, **kw):
        """aws_huffman_amd_decode_plan_reset_stored_item_symbol_ranges: (rc, error)."""
        eng = self.eng
        flat = np.asarray([v & ((1 << 64) - 1) for r in ranges for v in r], dtype=np.uint64)
        d_ranges = self.upload(flat) if "d_ranges" not in kw else kw["d_ranges"]
        eng.lib.aws_reset_error()
        rc = eng.lib.aws_huffman_amd_decode_plan_reset_stored_item_symbol_ranges(
            kw.get("plan", plan), kw.get("d_input", self.d_enc), kw.get("d_dir", self.d_dir), kw.get("d_index", self.d_index),
            kw.get("entries", self.entries), kw.get("items", self.n), kw.get("B", self.B), kw.get("d_off", self.d_off),
            kw.get("d_lens", None), kw.get("d_flags", self.d_flags), kw.get("enc_offset", self.enc_offset),
            kw.get("enc_length", self.total), d_ranges, len(ranges), None)
        return rc, eng.lib.aws_last_error() if rc else 0

    def locate(self, items, symbols, old=False, **kw):
        """One aws_huffman_amd_locate_stored_item_symbols call (old: aws_huffman_amd_locate_item_symbols): (bits, status)."""
        eng, n = self.eng, len(items)
        d_items, d_syms = self.upload(np.asarray(items, dtype=np.uint64)), self.upload(np.asarray(symbols, dtype=np.uint64))
        d_bits, d_status = eng.alloc(8 * (n + bi.GUARD_WORDS)), eng.alloc(8)
        self.owned += [d_bits, d_status]
        eng.fill(d_bits, 0xEE, 8 * (n + bi.GUARD_WORDS))
        eng.fill(d_status, 0xEE, 8)
        eng.lib.aws_reset_error()
        front = (eng.h, self.d_enc + self.enc_offset, kw.get("enc_length", self.total), kw.get("d_dir", self.d_dir),
                 kw.get("d_index", self.d_index), kw.get("entries", self.entries), kw.get("items", self.n), kw.get("B", self.B),
                 kw.get("d_off", self.d_off), kw.get("d_lens", None))
        back = (d_items, d_syms, n, d_bits, d_status, None)
        if old:
            rc = eng.lib.aws_huffman_amd_locate_item_symbols(*(front + back))
        else:
            rc = eng.lib.aws_huffman_amd_locate_stored_item_symbols(*(front + (kw.get("d_flags", self.d_flags),) + back))
        assert rc == 0, eng.lib.aws_last_error()
        eng.sync()
        got = eng.download(d_bits, 8 * (n + bi.GUARD_WORDS)).view(np.uint64)
        status = eng.download(d_status, 8).view(np.uint32)
        assert np.all(got[n:] == EE) and status[1] == 0xEEEEEEEE
        return got[:n].copy(), int(status[0])

    def piece(self, r, symbols):
        """What a range comes to, from the definition: (record, its symbols)."""
        item, first, count, _ = r
        if self.stored[item]:
            lo, hi = (first, first + count) if symbols else (first * self.B, min((first + count) * self.B, self.blobs[item].size))
            syms = self.blobs[item][lo:hi] if count else self.blobs[item][:0]
            return (0, 0, syms.size, 8 * syms.size), syms
        enc, first_bit, cap, syms = (self.symbol_item if symbols else self.item)(item, first, count)
        rec, out = pda.oracle_item(self.sc.oracle, self.ocoder, enc, first_bit, cap)
        assert rec[:2] in ((0, 0), pda.SHORT) and rec[2] == cap and np.array_equal(out, syms), (r, rec)
        return rec, syms

    def length_of(self, r, symbols):
        item, first, count, _ = r
        return count if symbols else (min((first + count) * self.B, self.blobs[item].size) - first * self.B if count else 0)

    def check_launch(self, plan, ranges, out_size, label="", symbols=False):
        """A plain launch of the plan: every byte of the output (MARKER where no range writes), every record."""
        eng = self.eng
        want = np.full(out_size, MARKER, np.uint8)
        recs = []
        for r in ranges:
            rec, syms = self.piece(r, symbols)
            recs.append(rec)
            want[r[3]:r[3] + syms.size] = syms
        d_out = eng.alloc(out_size)
        try:
            eng.fill(d_out, MARKER, out_size)
            eng.decode_launch(plan, self.d_enc, d_out)
            got = eng.download(d_out, out_size)
            res = eng.decode_results(plan, len(ranges))
        finally:
            eng.free(d_out)
        for i, rec in enumerate(recs):
            assert res[i] == rec, (label, i, ranges[i], bool(self.stored[ranges[i][0]]), res[i], rec)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (label, "first wrong byte at %d" % int(bad[0]))
        return got, recs

    def bits_of(self, item):
        """bits[s] = where symbol s of the item starts, from the packed buffer's first byte: a byte a symbol in a stored item."""
        if self.stored[item]:
            return (np.arange(self.blobs[item].size + 1, dtype=np.uint64) + np.uint64(int(self.offsets[item]))) * np.uint64(8)
        return self.symbol_bits(item)


def short_words(rng, n, code_lens):
    """Symbols the coder codes in fewer than 8 bits: lowercase words where it does, its 27 shortest codes' symbols where not."""
    alphabet = sa.ALPHABET
    if code_lens is not None and not np.all(np.asarray(code_lens)[alphabet] < 8):
        alphabet = np.argsort(np.asarray(code_lens), kind="stable")[:27].astype(np.uint8)
    return alphabet[rng.integers(0, alphabet.size, n)]


def receiver_blobs(rng, seed=907, code_lens=None):
    """batch_index_api.seeded_lengths with uniform and word items in turn, and stored items at the copy's wave and tile limits.
    (Words: short_words.)"""
    lengths = bi.seeded_lengths(seed)
    blobs = [pc.inputs(rng, n, "uniform") if i % 2 else short_words(rng, n, code_lens) for i, n in enumerate(lengths)]
    return blobs + [pc.inputs(rng, n, "uniform") for n in COPY_LENGTHS]


def seeded_ranges(pb, rng, count=60, symbols=False):
    """Whole items, the ragged last block, single blocks, empties, repeats, stored and coded mixed in any order; the item of
    every third range is drawn from the stored ones, of every third from the coded ones.  (ranges with their out_offsets one
    behind the other, 3 bytes between; the output size)"""
    some = [i for i in range(pb.n) if pb.n_blocks(i)]
    classes = ([i for i in some if pb.stored[i]], [i for i in some if not pb.stored[i]])
    spans = []
    for i in classes[0][:3] + classes[1][:3] + list(range(pb.n - len(COPY_LENGTHS), pb.n)):
        spans.append((i, 0, pb.blobs[i].size if symbols else pb.n_blocks(i)))     # a whole item
        spans.append((i, (pb.n_blocks(i) - 1) * pb.B, pb.blobs[i].size - (pb.n_blocks(i) - 1) * pb.B) if symbols
                     else (i, pb.n_blocks(i) - 1, 1))                               # its last block (ragged for most)
    spans.append((next(i for i in range(pb.n) if pb.n_blocks(i) == 0), 0, 0))       # an empty item's nothing
    while len(spans) < count:
        i = int(rng.choice(classes[min(len(spans) % 3, 1)]))  # (the fixed spans in front lean to the stored items)
        top = pb.blobs[i].size if symbols else pb.n_blocks(i)
        first = int(rng.integers(0, top + 1))
        most = min(top - first, 900) if symbols else top - first
        spans.append((i, first, int(rng.integers(0, most + 1)) if len(spans) % 5 else min(1, most)))
    spans += spans[3:6]                                                              # repeats
    in_stored = sum(1 for i, _, _ in spans if pb.stored[i])
    assert 3 * in_stored >= len(spans) and 3 * (len(spans) - in_stored) >= len(spans), (in_stored, len(spans))
    ranges, at = [], 3
    for k in rng.permutation(len(spans)):
        r = spans[k] + (at,)
        ranges.append(r)
        at += pb.length_of(r, symbols) + 3
    return ranges, at + 64


def poisoned_index(pb):
    """The index with the entries strictly inside each stored item's blocks overwritten."""
    bad = pb.index.astype(np.uint64).copy()
    for i in np.flatnonzero(pb.stored):
        bad[int(pb.dir[i][0]) + 1:int(pb.dir[i + 1][0])] = EE
    assert np.any(bad == EE)
    return pb.upload(bad)


def run_ranges(sc, name, B, poison=False):
    """Seeded ranges of blocks and of symbols, in stored and coded items, decoded and copied by a plain launch: offsets only at
    align 1, then the lengths array at align 16; each batch 5 bytes into a larger buffer.  poison: the index entries inside the
    stored items' blocks are overwritten first -- nothing changes."""
    eng, code_lens, ocoder, coder = bi.coder_of(sc, name)
    rng = np.random.default_rng(1601)
    plan = eng.empty_decode_plan()
    pbs = []
    try:
        for align, with_lens, count in ((1, False, 60),) if poison else ((1, False, 60), (16, True, 45)):
            pb = StoredPackedBatch(sc, eng, code_lens, ocoder, receiver_blobs(rng, 907 if align == 1 else 1019, code_lens), B, align=align, enc_offset=5)
            pbs.append(pb)
            assert pb.stored[-len(COPY_LENGTHS):].all() and 4 * pb.stored.sum() >= pb.n and 4 * (~pb.stored).sum() >= pb.n
            kw = dict(d_lens=pb.d_lens) if with_lens else {}
            if poison:
                kw["d_index"] = poisoned_index(pb)
            label = "%s, B %d, align %d" % (name, B, align)
            ranges, out_size = seeded_ranges(pb, rng, count)
            assert pb.reset(plan, ranges, **kw) == (0, 0), label
            assert eng.decode_stats(plan)["items"] == len(ranges)
            pb.check_launch(plan, ranges, out_size, label=label + ", blocks")
            ranges, out_size = seeded_ranges(pb, rng, count, symbols=True)
            assert pb.reset_symbols(plan, ranges, **kw) == (0, 0), label
            pb.check_launch(plan, ranges, out_size, label=label + ", symbols", symbols=True)
    finally:
        for p in pbs:
            p.close()
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        if coder is not None:
            sc.done(eng, coder)


# ----------------------------------------------------------------------------- 9: alignment sweep of the range copy
def run_alignment_sweep(sc):
    """Stored symbol ranges of 1 to 80 bytes and of 4096 + k bytes at every source misalignment crossed with every
    destination misalignment (out_offset is the caller's), a coded range among them now and then."""
    eng = sc.eng
    rng = np.random.default_rng(1607)
    blobs = [sa.words(rng, 700), pc.inputs(rng, 40_000, "uniform"), sa.words(rng, 90)]
    pb = StoredPackedBatch(sc, eng, sc.lens, sc.w.ocoder, blobs, 512, align=1, enc_offset=5)
    plan = eng.empty_decode_plan()
    try:
        assert list(pb.stored) == [False, True, False] and pb.d_enc % 16 == 0
        base = pb.enc_offset + int(pb.offsets[1])  # (the stored item's first byte, from a 16-byte boundary)
        lengths = list(range(1, 81)) + [4096 + k for k in range(0, 17)]
        ranges, at, seen = [], 0, set()
        for s in range(16):
            for d in range(16):
                n = lengths[(s * 16 + d) % len(lengths)] if (s + d) % 3 else 4096 + (s + d) % 17
                s0 = (s - base) % 16 + 16 * int(rng.integers(0, (40_000 - n) // 16 - 1))
                at = (at + 31) // 16 * 16 + d
                ranges.append((1, s0, n, at))
                seen.add(((base + s0) % 16, at % 16))
                at += n
                if (s + d) % 7 == 0:
                    at += 3
                    ranges.append((0, int(rng.integers(0, 600)), 50, at))
                    at += 50
        for k, n in enumerate(range(1, 81)):  # every short length once more, wherever it falls
            at += 5
            ranges.append((1, 1_000 + 97 * k, n, at))
            at += n
        assert len(seen) == 256
        assert pb.reset_symbols(plan, ranges) == (0, 0)
        pb.check_launch(plan, ranges, at + 64, label="alignment sweep", symbols=True)
    finally:
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        pb.close()


# ----------------------------------------------------------------------------- 11: locate
def run_locate(sc, name):
    """Positions 0, 1, B - 1, B, n - 1 and n of stored and coded items through the new call: a stored item gives
    8 * (offset + s); with NULL flags the call is aws_huffman_amd_locate_item_symbols word for word."""
    if name == "len8":
        ocoder, coder, lengths = pc.profile_coders(sc.w, name)
        eng, code_lens = harness.Engine(sc.lib, coder), np.asarray(lengths, dtype=np.int64)
    else:
        eng, code_lens, ocoder, coder = bi.coder_of(sc, name)
    rng = np.random.default_rng(1609)
    B = 64
    sizes = [700, 0, 3_000, 64, 129, 9_001, 1, 0, 4_096]
    blobs = [sa.words(rng, n) if i % 2 else pc.inputs(rng, n, "uniform") for i, n in enumerate(sizes)]
    pb = StoredPackedBatch(sc, eng, code_lens, ocoder, blobs, B, align=1, enc_offset=5)
    try:
        assert pb.stored.sum() >= 3 and (name == "len8" or (~pb.stored & (pb.dir[:-1, 1] > 0)).sum() >= 2)
        items, syms = [], []
        for i, n in enumerate(sizes):
            for s in sorted({s for s in (0, 1, B - 1, B, n - 1, n, n // 2) if 0 <= s <= n}):
                items.append(i)
                syms.append(s)
        want = np.asarray([pb.bits_of(i)[s] for i, s in zip(items, syms)], dtype=np.uint64)
        for lens in (None, pb.d_lens):
            got, status = pb.locate(items, syms, d_lens=lens)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (name, items[bad[0]], syms[bad[0]], int(got[bad[0]]), int(want[bad[0]]))
            assert status == ra.LOCATE_OK
        # what is not there: past a stored item's symbols, an item that is none
        stored = int(np.flatnonzero(pb.stored)[0])
        got, status = pb.locate([stored, pb.n, stored], [sizes[stored] + 1, 0, 5])
        assert [int(g) for g in got] == [ra.NO_BIT, ra.NO_BIT, 8 * (int(pb.offsets[stored]) + 5)] and status == ra.LOCATE_NOT_FOUND
        # NULL flags: the call without flags, word for word (a stored item's bytes read as codes, as that call reads them)
        mine, mine_status = pb.locate(items, syms, d_flags=None)
        theirs, their_status = pb.locate(items, syms, old=True)
        assert np.array_equal(mine, theirs) and mine_status == their_status
    finally:
        pb.close()
        if coder is not None:
            sc.done(eng, coder)


# ----------------------------------------------------------------------------- 12: damage
def run_damage(sc, name):
    """One row at a time, through both fills: refused, a plan without items whose launch writes nothing, and the same plan then
    takes a good fill."""
    eng, code_lens, ocoder, coder = bi.coder_of(sc, name)
    rng = np.random.default_rng(1613)
    B = 64
    sizes = [700, 0, 3_000, 64, 129, 5_000]
    blobs = [short_words(rng, n, code_lens) if i % 2 == 0 else pc.inputs(rng, n, "uniform") for i, n in enumerate(sizes)]
    pb = StoredPackedBatch(sc, eng, code_lens, ocoder, blobs, B, align=1, enc_offset=3)
    plan = eng.empty_decode_plan()
    n = pb.n
    assert list(pb.stored) == [False, False, False, True, False, True]
    out_size = 8_000 * n + 64
    d_out = eng.alloc(out_size)
    top = (1 << 64) - 1
    try:
        for symbols in (False, True):
            fill = pb.reset_symbols if symbols else pb.reset
            good = [(i, 0, pb.blobs[i].size if symbols else pb.n_blocks(i), 8_000 * i) for i in range(n)]

            def refused(label, ranges=None, **kw):
                assert fill(plan, good) == (0, 0) and eng.decode_stats(plan)["items"] == n, label
                assert fill(plan, good if ranges is None else ranges, **kw) == INVALID, (label, symbols)
                assert eng.decode_stats(plan)["items"] == 0, label
                eng.fill(d_out, MARKER, out_size)
                assert sc.lib.aws_huffman_amd_decode_plan_launch(plan, pb.d_enc, d_out, None) == 0, label
                eng.sync()
                assert np.all(eng.download(d_out, out_size) == MARKER), label

            def damaged(array, at, value, dtype=np.uint64):
                out = np.asarray(array).astype(np.int64).copy().reshape(-1)
                out[at] = value
                return pb.upload(out.astype(np.uint64)) if dtype == np.uint64 else flags_of(out)

            def flags_of(values):
                d = eng.alloc(n + 8)
                pb.owned.append(d)
                eng.upload(d, np.concatenate([np.asarray(values, dtype=np.uint8), np.full(8, FLAG_GUARD, np.uint8)]))
                return d

            flags = pb.stored.astype(np.uint8)
            two = flags.copy()
            two[5] = 2
            refused("a flag of 2 on a named stored item", d_flags=flags_of(two))
            two = flags.copy()
            two[2] = 2
            refused("a flag of 2 on a named coded item", d_flags=flags_of(two))
            assert fill(plan, good[:2] + good[3:], d_flags=flags_of(two)) == (0, 0)   # (on an item no range names: accepted)
            pb.check_launch(plan, good[:2] + good[3:], out_size, label="a flag of 2 that nobody names", symbols=symbols)
            wrong = pb.enc_lens.copy()
            wrong[5] -= 1
            refused("a stored item shorter than its symbols", d_lens=pb.upload(wrong))
            wrong[5] += 2
            refused("a stored item longer than its symbols", d_lens=pb.upload(wrong), enc_length=pb.total + 1)
            refused("the same by the offsets", d_off=damaged(pb.offsets, n, pb.total + 1), enc_length=pb.total + 1,
                    ranges=[good[5]])
            past = (5, 0, 5_001, 0) if symbols else (5, 0, pb.n_blocks(5) + 1, 0)
            refused("a range past a stored item", [past] + good)
            refused("a range that starts past a stored item", good + [(3, 65 if symbols else 2, 0, 0)])
            refused("first + count overflows", [(5, 1, top, 0)])
            refused("first + count overflows", [(5, top, 2, 0)])
            refused("item == item_count", good + [(n, 0, 0, 0)])
            refused("a directory that decreases", d_dir=damaged(pb.dir, 2 * 6, int(pb.dir[5][0]) - 1), ranges=[good[5]])
            refused("a directory past the index", entries=int(pb.dir[n][0]), ranges=[good[5]])
            refused("blocks that are not the symbols'", d_dir=damaged(pb.dir, 2 * 5 + 1, 5_000 + 64), ranges=[good[5]])
            refused("a stored item's bytes beyond encoded_length", enc_length=pb.total - 1, ranges=[good[5]])
            assert fill(plan, good[:5], enc_length=int(pb.offsets[5])) == (0, 0)
            assert fill(None, good) == INVALID
            assert fill(plan, good) == (0, 0)
            pb.check_launch(plan, good, out_size, label="behind the refusals", symbols=symbols)
            assert fill(plan, []) == (0, 0) and eng.decode_stats(plan)["items"] == 0
        # the same rows through the locate: not found
        two = pb.stored.astype(np.uint8)
        two[5] = 2
        d_two = eng.alloc(n + 8)
        pb.owned.append(d_two)
        eng.upload(d_two, np.concatenate([two, np.full(8, FLAG_GUARD, np.uint8)]))
        got, status = pb.locate([5, 3, 3], [7, 64, 65], d_flags=d_two)
        assert [int(g) for g in got] == [ra.NO_BIT, 8 * (int(pb.offsets[3]) + 64), ra.NO_BIT] and status == ra.LOCATE_NOT_FOUND
        wrong = pb.enc_lens.copy()
        wrong[3] -= 1
        got, status = pb.locate([3, 5], [1, 1], d_lens=pb.upload(wrong))
        assert [int(g) for g in got] == [ra.NO_BIT, 8 * (int(pb.offsets[5]) + 1)] and status == ra.LOCATE_NOT_FOUND
    finally:
        eng.free(d_out)
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        pb.close()
        if coder is not None:
            sc.done(eng, coder)


# ----------------------------------------------------------------------------- 13: plan lifecycle
def run_lifecycle(sc):
    """One decode plan through flagged ranges, unflagged ranges, aws_huffman_amd_decode_plan_reset_packed_stored_input and
    flagged ranges again, against fresh plans' outputs and statistics; the launches that are refused."""
    eng, lib = sc.eng, sc.lib
    rng = np.random.default_rng(1619)
    pb = StoredPackedBatch(sc, eng, sc.lens, sc.w.ocoder, receiver_blobs(rng, 1039), 512, align=1, enc_offset=0)
    plan = eng.empty_decode_plan()
    total = int(sum(b.size for b in pb.blobs))
    d_back, d_back_off = eng.alloc(total + 64), eng.alloc(8 * (pb.n + 1))
    try:
        flagged, size = seeded_ranges(pb, rng, 40)
        coded = [r for r in flagged if not pb.stored[r[0]]]
        by_symbol, size2 = seeded_ranges(pb, rng, 40, symbols=True)

        def fresh(fill, ranges, out_size, symbols, **kw):
            p = eng.empty_decode_plan()
            try:
                assert fill(p, ranges, **kw) == (0, 0)
                return pb.check_launch(p, ranges, out_size, "fresh", symbols)[0], eng.decode_stats(p)
            finally:
                lib.aws_huffman_amd_decode_plan_destroy(p)

        def packed_refused():
            lib.aws_reset_error()
            assert lib.aws_huffman_amd_decode_plan_launch_packed(plan, pb.d_enc, d_back, total, d_back_off, 1, None) == -1
            assert lib.aws_last_error() == fa.AWS_ERROR_INVALID_STATE

        # flagged ranges
        assert pb.reset(plan, flagged) == (0, 0)
        want, stats = fresh(pb.reset, flagged, size, False)
        assert eng.decode_stats(plan) == stats
        assert np.array_equal(pb.check_launch(plan, flagged, size, "first")[0], want)
        packed_refused()
        assert np.array_equal(pb.check_launch(plan, flagged, size, "first, behind the refusal")[0], want)
        # unflagged ranges: the call without flags
        assert pb.reset(plan, coded, d_flags=None) == (0, 0)
        want, stats = fresh(pb.reset, coded, size, False, d_flags=None)
        assert eng.decode_stats(plan) == stats
        assert np.array_equal(pb.check_launch(plan, coded, size, "second")[0], want)
        # the whole batch as a packed input with stored items: a packed launch, and a plain one is refused
        assert sa.reset_stored_input(eng, plan, pb.d_off, None, pb.d_flags, pb.n) == (0, 0)
        lib.aws_reset_error()
        assert lib.aws_huffman_amd_decode_plan_launch(plan, pb.d_enc, d_back, None) == -1
        assert lib.aws_last_error() == fa.AWS_ERROR_INVALID_STATE
        eng.fill(d_back, MARKER, total + 64)
        assert pda.launch_packed(eng, plan, pb.d_enc, d_back, total, d_back_off, 1) == (0, 0)
        assert np.array_equal(eng.download(d_back, total + 64), np.concatenate(pb.blobs + [np.full(64, MARKER, np.uint8)]))
        # flagged ranges again, of symbols
        assert pb.reset_symbols(plan, by_symbol) == (0, 0)
        want, stats = fresh(pb.reset_symbols, by_symbol, size2, True)
        assert eng.decode_stats(plan) == stats
        assert np.array_equal(pb.check_launch(plan, by_symbol, size2, "fourth", True)[0], want)
        packed_refused()
    finally:
        eng.free(d_back)
        eng.free(d_back_off)
        lib.aws_huffman_amd_decode_plan_destroy(plan)
        pb.close()


# ----------------------------------------------------------------------------- 14: the library's face
def header_api_names():
    text = open(HEADER).read()
    return re.findall(r"AWS_COMPRESSION_API\s+[\w\s\*]*?\b(aws_\w+)\s*\(", text)


def run_exports(so_path):
    names = header_api_names()
    assert names == NAMES, names
    listing = subprocess.check_output(["nm", "-D", "--defined-only", so_path], text=True)
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported], [n for n in names if n not in exported]


def run_product_without_a_gpu(product):
    """Against the product library on a machine without a GPU: the four calls raise AWS_ERROR_UNSUPPORTED_OPERATION and touch
    nothing they were handed.  (With a GPU present this has nothing to say: tests/test_gpu_stored_index.py speaks there.)"""
    if product.aws_huffman_amd_device_count() > 0:
        return
    handle = np.full(4096, 0x11, np.uint8)  # (stands for the plan or the engine: there is none without a GPU)
    memory = np.full(8192, 0xEE, np.uint8)
    h, m = handle.ctypes.data, memory.ctypes.data
    calls = [
        lambda: product.aws_huffman_amd_encode_plan_launch_packed_stored_indexed(
            h, m + 1024, m + 4096, 2048, m + 2048, m + 3072, 1, 64, m, m + 512, 8, m + 768, None),
        lambda: product.aws_huffman_amd_decode_plan_reset_stored_item_block_ranges(
            h, m, m + 512, 8, 1, 64, m + 1024, None, m + 3072, 0, 600, m + 2048, 1, None),
        lambda: product.aws_huffman_amd_decode_plan_reset_stored_item_symbol_ranges(
            h, m + 4096, m, m + 512, 8, 1, 64, m + 1024, None, m + 3072, 0, 600, m + 2048, 1, None),
        lambda: product.aws_huffman_amd_locate_stored_item_symbols(
            h, m + 4096, 600, m, m + 512, 8, 1, 64, m + 1024, None, m + 3072, m + 2048, m + 2056, 1, m + 2064, m + 2072, None),
    ]
    for call in calls:
        product.aws_reset_error()
        assert call() == -1
        assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    assert np.all(handle == 0x11) and np.all(memory == 0xEE)
