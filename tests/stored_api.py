"""ctypes face of include/aws/compression/huffman_amd_stored.h (packed batches that store an item raw when its code does not
shrink it) and what its tests share.  Used by tests/test_emulated_stored.py (emulator build) and tests/test_gpu_stored.py
(MI355X): every run_* scenario below is called by both, at the same sizes.

Every expectation comes from the oracle and numpy: L_i from packed_api.encoded_lengths, stored_i = (n_i > 0 and no carried
bits and L_i >= n_i), the offsets from packed_api.expected_offsets, the bytes of a coded item from packed_api.oracle_item,
the bytes of a stored item are the blob.  Nothing here asks the library what it should have done."""
import ctypes as C

import numpy as np

import build_api as ba
import fit_api as fa
import harness
import packed_api as pa
import packed_decode_api as pd
import parity_cases as pc
import plan_counts_api as pk

INVALID = (-1, harness.AWS_ERROR_INVALID_ARGUMENT)
INVALID_STATE = (-1, fa.AWS_ERROR_INVALID_STATE)
SHORT = harness.AWS_ERROR_SHORT_BUFFER
MARKER = pa.MARKER
SEG = pa.SEG
FLAG_GUARD = 0xEE  # what the flags array holds before a launch, and keeps behind its item_count bytes
# the copy's classes: a thread's items (HUFD_TINY_FEW_BYTES 128, HUFD_ENC_TINY_BYTES 512 -- in EDGE_LENGTHS --, HUFD_ENC_TINY_WAVE_BYTES
# 1024, HUFD_TINY_MANY_BYTES 2048), a wave's (HUFD_ENC_SOLO_BYTES 4096), a segment (16384); the receiver's wave / tile limits
# (HUFK_STORED_WAVE_BYTES 4096, HUFK_STORED_TILE_BYTES 16384) and two tiles; each at -1 / 0 / +1
CLASS_LENGTHS = [127, 128, 129, 2047, 2048, 2049, 2 * SEG - 1, 2 * SEG, 2 * SEG + 1]
ALPHABET = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz ", dtype=np.uint8)


def bind(lib):
    """Declares the three entry points of huffman_amd_stored.h (and those of the headers its scenarios call) on a loaded
    library.  The symbols are looked up here: on a build without them every test fails."""
    pk.bind(lib)
    pd.bind(lib)
    V, P = C.c_void_p, C.POINTER
    lib.aws_huffman_amd_encode_plan_launch_packed_stored.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_launch_packed_stored.argtypes = [V, V, V, C.c_uint64, V, V, C.c_uint32, V]
    lib.aws_huffman_amd_encode_plan_stored_size.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_stored_size.argtypes = [V, P(C.c_uint64), P(C.c_uint64), V]
    lib.aws_huffman_amd_decode_plan_reset_packed_stored_input.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_reset_packed_stored_input.argtypes = [V, V, V, V, C.c_size_t, V]
    lib.aws_huffman_amd_decode_plan_launch.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_launch.argtypes = [V, V, V, V]
    return lib


def launch_stored(eng, plan, d_in, d_out, capacity, d_offsets, d_stored, align, stream=None):
    """(rc, error)."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_encode_plan_launch_packed_stored(plan, d_in, d_out, int(capacity), d_offsets, d_stored, align, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def stored_size(eng, plan, stream=None):
    """(rc, error, stored_items, stored_bytes)."""
    items, size = C.c_uint64(), C.c_uint64()
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_encode_plan_stored_size(plan, C.byref(items), C.byref(size), stream)
    return rc, eng.lib.aws_last_error() if rc else 0, items.value, size.value


def reset_stored_input(eng, plan, d_offsets, d_lengths, d_stored, n, stream=None):
    """(rc, error)."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_decode_plan_reset_packed_stored_input(plan, d_offsets, d_lengths, d_stored, n, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def from_encode(eng, dplan, plan):
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_decode_plan_from_encode(dplan, plan, None)
    return rc, eng.lib.aws_last_error() if rc else 0


def words(rng, n):
    """Lowercase words: the test coder gives these symbols 5 to 7 bits."""
    return ALPHABET[rng.integers(0, ALPHABET.size, n)]


# ----------------------------------------------------------------------------- what a stored launch must leave
class Sent:
    """The definition applied to a batch: flags, lengths, offsets, and for a capacity the whole output and every record."""

    def __init__(self, oracle, ocoder, blobs, code_lens, overflows, eoss, align):
        self.oracle, self.ocoder, self.blobs, self.overflows, self.eoss, self.align = oracle, ocoder, blobs, overflows, eoss, align
        self.n = np.asarray([b.size for b in blobs], dtype=np.int64)
        ov = np.asarray([o[1] for o in overflows], dtype=np.int64)
        self.coded = pa.encoded_lengths(code_lens, blobs, ov) if len(blobs) else np.zeros(0, np.int64)
        self.stored = (self.n > 0) & (ov == 0) & (self.coded >= self.n)
        self.lens = np.where(self.stored, self.n, self.coded)
        self.offsets, self.reserved = pa.expected_offsets(self.lens, align)
        self.total = int(self.offsets[-1])
        self.counts = (int(self.stored.sum()), int(self.n[self.stored].sum()))

    def output(self, cap, size):
        """(the `size` bytes of the output, the records) for this capacity."""
        want = np.full(size, MARKER, np.uint8)
        recs = []
        for i, blob in enumerate(self.blobs):
            off = int(self.offsets[i])
            room = max(0, min(int(self.reserved[i]), cap - off))
            if self.stored[i]:
                fit = min(blob.size, room)
                want[off:off + fit] = blob[:fit]
                recs.append((0, 0, fit, fit, 0, 0) if fit == blob.size else (-1, SHORT, fit, fit, 0, 0))
            else:
                rec, data = pa.oracle_item(self.oracle, self.ocoder, blob, self.overflows[i], self.eoss[i], room)
                want[off:off + room] = data
                recs.append(rec)
        return want, recs


class Buffers:
    """Output, offsets and flags of a batch of n items in device memory, refilled with markers before every launch."""

    def __init__(self, eng, n, size, d_in):
        self.eng, self.n, self.size, self.d_in = eng, n, size, d_in
        self.d_out, self.d_off, self.d_flags = eng.alloc(size), eng.alloc(8 * (n + 1)), eng.alloc(n + 8)

    def refill(self):
        self.eng.fill(self.d_out, MARKER, self.size)
        self.eng.fill(self.d_off, 0xEE, 8 * (self.n + 1))
        self.eng.fill(self.d_flags, FLAG_GUARD, self.n + 8)

    def close(self):
        for p in (self.d_out, self.d_off, self.d_flags):
            self.eng.free(p)


def check_sent(eng, plan, sent, bufs, cap, label="", launch=True, stream=None):
    """One stored launch into `bufs` (or, launch False, what is there already) against `sent`: every byte of the output, every
    offset, every flag, every record, the two sizes."""
    n = len(sent.blobs)
    if launch:
        bufs.refill()
        assert launch_stored(eng, plan, bufs.d_in, bufs.d_out, cap, bufs.d_off, bufs.d_flags, sent.align, stream) == (0, 0), label
    got = eng.download(bufs.d_out, bufs.size)
    res = eng.encode_results(plan, n)
    want, recs = sent.output(cap, bufs.size)
    got_offsets = pa.download_u64(eng, bufs.d_off, n + 1)
    assert np.array_equal(got_offsets, sent.offsets), (label, sent.align, int(np.flatnonzero(got_offsets != sent.offsets)[0]))
    flags = eng.download(bufs.d_flags, n + 8)
    assert np.array_equal(flags[:n], sent.stored.astype(np.uint8)), (label, int(np.flatnonzero(flags[:n] != sent.stored)[0]))
    assert np.all(flags[n:] == FLAG_GUARD), (label, "bytes behind the flags were written")
    for i in range(n):
        assert res[i] == recs[i], (label, sent.align, cap, i, bool(sent.stored[i]), int(sent.offsets[i]), res[i], recs[i])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (label, sent.align, cap, "first wrong byte at %d" % int(bad[0]))
    assert pa.packed_size(eng, plan) == (0, 0, sent.total, int(sent.reserved.max()) if n else 0), (label, pa.packed_size(eng, plan))
    assert stored_size(eng, plan) == (0, 0) + sent.counts, (label, stored_size(eng, plan), sent.counts)


def run_launches(sc, eng, plan, d_in, blobs, overflows, eoss, aligns, caps_of=None, label="", code_lens=None, ocoder=None):
    """Stored launches of `plan` at every alignment, at exactly the total and at every capacity caps_of(sent) names."""
    sents = []
    for align in aligns:
        sent = Sent(sc.oracle, ocoder or sc.w.ocoder, blobs, sc.lens if code_lens is None else code_lens, overflows, eoss, align)
        caps = [sent.total] + (caps_of(sent) if caps_of else [])
        bufs = Buffers(eng, len(blobs), max([sent.total] + caps) + 64, d_in)
        try:
            for cap in caps:
                check_sent(eng, plan, sent, bufs, cap, "%s, align %d, capacity %d" % (label, align, cap))
        finally:
            bufs.close()
        sents.append(sent)
    return sents


# ----------------------------------------------------------------------------- 1, 10: the mixed batch, every plan fill
def mixed_blobs(rng):
    lengths = pk.EDGE_LENGTHS + CLASS_LENGTHS
    blobs = [words(rng, n) if i % 2 else pc.inputs(rng, n, "uniform") for i, n in enumerate(lengths)]
    blobs += [pc.inputs(rng, n, "uniform") if i % 2 else words(rng, n) for i, n in enumerate(lengths)]
    blobs += [words(rng, 100_000 + 37), pc.inputs(rng, 100_000 + 41, "uniform")]
    order = rng.permutation(len(blobs))
    return [blobs[i] for i in order]


def run_mixed(sc, fill):
    """Lowercase words and uniform bytes at every edge length, under the test coder: host, strided or device items."""
    eng = sc.eng
    rng = np.random.default_rng(1401)
    d_items = None
    if fill == "strided":
        # equal lengths a stride apart, words and uniform bytes in turn: several segments each, a tail of 77
        in_len, stride, count = 2 * SEG + 77, 2 * SEG + 200, 9
        blobs = [words(rng, in_len) if i % 2 else pc.inputs(rng, in_len, "uniform") for i in range(count)]
        host = pc.inputs(rng, 3 + count * stride + 64, "uniform")
        for i, b in enumerate(blobs):
            host[3 + i * stride:3 + i * stride + in_len] = b
        d_in = eng.alloc(host.size)
        eng.upload(d_in, host)
        plan = eng.plan_strided(True, count=count, in_offset=3, in_stride=stride, in_len=in_len, out_offset=0, out_stride=0,
                                out_capacity=0, first_bit=0, eos_padding=0xFF)
        overflows, eoss, aligns = [(0, 0)] * count, [0xFF] * count, (1, 16)
        close = lambda: eng.free(d_in)
    else:
        blobs = mixed_blobs(rng)
        b = pa.Batch(eng, blobs, rng)
        d_in, overflows, eoss, close = b.d_in, b.overflows, b.eoss, b.close
        if fill == "host":
            plan, aligns = eng.encode_plan(b.items), (1, 16, 4096)
        else:
            (plan, d_items), aligns = eng.encode_plan_from_device_items(b.items), (1, 16)
    try:
        sents = run_launches(sc, eng, plan, d_in, blobs, overflows, eoss, aligns, label="mixed/" + fill)
        sent = sents[0]
        some = int((sent.n > 0).sum())
        assert 4 * int(sent.stored.sum()) >= some and 4 * int(((sent.n > 0) & ~sent.stored).sum()) >= some, (fill, sent.counts, some)
        if fill != "strided":
            stats = eng.encode_stats(plan)
            assert stats["by_thread"] and stats["by_wave"] and stats["by_pieces"] and stats["empty"], stats  # (every kind of unit)
            assert set(sent.n[sent.stored]) >= {1, 15, 16, 17, 512, 4096, 16384, 16385} and sent.n[sent.stored].max() > 100_000
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        if d_items:
            eng.free(d_items)
        close()


# ----------------------------------------------------------------------------- 2: ties
def run_ties(sc):
    """len_i == in_len_i is stored: every non-empty item under a coder of 256 eight-bit codes, and items of the test coder's
    own eight-bit symbols."""
    lib = sc.lib
    rng = np.random.default_rng(1403)
    sizes = [0, 1, 17, 700, 5_000, SEG, 2 * SEG + 9, 64]
    # all lengths 8
    coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*([8] * 256)))
    assert coder
    eng = harness.Engine(lib, coder)
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    b = pa.Batch(eng, blobs, rng)
    plan = eng.encode_plan(b.items)
    try:
        ocoder = fa.oracle_coder(sc.oracle, ba.coder_rows(coder))
        sents = run_launches(sc, eng, plan, b.d_in, blobs, b.overflows, b.eoss, (1, 16), label="len8",
                             code_lens=np.full(256, 8, np.int64), ocoder=ocoder)
        assert np.array_equal(sents[0].stored, sents[0].n > 0) and np.array_equal(sents[0].coded, sents[0].n)
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        eng.close()
        lib.aws_huffman_amd_table_coder_destroy(coder)
    # the test coder's ten eight-bit symbols
    eight = np.flatnonzero(sc.lens == 8).astype(np.uint8)
    assert eight.size == 10
    eng = sc.eng
    blobs = [eight[rng.integers(0, eight.size, n)] for n in sizes] + [words(rng, 300)]
    b = pa.Batch(eng, blobs, rng)
    plan = eng.encode_plan(b.items)
    try:
        sents = run_launches(sc, eng, plan, b.d_in, blobs, b.overflows, b.eoss, (1, 16), label="eight-bit symbols")
        assert np.array_equal(sents[0].stored[:-1], sents[0].n[:-1] > 0) and not sents[0].stored[-1]
        assert np.array_equal(sents[0].coded[:-1], sents[0].n[:-1])
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 3: never stored
def run_never_stored(sc):
    """Items with carried overflow bits, however badly they code, and empty items."""
    eng = sc.eng
    rng = np.random.default_rng(1409)
    sizes = [40, 0, 700, 5_000, 0, SEG + 1, 90, 3, 2_000, 0, 33, 129]
    blobs = [pc.inputs(rng, n, "long") for n in sizes]  # (ten bits a symbol: every one of them would be stored)
    overflows = pa.carried(rng, len(blobs), every=2)
    b = pa.Batch(eng, blobs, rng, overflows=overflows)
    plan = eng.encode_plan(b.items)
    try:
        sents = run_launches(sc, eng, plan, b.d_in, blobs, b.overflows, b.eoss, (1, 16), label="never")
        for i, (blob, ov) in enumerate(zip(blobs, overflows)):
            assert bool(sents[0].stored[i]) == (blob.size > 0 and ov[1] == 0), i
        assert sents[0].stored.any() and (~sents[0].stored & (sents[0].n > 0)).any()
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 4: alignment sweep of the copy
def run_alignment_sweep(sc):
    """Stored items of 1 to 80 bytes and of 4 KiB + k at every source misalignment crossed with every destination
    misalignment (align 1: the destination follows from the lengths in front)."""
    eng = sc.eng
    rng = np.random.default_rng(1411)
    spans, at, dst, seen = [], 0, 0, set()
    lengths = list(range(1, 81)) + [4096 + k for k in range(0, 17)]
    for s in range(16):
        for d in range(16):
            n = lengths[(s * 16 + d) % len(lengths)] if (s + d) % 3 else 4096 + (s + d) % 17
            pad = (d - dst) % 16  # an item of `pad` bytes in front brings the destination to misalignment d
            if pad:
                at = (at + 31) // 16 * 16
                spans.append((at, pad))
                at += pad
                dst += pad
            at = (at + 31) // 16 * 16 + s
            spans.append((at, n))
            seen.add((at % 16, dst % 16))
            at += n
            dst += n
    for n in range(1, 81):  # every short length once more, wherever it falls
        at = (at + 31) // 16 * 16 + n % 16
        spans.append((at, n))
        at += n
    assert len(seen) == 256
    host = pc.inputs(rng, at, "long")
    b = pk.Placed(eng, host, spans)
    plan = eng.encode_plan(b.items)
    n = len(spans)
    try:
        sents = run_launches(sc, eng, plan, b.d_in, b.blobs, [(0, 0)] * n, [0xFF] * n, (1,), label="alignment sweep")
        assert sents[0].stored.all() and {(o % 16, int(x) % 16) for (o, _), x in zip(spans, sents[0].offsets)} >= seen
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 5: capacity clipping
def run_capacity_clipping(sc, aligns=(1, 16)):
    """The edge inside a stored item, at its first byte, one byte behind its last, and inside a coded item that stored ones
    follow."""
    eng = sc.eng
    rng = np.random.default_rng(1413)
    kinds = ["w", "u", "u", "w", "u", "w", "u", "u", "w", "u", "u"]
    sizes = [40, 700, 0, 5_000, 2 * SEG + 500, 300, 90, SEG + 1, 3 * SEG, 17, 4097]
    blobs = [words(rng, n) if k == "w" else pc.inputs(rng, n, "uniform") for k, n in zip(kinds, sizes)]
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
        sents = run_launches(sc, eng, plan, b.d_in, blobs, b.overflows, b.eoss, aligns, caps_of=caps_of, label="clip")
        s = sents[0].stored
        assert s[1] and s[4] and s[6] and s[7] and s[9] and s[10] and not (s[0] or s[3] or s[5] or s[8]), s
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 6: scan boundaries
def run_scan_boundaries(sc, tile, counts):
    """The offset scan in tiles of a few items (packed_api.SCAN_TILES), stored and coded items mixed."""
    eng = sc.eng
    rng = np.random.default_rng(1417 + tile)
    most = max(counts)
    sizes = rng.integers(1, 40, most)
    blobs = [words(rng, int(n)) if i % 3 else pc.inputs(rng, int(n), "uniform") for i, n in enumerate(sizes)]
    b = pa.Batch(eng, blobs, None, overflows=pa.carried(rng, most, every=5))
    try:
        with pa.pack_tile_items(sc.lib, tile):
            for n in counts:
                plan = eng.encode_plan(b.items[:n])
                try:
                    for align in (1, 16):
                        sent = Sent(sc.oracle, sc.w.ocoder, blobs[:n], sc.lens, b.overflows[:n], b.eoss[:n], align)
                        assert sent.stored.any() and not sent.stored.all()
                        bufs = Buffers(eng, n, sent.total + 64, b.d_in)
                        try:
                            bufs.refill()
                            assert launch_stored(eng, plan, b.d_in, bufs.d_out, sent.total, bufs.d_off, bufs.d_flags, align) == (0, 0)
                            label = "tile %d, %d items, align %d" % (tile, n, align)
                            assert np.array_equal(pa.download_u64(eng, bufs.d_off, n + 1), sent.offsets), label
                            flags = eng.download(bufs.d_flags, n + 8)
                            assert np.array_equal(flags[:n], sent.stored.astype(np.uint8)) and np.all(flags[n:] == FLAG_GUARD), label
                            assert pa.packed_size(eng, plan) == (0, 0, sent.total, int(sent.reserved.max())), label
                            assert stored_size(eng, plan) == (0, 0) + sent.counts, label
                            # the stored items' bytes and records whole (numpy), a sample of the coded ones (the oracle)
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
                            # nothing in an alignment gap or behind the total: every byte no item owns keeps the marker
                            owned = np.zeros(bufs.size, bool)
                            ends = sent.offsets[:-1] + sent.lens
                            edges = np.zeros(bufs.size + 1, np.int64)
                            np.add.at(edges, sent.offsets[:-1], 1)
                            np.add.at(edges, ends, -1)
                            owned = np.cumsum(edges)[:-1] > 0
                            assert np.all(got[~owned] == MARKER) and not owned[sent.total:].any(), label
                        finally:
                            bufs.close()
                finally:
                    sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
    finally:
        sc.lib.aws_huffman_amd_testing_set_pack_tile_items(0)
        b.close()


# ----------------------------------------------------------------------------- 7: round trip
class Received:
    """What the receiver must make of a sender's output: sym_i (the oracle's for a coded item, the length for a stored one),
    offsets from them, and for a capacity the whole output and every record."""

    def __init__(self, sc, sent, ocoder=None, min_bits=None):
        self.sent = sent
        n = len(sent.blobs)
        streams = []
        for i, blob in enumerate(sent.blobs):
            if sent.stored[i]:
                streams.append((blob, 0))
            else:
                rec, data = pa.oracle_item(sent.oracle, sent.ocoder, blob, sent.overflows[i], sent.eoss[i], int(sent.lens[i]))
                assert rec[:2] == (0, 0) and rec[3] == sent.lens[i], (i, rec)
                streams.append((data.copy(), 0))
        coded = [i for i in range(n) if not sent.stored[i]]
        self.expect = pd.Expect(sent.oracle, ocoder or sent.ocoder, streams, min_bits or sc.min_bits, only=coded)
        self.syms = np.asarray([sent.n[i] if sent.stored[i] else self.expect.full[i][0][2] for i in range(n)], dtype=np.int64)
        self.offsets, self.reserved = pa.expected_offsets(self.syms, 1)
        self.total = int(self.offsets[-1])

    def output(self, cap, size):
        want = np.full(size, MARKER, np.uint8)
        room = pd.rooms(self.offsets, self.syms, cap)
        recs = []
        for i, blob in enumerate(self.sent.blobs):
            off = int(self.offsets[i])
            if self.sent.stored[i]:
                fits = room[i] == blob.size
                if fits:
                    want[off:off + blob.size] = blob
                recs.append((0, 0, blob.size, 8 * blob.size) if fits else (-1, SHORT, 0, 0))
            else:
                rec, data = self.expect.item(i, int(room[i]))
                want[off:off + int(room[i])] = data
                recs.append(rec)
        return want, recs


def check_received(eng, dplan, d_in, recv, cap, d_back, d_back_off, size, label="", launch=True, stream=None):
    n = len(recv.sent.blobs)
    if launch:
        eng.fill(d_back, MARKER, size)
        eng.fill(d_back_off, 0xEE, 8 * (n + 1))
        assert pd.launch_packed(eng, dplan, d_in, d_back, cap, d_back_off, 1, stream) == (0, 0), label
    got = eng.download(d_back, size)
    res = eng.decode_results(dplan, n)
    want, recs = recv.output(cap, size)
    got_offsets = pa.download_u64(eng, d_back_off, n + 1)
    assert np.array_equal(got_offsets, recv.offsets), (label, int(np.flatnonzero(got_offsets != recv.offsets)[0]))
    for i in range(n):
        assert res[i] == recs[i], (label, cap, i, bool(recv.sent.stored[i]), res[i], recs[i])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (label, cap, "first wrong byte at %d" % int(bad[0]))
    assert pd.packed_size(eng, dplan) == (0, 0, recv.total, int(recv.reserved.max()) if n else 0), (label, pd.packed_size(eng, dplan))


def round_trip_blobs(rng):
    sizes = [70_000, 300, 0, 20_000, SEG, 1, 140_000, 900, 4095, 4096, 100_000, 17, 2 * SEG + 1, 40]
    kinds = ["u", "w", "u", "w", "u", "u", "w", "u", "u", "u", "u", "w", "u", "u"]
    return [words(rng, n) if k == "w" else pc.inputs(rng, n, "uniform") for k, n in zip(kinds, sizes)]


def run_round_trip(sc, align=1, graphs=None, with_lengths=False):
    """The sender's three arrays straight into the receiver's reset, a size query, a launch, a clipped launch; `graphs`
    (packed_api.HipGraphs): both launches once more from captured graphs."""
    eng = sc.eng
    rng = np.random.default_rng(1419)
    blobs = round_trip_blobs(rng)
    n = len(blobs)
    b = pa.Batch(eng, blobs, rng, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    dplan = eng.empty_decode_plan()
    sent = Sent(sc.oracle, sc.w.ocoder, blobs, sc.lens, b.overflows, b.eoss, align)
    recv = Received(sc, sent)
    assert sent.stored.sum() >= 4 and (~sent.stored & (sent.n > 0)).sum() >= 4
    assert np.array_equal(recv.syms, sent.n)
    bufs = Buffers(eng, n, sent.total + 64, b.d_in)
    size = recv.total + 64
    d_back, d_back_off, d_lens = eng.alloc(size), eng.alloc(8 * (n + 1)), None
    stream = C.c_void_p(eng.stream) if graphs else None
    execs = []
    try:
        check_sent(eng, plan, sent, bufs, sent.total, "round trip, sender", stream=stream)
        if with_lengths or align > 1:  # (an alignment leaves gaps: the receiver needs the lengths, as for any packed buffer)
            d_lens = pd.upload_u64(eng, sent.lens)
        assert reset_stored_input(eng, dplan, bufs.d_off, d_lens, bufs.d_flags, n) == (0, 0)
        # a size query
        eng.fill(d_back_off, 0xEE, 8 * (n + 1))
        assert pd.launch_packed(eng, dplan, bufs.d_out, None, 0, d_back_off, 1, stream) == (0, 0)
        assert pd.packed_size(eng, dplan)[:3] == (0, 0, recv.total)
        assert np.array_equal(pa.download_u64(eng, d_back_off, n + 1), recv.offsets)
        check_received(eng, dplan, bufs.d_out, recv, recv.total, d_back, d_back_off, size, "round trip", stream=stream)
        clipped = [int(recv.offsets[6]) + 5, int(recv.offsets[10]), int(recv.offsets[10] + recv.syms[10]) - 1, 0]
        for cap in clipped:
            check_received(eng, dplan, bufs.d_out, recv, cap, d_back, d_back_off, size, "round trip, clipped", stream=stream)
        if graphs:
            graphs.call("hipStreamSynchronize", stream)
            execs.append(graphs.capture(stream, lambda: launch_stored(
                eng, plan, b.d_in, bufs.d_out, sent.total, bufs.d_off, bufs.d_flags, align, stream)))
            execs.append(graphs.capture(stream, lambda: pd.launch_packed(
                eng, dplan, bufs.d_out, d_back, recv.total, d_back_off, 1, stream)))
            bufs.refill()
            eng.fill(d_back, MARKER, size)
            eng.fill(d_back_off, 0xEE, 8 * (n + 1))
            eng.sync()
            for g in execs:
                graphs.call("hipGraphLaunch", g, stream)
            graphs.call("hipStreamSynchronize", stream)
            check_sent(eng, plan, sent, bufs, sent.total, "replayed sender", launch=False)
            check_received(eng, dplan, bufs.d_out, recv, recv.total, d_back, d_back_off, size, "replayed receiver", launch=False)
    finally:
        for g in execs:
            graphs.call("hipGraphExecDestroy", g)
        for p in (d_back, d_back_off) + ((d_lens,) if d_lens else ()):
            eng.free(p)
        bufs.close()
        sc.lib.aws_huffman_amd_decode_plan_destroy(dplan)
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 8: the receiver's checks, the two INVALID_STATE arms
def run_receiver_checks(sc):
    eng = sc.eng
    lib = sc.lib
    rng = np.random.default_rng(1421)
    blobs = [pc.inputs(rng, 300, "uniform"), words(rng, 5_000), pc.inputs(rng, 20_000, "uniform"), words(rng, 40)]
    n = len(blobs)
    b = pa.Batch(eng, blobs, rng, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    dplan, other = eng.empty_decode_plan(), eng.empty_decode_plan()
    sent = Sent(sc.oracle, sc.w.ocoder, blobs, sc.lens, b.overflows, b.eoss, 1)
    bufs = Buffers(eng, n, sent.total + 64, b.d_in)
    d_back, d_back_off = eng.alloc(sum(x.size for x in blobs) + 64), eng.alloc(8 * (n + 1))
    d_bad = eng.alloc(n)
    try:
        # argument checks of the sender
        assert launch_stored(eng, plan, b.d_in, bufs.d_out, sent.total, bufs.d_off, None, 1) == INVALID
        assert launch_stored(eng, plan, b.d_in, bufs.d_out, sent.total, None, bufs.d_flags, 1) == INVALID
        assert launch_stored(eng, plan, b.d_in, bufs.d_out, sent.total, bufs.d_off, bufs.d_flags, 3) == INVALID
        assert stored_size(eng, plan)[:2] == INVALID  # (no stored launch yet)
        check_sent(eng, plan, sent, bufs, sent.total, "checks, sender")
        assert list(sent.stored) == [True, False, True, False]
        # aws_huffman_amd_decode_plan_from_encode behind a stored launch
        assert from_encode(eng, dplan, plan) == INVALID_STATE
        # a flag byte of 2
        flags = sent.stored.astype(np.uint8)
        flags[1] = 2
        eng.upload(d_bad, flags)
        assert reset_stored_input(eng, dplan, bufs.d_off, None, d_bad, n) == INVALID
        assert eng.decode_stats(dplan)["items"] == 0
        # NULL flags: the plan aws_huffman_amd_decode_plan_reset_packed_input leaves
        assert reset_stored_input(eng, dplan, bufs.d_off, None, None, n) == (0, 0)
        assert pd.reset_packed_input(eng, other, bufs.d_off, None, n) == (0, 0)
        assert eng.decode_stats(dplan) == eng.decode_stats(other) and eng.decode_stats(dplan)["items"] == n
        assert lib.aws_huffman_amd_decode_plan_launch(dplan, bufs.d_out, d_back, None) == 0  # (a plain launch is its right)
        eng.decode_results(dplan, n)
        # a plain launch of a flagged plan
        assert reset_stored_input(eng, dplan, bufs.d_off, None, bufs.d_flags, n) == (0, 0)
        lib.aws_reset_error()
        assert lib.aws_huffman_amd_decode_plan_launch(dplan, bufs.d_out, d_back, None) == -1
        assert lib.aws_last_error() == fa.AWS_ERROR_INVALID_STATE
        recv = Received(sc, sent)
        check_received(eng, dplan, bufs.d_out, recv, recv.total, d_back, d_back_off, recv.total + 64, "checks, receiver")
        # a later plain packed launch of the same encode plan clears the state and behaves as before
        pa.check_launch(sc.oracle, sc.w.ocoder, eng, plan, b.d_in, blobs, sc.lens, b.overflows, b.eoss, 1, label="packed again")
        assert stored_size(eng, plan)[:2] == INVALID
        d_out, d_off = eng.alloc(2 * sum(x.size for x in blobs) + 64), eng.alloc(8 * (n + 1))
        try:
            assert pa.launch_packed(eng, plan, b.d_in, d_out, 2 * sum(x.size for x in blobs), d_off, 1) == (0, 0)
            assert from_encode(eng, dplan, plan) == (0, 0)
            eng.fill(d_back, MARKER, sum(x.size for x in blobs) + 64)
            assert lib.aws_huffman_amd_decode_plan_launch(dplan, d_out, d_back, None) == 0
            assert all(r[:3] == (0, 0, x.size) for r, x in zip(eng.decode_results(dplan, n), blobs))
        finally:
            eng.free(d_out)
            eng.free(d_off)
        # an empty plan: offsets[0] = 0 and nothing else
        empty = eng.empty_encode_plan()
        bufs.refill()
        assert launch_stored(eng, empty, b.d_in, bufs.d_out, sent.total, bufs.d_off, bufs.d_flags, 1) == (0, 0)
        off = eng.download(bufs.d_off, 16).view(np.uint64)
        assert off[0] == 0 and off[1] == 0xEEEEEEEEEEEEEEEE
        assert np.all(eng.download(bufs.d_flags, n + 8) == FLAG_GUARD) and np.all(eng.download(bufs.d_out, bufs.size) == MARKER)
        assert stored_size(eng, empty) == (0, 0, 0, 0)
        lib.aws_huffman_amd_encode_plan_destroy(empty)
    finally:
        for p in (d_back, d_back_off, d_bad):
            eng.free(p)
        bufs.close()
        lib.aws_huffman_amd_decode_plan_destroy(dplan)
        lib.aws_huffman_amd_decode_plan_destroy(other)
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 9: a fitted engine
def run_fitted(sc, memset_async):
    """count -> fit -> stored launch on one stream, nothing waited for in between, over text with a few binary items: the
    fitted code is the host's for the data's counts, and the binary items are stored.  memset_async(eng, dptr, size, stream)
    clears the counts in stream order."""
    lib = sc.lib
    rng = np.random.default_rng(1423)
    sizes = [3_000, 40_000, 700, 20_000, 90, SEG + 5, 5_000, 300, 2_000, 60_000]
    binary = {2, 5, 8}
    blobs = [pc.inputs(rng, n, "uniform") if i in binary else harness.printable_map(rng.integers(0, 256, n, dtype=np.uint8))
             for i, n in enumerate(sizes)]
    n = len(blobs)
    eng = fa.FittedEngine(lib, 4, 12)
    b = pa.Batch(eng, blobs, None, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    capacity = 2 * sum(sizes)
    bufs = Buffers(eng, n, capacity + 64, b.d_in)
    stream = C.c_void_p(eng.stream)
    try:
        bufs.refill()
        eng.fill(eng.d_status, 0xEE, 4)
        memset_async(eng, eng.d_counts, 256 * 8, stream)
        assert pk.plan_counts(eng, plan, b.d_in, eng.d_counts, stream) == (0, 0)
        assert eng.fit_counts_async(None, stream) == (0, 0)
        assert launch_stored(eng, plan, b.d_in, bufs.d_out, capacity, bufs.d_off, bufs.d_flags, 1, stream) == (0, 0)
        assert lib.aws_huffman_amd_stream_synchronize(eng.h, stream) == 0
        assert eng.status() == fa.FIT_OK
        lengths = fa.host_lengths(lib, ba.bincount(np.concatenate(blobs)), eng.lo, eng.hi)
        assert eng.bits() == lengths
        ocoder = fa.oracle_coder(sc.oracle, fa.host_rows(lib, lengths))
        sent = Sent(sc.oracle, ocoder, blobs, np.asarray(lengths, dtype=np.int64), b.overflows, b.eoss, 1)
        assert set(np.flatnonzero(sent.stored)) == binary, (np.flatnonzero(sent.stored), sent.coded, sent.n)
        check_sent(eng, plan, sent, bufs, capacity, "fitted", launch=False)
    finally:
        bufs.close()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        eng.close()


# ----------------------------------------------------------------------------- the library's face
def run_exports(so_path):
    """The shared library exports the three new entry points."""
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", so_path], capture_output=True, text=True, check=True).stdout
    for name in ("aws_huffman_amd_encode_plan_launch_packed_stored", "aws_huffman_amd_encode_plan_stored_size",
                 "aws_huffman_amd_decode_plan_reset_packed_stored_input"):
        assert (" T " + name + "\n") in out, name
