"""ctypes face of include/aws/compression/huffman_amd_constant.h (packed batches that keep an item of one repeated byte as
its length and that byte) and what its tests share.  Used by tests/test_emulated_constant.py (emulator build) and
tests/test_gpu_constant.py (MI355X): every run_* scenario below is called by both, at the same sizes.

Every expectation comes from the oracle and numpy: L_i from packed_api.encoded_lengths; constant_i = (no carried bits and
n_i > 9 and L_i > 9 and every byte the first); stored_i = the rule of stored_api.Sent where the item is not constant; the
offsets from packed_api.expected_offsets; the bytes of a coded item from packed_api.oracle_item, of a stored item the blob, of
a constant item n_i as 8 little-endian bytes and the value.  Nothing here asks the library what it should have done."""
import ctypes as C

import numpy as np

import build_api as ba
import fit_api as fa
import harness
import packed_api as pa
import packed_decode_api as pd
import parity_cases as pc
import plan_counts_api as pk
import stored_api as sa

INVALID = sa.INVALID
INVALID_STATE = sa.INVALID_STATE
SHORT = sa.SHORT
MARKER = pa.MARKER
SEG = pa.SEG
KIND_GUARD = sa.FLAG_GUARD
CODED, STORED, CONSTANT = 0, 1, 2
HEAD = 9  # AWS_HUFFMAN_AMD_CONSTANT_BYTES
MAX_COUNT = 1 << 32  # AWS_HUFFMAN_AMD_CONSTANT_MAX_COUNT
# the rule's own bounds, the classes of the copy and the detection (stored_api.CLASS_LENGTHS), segments at -1 / +1, five segments
RULE_LENGTHS = [0, 1, 9, 10, 11, 16, 17] + sa.CLASS_LENGTHS + [SEG - 1, SEG + 1, 2 * SEG - 1, 2 * SEG + 1, 5 * SEG + 3]


def bind(lib):
    """Declares the four entry points of huffman_amd_constant.h (and those of the headers its scenarios call) on a loaded
    library.  The symbols are looked up here: on a build without them every test fails."""
    sa.bind(lib)
    V, P = C.c_void_p, C.POINTER
    lib.aws_huffman_amd_encode_plan_launch_packed_constant.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_launch_packed_constant.argtypes = [V, V, V, C.c_uint64, V, V, C.c_uint32, V]
    lib.aws_huffman_amd_encode_plan_constant_size.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_constant_size.argtypes = [V, P(C.c_uint64), P(C.c_uint64), V]
    lib.aws_huffman_amd_decode_plan_reset_packed_constant_input.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_reset_packed_constant_input.argtypes = [V, V, V, V, V, C.c_size_t, V]
    return lib


def launch_constant(eng, plan, d_in, d_out, capacity, d_offsets, d_kinds, align, stream=None):
    """(rc, error)."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_encode_plan_launch_packed_constant(plan, d_in, d_out, int(capacity), d_offsets, d_kinds, align, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def constant_size(eng, plan, stream=None):
    """(rc, error, constant_items, constant_bytes)."""
    items, size = C.c_uint64(), C.c_uint64()
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_encode_plan_constant_size(plan, C.byref(items), C.byref(size), stream)
    return rc, eng.lib.aws_last_error() if rc else 0, items.value, size.value


def reset_constant_input(eng, plan, d_packed, d_offsets, d_lengths, d_kinds, n, stream=None):
    """(rc, error)."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_decode_plan_reset_packed_constant_input(plan, d_packed, d_offsets, d_lengths, d_kinds, n, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def head(n, value):
    """The 9 bytes of a constant item."""
    return np.concatenate([np.frombuffer(int(n).to_bytes(8, "little"), np.uint8), np.asarray([value], np.uint8)])


def run_of(value, n):
    return np.full(n, value, np.uint8)


# ----------------------------------------------------------------------------- what a constant launch must leave
class Sent:
    """The definition applied to a batch: kinds, lengths, offsets, and for a capacity the whole output and every record."""

    def __init__(self, oracle, ocoder, blobs, code_lens, overflows, eoss, align):
        self.oracle, self.ocoder, self.blobs, self.overflows, self.eoss, self.align = oracle, ocoder, blobs, overflows, eoss, align
        self.n = np.asarray([b.size for b in blobs], dtype=np.int64)
        ov = np.asarray([o[1] for o in overflows], dtype=np.int64)
        self.coded = pa.encoded_lengths(code_lens, blobs, ov) if len(blobs) else np.zeros(0, np.int64)
        same = np.asarray([bool(b.size) and bool(np.all(b == b[0])) for b in blobs], dtype=bool)
        self.constant = (ov == 0) & (self.n > HEAD) & (self.coded > HEAD) & same
        self.stored = (self.n > 0) & (ov == 0) & (self.coded >= self.n) & ~self.constant
        self.kinds = (2 * self.constant + self.stored).astype(np.uint8)
        self.lens = np.where(self.constant, HEAD, np.where(self.stored, self.n, self.coded))
        self.offsets, self.reserved = pa.expected_offsets(self.lens, align)
        self.total = int(self.offsets[-1])
        self.counts = (int(self.stored.sum()), int(self.n[self.stored].sum()))
        self.constant_counts = (int(self.constant.sum()), int(self.n[self.constant].sum()))

    def output(self, cap, size):
        """(the `size` bytes of the output, the records) for this capacity."""
        want = np.full(size, MARKER, np.uint8)
        recs = []
        for i, blob in enumerate(self.blobs):
            off = int(self.offsets[i])
            room = max(0, min(int(self.reserved[i]), cap - off))
            if self.constant[i]:
                if cap - off >= HEAD:
                    want[off:off + HEAD] = head(blob.size, blob[0])
                    recs.append((0, 0, blob.size, HEAD, 0, 0))
                else:
                    recs.append((-1, SHORT, 0, 0, 0, 0))
            elif self.stored[i]:
                fit = min(blob.size, room)
                want[off:off + fit] = blob[:fit]
                recs.append((0, 0, fit, fit, 0, 0) if fit == blob.size else (-1, SHORT, fit, fit, 0, 0))
            else:
                rec, data = pa.oracle_item(self.oracle, self.ocoder, blob, self.overflows[i], self.eoss[i], room)
                want[off:off + room] = data
                recs.append(rec)
        return want, recs


def check_sent(eng, plan, sent, bufs, cap, label="", launch=True, stream=None):
    """One constant launch into `bufs` (stored_api.Buffers; or, launch False, what is there already) against `sent`: every
    byte of the output, every offset, every kind and the guard behind them, every record, the three sizes."""
    n = len(sent.blobs)
    if launch:
        bufs.refill()
        assert launch_constant(eng, plan, bufs.d_in, bufs.d_out, cap, bufs.d_off, bufs.d_flags, sent.align, stream) == (0, 0), label
    got = eng.download(bufs.d_out, bufs.size)
    res = eng.encode_results(plan, n)
    want, recs = sent.output(cap, bufs.size)
    got_offsets = pa.download_u64(eng, bufs.d_off, n + 1)
    assert np.array_equal(got_offsets, sent.offsets), (label, sent.align, int(np.flatnonzero(got_offsets != sent.offsets)[0]))
    kinds = eng.download(bufs.d_flags, n + 8)
    assert np.array_equal(kinds[:n], sent.kinds), (label, int(np.flatnonzero(kinds[:n] != sent.kinds)[0]), kinds[:n], sent.kinds)
    assert np.all(kinds[n:] == KIND_GUARD), (label, "bytes behind the kinds were written")
    for i in range(n):
        assert res[i] == recs[i], (label, sent.align, cap, i, int(sent.kinds[i]), int(sent.offsets[i]), res[i], recs[i])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (label, sent.align, cap, "first wrong byte at %d" % int(bad[0]))
    assert pa.packed_size(eng, plan) == (0, 0, sent.total, int(sent.reserved.max()) if n else 0), (label, pa.packed_size(eng, plan))
    assert sa.stored_size(eng, plan) == (0, 0) + sent.counts, (label, sa.stored_size(eng, plan), sent.counts)
    assert constant_size(eng, plan) == (0, 0) + sent.constant_counts, (label, constant_size(eng, plan), sent.constant_counts)


def run_launches(sc, eng, plan, d_in, blobs, overflows, eoss, aligns, caps_of=None, label="", code_lens=None, ocoder=None):
    """Constant launches of `plan` at every alignment, at exactly the total and at every capacity caps_of(sent) names."""
    sents = []
    for align in aligns:
        sent = Sent(sc.oracle, ocoder or sc.w.ocoder, blobs, sc.lens if code_lens is None else code_lens, overflows, eoss, align)
        caps = [sent.total] + (caps_of(sent) if caps_of else [])
        bufs = sa.Buffers(eng, len(blobs), max([sent.total] + caps) + 64, d_in)
        try:
            for cap in caps:
                check_sent(eng, plan, sent, bufs, cap, "%s, align %d, capacity %d" % (label, align, cap))
        finally:
            bufs.close()
        sents.append(sent)
    return sents


def placed(eng, rng, blobs, starts=None):
    """The blobs in one input allocation, item i at a source offset of starts[i] mod 16 (default: i mod 16), a guard of other
    bytes around each: an item read past either end would not look constant."""
    spans, at = [], 0
    for i, b in enumerate(blobs):
        s = (starts[i] if starts else i) % 16
        at = (at + 31) // 16 * 16 + s
        spans.append((at, b.size))
        at += b.size
    host = pc.inputs(rng, at + 16, "long")
    for (o, n), b in zip(spans, blobs):
        host[o:o + n] = b
        for g in (o - 1, o + n):  # (the byte on either side differs from the item's)
            if 0 <= g < host.size and n and not any(so <= g < so + sn for so, sn in spans):
                host[g] = b[0] ^ 0x5A
    return pk.Placed(eng, host, spans)


def longest_code(sc):
    return int(np.argmax(sc.lens))


# ----------------------------------------------------------------------------- 1: the rule's bounds, starts, values
def run_rule_boundaries(sc):
    """Constant items of every length of RULE_LENGTHS, of 0x00, 0xFF and the byte with the coder's longest code, every source
    start 0 .. 15 mod 16."""
    eng = sc.eng
    rng = np.random.default_rng(1501)
    values = [0x00, 0xFF, longest_code(sc)]
    blobs, starts = [], []
    for r, value in enumerate(values):
        for k, n in enumerate(RULE_LENGTHS):
            blobs.append(run_of(value, n))
            starts.append(5 * k + 7 * r)
    assert {s % 16 for s, b in zip(starts, blobs) if b.size > HEAD} == set(range(16))
    b = placed(eng, rng, blobs, starts)
    plan = eng.encode_plan(b.items)
    n = len(blobs)
    try:
        sents = run_launches(sc, eng, plan, b.d_in, b.blobs, [(0, 0)] * n, [0xFF] * n, (1, 16), label="rule")
        s = sents[0]
        assert not s.constant[s.n <= HEAD].any() and s.constant[s.n >= 16].all(), (s.n, s.kinds)
        assert {int(x) % 16 for x in s.offsets[:-1][s.constant]} == set(range(16))  # (the 9 bytes at every destination too)
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 2: one byte changed
def changed_blobs(sc):
    """Constant items with one byte changed: the first, the last, 15, 16, SEG - 1, SEG, and the last byte of the last segment
    (= the last), wherever the item has that position."""
    blobs = []
    for k, n in enumerate([17, 129, 2049, SEG, SEG + 1, 2 * SEG + 1, 5 * SEG + 3]):
        for pos in sorted({0, n - 1, 15, 16, SEG - 1, SEG} & set(range(n))):
            value = [0x00, 0x61, longest_code(sc)][(k + pos) % 3]  # (a byte with a short code among them: coded, not stored)
            blob = run_of(value, n)
            blob[pos] ^= 0x01 if pos % 2 else 0x80
            blobs.append(blob)
    return blobs


def run_one_byte_changed(sc):
    """Each comes out stored or coded by the old rule, bit for bit what aws_huffman_amd_encode_plan_launch_packed_stored gives."""
    eng = sc.eng
    rng = np.random.default_rng(1503)
    blobs = changed_blobs(sc)
    n = len(blobs)
    b = placed(eng, rng, blobs)
    plan = eng.encode_plan(b.items)
    try:
        for align in (1, 16):
            sent = Sent(sc.oracle, sc.w.ocoder, b.blobs, sc.lens, [(0, 0)] * n, [0xFF] * n, align)
            old = sa.Sent(sc.oracle, sc.w.ocoder, b.blobs, sc.lens, [(0, 0)] * n, [0xFF] * n, align)
            assert not sent.constant.any() and np.array_equal(sent.stored, old.stored) and sent.total == old.total
            assert sent.stored.any() and not sent.stored.all()
            ours, theirs = sa.Buffers(eng, n, sent.total + 64, b.d_in), sa.Buffers(eng, n, sent.total + 64, b.d_in)
            try:
                sa.check_sent(eng, plan, old, theirs, old.total, "changed, stored launch")
                want = (eng.download(theirs.d_out, theirs.size), eng.download(theirs.d_off, 8 * (n + 1)),
                        eng.download(theirs.d_flags, n + 8), eng.encode_results(plan, n))
                check_sent(eng, plan, sent, ours, sent.total, "changed, constant launch")
                got = (eng.download(ours.d_out, ours.size), eng.download(ours.d_off, 8 * (n + 1)),
                       eng.download(ours.d_flags, n + 8), eng.encode_results(plan, n))
                assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3] == want[3]
            finally:
                ours.close()
                theirs.close()
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 3: coders
def run_one_bit_value(sc):
    """A table coder whose value byte has a 1-bit code: an item of 10 to 72 such bytes has len_i <= 9 and is coded; from 73 on
    it is constant."""
    lib = sc.lib
    rng = np.random.default_rng(1507)
    value = 0x41
    lengths = [10] * 256  # a complete code: 1/2 + 1/4 + 2/512 + 252/1024 = 1
    lengths[value], lengths[0x42], lengths[0x43], lengths[0x44] = 1, 2, 9, 9
    coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*lengths))
    assert coder
    eng = harness.Engine(lib, coder)
    sizes = [9, 10, 11, 64, 72, 73, 80, 200, 5_000]
    blobs = [run_of(value, n) for n in sizes] + [run_of(0x42, 36), run_of(0x42, 37), run_of(0x00, 10)]
    n = len(blobs)
    b = placed(eng, rng, blobs)
    plan = eng.encode_plan(b.items)
    try:
        ocoder = fa.oracle_coder(sc.oracle, ba.coder_rows(coder))
        sents = run_launches(sc, eng, plan, b.d_in, b.blobs, [(0, 0)] * n, [0xFF] * n, (1, 16), label="one-bit value",
                             code_lens=np.asarray(lengths, np.int64), ocoder=ocoder)
        assert list(sents[0].kinds) == [CODED] * 5 + [CONSTANT] * 4 + [CODED, CONSTANT, CONSTANT], sents[0].kinds
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        eng.close()
        lib.aws_huffman_amd_table_coder_destroy(coder)


def run_hole_at_the_value(sc):
    """A coder without a code for the value: the symbol counts 0 bits, so len_i is 0 and the item is never constant."""
    rng = np.random.default_rng(1509)
    blobs = [run_of(7, 40), run_of(200, 5_000), run_of(8, 40), run_of(7, SEG + 9), sa.words(rng, 300), run_of(201, 5_000)]
    n = len(blobs)
    eng, coder = sc.engine(holes=True)
    b = placed(eng, rng, blobs)
    plan = eng.encode_plan(b.items)
    try:
        sents = run_launches(sc, eng, plan, b.d_in, b.blobs, [(0, 0)] * n, [0xFF] * n, (1, 16), label="hole",
                             code_lens=sc.lens_holes, ocoder=sc.w.ocoder_holes)
        assert list(sents[0].kinds) == [CODED, CODED, CONSTANT, CODED, CODED, CONSTANT], sents[0].kinds
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        sc.done(eng, coder)


# ----------------------------------------------------------------------------- 4: carried bits
def run_carried_bits(sc):
    """An item that carries overflow bits in is never constant (and never stored)."""
    eng = sc.eng
    rng = np.random.default_rng(1511)
    sizes = [40, 0, 700, 5_000, 10, SEG + 1, 90, 17, 2_000, 3 * SEG, 33, 129]
    blobs = [run_of([0x00, 0xFF, 0x61][i % 3], n) for i, n in enumerate(sizes)]
    overflows = pa.carried(rng, len(blobs), every=2)
    b = pa.Batch(eng, blobs, rng, overflows=overflows)
    plan = eng.encode_plan(b.items)
    try:
        sents = run_launches(sc, eng, plan, b.d_in, blobs, b.overflows, b.eoss, (1, 16), label="carried")
        for i, (blob, ov) in enumerate(zip(blobs, overflows)):
            assert bool(sents[0].constant[i]) == (blob.size > HEAD and ov[1] == 0), i
        assert sents[0].constant.any() and (~sents[0].constant & (sents[0].n > HEAD)).any()
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 5: the mixed batch, every fill, every road
def mixed_blobs(rng):
    """Words, uniform bytes and runs of one byte at the edge lengths, shuffled: all three kinds of every class of unit."""
    lengths = pk.EDGE_LENGTHS + sa.CLASS_LENGTHS
    makers = [lambda n: sa.words(rng, n), lambda n: pc.inputs(rng, n, "uniform"), lambda n: run_of(int(rng.integers(0, 256)), n)]
    blobs = [makers[(i + r) % 3](n) for r in range(3) for i, n in enumerate(lengths)]
    blobs += [sa.words(rng, 70_000 + 37), pc.inputs(rng, 70_000 + 41, "uniform"), run_of(0, 5 * SEG + 77)]
    order = rng.permutation(len(blobs))
    return [blobs[i] for i in order]


def run_mixed(sc, fill, road=None):
    """All three kinds at every edge length, under the test coder: host, strided or device items; `road`: the encode road."""
    rng = np.random.default_rng(1513)
    eng, coder = sc.engine(road) if road else (sc.eng, None)
    d_items = None
    if fill == "strided":
        in_len, stride, count = 2 * SEG + 77, 2 * SEG + 200, 9
        makers = [lambda: sa.words(rng, in_len), lambda: pc.inputs(rng, in_len, "uniform"), lambda: run_of(0xFF, in_len)]
        blobs = [makers[i % 3]() for i in range(count)]
        host = pc.inputs(rng, 3 + count * stride + 64, "uniform")
        for i, blob in enumerate(blobs):
            host[3 + i * stride:3 + i * stride + in_len] = blob
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
            plan, aligns = eng.encode_plan(b.items), ((1, 16, 4096) if road is None else (1,))
        else:
            (plan, d_items), aligns = eng.encode_plan_from_device_items(b.items), (1, 16)
    try:
        sents = run_launches(sc, eng, plan, d_in, blobs, overflows, eoss, aligns, label="mixed/%s/%s" % (fill, road))
        sent = sents[0]
        some = int((sent.n > 0).sum())
        assert all(5 * int((sent.kinds[sent.n > 0] == k).sum()) >= some for k in (CODED, STORED, CONSTANT)), (fill, sent.kinds)
        if fill != "strided":
            stats = eng.encode_stats(plan)
            # every kind of unit (a wave takes items only where the one-pass encoder applies)
            assert stats["by_thread"] and (stats["by_wave"] or road) and stats["by_pieces"] and stats["empty"], stats
            assert set(sent.n[sent.constant]) >= {15, 16, 17, 512, 4096, 16384, 16385} and sent.n[sent.constant].max() > 5 * SEG
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        if d_items:
            eng.free(d_items)
        close()
        if coder:
            sc.done(eng, coder)


# ----------------------------------------------------------------------------- 6: scan boundaries
def run_scan_boundaries(sc, tile, counts):
    """The offset scan in tiles of a few items (packed_api.SCAN_TILES), all three kinds mixed: offsets, kinds, sizes, the bytes
    and records of the constant and stored items whole (numpy), a sample of the coded ones (the oracle), the gaps."""
    eng = sc.eng
    rng = np.random.default_rng(1517 + tile)
    most = max(counts)
    sizes = rng.integers(1, 40, most)
    blobs = [run_of(i % 251, int(n)) if i % 4 == 2 else (sa.words(rng, int(n)) if i % 3 else pc.inputs(rng, int(n), "uniform"))
             for i, n in enumerate(sizes)]
    b = pa.Batch(eng, blobs, None, overflows=pa.carried(rng, most, every=5))
    try:
        with pa.pack_tile_items(sc.lib, tile):
            for n in counts:
                plan = eng.encode_plan(b.items[:n])
                try:
                    for align in (1, 16):
                        sent = Sent(sc.oracle, sc.w.ocoder, blobs[:n], sc.lens, b.overflows[:n], b.eoss[:n], align)
                        assert all((sent.kinds == k).any() for k in (CODED, STORED, CONSTANT))
                        bufs = sa.Buffers(eng, n, sent.total + 64, b.d_in)
                        try:
                            bufs.refill()
                            assert launch_constant(eng, plan, b.d_in, bufs.d_out, sent.total, bufs.d_off, bufs.d_flags, align) == (0, 0)
                            label = "tile %d, %d items, align %d" % (tile, n, align)
                            assert np.array_equal(pa.download_u64(eng, bufs.d_off, n + 1), sent.offsets), label
                            kinds = eng.download(bufs.d_flags, n + 8)
                            assert np.array_equal(kinds[:n], sent.kinds) and np.all(kinds[n:] == KIND_GUARD), label
                            assert pa.packed_size(eng, plan) == (0, 0, sent.total, int(sent.reserved.max())), label
                            assert sa.stored_size(eng, plan) == (0, 0) + sent.counts, label
                            assert constant_size(eng, plan) == (0, 0) + sent.constant_counts, label
                            got = eng.download(bufs.d_out, bufs.size)
                            res = pa.results_array(eng, plan, n)
                            # stored items: their bytes and records
                            want = np.concatenate(blobs[:n])
                            lens = sent.n
                            at = np.repeat(sent.offsets[:-1] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()))
                            mask = np.repeat(sent.stored, lens)
                            assert np.array_equal(got[at[mask]], want[mask]), label
                            st, co = sent.stored, sent.constant
                            assert np.all(res["rc"][st | co] == 0) and np.all(res["num_bits"][st | co] == 0), label
                            assert np.array_equal(res["produced"][st].astype(np.int64), lens[st]), label
                            assert np.array_equal(res["consumed"][st | co].astype(np.int64), lens[st | co]), label
                            # constant items: their 9 bytes and records
                            assert np.all(res["produced"][co] == HEAD), label
                            heads = got[(sent.offsets[:-1][co])[:, None] + np.arange(HEAD)[None, :]]
                            first = np.asarray([blobs[i][0] for i in np.flatnonzero(co)], np.uint8)
                            assert np.array_equal(heads[:, 8], first) and np.all(heads[:, 1:8] == 0), label
                            assert np.array_equal(heads[:, 0].astype(np.int64), lens[co]), label
                            for i in list(range(0, n, 97)) + [n - 1]:
                                if not (st[i] or co[i]):
                                    room = int(sent.reserved[i])
                                    rec, data = pa.oracle_item(sc.oracle, sc.w.ocoder, blobs[i], b.overflows[i], b.eoss[i], room)
                                    off = int(sent.offsets[i])
                                    assert np.array_equal(got[off:off + room], data), (label, i)
                                    assert (res["rc"][i], res["error"][i], res["consumed"][i], res["produced"][i]) == rec[:4], (label, i)
                            # nothing in an alignment gap or behind the total: every byte no item owns keeps the marker
                            edges = np.zeros(bufs.size + 1, np.int64)
                            np.add.at(edges, sent.offsets[:-1], 1)
                            np.add.at(edges, sent.offsets[:-1] + sent.lens, -1)
                            owned = np.cumsum(edges)[:-1] > 0
                            assert np.all(got[~owned] == MARKER) and not owned[sent.total:].any(), label
                        finally:
                            bufs.close()
                finally:
                    sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
    finally:
        sc.lib.aws_huffman_amd_testing_set_pack_tile_items(0)
        b.close()


# ----------------------------------------------------------------------------- 7: capacity
def run_capacity(sc, aligns=(1, 16)):
    """The edge at every byte of a constant item's 9 bytes and at the item boundaries around it: all 9 bytes or none."""
    eng = sc.eng
    rng = np.random.default_rng(1519)
    blobs = [sa.words(rng, 40), run_of(0x00, 700), pc.inputs(rng, 90, "uniform"), run_of(0xFF, SEG + 5), run_of(0x61, 0),
             run_of(0x20, 17), sa.words(rng, 500), run_of(0x00, 4097)]
    b = pa.Batch(eng, blobs, rng)
    plan = eng.encode_plan(b.items)

    def caps_of(sent):
        caps = [0, sent.total - 1, sent.total + 5]
        for k, i in enumerate(np.flatnonzero(sent.constant)):
            off = int(sent.offsets[i])
            caps += (list(range(off - 1, off + HEAD + 2)) if k < 2 else [off, off + HEAD - 1, off + HEAD]) + [int(sent.offsets[i + 1]) - 1, int(sent.offsets[i + 1]), int(sent.offsets[i + 1]) + 1]
        return sorted(set(c for c in caps if 0 <= c))

    try:
        sents = run_launches(sc, eng, plan, b.d_in, blobs, b.overflows, b.eoss, aligns, caps_of=caps_of, label="capacity")
        assert list(sents[0].kinds) == [CODED, CONSTANT, STORED, CONSTANT, CODED, CONSTANT, CODED, CONSTANT], sents[0].kinds
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 8: round trip
class Received:
    """What the receiver must make of a sender's output: sym_i (the oracle's for a coded item, n_i for a stored or constant
    one), offsets from them, and for a capacity the whole output and every record."""

    def __init__(self, sc, sent, ocoder=None, min_bits=None):
        self.sent = sent
        n = len(sent.blobs)
        raw = sent.stored | sent.constant
        streams = []
        for i, blob in enumerate(sent.blobs):
            if raw[i]:
                streams.append((blob, 0))
            else:
                rec, data = pa.oracle_item(sent.oracle, sent.ocoder, blob, sent.overflows[i], sent.eoss[i], int(sent.lens[i]))
                assert rec[:2] == (0, 0) and rec[3] == sent.lens[i], (i, rec)
                streams.append((data.copy(), 0))
        coded = [i for i in range(n) if not raw[i]]
        self.raw = raw
        self.expect = pd.Expect(sent.oracle, ocoder or sent.ocoder, streams, min_bits or sc.min_bits, only=coded)
        self.syms = np.asarray([sent.n[i] if raw[i] else self.expect.full[i][0][2] for i in range(n)], dtype=np.int64)
        self.offsets, self.reserved = pa.expected_offsets(self.syms, 1)
        self.total = int(self.offsets[-1])

    def output(self, cap, size):
        want = np.full(size, MARKER, np.uint8)
        room = pd.rooms(self.offsets, self.syms, cap)
        recs = []
        for i, blob in enumerate(self.sent.blobs):
            off = int(self.offsets[i])
            if self.raw[i]:
                fits = room[i] == blob.size
                if fits:
                    want[off:off + blob.size] = blob
                bits = 8 * HEAD if self.sent.constant[i] else 8 * blob.size
                recs.append((0, 0, blob.size, bits) if fits else (-1, SHORT, 0, 0))
            else:
                rec, data = self.expect.item(i, int(room[i]))
                want[off:off + int(room[i])] = data
                recs.append(rec)
        return want, recs


def check_received(eng, dplan, d_in, recv, cap, d_back, d_back_off, size, label="", stream=None):
    n = len(recv.sent.blobs)
    eng.fill(d_back, MARKER, size)
    eng.fill(d_back_off, 0xEE, 8 * (n + 1))
    assert pd.launch_packed(eng, dplan, d_in, d_back, cap, d_back_off, 1, stream) == (0, 0), label
    got = eng.download(d_back, size)
    res = eng.decode_results(dplan, n)
    want, recs = recv.output(cap, size)
    got_offsets = pa.download_u64(eng, d_back_off, n + 1)
    assert np.array_equal(got_offsets, recv.offsets), (label, int(np.flatnonzero(got_offsets != recv.offsets)[0]))
    for i in range(n):
        assert res[i] == recs[i], (label, cap, i, int(recv.sent.kinds[i]), res[i], recs[i])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (label, cap, "first wrong byte at %d" % int(bad[0]))
    assert pd.packed_size(eng, dplan) == (0, 0, recv.total, int(recv.reserved.max()) if n else 0), (label, pd.packed_size(eng, dplan))


def round_trip_blobs(rng):
    """All three kinds; constant items a lane, a wave and tiles fill (below 4096, to 16384, several tiles, a tail), at
    destinations of every alignment (the odd lengths in front)."""
    sizes = [30_000, 300, 0, 20_000, SEG, 1, 20_000, 900, 4095, 4096, 20_000 + 3, 17, 2 * SEG + 1, 40, 10, 4097, 5 * SEG + 13, 33]
    kinds = ["u", "w", "u", "c", "c", "u", "w", "c", "c", "c", "u", "c", "c", "u", "c", "c", "c", "w"]
    make = {"w": lambda n: sa.words(rng, n), "u": lambda n: pc.inputs(rng, n, "uniform"),
            "c": lambda n: run_of(int(rng.integers(0, 256)), n)}
    return [make[k](n) for k, n in zip(kinds, sizes)]


def run_round_trip(sc, align=1, with_lengths=False):
    """The sender's arrays straight into the receiver's reset, a size query, a launch, and the capacity at every item
    boundary (and a byte to either side of the constant items')."""
    eng = sc.eng
    rng = np.random.default_rng(1523)
    blobs = round_trip_blobs(rng)
    n = len(blobs)
    b = pa.Batch(eng, blobs, rng, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    dplan = eng.empty_decode_plan()
    sent = Sent(sc.oracle, sc.w.ocoder, blobs, sc.lens, b.overflows, b.eoss, align)
    recv = Received(sc, sent)
    assert all((sent.kinds == k).sum() >= 3 for k in (CODED, STORED, CONSTANT)), sent.kinds
    assert np.array_equal(recv.syms, sent.n)
    bufs = sa.Buffers(eng, n, sent.total + 64, b.d_in)
    size = recv.total + 64
    d_back, d_back_off, d_lens = eng.alloc(size), eng.alloc(8 * (n + 1)), None
    try:
        check_sent(eng, plan, sent, bufs, sent.total, "round trip, sender")
        if with_lengths or align > 1:  # (an alignment leaves gaps: the receiver needs the lengths, as for any packed buffer)
            d_lens = pd.upload_u64(eng, sent.lens)
        assert reset_constant_input(eng, dplan, bufs.d_out, bufs.d_off, d_lens, bufs.d_flags, n) == (0, 0)
        # a size query
        eng.fill(d_back_off, 0xEE, 8 * (n + 1))
        assert pd.launch_packed(eng, dplan, bufs.d_out, None, 0, d_back_off, 1) == (0, 0)
        assert pd.packed_size(eng, dplan)[:3] == (0, 0, recv.total)
        assert np.array_equal(pa.download_u64(eng, d_back_off, n + 1), recv.offsets)
        check_received(eng, dplan, bufs.d_out, recv, recv.total, d_back, d_back_off, size, "round trip")
        caps = {0, recv.total - 1}
        for i in range(n):
            caps |= {int(recv.offsets[i]), int(recv.offsets[i + 1])}
            if sent.constant[i]:
                caps |= {int(recv.offsets[i + 1]) - 1, int(recv.offsets[i + 1]) + 1, int(recv.offsets[i]) + HEAD}
        for cap in sorted(caps):
            check_received(eng, dplan, bufs.d_out, recv, cap, d_back, d_back_off, size, "round trip, clipped")
    finally:
        for p in (d_back, d_back_off) + ((d_lens,) if d_lens else ()):
            eng.free(p)
        bufs.close()
        sc.lib.aws_huffman_amd_decode_plan_destroy(dplan)
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 9: refusals, states, resets to and from other fills
def run_checks(sc):
    eng = sc.eng
    lib = sc.lib
    rng = np.random.default_rng(1529)
    blobs = [pc.inputs(rng, 300, "uniform"), sa.words(rng, 5_000), run_of(0x00, 20_000), sa.words(rng, 40), run_of(0xFF, 64)]
    n = len(blobs)
    b = pa.Batch(eng, blobs, rng, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    dplan, other = eng.empty_decode_plan(), eng.empty_decode_plan()
    sent = Sent(sc.oracle, sc.w.ocoder, blobs, sc.lens, b.overflows, b.eoss, 1)
    recv = Received(sc, sent)
    bufs = sa.Buffers(eng, n, sent.total + 64, b.d_in)
    size = recv.total + 64
    d_back, d_back_off = eng.alloc(size), eng.alloc(8 * (n + 1))
    d_bad, d_packed, d_lens = eng.alloc(n), eng.alloc(bufs.size), pd.upload_u64(eng, sent.lens)
    try:
        # argument checks of the sender
        assert launch_constant(eng, plan, b.d_in, bufs.d_out, sent.total, bufs.d_off, None, 1) == INVALID
        assert launch_constant(eng, plan, b.d_in, bufs.d_out, sent.total, None, bufs.d_flags, 1) == INVALID
        assert launch_constant(eng, plan, b.d_in, bufs.d_out, sent.total, bufs.d_off, bufs.d_flags, 3) == INVALID
        assert launch_constant(eng, plan, b.d_in, None, 5, bufs.d_off, bufs.d_flags, 1) == INVALID
        assert constant_size(eng, plan)[:2] == INVALID  # (no constant launch yet)
        # a stored launch is not a constant one; a constant one is both
        old = sa.Sent(sc.oracle, sc.w.ocoder, blobs, sc.lens, b.overflows, b.eoss, 1)
        theirs = sa.Buffers(eng, n, old.total + 64, b.d_in)
        try:
            sa.check_sent(eng, plan, old, theirs, old.total, "checks, stored launch")
        finally:
            theirs.close()
        assert constant_size(eng, plan)[:2] == INVALID
        check_sent(eng, plan, sent, bufs, sent.total, "checks, sender")
        assert list(sent.kinds) == [STORED, CODED, CONSTANT, CODED, CONSTANT]
        assert sa.from_encode(eng, dplan, plan) == INVALID_STATE
        # the older receiver still refuses a flag byte of 2
        assert sa.reset_stored_input(eng, dplan, bufs.d_off, None, bufs.d_flags, n) == INVALID
        assert eng.decode_stats(dplan)["items"] == 0

        def refused(kinds=None, packed=None, lens=False):
            """The reset with these kinds / this packed buffer in place of the sender's: refused, and a plan without items."""
            if kinds is not None:
                eng.upload(d_bad, np.asarray(kinds, np.uint8))
            if packed is not None:
                eng.upload(d_packed, packed)
            got = reset_constant_input(eng, dplan, d_packed if packed is not None else bufs.d_out, bufs.d_off,
                                       d_lens if lens else None, d_bad if kinds is not None else bufs.d_flags, n)
            return got == INVALID and eng.decode_stats(dplan)["items"] == 0

        good = eng.download(bufs.d_out, bufs.size)
        at = int(sent.offsets[2])
        assert np.array_equal(good[at:at + HEAD], head(20_000, 0x00))

        def with_count(count):
            packed = good.copy()
            packed[at:at + 8] = np.frombuffer(int(count).to_bytes(8, "little"), np.uint8)
            return packed

        # a kind above 2; a constant item whose packed length is not 9 (by the next offset, and by the lengths)
        assert refused(kinds=[1, 0, 3, 0, 2]) and refused(kinds=[1, 0, 255, 0, 2])
        assert refused(kinds=[2, 0, 2, 0, 2]) and refused(kinds=[1, 0, 2, 2, 2], lens=True)
        # a count of 9 or less, a count above the bound -- either side of each
        assert refused(packed=with_count(9)) and refused(packed=with_count(0)) and refused(packed=with_count(MAX_COUNT + 1))
        assert refused(packed=with_count(1 << 63)) and refused(packed=with_count((1 << 64) - 1))
        for count in (10, MAX_COUNT):
            eng.upload(d_packed, with_count(count))
            assert reset_constant_input(eng, dplan, d_packed, bufs.d_off, None, bufs.d_flags, n) == (0, 0), count
            eng.fill(d_back_off, 0xEE, 8 * (n + 1))
            assert pd.launch_packed(eng, dplan, d_packed, None, 0, d_back_off, 1) == (0, 0)  # (a size query: no room is asked for)
            assert pd.packed_size(eng, dplan)[:3] == (0, 0, recv.total - 20_000 + count), count
        # arguments
        assert reset_constant_input(eng, dplan, None, bufs.d_off, None, bufs.d_flags, n) == INVALID
        assert reset_constant_input(eng, dplan, bufs.d_out, None, None, bufs.d_flags, n) == INVALID
        # NULL kinds: the plan aws_huffman_amd_decode_plan_reset_packed_input leaves, which a plain launch may take
        assert reset_constant_input(eng, dplan, bufs.d_out, bufs.d_off, None, None, n) == (0, 0)
        assert pd.reset_packed_input(eng, other, bufs.d_off, None, n) == (0, 0)
        assert eng.decode_stats(dplan) == eng.decode_stats(other) and eng.decode_stats(dplan)["items"] == n
        assert lib.aws_huffman_amd_decode_plan_launch(dplan, bufs.d_out, d_back, None) == 0
        eng.decode_results(dplan, n)
        # a plain launch of a plan reset with kinds
        assert reset_constant_input(eng, dplan, bufs.d_out, bufs.d_off, None, bufs.d_flags, n) == (0, 0)
        lib.aws_reset_error()
        assert lib.aws_huffman_amd_decode_plan_launch(dplan, bufs.d_out, d_back, None) == -1
        assert lib.aws_last_error() == fa.AWS_ERROR_INVALID_STATE
        check_received(eng, dplan, bufs.d_out, recv, recv.total, d_back, d_back_off, size, "checks, receiver")
        # to two older fills and back: each behaves as a fresh plan does
        assert pd.reset_packed_input(eng, dplan, bufs.d_off, None, n) == (0, 0)
        assert eng.decode_stats(dplan) == eng.decode_stats(other)
        assert lib.aws_huffman_amd_decode_plan_launch(dplan, bufs.d_out, d_back, None) == 0
        eng.decode_results(dplan, n)
        assert reset_constant_input(eng, dplan, bufs.d_out, bufs.d_off, d_lens, bufs.d_flags, n) == (0, 0)
        check_received(eng, dplan, bufs.d_out, recv, recv.total, d_back, d_back_off, size, "back from a packed input")
        as_stored = sent.kinds.copy()
        as_stored[sent.constant] = 0  # (the older reset with flags: the constant items' heads taken for codes -- only the plan's shape is asked)
        eng.upload(d_bad, as_stored)
        assert sa.reset_stored_input(eng, dplan, bufs.d_off, None, d_bad, n) == (0, 0)
        fresh = eng.empty_decode_plan()
        assert sa.reset_stored_input(eng, fresh, bufs.d_off, None, d_bad, n) == (0, 0)
        assert eng.decode_stats(dplan) == eng.decode_stats(fresh)
        lib.aws_huffman_amd_decode_plan_destroy(fresh)
        assert reset_constant_input(eng, dplan, bufs.d_out, bufs.d_off, None, bufs.d_flags, n) == (0, 0)
        check_received(eng, dplan, bufs.d_out, recv, recv.total, d_back, d_back_off, size, "back from a stored input")
        # a later stored launch, then a plain packed launch of the same encode plan clear the state
        theirs = sa.Buffers(eng, n, old.total + 64, b.d_in)
        try:
            sa.check_sent(eng, plan, old, theirs, old.total, "stored again")
        finally:
            theirs.close()
        assert constant_size(eng, plan)[:2] == INVALID
        pa.check_launch(sc.oracle, sc.w.ocoder, eng, plan, b.d_in, blobs, sc.lens, b.overflows, b.eoss, 1, label="packed again")
        assert constant_size(eng, plan)[:2] == INVALID and sa.stored_size(eng, plan)[:2] == INVALID
        # an empty plan: offsets[0] = 0 and nothing else
        empty = eng.empty_encode_plan()
        bufs.refill()
        assert launch_constant(eng, empty, b.d_in, bufs.d_out, sent.total, bufs.d_off, bufs.d_flags, 1) == (0, 0)
        off = eng.download(bufs.d_off, 16).view(np.uint64)
        assert off[0] == 0 and off[1] == 0xEEEEEEEEEEEEEEEE
        assert np.all(eng.download(bufs.d_flags, n + 8) == KIND_GUARD) and np.all(eng.download(bufs.d_out, bufs.size) == MARKER)
        assert constant_size(eng, empty) == (0, 0, 0, 0) and sa.stored_size(eng, empty) == (0, 0, 0, 0)
        lib.aws_huffman_amd_encode_plan_destroy(empty)
    finally:
        for p in (d_back, d_back_off, d_bad, d_packed, d_lens):
            eng.free(p)
        bufs.close()
        lib.aws_huffman_amd_decode_plan_destroy(dplan)
        lib.aws_huffman_amd_decode_plan_destroy(other)
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 9b: a coder whose decode plans the host lays out
def run_host_laid_plan(sc):
    """A coder of 256 eight-bit codes: its decode plans are laid out by the host's loop, which restates the planner's checks
    of the kinds and heads.  Every item that is not constant is stored or empty (a tie is stored)."""
    lib = sc.lib
    rng = np.random.default_rng(1527)
    coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*([8] * 256)))
    assert coder
    eng = harness.Engine(lib, coder)
    blobs = [run_of(0x00, 700), pc.inputs(rng, 300, "uniform"), run_of(0x41, 0), run_of(0xFF, 5 * SEG + 13), run_of(0x20, 10),
             sa.words(rng, 40), run_of(0x07, 9), run_of(0x08, 4096)]
    n = len(blobs)
    b = pa.Batch(eng, blobs, rng, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    dplan = eng.empty_decode_plan()
    d_packed = None
    try:
        ocoder = fa.oracle_coder(sc.oracle, ba.coder_rows(coder))
        lens8 = np.full(256, 8, np.int64)
        sent = Sent(sc.oracle, ocoder, blobs, lens8, b.overflows, b.eoss, 1)
        assert list(sent.kinds) == [CONSTANT, STORED, CODED, CONSTANT, CONSTANT, STORED, STORED, CONSTANT], sent.kinds
        recv = Received(sc, sent, ocoder=ocoder, min_bits=8)
        bufs = sa.Buffers(eng, n, sent.total + 64, b.d_in)
        size = recv.total + 64
        d_back, d_back_off, d_packed = eng.alloc(size), eng.alloc(8 * (n + 1)), eng.alloc(bufs.size)
        try:
            check_sent(eng, plan, sent, bufs, sent.total, "eight-bit codes, sender")
            assert reset_constant_input(eng, dplan, bufs.d_out, bufs.d_off, None, bufs.d_flags, n) == (0, 0)
            for cap in (recv.total, int(recv.offsets[3]) + 5, int(recv.offsets[4]), 0):
                check_received(eng, dplan, bufs.d_out, recv, cap, d_back, d_back_off, size, "eight-bit codes, receiver")
            good = eng.download(bufs.d_out, bufs.size)
            at = int(sent.offsets[3])
            for count, want in ((9, INVALID), (MAX_COUNT + 1, INVALID), (10, (0, 0))):
                packed = good.copy()
                packed[at:at + 8] = np.frombuffer(int(count).to_bytes(8, "little"), np.uint8)
                eng.upload(d_packed, packed)
                assert reset_constant_input(eng, dplan, d_packed, bufs.d_off, None, bufs.d_flags, n) == want, count
                assert eng.decode_stats(dplan)["items"] == (n if want == (0, 0) else 0), count
            eng.upload(d_packed, np.asarray([2, 1, 0, 2, 3, 1, 1, 2], np.uint8))
            assert reset_constant_input(eng, dplan, bufs.d_out, bufs.d_off, None, d_packed, n) == INVALID
            eng.upload(d_packed, np.asarray([2, 2, 0, 2, 2, 1, 1, 2], np.uint8))  # (an item of 300 bytes called constant)
            assert reset_constant_input(eng, dplan, bufs.d_out, bufs.d_off, None, d_packed, n) == INVALID
        finally:
            for p in (d_back, d_back_off, d_packed):
                eng.free(p)
            bufs.close()
    finally:
        lib.aws_huffman_amd_decode_plan_destroy(dplan)
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        eng.close()
        lib.aws_huffman_amd_table_coder_destroy(coder)


# ----------------------------------------------------------------------------- 10: a fitted engine
def run_fitted(sc, memset_async):
    """count -> fit -> constant launch on one stream, nothing waited for in between, over text with binary and constant items;
    then the round trip under the fitted code.  memset_async(eng, dptr, size, stream) clears the counts in stream order."""
    lib = sc.lib
    rng = np.random.default_rng(1531)
    sizes = [3_000, 40_000, 700, 20_000, 90, SEG + 5, 5_000, 300, 2_000, 30_000]
    binary, runs = {2, 5}, {1: 0x00, 4: 0x65, 8: 0xFF}
    blobs = [pc.inputs(rng, n, "uniform") if i in binary else (run_of(runs[i], n) if i in runs else
             harness.printable_map(rng.integers(0, 256, n, dtype=np.uint8))) for i, n in enumerate(sizes)]
    n = len(blobs)
    eng = fa.FittedEngine(lib, 4, 12)
    b = pa.Batch(eng, blobs, None, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    dplan = eng.empty_decode_plan()
    capacity = 2 * sum(sizes)
    bufs = sa.Buffers(eng, n, capacity + 64, b.d_in)
    size = sum(sizes) + 64
    d_back, d_back_off = eng.alloc(size), eng.alloc(8 * (n + 1))
    stream = C.c_void_p(eng.stream)
    try:
        bufs.refill()
        eng.fill(eng.d_status, 0xEE, 4)
        memset_async(eng, eng.d_counts, 256 * 8, stream)
        assert pk.plan_counts(eng, plan, b.d_in, eng.d_counts, stream) == (0, 0)
        assert eng.fit_counts_async(None, stream) == (0, 0)
        assert launch_constant(eng, plan, b.d_in, bufs.d_out, capacity, bufs.d_off, bufs.d_flags, 1, stream) == (0, 0)
        assert lib.aws_huffman_amd_stream_synchronize(eng.h, stream) == 0
        assert eng.status() == fa.FIT_OK
        lengths = fa.host_lengths(lib, ba.bincount(np.concatenate(blobs)), eng.lo, eng.hi)
        assert eng.bits() == lengths
        ocoder = fa.oracle_coder(sc.oracle, fa.host_rows(lib, lengths))
        sent = Sent(sc.oracle, ocoder, blobs, np.asarray(lengths, dtype=np.int64), b.overflows, b.eoss, 1)
        assert set(np.flatnonzero(sent.stored)) == binary and set(np.flatnonzero(sent.constant)) == set(runs), sent.kinds
        check_sent(eng, plan, sent, bufs, capacity, "fitted", launch=False)
        recv = Received(sc, sent, ocoder=ocoder, min_bits=min(lengths))
        assert reset_constant_input(eng, dplan, bufs.d_out, bufs.d_off, None, bufs.d_flags, n) == (0, 0)
        check_received(eng, dplan, bufs.d_out, recv, recv.total, d_back, d_back_off, size, "fitted, receiver")
    finally:
        eng.free(d_back)
        eng.free(d_back_off)
        bufs.close()
        lib.aws_huffman_amd_decode_plan_destroy(dplan)
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        eng.close()


# ----------------------------------------------------------------------------- 11 (MI355X): the sender's launch captured and replayed
def run_replays(sc, graphs):
    """ONE captured constant launch, replayed three times over different data in the same places: which items are constant
    changes between replays, so every replay finds the detection's words as a launch must leave them."""
    eng = sc.eng
    rng = np.random.default_rng(1533)
    sizes = [70_000, 300, 0, 20_000, SEG, 17, 40_000, 900, 4096, 10, 2 * SEG + 1, 40]
    n = len(sizes)
    makers = [lambda m: sa.words(rng, m), lambda m: pc.inputs(rng, m, "uniform"), lambda m: run_of(int(rng.integers(0, 256)), m)]
    rounds = [[makers[(i + r) % 3](m) for i, m in enumerate(sizes)] for r in range(4)]
    b = pa.Batch(eng, rounds[0], rng, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    sents = [Sent(sc.oracle, sc.w.ocoder, blobs, sc.lens, b.overflows, b.eoss, 1) for blobs in rounds]
    capacity = max(s.total for s in sents)
    bufs = sa.Buffers(eng, n, capacity + 64, b.d_in)
    stream = C.c_void_p(eng.stream)
    execs = []
    try:
        check_sent(eng, plan, sents[0], bufs, capacity, "before the capture", stream=stream)  # (the first launch may allocate)
        graphs.call("hipStreamSynchronize", stream)
        execs.append(graphs.capture(stream, lambda: launch_constant(
            eng, plan, b.d_in, bufs.d_out, capacity, bufs.d_off, bufs.d_flags, 1, stream)))
        for r in (1, 2, 3):
            host = b.host_in.copy()
            for o, blob in zip(b.in_offs, rounds[r]):
                host[o:o + blob.size] = blob
            eng.upload(b.d_in, host)
            bufs.refill()
            eng.sync()
            graphs.call("hipGraphLaunch", execs[0], stream)
            graphs.call("hipStreamSynchronize", stream)
            assert not np.array_equal(sents[r].kinds, sents[r - 1].kinds)
            check_sent(eng, plan, sents[r], bufs, capacity, "replay %d" % r, launch=False)
    finally:
        for g in execs:
            graphs.call("hipGraphExecDestroy", g)
        bufs.close()
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- the library's face
def run_exports(so_path):
    """The shared library exports the four new entry points, and the header says what the issue fixes."""
    import os
    import re
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", so_path], capture_output=True, text=True, check=True).stdout
    for name in ("aws_huffman_amd_encode_plan_launch_packed_constant", "aws_huffman_amd_encode_plan_constant_size",
                 "aws_huffman_amd_decode_plan_reset_packed_constant_input"):
        assert (" T " + name + "\n") in out, name
    text = open(os.path.join(harness.REPO, "include", "aws", "compression", "huffman_amd_constant.h")).read()
    assert "#include <aws/compression/huffman_amd_stored.h>" in text
    for name, value in (("ITEM_CODED", CODED), ("ITEM_STORED", STORED), ("ITEM_CONSTANT", CONSTANT), ("CONSTANT_BYTES", HEAD)):
        assert re.search(r"#define AWS_HUFFMAN_AMD_%s %d\b" % (name, value), text), name
    assert int(re.search(r"#define AWS_HUFFMAN_AMD_CONSTANT_MAX_COUNT (\w+)", text).group(1).rstrip("ul"), 16) == MAX_COUNT
