"""ctypes face of include/aws/compression/huffman_amd_index.h (the block index of a stream, decode plans over ranges of
blocks) and what its tests share.  Used by tests/test_emulated_index.py (emulator build) and tests/test_gpu_index.py
(MI355X): every run_* scenario below is called by both, at the same sizes.

Expected values never come from the library under test: the index is numpy's cumsum of the coder's code lengths over the
data, taken at the block edges (and pinned to the oracle's length query at three of them); a range's output is the data's
own slice; its record and guard bytes are the oracle's decode of the range's encoded bytes
(packed_decode_api.oracle_item)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import build_api as ba
import fit_api as fa
import harness
import packed_api as pa
import packed_decode_api as pda
import parity_cases as pc

INDEX_OK, INDEX_SYMBOL_WITHOUT_CODE = 0, 1
INVALID = (-1, harness.AWS_ERROR_INVALID_ARGUMENT)
UNSUPPORTED = (-1, harness.AWS_ERROR_UNSUPPORTED_OPERATION)
STATE = (-1, fa.AWS_ERROR_INVALID_STATE)
MARKER = pa.MARKER
GUARD_WORDS = 4  # uint64 words behind index[n_blocks] that a call must leave alone
HEADER = os.path.join(harness.REPO, "include", "aws", "compression", "huffman_amd_index.h")


class BlockRange(C.Structure):
    """struct aws_huffman_amd_block_range"""
    _fields_ = [("first_block", C.c_uint64), ("block_count", C.c_uint64), ("out_offset", C.c_uint64)]


def bind(lib):
    """Declares the entry points of huffman_amd_index.h (and of the build, fit and packed headers) on a loaded product (or
    emulator) library."""
    fa.bind(lib)
    V = C.c_void_p
    lib.aws_huffman_amd_block_index.restype = C.c_int
    lib.aws_huffman_amd_block_index.argtypes = [V, V, C.c_uint64, C.c_uint64, V, V, V]
    lib.aws_huffman_amd_decode_plan_reset_block_ranges.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_reset_block_ranges.argtypes = [V, V, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, V,
                                                                   C.c_size_t, V]
    lib.aws_huffman_amd_testing_set_index_tile_blocks.restype = None
    lib.aws_huffman_amd_testing_set_index_tile_blocks.argtypes = [C.c_uint32]
    return lib


class index_tile_blocks:
    """with index_tile_blocks(lib, 3): index calls inside scan three blocks a workgroup (restored to the rule behind it)."""

    def __init__(self, lib, blocks):
        self.lib, self.blocks = lib, blocks

    def __enter__(self):
        self.lib.aws_huffman_amd_testing_set_index_tile_blocks(self.blocks)

    def __exit__(self, *exc):
        self.lib.aws_huffman_amd_testing_set_index_tile_blocks(0)


def block_index(eng, d_in, length, block_symbols, d_index, d_status, stream=None):
    """(rc, error) of the enqueue."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_block_index(eng.h, d_in, int(length), int(block_symbols), d_index, d_status, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def reset_block_ranges(eng, plan, d_index, length, block_symbols, enc_offset, enc_length, d_ranges, n, stream=None):
    """(rc, error)."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_decode_plan_reset_block_ranges(plan, d_index, int(length), int(block_symbols), int(enc_offset),
                                                                int(enc_length), d_ranges, n, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def n_blocks_of(length, block_symbols):
    return (int(length) + block_symbols - 1) // block_symbols


def expected_index(code_lens, data, block_symbols):
    """index[k] = the code bits of data[:min(k * block_symbols, len)], k = 0 .. n_blocks (a symbol without a code: 0 bits)."""
    bits = np.concatenate([[0], np.cumsum(np.asarray(code_lens, dtype=np.int64)[data])]).astype(np.int64)
    edges = np.minimum(np.arange(n_blocks_of(data.size, block_symbols) + 1, dtype=np.int64) * block_symbols, data.size)
    return bits[edges]


def pin_to_oracle(oracle, ocoder, data, block_symbols, index):
    """The first edge, a middle one and the last against aws_huffman_get_encoded_length of the symbols in front of them."""
    nb = index.size - 1
    for k in sorted({min(1, nb), nb // 2, nb}):
        want = oracle.encoded_length(oracle.new_encoder(ocoder), data[:min(k * block_symbols, data.size)])
        assert (int(index[k]) + 7) // 8 == want, (k, int(index[k]), want)


def device_index(eng, data, block_symbols, misalign=0, d_data=None):
    """One call over `data` laid `misalign` bytes behind an allocation's start (or at d_data): (index as int64[n_blocks + 1],
    status).  The guard words behind the index and the 0xEE the status was filled with are checked here."""
    nb = n_blocks_of(data.size, block_symbols)
    own = d_data is None
    if own:
        d_data = eng.alloc(data.size + misalign + 16)
        if data.size:
            eng.upload(d_data, data, offset=misalign)
    d_index, d_status = eng.alloc(8 * (nb + 1 + GUARD_WORDS)), eng.alloc(8)
    try:
        eng.fill(d_index, 0xEE, 8 * (nb + 1 + GUARD_WORDS))
        eng.fill(d_status, 0xEE, 8)
        assert block_index(eng, d_data + misalign, data.size, block_symbols, d_index, d_status) == (0, 0)
        eng.sync()
        got = eng.download(d_index, 8 * (nb + 1 + GUARD_WORDS)).view(np.uint64)
        status = eng.download(d_status, 8).view(np.uint32)
        assert np.all(got[nb + 1:] == 0xEEEEEEEEEEEEEEEE), "words behind index[n_blocks] were written"
        assert status[1] == 0xEEEEEEEE
        return got[:nb + 1].astype(np.int64), int(status[0])
    finally:
        eng.free(d_index)
        eng.free(d_status)
        if own:
            eng.free(d_data)


def check_index(sc, eng, code_lens, ocoder, data, block_symbols, misalign=0, want_status=INDEX_OK, label=""):
    want = expected_index(code_lens, data, block_symbols)
    pin_to_oracle(sc.oracle, ocoder, data, block_symbols, want)
    got, status = device_index(eng, data, block_symbols, misalign)
    assert status == want_status, (label, status)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (label, block_symbols, misalign, data.size, "first wrong entry %d" % int(bad[0]), int(got[bad[0]]),
                           int(want[bad[0]]))
    return want


# ----------------------------------------------------------------------------- 1 .. 4: the index
EDGE_LENGTHS = [0, 1, 63, 64, 65, 64 * 7 + 17, 40_001]
EDGE_MISALIGN = [0, 1, 3, 15]
BLOCK_SIZES = [64, 512, 16_384]
DATA_KINDS = ["uniform", "printable", "shortest code", "longest code"]
N_SYMBOLS = 200_003
SCAN_TILES = [1, 3, 256]
OTHER_CODERS = ["hpack_lengths", "len4to15", "holes"]


def data_of(sc, kind, n, seed=811):
    rng = np.random.default_rng(seed)
    if kind in ("uniform", "printable"):
        return pc.inputs(rng, n, kind)
    coded = np.flatnonzero(sc.lens)
    pick = coded[np.argmin(sc.lens[coded])] if kind == "shortest code" else coded[np.argmax(sc.lens[coded])]
    return np.full(n, int(pick), np.uint8)


def run_index_edges(sc):
    """Test coder, blocks of 64: nothing, less than a block, a block, a block and a symbol, a ragged tail, many tiles of the
    hot kernel; the input 0, 1, 3 and 15 bytes off a 16-byte boundary."""
    for n in EDGE_LENGTHS:
        data = data_of(sc, "uniform", n, seed=800 + n % 97)
        for m in EDGE_MISALIGN:
            got = check_index(sc, sc.eng, sc.lens, sc.w.ocoder, data, 64, m, label="edges")
            assert got[0] == 0 and got.size == n_blocks_of(n, 64) + 1


def run_block_sizes(sc, block_symbols, kind):
    data = data_of(sc, kind, N_SYMBOLS)
    check_index(sc, sc.eng, sc.lens, sc.w.ocoder, data, block_symbols, label=kind)
    check_index(sc, sc.eng, sc.lens, sc.w.ocoder, data[:-5], block_symbols, misalign=7, label=kind + " off by 7")


def run_scan_tiles(sc, tile):
    data = data_of(sc, "uniform", N_SYMBOLS)
    with index_tile_blocks(sc.lib, tile):
        check_index(sc, sc.eng, sc.lens, sc.w.ocoder, data, 64, label="tile %d" % tile)


def run_other_coders(sc, name):
    """HPACK's lengths (30-bit codes), codes of 4 .. 15 bits, and the test coder less symbols 7 and 200: there the status
    says so and the index counts 0 bits for them."""
    data = data_of(sc, "uniform", 100_003, seed=823)
    if name == "holes":
        eng, coder = sc.engine(holes=True)
        code_lens, ocoder, want_status = sc.lens_holes, sc.w.ocoder_holes, INDEX_SYMBOL_WITHOUT_CODE
        assert np.any(data == 7) and np.any(data == 200)
    else:
        ocoder, coder, lengths = pc.profile_coders(sc.w, name)
        eng, code_lens, want_status = harness.Engine(sc.lib, coder), np.asarray(lengths, dtype=np.int64), INDEX_OK
        assert code_lens.max() == {"hpack_lengths": 30, "len4to15": 15}[name]
    try:
        for block_symbols in (64, 4096):
            check_index(sc, eng, code_lens, ocoder, data, block_symbols, want_status=want_status, label=name)
        if name == "holes":  # ... and a stream that meets neither symbol says OK
            clean = data.copy()
            clean[clean == 7] = 8
            clean[clean == 200] = 201
            check_index(sc, eng, code_lens, ocoder, clean, 64, label="holes, none met")
    finally:
        sc.done(eng, coder)


# ----------------------------------------------------------------------------- 5: behind a fit, on one stream
def enqueue_fit_and_index(eng, clear, d_in, length, block_symbols, d_index, d_status, stream):
    """clear the counts, count, fit, index: four steps on `stream`, nothing waited for in between."""
    clear(eng, eng.d_counts, 256 * 8, stream)
    assert eng.lib.aws_huffman_amd_symbol_counts(-1, d_in, length, eng.d_counts, stream) == 0
    assert eng.fit_counts_async(None, stream) == (0, 0)
    assert block_index(eng, d_in, length, block_symbols, d_index, d_status, stream) == (0, 0)


def check_fitted_index(eng, data, block_symbols, d_index, d_status):
    """Behind such a chain: the index is the cumsum of the lengths the fit left in device_num_bits."""
    nb = n_blocks_of(data.size, block_symbols)
    assert eng.status() == fa.FIT_OK
    lengths = eng.bits()
    assert min(lengths) >= eng.lo and max(lengths) <= eng.hi
    want = expected_index(lengths, data, block_symbols)
    got = pa.download_u64(eng, d_index, nb + 1)
    assert int(eng.download(d_status, 4).view(np.uint32)[0]) == INDEX_OK
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, ("first wrong entry %d" % int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    return lengths, want


def run_fitted_engine(lib, clear, block_symbols=512, n=N_SYMBOLS):
    """A (4, 12) engine: never fitted, the index call is refused and writes nothing; then clear, count, fit, index enqueued
    back to back.  clear(engine, dptr, size, stream): a memset that is a command of the stream."""
    eng = fa.FittedEngine(lib, 4, 12)
    data = fa.shape_bytes("printable", n, 831)
    nb = n_blocks_of(n, block_symbols)
    d_in, d_index, d_status = eng.alloc(n), eng.alloc(8 * (nb + 1)), eng.alloc(4)
    try:
        eng.upload(d_in, data)
        eng.fill(d_index, 0xEE, 8 * (nb + 1))
        eng.fill(d_status, 0xEE, 4)
        assert block_index(eng, d_in, n, block_symbols, d_index, d_status) == STATE
        eng.sync()
        assert np.all(eng.download(d_index, 8 * (nb + 1)) == 0xEE) and np.all(eng.download(d_status, 4) == 0xEE)
        enqueue_fit_and_index(eng, clear, d_in, n, block_symbols, d_index, d_status, C.c_void_p(eng.stream))
        eng.sync()
        lengths, _ = check_fitted_index(eng, data, block_symbols, d_index, d_status)
        assert not fa.is_flat(lengths)
    finally:
        for d in (d_in, d_index, d_status):
            eng.free(d)
        eng.close()


# ----------------------------------------------------------------------------- 6 .. 8: ranges through a decode plan
class Stream:
    """One stream on the device: its symbols, what the oracle encodes them to (behind `enc_offset` bytes of something else,
    in front of 64 more), and its index -- made by the device, checked against numpy's before anything is built on it."""

    def __init__(self, sc, eng, code_lens, ocoder, data, block_symbols, enc_offset=0, index_eng=None):
        self.sc, self.eng, self.ocoder, self.data, self.B = sc, eng, ocoder, data, block_symbols
        self.n, self.nb = int(data.size), n_blocks_of(data.size, block_symbols)
        self.index = expected_index(code_lens, data, block_symbols)
        got, status = device_index(index_eng or eng, data, block_symbols)
        assert status == INDEX_OK and np.array_equal(got, self.index)
        self.enc = sc.oracle.encode_all(ocoder, data, eos_padding=0xFF)
        assert self.enc.size == (int(self.index[-1]) + 7) // 8
        self.enc_offset = enc_offset
        host = np.full(enc_offset + self.enc.size + 64, 0x5A, np.uint8)
        host[enc_offset:enc_offset + self.enc.size] = self.enc
        self.d_enc = eng.alloc(host.size)
        eng.upload(self.d_enc, host)
        self.d_index = pda.upload_u64(eng, self.index)
        self.owned = [self.d_enc, self.d_index]

    def close(self):
        for d in self.owned:
            self.eng.free(d)

    def upload_ranges(self, ranges):
        arr = (BlockRange * max(len(ranges), 1))(*[BlockRange(*r) for r in ranges])
        d = self.eng.alloc(C.sizeof(arr))
        self.eng.upload(d, np.frombuffer(arr, dtype=np.uint8))
        self.owned.append(d)
        return d

    def reset(self, plan, ranges, d_index=None, enc_length=None, block_symbols=None):
        return reset_block_ranges(self.eng, plan, d_index or self.d_index, self.n, self.B if block_symbols is None else block_symbols, self.enc_offset,
                                  self.enc.size if enc_length is None else enc_length, self.upload_ranges(ranges), len(ranges))

    def item(self, first_block, count):
        """What a range comes to, from the definition: (encoded slice, first bit, capacity, symbols)."""
        b1 = first_block + count
        lo, hi = first_block * self.B, min(b1 * self.B, self.n)
        if count == 0:
            return self.enc[:0], 0, 0, self.data[:0]
        i0, i1 = int(self.index[first_block]), int(self.index[b1])
        return self.enc[i0 // 8:(i1 + 7) // 8], i0 % 8, hi - lo, self.data[lo:hi]

    def check_launch(self, plan, ranges, out_size, label=""):
        """A plain launch of the range plan: every byte of the output (MARKER where no range writes), and every record the
        oracle's for the range's own encoded bytes -- success, or SHORT_BUFFER where the last byte's spare bits spell a
        symbol; either way produced == out_capacity."""
        eng = self.eng
        want = np.full(out_size, MARKER, np.uint8)
        recs = []
        for first, count, out_off in ranges:
            enc, first_bit, cap, syms = self.item(first, count)
            rec, out = pda.oracle_item(self.sc.oracle, self.ocoder, enc, first_bit, cap)
            assert rec[:2] in ((0, 0), pda.SHORT) and rec[2] == cap, (label, first, count, rec)
            assert np.array_equal(out, syms), (label, first, count)
            recs.append(rec)
            want[out_off:out_off + cap] = syms
        d_out = eng.alloc(out_size)
        try:
            eng.fill(d_out, MARKER, out_size)
            eng.decode_launch(plan, self.d_enc, d_out)
            got = eng.download(d_out, out_size)
            res = eng.decode_results(plan, len(ranges))
        finally:
            eng.free(d_out)
        for i, rec in enumerate(recs):
            assert res[i] == rec, (label, i, ranges[i], res[i], rec)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (label, "first wrong byte at %d" % int(bad[0]))
        return recs


EVERY_BLOCK_SYMBOLS = 300_007


def run_every_block(sc, block_symbols):
    """Every block its own range, in order, a byte of MARKER between the outputs of two blocks."""
    data = data_of(sc, "uniform", EVERY_BLOCK_SYMBOLS, seed=841)
    st = Stream(sc, sc.eng, sc.lens, sc.w.ocoder, data, block_symbols)
    plan = sc.eng.empty_decode_plan()
    try:
        assert set(int(b) for b in st.index[:-1] % 8) == set(range(8)), "the blocks' first bits do not take all eight values"
        ranges = [(k, 1, k * (block_symbols + 1)) for k in range(st.nb)]
        assert st.reset(plan, ranges) == (0, 0)
        stats = sc.eng.decode_stats(plan)
        assert stats["items"] == st.nb, stats
        # (64 symbols: some 75 bytes, a thread's; 512: some 600, a wave's; 16 384: 19 KB, pieces -- the ragged last block
        # may be one class down)
        road = {64: "by_thread", 512: "by_wave", 16_384: "by_pieces"}[block_symbols]
        assert stats[road] >= st.nb - 1, (block_symbols, stats)
        recs = st.check_launch(plan, ranges, st.nb * (block_symbols + 1) + 64, label="every block of %d" % block_symbols)
        return recs
    finally:
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        st.close()


MiB = 1 << 20
RANGES_SYMBOLS = 8 * MiB - 3_000  # (the last block is ragged)


RANGES_ENC_OFFSETS = [0, 5]


def run_ranges(sc, enc_offset):
    """8 MiB, blocks of 16 384: the first block, the last (ragged) one, three blocks entered inside a byte (two chunks), all
    blocks, two ranges that overlap, an empty one -- listed so that first_block goes down as well as up.  enc_offset 5: the
    stream lies 5 bytes into a larger buffer."""
    data = data_of(sc, "uniform", RANGES_SYMBOLS, seed=853)
    B = 16_384
    st = Stream(sc, sc.eng, sc.lens, sc.w.ocoder, data, B, enc_offset=enc_offset)
    plan = sc.eng.empty_decode_plan()
    try:
        inside = next(k for k in range(200, st.nb) if st.index[k] % 8)
        spans = [(st.nb - 1, 1), (0, st.nb), (inside, 3), (12, 4), (10, 4), (5, 0), (0, 1)]
        assert st.item(inside, 3)[0].size > pda.CHUNK and st.item(st.nb - 1, 1)[2] < B
        ranges, at = [], 3
        for first, count in spans:
            ranges.append((first, count, at))
            at += st.item(first, count)[2] + 3
        assert st.reset(plan, ranges) == (0, 0)
        stats = sc.eng.decode_stats(plan)
        assert stats["items"] == len(ranges) and stats["empty"] == 1, stats
        st.check_launch(plan, ranges, at + 64, label="ranges, stream at %d" % enc_offset)
    finally:
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        st.close()


def run_printable_fitted(sc, clear, block_symbols=512):
    """Printable text under a coder fitted within (4, 12): the sender counts, fits and indexes on the device; the receiver,
    an engine made by fit_lengths from the sender's 256 bytes, decodes every block as a range of the device's index."""
    lib = sc.lib
    data = fa.shape_bytes("printable", EVERY_BLOCK_SYMBOLS, 861)
    n, nb = int(data.size), n_blocks_of(data.size, block_symbols)
    sender, receiver = fa.FittedEngine(lib, 4, 12), fa.FittedEngine(lib, 4, 12)
    d_in, d_index, d_status = sender.alloc(n), sender.alloc(8 * (nb + 1)), sender.alloc(4)
    st = plan = None
    try:
        sender.upload(d_in, data)
        enqueue_fit_and_index(sender, clear, d_in, n, block_symbols, d_index, d_status, C.c_void_p(sender.stream))
        sender.sync()
        lengths, want = check_fitted_index(sender, data, block_symbols, d_index, d_status)
        assert min(lengths) < 8, sorted(set(lengths))  # (shorter codes than the test coder's)
        assert receiver.fit_lengths_async(sender.d_bits) == (0, 0)
        assert receiver.status() == fa.FIT_OK
        ocoder = fa.oracle_coder(sc.oracle, fa.host_rows(lib, lengths))
        st = Stream(sc, receiver, lengths, ocoder, data, block_symbols, index_eng=sender)
        plan = receiver.empty_decode_plan()
        ranges = [(k, 1, k * block_symbols) for k in range(nb)]
        # (the index the device made, where it was made)
        assert reset_block_ranges(receiver, plan, d_index, n, block_symbols, 0, st.enc.size, st.upload_ranges(ranges), nb) == (0, 0)
        assert set(int(b) for b in want[:-1] % 8) == set(range(8))
        st.check_launch(plan, ranges, n + 64, label="printable, fitted")
    finally:
        if plan:
            lib.aws_huffman_amd_decode_plan_destroy(plan)
        if st:
            st.close()
        for d in (d_in, d_index, d_status):
            sender.free(d)
        sender.close()
        receiver.close()


# ----------------------------------------------------------------------------- 9 .. 11: refusals, no GPU, exports
def run_refusals(sc):
    eng, lib = sc.eng, sc.lib
    data = data_of(sc, "uniform", 40_000, seed=871)
    B = 64
    st = Stream(sc, eng, sc.lens, sc.w.ocoder, data, B)
    nb = st.nb
    plan = eng.empty_decode_plan()
    good = [(k, 1, k * B) for k in range(nb)]
    out_size = st.n + 64
    d_out = eng.alloc(out_size)
    try:
        def refused(call, label):
            assert st.reset(plan, good) == (0, 0) and eng.decode_stats(plan)["items"] == nb, label
            assert call() == INVALID, label
            assert eng.decode_stats(plan)["items"] == 0, label
            eng.fill(d_out, MARKER, out_size)
            assert lib.aws_huffman_amd_decode_plan_launch(plan, st.d_enc, d_out, None) == 0, label
            eng.sync()
            assert np.all(eng.download(d_out, out_size) == MARKER), label

        refused(lambda: st.reset(plan, good + [(nb, 1, 0)]), "a range that starts past the last block")
        refused(lambda: st.reset(plan, [(nb - 1, 2, 0)] + good), "a range that ends past the last block")
        refused(lambda: st.reset(plan, [(1, (1 << 64) - 1, 0)]), "first_block + block_count overflows")
        refused(lambda: st.reset(plan, [((1 << 64) - 1, 2, 0)]), "first_block + block_count overflows")
        lowered = st.index.copy()
        lowered[7] = lowered[6] - 1
        d_lowered = pda.upload_u64(eng, lowered)
        st.owned.append(d_lowered)
        refused(lambda: st.reset(plan, good, d_index=d_lowered), "an index with one entry lowered")
        refused(lambda: st.reset(plan, good, enc_length=st.enc.size - 1), "encoded_length one byte short")
        assert st.reset(plan, good[:-1], enc_length=(int(st.index[nb - 1]) + 7) // 8) == (0, 0)  # (what those ranges need)
        for bad in (0, 63, 1 << 25):
            refused(lambda: st.reset(plan, good, block_symbols=bad), "block_symbols %d" % bad)
        d_ranges = st.upload_ranges(good)
        refused(lambda: reset_block_ranges(eng, plan, None, st.n, B, 0, st.enc.size, d_ranges, nb), "NULL index")
        refused(lambda: reset_block_ranges(eng, plan, st.d_index, st.n, B, 0, st.enc.size, None, nb), "NULL ranges")
        refused(lambda: reset_block_ranges(eng, plan, st.d_index + 4, st.n, B, 0, st.enc.size, d_ranges, nb), "misaligned index")
        assert reset_block_ranges(eng, None, st.d_index, st.n, B, 0, st.enc.size, d_ranges, nb) == INVALID
        # a later good reset of the same plan works
        assert st.reset(plan, good) == (0, 0)
        st.check_launch(plan, good, out_size, label="behind the refusals")
        # no ranges at all: a plan without items, success
        assert st.reset(plan, []) == (0, 0) and eng.decode_stats(plan)["items"] == 0

        # the index call's own arguments: nothing is written
        d_index, d_status = eng.alloc(8 * (nb + 1)), eng.alloc(4)
        st.owned += [d_index, d_status]
        eng.fill(d_index, 0xEE, 8 * (nb + 1))
        eng.fill(d_status, 0xEE, 4)
        d_in = eng.alloc(st.n)
        st.owned.append(d_in)
        eng.upload(d_in, data)
        assert block_index(eng, d_in, st.n, B, None, d_status) == INVALID
        assert block_index(eng, d_in, st.n, B, d_index + 4, d_status) == INVALID
        assert block_index(eng, d_in, st.n, B, d_index, d_status + 2) == INVALID
        assert block_index(eng, None, st.n, B, d_index, d_status) == INVALID
        for bad in (0, 63, 96, 1 << 25):
            assert block_index(eng, d_in, st.n, bad, d_index, d_status) == INVALID, bad
        lib.aws_reset_error()
        assert lib.aws_huffman_amd_block_index(None, d_in, st.n, B, d_index, d_status, None) == -1
        assert lib.aws_last_error() == harness.AWS_ERROR_INVALID_ARGUMENT
        eng.sync()
        assert np.all(eng.download(d_index, 8 * (nb + 1)) == 0xEE) and np.all(eng.download(d_status, 4) == 0xEE)
        # the status is optional, a NULL input of no symbols is taken, the largest block is
        assert block_index(eng, d_in, st.n, B, d_index, None) == (0, 0)
        assert block_index(eng, None, 0, B, d_index, d_status) == (0, 0)
        assert block_index(eng, d_in, st.n, 1 << 24, d_index, d_status) == (0, 0)
        eng.sync()
        assert np.array_equal(pa.download_u64(eng, d_index, 2), [0, int(st.index[-1])])
    finally:
        eng.free(d_out)
        lib.aws_huffman_amd_decode_plan_destroy(plan)
        st.close()


def run_product_without_a_gpu(product):
    """Against the product library on a machine without a GPU: both entry points raise AWS_ERROR_UNSUPPORTED_OPERATION and
    touch nothing they were handed.  (With a GPU present this has nothing to say: tests/test_gpu_index.py speaks there.)"""
    if product.aws_huffman_amd_device_count() > 0:
        return
    handle = np.full(4096, 0x11, np.uint8)  # (stands for the engine and the plan: there is neither without a GPU)
    memory = np.full(4096, 0xEE, np.uint8)
    ranges = np.zeros(24, np.uint8)
    h, m, r = handle.ctypes.data, memory.ctypes.data, ranges.ctypes.data
    product.aws_reset_error()
    assert product.aws_huffman_amd_block_index(h, m + 1024, 512, 64, m, m + 512, None) == -1
    assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    product.aws_reset_error()
    assert product.aws_huffman_amd_decode_plan_reset_block_ranges(h, m, 512, 64, 0, 600, r, 1, None) == -1
    assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    assert np.all(handle == 0x11) and np.all(memory == 0xEE) and not ranges.any()


def header_api_names():
    text = open(HEADER).read()
    return re.findall(r"AWS_COMPRESSION_API\s+[\w\s\*]*?\b(aws_\w+)\s*\(", text)


def run_exports(so_path):
    names = header_api_names()
    assert set(names) == {"aws_huffman_amd_block_index", "aws_huffman_amd_decode_plan_reset_block_ranges",
                          "aws_huffman_amd_testing_set_index_tile_blocks"}, names
    listing = subprocess.check_output(["nm", "-D", "--defined-only", so_path], text=True)
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported], [n for n in names if n not in exported]
