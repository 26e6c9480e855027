"""ctypes face of include/aws/compression/huffman_amd_ranges.h (where a symbol of an indexed stream starts, decode plans
over ranges of symbols) and what its tests share.  Used by tests/test_emulated_ranges.py (emulator build) and
tests/test_gpu_ranges.py (MI355X): every run_* scenario below is called by both, at the same sizes.

Expected values never come from the library under test: the bit a symbol starts at is numpy's cumsum of the coder's code
lengths over the data; a range's output is the data's own slice; its record is the oracle's decode of the range's encoded
bytes (packed_decode_api.oracle_item)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import fit_api as fa
import harness
import index_api as ia
import packed_api as pa
import packed_decode_api as pda
import parity_cases as pc

LOCATE_OK, LOCATE_NOT_FOUND = 0, 1
NO_BIT = (1 << 64) - 1
INVALID, UNSUPPORTED, STATE, MARKER = ia.INVALID, ia.UNSUPPORTED, ia.STATE, ia.MARKER
GUARD_WORDS = 4  # uint64 words behind device_bits[count - 1] that a call must leave alone
HEADER = os.path.join(harness.REPO, "include", "aws", "compression", "huffman_amd_ranges.h")


class SymbolRange(C.Structure):
    """struct aws_huffman_amd_symbol_range"""
    _fields_ = [("first_symbol", C.c_uint64), ("symbol_count", C.c_uint64), ("out_offset", C.c_uint64)]


def bind(lib):
    """Declares the entry points of huffman_amd_ranges.h (and of the headers below it) on a loaded product (or emulator)
    library."""
    ia.bind(lib)
    V = C.c_void_p
    lib.aws_huffman_amd_locate_symbols.restype = C.c_int
    lib.aws_huffman_amd_locate_symbols.argtypes = [V, V, C.c_uint64, V, C.c_uint64, C.c_uint64, V, C.c_size_t, V, V, V]
    lib.aws_huffman_amd_decode_plan_reset_symbol_ranges.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_reset_symbol_ranges.argtypes = [V, V, V, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, V,
                                                                    C.c_size_t, V]
    lib.aws_huffman_amd_testing_set_locate_lone_symbols.restype = None
    lib.aws_huffman_amd_testing_set_locate_lone_symbols.argtypes = [C.c_uint32]
    return lib


class lone_symbols:
    """with lone_symbols(lib, 100): a position up to 100 codes behind its block's first is a lane's walk, one further
    behind a workgroup's (restored to the built-in rule behind it)."""

    def __init__(self, lib, symbols):
        self.lib, self.symbols = lib, symbols

    def __enter__(self):
        self.lib.aws_huffman_amd_testing_set_locate_lone_symbols(self.symbols)

    def __exit__(self, *exc):
        self.lib.aws_huffman_amd_testing_set_locate_lone_symbols(0)


def locate_call(eng, d_enc, enc_length, d_index, length, block_symbols, d_symbols, count, d_bits, d_status, stream=None):
    """(rc, error) of the enqueue."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_locate_symbols(eng.h, d_enc, int(enc_length), d_index, int(length), int(block_symbols), d_symbols,
                                                int(count), d_bits, d_status, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def reset_symbol_ranges(eng, plan, d_input, d_index, length, block_symbols, enc_offset, enc_length, d_ranges, n, stream=None):
    """(rc, error)."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_decode_plan_reset_symbol_ranges(plan, d_input, d_index, int(length), int(block_symbols),
                                                                 int(enc_offset), int(enc_length), d_ranges, n, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def symbol_bits(code_lens, data):
    """bits[s] = the bit symbol s starts at, s = 0 .. len (a symbol without a code: 0 bits)."""
    return np.concatenate([[0], np.cumsum(np.asarray(code_lens, dtype=np.int64)[data])]).astype(np.uint64)


def locate(eng, st, positions, want_rc=(0, 0)):
    """One call over `positions` of the stream `st` (an index_api.Stream): (bits as uint64[count], status).  The guard
    words behind the results and the 0xEE behind the status are checked here."""
    pos = np.asarray(positions, dtype=np.uint64)
    n = int(pos.size)
    d_pos, d_bits, d_status = pda.upload_u64(eng, pos), eng.alloc(8 * (n + GUARD_WORDS)), eng.alloc(8)
    try:
        eng.fill(d_bits, 0xEE, 8 * (n + GUARD_WORDS))
        eng.fill(d_status, 0xEE, 8)
        got_rc = locate_call(eng, st.d_enc + st.enc_offset, st.enc.size, st.d_index, st.n, st.B, d_pos, n, d_bits, d_status)
        assert got_rc == want_rc, got_rc
        eng.sync()
        got = eng.download(d_bits, 8 * (n + GUARD_WORDS)).view(np.uint64)
        status = eng.download(d_status, 8).view(np.uint32)
        assert np.all(got[n:] == 0xEEEEEEEEEEEEEEEE), "words behind device_bits[count - 1] were written"
        assert status[1] == 0xEEEEEEEE
        return got[:n].copy(), int(status[0])
    finally:
        for d in (d_pos, d_bits, d_status):
            eng.free(d)


def check_locate(eng, st, bits, positions, label=""):
    """Positions inside the stream (s <= length): every result numpy's, status OK."""
    pos = np.asarray(positions, dtype=np.int64)
    got, status = locate(eng, st, pos)
    want = bits[pos]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (label, "first wrong position %d" % int(pos[bad[0]]), int(got[bad[0]]), int(want[bad[0]]))
    assert status == LOCATE_OK, (label, status)
    return got


# ----------------------------------------------------------------------------- 1: edges
EDGE_SYMBOLS = 40_001


def run_locate_edges(sc, kind):
    """40 001 symbols in blocks of 64: the stream's first symbols, a block's last and the next one's first two, the last
    symbol, `length` itself and one past it (NO_BIT and the flag); every position of blocks 0, 311 and the ragged last one;
    no position at all."""
    n, B = EDGE_SYMBOLS, 64
    data = ia.data_of(sc, kind, n, seed=907)
    bits = symbol_bits(sc.lens, data)
    st = ia.Stream(sc, sc.eng, sc.lens, sc.w.ocoder, data, B)
    try:
        assert n % B and st.nb - 1 > 311
        check_locate(sc.eng, st, bits, [0, 1, 63, 64, 65, n - 1, n], label=kind)
        got, status = locate(sc.eng, st, [5, n + 1, n, 1 << 63, NO_BIT])
        assert [int(g) for g in got] == [int(bits[5]), NO_BIT, int(bits[n]), NO_BIT, NO_BIT] and status == LOCATE_NOT_FOUND
        for b in (0, 311, st.nb - 1):
            check_locate(sc.eng, st, bits, np.arange(b * B, min((b + 1) * B, n) + 1), label="%s, block %d" % (kind, b))
        got, status = locate(sc.eng, st, [])
        assert got.size == 0 and status == LOCATE_OK
    finally:
        st.close()


# ----------------------------------------------------------------------------- 2: both roads and their boundary
ROADS_SYMBOLS = 200_003
ROADS_BLOCKS = [64, 512, 16_384]
ROADS_LIMITS = ["1", "100", "above"]


def roads_positions(n, B, limit):
    """k in {1, limit - 1, limit, limit + 1, B - 1} in a middle block and in the ragged last one, and 2 000 anywhere."""
    nb = ia.n_blocks_of(n, B)
    pos = []
    for b in (nb // 2, nb - 1):
        for k in (1, limit - 1, limit, limit + 1, B - 1):
            if 0 < k < B and b * B + k < n:
                pos.append(b * B + k)
    pos += [int(p) for p in np.random.default_rng(911).integers(0, n + 1, 2000)]
    return np.array(pos, dtype=np.int64)


def run_roads(sc, block_symbols, limit_name, results):
    """`results`: {block_symbols: located bits} shared by the three limits of a block size -- the same positions come to
    the same bits whichever road took them."""
    n, B = ROADS_SYMBOLS, block_symbols
    limit = {"1": 1, "100": 100, "above": B + 1}[limit_name]
    data = ia.data_of(sc, "uniform", n, seed=913)
    bits = symbol_bits(sc.lens, data)
    st = ia.Stream(sc, sc.eng, sc.lens, sc.w.ocoder, data, B)
    try:
        with lone_symbols(sc.lib, limit):
            # (the boundary cases of every limit, located under this one)
            pos = np.unique(np.concatenate([roads_positions(n, B, lim) for lim in (1, 100, B + 1)]))
            got = check_locate(sc.eng, st, bits, pos, label="B %d, limit %s" % (B, limit_name))
        assert set(int(b) for b in got % 8) == set(range(8)), "the located bits do not take all eight values mod 8"
        assert np.array_equal(results.setdefault(B, got), got), "the results depend on the limit"
    finally:
        st.close()


# ----------------------------------------------------------------------------- 3: other coders
def run_other_coder(sc, name):
    """HPACK's lengths (30-bit codes) and codes of 4 .. 15 bits, both through linked tables, in blocks of 64 and 4 096, on
    either road; a coder of 8-bit codes, in closed form."""
    ocoder, coder, lengths = pc.profile_coders(sc.w, name)
    eng, code_lens = harness.Engine(sc.lib, coder), np.asarray(lengths, dtype=np.int64)
    data = ia.data_of(sc, "uniform", 100_003, seed=919)
    bits = symbol_bits(code_lens, data)
    pos = np.concatenate([[0, 1, 63, 64, 65, 4095, 4096, 4097, data.size - 1, data.size],
                          np.random.default_rng(921).integers(0, data.size + 1, 600)])
    try:
        for B in (64, 4096):
            st = ia.Stream(sc, eng, code_lens, ocoder, data, B)
            try:
                for limit in (1, 0):
                    with lone_symbols(sc.lib, limit):
                        check_locate(eng, st, bits, pos, label="%s, B %d, limit %d" % (name, B, limit))
            finally:
                st.close()
    finally:
        eng.close()


def run_never_in_step(sc):
    """Symbols 28 .. 255 of the 4 .. 15-bit coder: codes of 9, 12 and 15 bits only, three phases that never merge.  Blocks of
    16 384, a workgroup a position: the news of a block's true entry travels a lane a round."""
    ocoder, coder, lengths = pc.profile_coders(sc.w, "len4to15")
    eng, code_lens = harness.Engine(sc.lib, coder), np.asarray(lengths, dtype=np.int64)
    n, B = 300_000, 16_384
    data = np.random.default_rng(923).integers(28, 256, n).astype(np.uint8)
    assert set(int(l) for l in code_lens[28:]) == {9, 12, 15}
    bits = symbol_bits(code_lens, data)
    pos = np.concatenate([[1, 2, B - 1, B + 1, 5 * B + 8000, n - 1, n], np.random.default_rng(925).integers(0, n + 1, 60)])
    st = None
    try:
        st = ia.Stream(sc, eng, code_lens, ocoder, data, B)
        with lone_symbols(sc.lib, 1):
            check_locate(eng, st, bits, pos, label="never in step")
    finally:
        if st:
            st.close()
        eng.close()


# ----------------------------------------------------------------------------- 4: a walk that stops
HOLES_SYMBOLS = 40_000


def holes_stream(sc, front=0):
    data = ia.data_of(sc, "uniform", HOLES_SYMBOLS, seed=929)
    return data, ia.Stream(sc, sc.eng, sc.lens, sc.w.ocoder, data, 64, enc_offset=front)


def run_walk_that_stops(sc):
    """A stream of the full test coder located by an engine whose coder lacks symbols 7 and 200: behind the first 7 of its
    block a position is not found (the window there is no code of that engine); blocks that hold neither symbol are exact,
    on either road.  The same stream with other bytes in front of it and behind it: the same results."""
    eng, coder = sc.engine(holes=True)
    B = 64
    seen = []
    try:
        for front, around in ((0, 0x00), (48, 0xFF)):
            data, st = holes_stream(sc, front)
            try:
                # (other bytes around the stream than Stream's own 0x5A)
                if front:
                    sc.eng.fill(st.d_enc, around, front)
                sc.eng.fill(st.d_enc + front + st.enc.size, around, 64)
                sc.eng.sync()
                bits = symbol_bits(sc.lens, data)
                blocks = data[:data.size // B * B].reshape(-1, B)
                holed = (blocks == 7) | (blocks == 200)
                clean = np.flatnonzero(~holed.any(axis=1))
                with_7 = np.flatnonzero((blocks == 7).any(axis=1))
                assert clean.size >= 12 and with_7.size >= 40
                for limit in (1, 0):
                    with lone_symbols(sc.lib, limit):
                        pos = (clean[:12, None] * B + np.arange(B)[None, :]).ravel()
                        got, status = locate(eng, st, pos)
                        assert np.array_equal(got, bits[pos]) and status == LOCATE_OK, limit
                        # behind the first 7 (or 200) of its block: the walk meets a window without a code
                        stops = []
                        for b in with_7[:40]:
                            first = int(np.flatnonzero(holed[b])[0])
                            if first + 1 < B:
                                stops += [b * B + first + 1, b * B + B - 1]
                        got, status = locate(eng, st, stops)
                        assert np.all(got == NO_BIT) and status == LOCATE_NOT_FOUND, limit
                        # ... and in front of it, the symbol itself included, exact
                        fronts = [b * B + int(np.flatnonzero(holed[b])[0]) for b in with_7[:40]]
                        got, status = locate(eng, st, fronts)
                        assert np.array_equal(got, bits[fronts]) and status == LOCATE_OK, limit
                mixed = np.random.default_rng(931).integers(0, data.size + 1, 3000)
                seen.append(locate(eng, st, mixed))
            finally:
                st.close()
        assert np.array_equal(seen[0][0], seen[1][0]) and seen[0][1] == seen[1][1] == LOCATE_NOT_FOUND
    finally:
        sc.done(eng, coder)


# ----------------------------------------------------------------------------- 5 .. 7: range plans
class Ranges:
    """Symbol ranges of an index_api.Stream through a decode plan."""

    def __init__(self, st, eng=None):
        self.st, self.eng = st, eng or st.eng
        self.bits = None

    def upload(self, ranges):
        arr = (SymbolRange * max(len(ranges), 1))(*[SymbolRange(*r) for r in ranges])
        d = self.eng.alloc(C.sizeof(arr))
        self.eng.upload(d, np.frombuffer(arr, dtype=np.uint8))
        self.st.owned.append(d)
        return d

    def reset(self, plan, ranges, d_index=None, enc_length=None, block_symbols=None, d_input="own"):
        st = self.st
        return reset_symbol_ranges(self.eng, plan, st.d_enc if d_input == "own" else d_input, d_index or st.d_index, st.n,
                                   st.B if block_symbols is None else block_symbols, st.enc_offset,
                                   st.enc.size if enc_length is None else enc_length, self.upload(ranges), len(ranges))

    def item(self, s0, count):
        """What a range comes to, from the definition: (encoded slice, first bit, capacity, symbols)."""
        st = self.st
        if count == 0:
            return st.enc[:0], 0, 0, st.data[:0]
        i0, i1 = int(self.bits[s0]), int(self.bits[s0 + count])
        return st.enc[i0 // 8:(i1 + 7) // 8], i0 % 8, count, st.data[s0:s0 + count]

    def check_launch(self, plan, ranges, out_size, label=""):
        """A plain launch of the plan: every byte of the output (MARKER where no range writes), and every record the
        oracle's for the range's own encoded bytes, first bit and capacity."""
        st, eng = self.st, self.eng
        want = np.full(out_size, MARKER, np.uint8)
        recs = []
        for s0, count, out_off in ranges:
            enc, first_bit, cap, syms = self.item(s0, count)
            rec, out = pda.oracle_item(st.sc.oracle, st.ocoder, enc, first_bit, cap)
            assert rec[:2] in ((0, 0), pda.SHORT) and rec[2] == cap, (label, s0, count, rec)
            assert np.array_equal(out, syms), (label, s0, count)
            recs.append(rec)
            want[out_off:out_off + cap] = syms
        d_out = eng.alloc(out_size)
        try:
            eng.fill(d_out, MARKER, out_size)
            eng.decode_launch(plan, st.d_enc, d_out)
            got = eng.download(d_out, out_size)
            res = eng.decode_results(plan, len(ranges))
        finally:
            eng.free(d_out)
        for i, rec in enumerate(recs):
            assert res[i] == rec, (label, i, ranges[i], res[i], rec)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (label, "first wrong byte at %d" % int(bad[0]))
        return recs


def run_range_plans(sc, enc_offset):
    """8 MiB less 3 000 symbols in blocks of 16 384: ranges inside one block (60 symbols, 5 000), across one block boundary
    and across three, the whole stream, the last symbol alone, two that overlap, an empty one at `length`, one of whole
    blocks -- listed so that first_symbol goes down as well as up, 3 bytes of MARKER between their outputs."""
    n, B = ia.RANGES_SYMBOLS, 16_384
    data = ia.data_of(sc, "uniform", n, seed=853)
    st = ia.Stream(sc, sc.eng, sc.lens, sc.w.ocoder, data, B, enc_offset=enc_offset)
    rg = Ranges(st)
    rg.bits = symbol_bits(sc.lens, data)
    plan, block_plan = sc.eng.empty_decode_plan(), sc.eng.empty_decode_plan()
    try:
        spans = [(n - 1, 1), (0, n), (300 * B + 7_000, 5_000), (40 * B - 100, 2 * B + 300), (17 * B + 100, 60), (9 * B - 30, 70),
                 (200 * B + 5, 9_000), (200 * B + 4_000, 9_000), (n, 0), (12 * B, 4 * B), (3, 1)]
        ranges, at = [], 3
        for s0, count in spans:
            ranges.append((s0, count, at))
            at += count + 3
        assert rg.reset(plan, ranges) == (0, 0)
        stats = sc.eng.decode_stats(plan)
        assert stats["items"] == len(ranges) and stats["empty"] == 1 and stats["by_thread"] >= 3, stats
        recs = rg.check_launch(plan, ranges, at + 64, label="symbol ranges, stream at %d" % enc_offset)
        # the 60 symbols alone: a thread's work, whatever the block
        assert rg.reset(plan, [(17 * B + 100, 60, 0)]) == (0, 0)
        stats = sc.eng.decode_stats(plan)
        assert stats["items"] == 1 and stats["by_thread"] == 1, stats
        rg.check_launch(plan, [(17 * B + 100, 60, 0)], 128, label="60 symbols")
        # whole blocks: the item, its record and the plan's statistics are those of a plan over the blocks
        assert rg.reset(plan, [(12 * B, 4 * B, 5)]) == (0, 0)
        assert st.reset(block_plan, [(12, 4, 5)]) == (0, 0)
        assert sc.eng.decode_stats(plan) == sc.eng.decode_stats(block_plan)
        mine = rg.check_launch(plan, [(12 * B, 4 * B, 5)], 4 * B + 64, label="whole blocks")
        theirs = st.check_launch(block_plan, [(12, 4, 5)], 4 * B + 64, label="whole blocks, by blocks")
        assert mine == theirs == [recs[9]]
    finally:
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        sc.lib.aws_huffman_amd_decode_plan_destroy(block_plan)
        st.close()


def run_odd_pieces(sc):
    """300 007 symbols in blocks of 512, cut into consecutive ranges of 1 000 laid back to back: the output is the data."""
    n, B = ia.EVERY_BLOCK_SYMBOLS, 512
    data = ia.data_of(sc, "uniform", n, seed=941)
    st = ia.Stream(sc, sc.eng, sc.lens, sc.w.ocoder, data, B)
    rg = Ranges(st)
    rg.bits = symbol_bits(sc.lens, data)
    plan = sc.eng.empty_decode_plan()
    try:
        ranges = [(s, min(1000, n - s), s) for s in range(0, n, 1000)]
        assert ranges[-1][1] == 7
        assert rg.reset(plan, ranges) == (0, 0)
        assert sc.eng.decode_stats(plan)["items"] == len(ranges)
        rg.check_launch(plan, ranges, n + 64, label="pieces of 1000")
    finally:
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        st.close()


def run_fitted(sc, clear, block_symbols=512):
    """Printable text under a coder fitted within (4, 12): the sender counts, fits and indexes on the device; the receiver,
    an engine made by fit_lengths from the sender's 256 bytes, decodes ranges of 777 symbols of the device's index.  A
    fitted engine before any fit: AWS_ERROR_INVALID_STATE from both calls."""
    lib = sc.lib
    data = fa.shape_bytes("printable", ia.EVERY_BLOCK_SYMBOLS, 861)
    n, nb = int(data.size), ia.n_blocks_of(data.size, block_symbols)
    sender, receiver = fa.FittedEngine(lib, 4, 12), fa.FittedEngine(lib, 4, 12)
    d_in, d_index, d_status = sender.alloc(n), sender.alloc(8 * (nb + 1)), sender.alloc(4)
    st = plan = None
    try:
        plan = receiver.empty_decode_plan()
        d_some = receiver.alloc(64)
        try:
            receiver.fill(d_some, 0, 64)
            assert locate_call(receiver, d_some, 8, d_some, 8, 64, d_some, 1, d_some + 32, None) == STATE
            assert reset_symbol_ranges(receiver, plan, d_some, d_some, 8, 64, 0, 8, d_some + 32, 1) == STATE
        finally:
            receiver.free(d_some)
        sender.upload(d_in, data)
        ia.enqueue_fit_and_index(sender, clear, d_in, n, block_symbols, d_index, d_status, C.c_void_p(sender.stream))
        sender.sync()
        lengths, want = ia.check_fitted_index(sender, data, block_symbols, d_index, d_status)
        assert receiver.fit_lengths_async(sender.d_bits) == (0, 0)  # (no wait: the reset below is behind it on the stream)
        ocoder = fa.oracle_coder(sc.oracle, fa.host_rows(lib, lengths))
        st = ia.Stream(sc, receiver, lengths, ocoder, data, block_symbols, index_eng=sender)
        assert receiver.status() == fa.FIT_OK
        rg = Ranges(st, receiver)
        rg.bits = symbol_bits(lengths, data)
        ranges = [(s, min(777, n - s), s) for s in range(0, n, 777)]
        # (the index the device made, where it was made)
        assert reset_symbol_ranges(receiver, plan, st.d_enc, d_index, n, block_symbols, 0, st.enc.size, rg.upload(ranges),
                                   len(ranges)) == (0, 0)
        rg.check_launch(plan, ranges, n + 64, label="printable, fitted")
    finally:
        if plan:
            lib.aws_huffman_amd_decode_plan_destroy(plan)
        if st:
            st.close()
        for d in (d_in, d_index, d_status):
            sender.free(d)
        sender.close()
        receiver.close()


# ----------------------------------------------------------------------------- 9 .. 10: refusals, no GPU, exports
def run_refusals(sc):
    eng, lib = sc.eng, sc.lib
    data, st = holes_stream(sc)
    B, n = st.B, st.n
    rg = Ranges(st)
    rg.bits = symbol_bits(sc.lens, data)
    plan = eng.empty_decode_plan()
    good = [(s, min(100, n - s), s) for s in range(0, n, 100)]
    out_size = n + 64
    d_out = eng.alloc(out_size)
    holes_eng, holes_coder = sc.engine(holes=True)
    holes_plan = holes_eng.empty_decode_plan()
    try:
        def refused(call, label, plan=plan, eng=eng, want=INVALID):
            assert call() == want, label
            assert eng.decode_stats(plan)["items"] == 0, label
            eng.fill(d_out, MARKER, out_size)
            assert lib.aws_huffman_amd_decode_plan_launch(plan, st.d_enc, d_out, None) == 0, label
            eng.sync()
            assert np.all(eng.download(d_out, out_size) == MARKER), label

        def refused_after_good(call, label):
            assert rg.reset(plan, good) == (0, 0) and eng.decode_stats(plan)["items"] == len(good), label
            refused(call, label)

        refused_after_good(lambda: rg.reset(plan, good + [(n + 1, 0, 0)]), "a range that starts past length")
        refused_after_good(lambda: rg.reset(plan, [(n - 5, 6, 0)] + good), "a range that ends past length")
        refused_after_good(lambda: rg.reset(plan, [(5, (1 << 64) - 1, 0)]), "first_symbol + symbol_count overflows")
        refused_after_good(lambda: rg.reset(plan, [((1 << 64) - 1, 2, 0)]), "first_symbol + symbol_count overflows")
        lowered = st.index.copy()
        lowered[7] = lowered[6] - 1
        d_lowered = pda.upload_u64(eng, lowered)
        st.owned.append(d_lowered)
        refused_after_good(lambda: rg.reset(plan, [(6 * B + 5, 10, 0)], d_index=d_lowered), "an index entry lowered at a range's block")
        assert rg.reset(plan, [(8 * B + 5, 10, 0)], d_index=d_lowered) == (0, 0)  # (a block whose two entries are whole)
        refused_after_good(lambda: rg.reset(plan, [(n - 20, 10, 0)], enc_length=st.enc.size - 1), "encoded_length one byte short")
        # (what these ranges' blocks need)
        assert rg.reset(plan, good[:60], enc_length=(int(st.index[(60 * 100 + B - 1) // B]) + 7) // 8) == (0, 0)
        # an end that is not found: the engine without symbols 7 and 200, a range that starts behind a block's first 7
        blocks = data[:n // B * B].reshape(-1, B)
        b = int(np.flatnonzero(((blocks[:, :40] == 7) | (blocks[:, :40] == 200)).any(axis=1))[0])
        holes_rg = Ranges(st, holes_eng)
        refused(lambda: holes_rg.reset(holes_plan, [(b * B + 50, 5, 0)]), "a range with an end that is not found", holes_plan, holes_eng)
        for bad in (0, 63, 1 << 25):
            refused_after_good(lambda: rg.reset(plan, good, block_symbols=bad), "block_symbols %d" % bad)
        d_ranges = rg.upload(good)
        args = (st.n, B, 0, st.enc.size)
        refused_after_good(lambda: reset_symbol_ranges(eng, plan, st.d_enc, None, *args, d_ranges, len(good)), "NULL index")
        refused_after_good(lambda: reset_symbol_ranges(eng, plan, st.d_enc, st.d_index + 4, *args, d_ranges, len(good)), "misaligned index")
        refused_after_good(lambda: reset_symbol_ranges(eng, plan, st.d_enc, st.d_index, *args, None, len(good)), "NULL ranges")
        refused_after_good(lambda: reset_symbol_ranges(eng, plan, st.d_enc, st.d_index, *args, d_ranges + 4, len(good)), "misaligned ranges")
        refused_after_good(lambda: reset_symbol_ranges(eng, plan, None, st.d_index, *args, d_ranges, len(good)), "NULL input")
        assert reset_symbol_ranges(eng, None, st.d_enc, st.d_index, *args, d_ranges, len(good)) == INVALID
        # a later good reset of the same plan works
        assert rg.reset(plan, good) == (0, 0)
        rg.check_launch(plan, good, out_size, label="behind the refusals")
        # no ranges at all: a plan without items, success
        assert rg.reset(plan, []) == (0, 0) and eng.decode_stats(plan)["items"] == 0

        # the locate call's own arguments: nothing is written
        pos = np.arange(0, n, 37, dtype=np.uint64)
        d_pos, d_bits, d_status = pda.upload_u64(eng, pos), eng.alloc(8 * pos.size), eng.alloc(4)
        st.owned += [d_pos, d_bits, d_status]
        eng.fill(d_bits, 0xEE, 8 * pos.size)
        eng.fill(d_status, 0xEE, 4)
        call = lambda **k: locate_call(eng, k.get("enc", st.d_enc), st.enc.size, k.get("index", st.d_index), n, k.get("B", B),
                                       k.get("pos", d_pos), pos.size, k.get("bits", d_bits), k.get("status", d_status))
        assert call(index=None) == INVALID and call(index=st.d_index + 4) == INVALID
        assert call(pos=None) == INVALID and call(pos=d_pos + 4) == INVALID
        assert call(bits=None) == INVALID and call(bits=d_bits + 4) == INVALID
        assert call(status=d_status + 2) == INVALID and call(enc=None) == INVALID
        for bad in (0, 63, 96, 1 << 25):
            assert call(B=bad) == INVALID, bad
        lib.aws_reset_error()
        assert lib.aws_huffman_amd_locate_symbols(None, st.d_enc, st.enc.size, st.d_index, n, B, d_pos, pos.size, d_bits, d_status, None) == -1
        assert lib.aws_last_error() == harness.AWS_ERROR_INVALID_ARGUMENT
        eng.sync()
        assert np.all(eng.download(d_bits, 8 * pos.size) == 0xEE) and np.all(eng.download(d_status, 4) == 0xEE)
        # the status is optional
        assert call(status=None) == (0, 0)
        eng.sync()
        assert np.array_equal(pa.download_u64(eng, d_bits, pos.size), rg.bits[pos.astype(np.int64)])
    finally:
        eng.free(d_out)
        lib.aws_huffman_amd_decode_plan_destroy(plan)
        lib.aws_huffman_amd_decode_plan_destroy(holes_plan)
        sc.done(holes_eng, holes_coder)
        st.close()


def run_product_without_a_gpu(product):
    """Against the product library on a machine without a GPU: both entry points raise AWS_ERROR_UNSUPPORTED_OPERATION and
    touch nothing they were handed.  (With a GPU present this has nothing to say: tests/test_gpu_ranges.py speaks there.)"""
    if product.aws_huffman_amd_device_count() > 0:
        return
    handle = np.full(4096, 0x11, np.uint8)  # (stands for the engine and the plan: there is neither without a GPU)
    memory = np.full(4096, 0xEE, np.uint8)
    ranges = np.zeros(24, np.uint8)
    h, m, r = handle.ctypes.data, memory.ctypes.data, ranges.ctypes.data
    product.aws_reset_error()
    assert product.aws_huffman_amd_locate_symbols(h, m + 1024, 600, m, 512, 64, m + 2048, 4, m + 3072, m + 512, None) == -1
    assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    product.aws_reset_error()
    assert product.aws_huffman_amd_decode_plan_reset_symbol_ranges(h, m + 1024, m, 512, 64, 0, 600, r, 1, None) == -1
    assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    assert np.all(handle == 0x11) and np.all(memory == 0xEE) and not ranges.any()


def header_api_names():
    text = open(HEADER).read()
    return re.findall(r"AWS_COMPRESSION_API\s+[\w\s\*]*?\b(aws_\w+)\s*\(", text)


def run_exports(so_path):
    names = header_api_names()
    assert set(names) == {"aws_huffman_amd_locate_symbols", "aws_huffman_amd_decode_plan_reset_symbol_ranges",
                          "aws_huffman_amd_testing_set_locate_lone_symbols"}, names
    listing = subprocess.check_output(["nm", "-D", "--defined-only", so_path], text=True)
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported], [n for n in names if n not in exported]
