"""ctypes face of include/aws/compression/huffman_amd_fit.h (coders fitted on the device) and what its tests share: the
count vectors, the host's lengths and the tables written out in Python from the canonical rows, one check of a fit against
both, and the oracle's coder of a fit.  Used by tests/test_emulated_fit.py (emulator build) and tests/test_gpu_fit.py
(MI355X): every run_* scenario below is called by both, at the same sizes.  Nothing here asks a second engine what a table
should hold."""
import ctypes as C
import types

import numpy as np

import build_api as ba
import harness
import packed_api as pa
import packed_decode_api as pda
import parity_cases as pc

AWS_ERROR_INVALID_STATE = 38
FIT_OK, FIT_COUNTS_TOO_LARGE, FIT_LENGTH_ZERO, FIT_LENGTH_OUT_OF_BOUNDS, FIT_KRAFT_ABOVE_ONE = 0, 1, 2, 3, 4
# (min_bits, max_bits) of the engines under test.  256 coded symbols and Kraft: with max_bits == 8 no length may be shorter
# than 8, with min_bits == 8 the optimal code has none longer, so a fit from counts within (7, 8), (4, 8) or (8, 12) can
# only ever yield the flat 8-bit code; the others have max_bits 9, 10, 11 and 12 with room for a spread of lengths
BOUNDS = [(4, 12), (4, 10), (5, 9), (7, 8), (4, 8), (8, 12), (4, 9), (7, 9), (4, 11), (6, 11), (7, 12)]
ROAD_ONE_PASS = pc.ROAD_ONE_PASS
ROAD_OF = {None: pc.ROAD_ONE_PASS, "three-kernel": pc.ROAD_TWO_PASS, "one-pass-fails": pc.ROAD_GAVE_UP}
INVALID = (-1, harness.AWS_ERROR_INVALID_ARGUMENT)


def only_flat(lo, hi):
    """Bounds under which every fit from counts is the flat 8-bit code."""
    return lo == 8 or hi == 8


def bind(lib):
    """Declares the entry points of huffman_amd_fit.h (and of huffman_amd_build.h, huffman_amd_packed.h) on a loaded
    product (or emulator) library."""
    ba.bind(lib)
    pda.bind(lib)
    V, P = C.c_void_p, C.POINTER
    lib.aws_huffman_amd_engine_new_fitted.restype = C.c_int
    lib.aws_huffman_amd_engine_new_fitted.argtypes = [P(V), C.c_int, C.c_uint32, C.c_uint32]
    lib.aws_huffman_amd_engine_fit_counts.restype = C.c_int
    lib.aws_huffman_amd_engine_fit_counts.argtypes = [V, V, V, V, V]
    lib.aws_huffman_amd_engine_fit_lengths.restype = C.c_int
    lib.aws_huffman_amd_engine_fit_lengths.argtypes = [V, V, V, V]
    lib.aws_huffman_amd_engine_is_fitted.restype = C.c_bool
    lib.aws_huffman_amd_engine_is_fitted.argtypes = [V]
    lib.aws_huffman_amd_testing_engine_tables.restype = C.c_int
    lib.aws_huffman_amd_testing_engine_tables.argtypes = [V, P(C.c_uint64), P(C.c_uint16), C.c_size_t]
    return lib


def new_fitted(lib, lo, hi, device=-1):
    """(rc, error, handle)."""
    h = C.c_void_p()
    lib.aws_reset_error()
    rc = lib.aws_huffman_amd_engine_new_fitted(C.byref(h), device, lo, hi)
    return rc, lib.aws_last_error() if rc else 0, h


class FittedEngine(harness.Engine):
    """harness.Engine over aws_huffman_amd_engine_new_fitted, with the three small device arrays a fit talks through."""

    def __init__(self, lib, lo, hi, device=-1):
        rc, err, h = new_fitted(lib, lo, hi, device)
        if rc != 0:
            raise RuntimeError("aws_huffman_amd_engine_new_fitted failed, error %d" % err)
        self.lib, self.h, self.lo, self.hi = lib, h, lo, hi
        self.stream = lib.aws_huffman_amd_engine_stream(h)
        self.d_counts, self.d_bits, self.d_status = self.alloc(256 * 8), self.alloc(256), self.alloc(4)

    def close(self):
        if self.h:
            for p in (self.d_counts, self.d_bits, self.d_status):
                self.free(p)
        super().close()

    def fit_counts_async(self, d_counts=None, stream=None):
        """Enqueued, not waited for: (rc, error)."""
        self.lib.aws_reset_error()
        rc = self.lib.aws_huffman_amd_engine_fit_counts(self.h, d_counts or self.d_counts, self.d_bits, self.d_status, stream)
        return rc, self.lib.aws_last_error() if rc else 0

    def fit_lengths_async(self, d_bits, stream=None):
        self.lib.aws_reset_error()
        rc = self.lib.aws_huffman_amd_engine_fit_lengths(self.h, d_bits, self.d_status, stream)
        return rc, self.lib.aws_last_error() if rc else 0

    def status(self):
        return int(self.download(self.d_status, 4).view(np.uint32)[0])

    def bits(self):
        return [int(b) for b in self.download(self.d_bits, 256)]

    def fit_counts(self, counts):
        """The counts uploaded and fitted on the engine's stream: (status, the 256 bytes of device_num_bits)."""
        self.upload(self.d_counts, np.asarray([int(c) for c in counts], dtype=np.uint64).view(np.uint8))
        self.fill(self.d_status, 0xEE, 4)
        assert self.fit_counts_async() == (0, 0)
        return self.status(), self.bits()

    def fit_lengths(self, lengths):
        """(status) of a fit from these 256 lengths, uploaded to the engine's own 256 bytes."""
        self.upload(self.d_bits, np.asarray(lengths, dtype=np.uint8))
        self.fill(self.d_status, 0xEE, 4)
        assert self.fit_lengths_async(self.d_bits) == (0, 0)
        return self.status()

    def tables(self):
        return engine_tables(self.lib, self.h, self.hi)


def engine_tables(lib, handle, max_bits):
    """aws_huffman_amd_testing_engine_tables: (encode table as uint64[256], decode table as uint16[1 << max_bits])."""
    enc = np.zeros(256, np.uint64)
    lut = np.zeros(1 << max_bits, np.uint16)
    rc = lib.aws_huffman_amd_testing_engine_tables(handle, enc.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   lut.ctypes.data_as(C.POINTER(C.c_uint16)), lut.size)
    assert rc == 0, lib.aws_last_error()
    return enc, lut


# ----------------------------------------------------------------------------- the count vectors of the issue
def printable_counts():
    return ba.bincount(harness.printable_map(harness.splitmix64_bytes(3, 100_000)))


def geometric_bytes(n, seed, p=0.25):
    rng = np.random.default_rng(seed)
    return np.minimum(rng.geometric(p, n) - 1, 255).astype(np.uint8)


def named_vectors():
    one_heavy = [0] * 256
    one_heavy[0x41] = 10 ** 12
    rng = np.random.default_rng(77)
    return [("zero", [0] * 256), ("equal", [7] * 256), ("one heavy", one_heavy), ("skewed", ba.skewed_geometric_counts()),
            ("printable", [int(c) for c in printable_counts()]), ("ties", [int(c) for c in rng.integers(1, 4, 256)]),
            ("2^49 each", [1 << 49] * 256)]


def random_vectors(n=200, seed=78):
    """Half with many equal counts (a handful of small values), half spread over many magnitudes."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 2 == 0:
            out.append(("random ties %d" % i, [int(c) for c in rng.integers(0, int(rng.integers(2, 9)), 256)]))
        else:
            shift = rng.integers(0, 41, 256)
            out.append(("random wide %d" % i, [int(c) >> int(s) for c, s in zip(rng.integers(0, 1 << 48, 256), shift)]))
    return out


def too_large_vector():
    """Sums to exactly 2^58."""
    return [1 << 50] * 256


def host_lengths(lib, counts, lo, hi):
    rc, err, lengths = ba.lengths_from_counts(lib, counts, lo, hi, ba.CODE_EVERY_SYMBOL)
    assert rc == 0, err
    return lengths


def host_rows(lib, lengths):
    """[(pattern, num_bits)] * 256 of aws_huffman_amd_table_coder_from_lengths."""
    coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*lengths))
    assert coder
    rows = ba.coder_rows(coder)
    lib.aws_huffman_amd_table_coder_destroy(coder)
    return rows


def expected_tables(rows, max_bits):
    """The two tables written out from the rows: entry s of the encode table is length << 32 | code; entry w of the decode
    table is symbol << 8 | length of the one code that is a prefix of the max_bits-bit window w, 0 where there is none."""
    enc = np.asarray([(n << 32) | p for p, n in rows], dtype=np.uint64)
    lut = np.zeros(1 << max_bits, np.uint16)
    owned = np.zeros(1 << max_bits, bool)
    for s, (p, n) in enumerate(rows):
        if n:
            first, span = p << (max_bits - n), 1 << (max_bits - n)
            assert not owned[first:first + span].any(), "not a prefix code"
            owned[first:first + span] = True
            lut[first:first + span] = (s << 8) | n
    return enc, lut


def check_fit(lib, eng, counts, label="", tables=True):
    """One fit of `counts` on `eng`: status 0, the device's lengths byte for byte the host's, and (tables) both tables entry
    for entry what the host's canonical coder of those lengths says.  Returns the lengths."""
    status, got = eng.fit_counts(counts)
    want = host_lengths(lib, counts, eng.lo, eng.hi)
    assert status == FIT_OK, (label, eng.lo, eng.hi, status)
    assert got == want, (label, eng.lo, eng.hi, [(s, g, w) for s, (g, w) in enumerate(zip(got, want)) if g != w][:8])
    if tables:
        enc, lut = eng.tables()
        want_enc, want_lut = expected_tables(host_rows(lib, want), eng.hi)
        assert np.array_equal(enc, want_enc), (label, eng.lo, eng.hi, int(np.flatnonzero(enc != want_enc)[0]))
        assert np.array_equal(lut, want_lut), (label, eng.lo, eng.hi, int(np.flatnonzero(lut != want_lut)[0]))
    return want


def oracle_coder(oracle, rows):
    return oracle.lib.oracle_table_coder_new((C.c_uint32 * 256)(*[p for p, _ in rows]), (C.c_uint8 * 256)(*[n for _, n in rows]))


# ----------------------------------------------------------------------------- what the two test files run alike
def run_lengths_equal_host(lib, engines):
    """test_device_lengths_equal_host_lengths: every vector under every bound; then a vector summing to 2^58 is refused and
    leaves the tables as the fit before left them."""
    vectors = named_vectors() + random_vectors()
    for eng in engines:
        for label, counts in vectors:
            check_fit(lib, eng, counts, label, tables=False)
        enc, lut = eng.tables()
        eng.fill(eng.d_bits, 0xAB, 256)
        status, bits = eng.fit_counts(too_large_vector())
        assert status == FIT_COUNTS_TOO_LARGE, (eng.lo, eng.hi, status)
        assert bits == [0xAB] * 256
        enc2, lut2 = eng.tables()
        assert np.array_equal(enc, enc2) and np.array_equal(lut, lut2), (eng.lo, eng.hi)
        # (one count short of it is taken)
        almost = too_large_vector()
        almost[255] -= 1
        check_fit(lib, eng, almost, "2^58 - 1", tables=False)


def run_tables_equal_host(lib, engines):
    """test_device_tables_equal_host_engine_tables: a dozen vectors, both tables."""
    vectors = named_vectors() + random_vectors()[:6]
    for eng in engines:
        for label, counts in vectors:
            check_fit(lib, eng, counts, label)


def run_fit_lengths(lib, first):
    """test_fit_lengths: `first` is a (4, 12) engine.  A receiver fitted from the sender's 256 bytes in device memory has
    the sender's tables; four refusals leave both tables as they were; a Kraft sum below 1 is taken and leaves the windows
    nobody owns 0; a length the engine did not declare is refused."""
    assert (first.lo, first.hi) == (4, 12)
    lengths = check_fit(lib, first, printable_counts(), "printable")
    enc, lut = first.tables()
    second = FittedEngine(lib, 4, 12)
    narrow = FittedEngine(lib, 4, 10)
    try:
        # the receiver's half, from the first engine's own 256 bytes in device memory
        second.fill(second.d_status, 0xEE, 4)
        assert second.fit_lengths_async(first.d_bits) == (0, 0)
        assert second.status() == FIT_OK
        enc2, lut2 = second.tables()
        assert np.array_equal(enc, enc2) and np.array_equal(lut, lut2)
        # refused, the tables as they were
        for bad, why in (([0] + lengths[1:], FIT_LENGTH_ZERO), ([3] + lengths[1:], FIT_LENGTH_OUT_OF_BOUNDS),
                         (lengths[:200] + [13] + lengths[201:], FIT_LENGTH_OUT_OF_BOUNDS), ([7] * 256, FIT_KRAFT_ABOVE_ONE)):
            assert second.fit_lengths(bad) == why, (bad[:4], why)
            enc2, lut2 = second.tables()
            assert np.array_equal(enc, enc2) and np.array_equal(lut, lut2), why
        # Kraft below 1: accepted, and the windows nobody owns say "no code" -- here one pair of 10-bit windows, behind
        # the 9-bit code
        short = [8] * 255 + [9]
        assert narrow.fit_lengths(short) == FIT_OK
        enc3, lut3 = narrow.tables()
        want_enc, want_lut = expected_tables(host_rows(lib, short), 10)
        assert np.array_equal(enc3, want_enc) and np.array_equal(lut3, want_lut)
        assert list(np.flatnonzero(lut3 == 0)) == [1022, 1023]
        # a length the (4, 10) engine did not declare
        assert narrow.fit_lengths([8] * 254 + [7, 11]) == FIT_LENGTH_OUT_OF_BOUNDS
        assert np.array_equal(narrow.tables()[1], want_lut)
    finally:
        second.close()
        narrow.close()


def run_interface_errors(lib):
    """test_interface_errors: bounds, devices and pointers aws_huffman_amd_engine_new_fitted refuses (the caller's pointer
    as it was); NULL and plain-engine arguments of the fits; the never-fitted state -- plans are made, no launch is taken,
    nothing is written -- and the same plans taken behind the first fit; the optional status and lengths."""
    h = C.c_void_p(0x1234)
    for lo, hi in ((3, 12), (4, 13), (8, 8), (9, 12), (4, 7)):
        lib.aws_reset_error()
        assert lib.aws_huffman_amd_engine_new_fitted(C.byref(h), -1, lo, hi) == -1, (lo, hi)
        assert lib.aws_last_error() == harness.AWS_ERROR_INVALID_ARGUMENT and h.value == 0x1234, (lo, hi)
    # (the first device that does not exist: a node of eight has a device 7)
    assert new_fitted(lib, 4, 12, device=lib.aws_huffman_amd_device_count())[:2] == INVALID
    lib.aws_reset_error()
    assert lib.aws_huffman_amd_engine_new_fitted(None, -1, 4, 12) == -1
    assert lib.aws_last_error() == harness.AWS_ERROR_INVALID_ARGUMENT

    eng = FittedEngine(lib, 5, 11)
    patterns, lens = harness.load_table()
    coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    plain = harness.Engine(lib, coder)
    d_in, d_out, d_off = eng.alloc(4096), eng.alloc(4096), eng.alloc(64)
    plan = dplan = None
    try:
        assert lib.aws_huffman_amd_engine_is_fitted(eng.h) and not lib.aws_huffman_amd_engine_is_fitted(plain.h)
        assert lib.aws_huffman_amd_engine_max_code_bits(eng.h) == 11
        assert lib.aws_huffman_amd_engine_can_decode(eng.h) and lib.aws_huffman_amd_engine_encodes_in_one_pass(eng.h)

        def error_of(call, *args):
            lib.aws_reset_error()
            rc = call(*args)
            return rc, lib.aws_last_error() if rc else 0

        # NULL arguments, an engine with a coder
        fit_counts, fit_lengths = lib.aws_huffman_amd_engine_fit_counts, lib.aws_huffman_amd_engine_fit_lengths
        assert error_of(fit_counts, None, eng.d_counts, eng.d_bits, eng.d_status, None) == INVALID
        assert error_of(fit_counts, eng.h, None, eng.d_bits, eng.d_status, None) == INVALID
        assert error_of(fit_lengths, None, eng.d_bits, eng.d_status, None) == INVALID
        assert error_of(fit_lengths, eng.h, None, eng.d_status, None) == INVALID
        assert error_of(fit_counts, plain.h, eng.d_counts, eng.d_bits, eng.d_status, None) == INVALID
        assert error_of(fit_lengths, plain.h, eng.d_bits, eng.d_status, None) == INVALID
        assert error_of(lib.aws_huffman_amd_testing_engine_tables, eng.h, None, None, 1 << 11) == INVALID

        # never fitted: plans are made (their geometry is the bounds'), no launch is taken, nothing is written
        eng.fill(d_in, 0x41, 4096)
        eng.fill(d_out, 0xC3, 4096)
        eng.fill(d_off, 0xEE, 64)
        plan = eng.encode_plan([dict(in_offset=0, in_len=1000, out_offset=0, out_capacity=2000)])
        dplan = eng.decode_plan([dict(in_offset=0, in_len=1000, out_offset=0, out_capacity=2000)])
        state = (-1, AWS_ERROR_INVALID_STATE)
        assert error_of(lib.aws_huffman_amd_encode_plan_launch, plan, d_in, d_out, False, None) == state
        assert error_of(lib.aws_huffman_amd_encode_plan_launch, plan, d_in, d_out, True, None) == state
        assert error_of(lib.aws_huffman_amd_encode_plan_launch_packed, plan, d_in, d_out, 4096, d_off, 1, None) == state
        assert error_of(lib.aws_huffman_amd_decode_plan_launch, dplan, d_in, d_out, None) == state
        assert error_of(lib.aws_huffman_amd_decode_plan_launch_packed, dplan, d_in, d_out, 4096, d_off, 1, None) == state
        eng.sync()
        assert np.all(eng.download(d_out, 4096) == 0xC3) and np.all(eng.download(d_off, 64) == 0xEE)
        # ... and behind the first fit the same plans are
        status, _ = eng.fit_counts(printable_counts())
        assert status == FIT_OK
        assert error_of(lib.aws_huffman_amd_encode_plan_launch, plan, d_in, d_out, False, None) == (0, 0)
        eng.sync()
        # the status and the lengths are optional
        assert error_of(fit_counts, eng.h, eng.d_counts, None, None, None) == (0, 0)
        assert error_of(fit_lengths, eng.h, eng.d_bits, None, None) == (0, 0)
        eng.sync()
    finally:
        if plan:
            lib.aws_huffman_amd_encode_plan_destroy(plan)
        if dplan:
            lib.aws_huffman_amd_decode_plan_destroy(dplan)
        for d in (d_in, d_out, d_off):
            eng.free(d)
        eng.close()
        plain.close()
        lib.aws_huffman_amd_table_coder_destroy(coder)


# ----------------------------------------------------------------------------- data shapes, and a fitted engine against the oracle
SHAPES = ["printable", "geometric", "uniform", "one byte"]
PARITY_SIZES = [0, 1, 15, 300, 3000, 40000, 100003]  # nothing, a thread's or a wave's, three segments / two chunks, many


def shape_bytes(shape, n, seed):
    if shape == "printable":
        return harness.printable_map(harness.splitmix64_bytes(seed, n))
    if shape == "geometric":
        return geometric_bytes(n, seed)
    if shape == "uniform":
        return harness.splitmix64_bytes(seed, n)
    assert shape == "one byte"
    return np.full(n, 0x5A, np.uint8)


def is_flat(lengths):
    return min(lengths) == max(lengths)


class Fit:
    """What one fit of `counts` on `eng` comes to, checked against the host on the way: the lengths, the canonical rows, the
    oracle's coder of those rows."""

    def __init__(self, lib, oracle, eng, counts, label=""):
        self.lengths = check_fit(lib, eng, counts, label)
        self.rows = host_rows(lib, self.lengths)
        self.ocoder = oracle_coder(oracle, self.rows)
        self.code_lens = np.asarray(self.lengths, dtype=np.int64)


def decode_room(n_bytes, lengths):
    """Room for everything n_bytes of input can decode to."""
    return n_bytes * 8 // min(lengths) + 8


def parity_data(shape):
    """The symbols run_parity fits and codes for `shape`: PARITY_SIZES items cut from one array."""
    return shape_bytes(shape, sum(PARITY_SIZES), 41)


def sweep_lengths(lib, bounds, shape):
    """The host's lengths for parity_data(shape) under `bounds`: what run_parity's fit must come to (check_fit)."""
    return host_lengths(lib, ba.bincount(parity_data(shape)), *bounds)


def run_sweep_saw_a_spread(lib, cases):
    """cases: the (bounds, shape) pairs a file's parity tests run.  Bounds with min_bits == 8 or max_bits == 8 give the flat
    8-bit code whatever the data (Kraft, 256 coded symbols); every other pair of bounds must meet at least one shape whose
    code has more than one length -- or the sweep tests flat codes only and says nothing of the bounds."""
    seen = {}
    for bounds, shape in cases:
        seen.setdefault(bounds, {})[shape] = sorted(set(sweep_lengths(lib, bounds, shape)))
    assert set(seen) == set(BOUNDS), sorted(set(BOUNDS) - set(seen))
    for (lo, hi), by_shape in seen.items():
        if only_flat(lo, hi):
            assert all(ls == [8] for ls in by_shape.values()), ((lo, hi), by_shape)
    flat_only = {b: by_shape for b, by_shape in seen.items() if not only_flat(*b) and all(len(ls) == 1 for ls in by_shape.values())}
    assert not flat_only, "bounds whose shapes all fitted a flat code; the sets of lengths seen per pair: %r" % (seen,)


def run_parity(lib, oracle, bounds, shape, road=None, decode=True):
    """test_fitted_engine_parity for one data shape on one engine fitted within `bounds`, made under the encode road `road`
    (harness.ENCODE_ROADS): the batch through every encode and (decode=True) decode launch, record for record and byte for
    byte against the oracle's table coder of the canonical rows."""
    with harness.encode_road(lib, road):
        eng = FittedEngine(lib, *bounds)
    try:
        _parity(lib, oracle, eng, shape, road, decode)
    finally:
        eng.close()


def _parity(lib, oracle, eng, shape, road, decode):
    want_road = ROAD_OF[road]
    rng = np.random.default_rng(SHAPES.index(shape) + 500)
    data = parity_data(shape)
    cuts = np.cumsum([0] + PARITY_SIZES)
    blobs = [data[a:b].copy() for a, b in zip(cuts[:-1], cuts[1:])]
    n = len(blobs)
    fit = Fit(lib, oracle, eng, ba.bincount(data), shape)  # (the device's lengths are the host's: check_fit)
    if only_flat(eng.lo, eng.hi):
        assert fit.lengths == [8] * 256, (eng.lo, eng.hi, sorted(set(fit.lengths)))
    if (eng.lo, eng.hi) == (4, 12):
        assert is_flat(fit.lengths) == (shape == "uniform"), sorted(set(fit.lengths))
    assert min(fit.lengths) >= eng.lo and max(fit.lengths) <= eng.hi
    # (the one-pass rule reads the bounds, 4 <= min_bits and max_bits <= 12 for every fitted engine; the road switch decides)
    assert bool(lib.aws_huffman_amd_engine_encodes_in_one_pass(eng.h)) == (road != "three-kernel")
    host_in, in_offs = pa.lay_out(blobs, rng, first=1)
    enc_lens = pa.encoded_lengths(fit.code_lens, blobs, [0] * n)
    caps = [int(l) + 2 for l in enc_lens]
    out_offs = [int(o) for o in np.cumsum([3] + [c + 3 for c in caps])[:-1]]
    out_size = out_offs[-1] + caps[-1] + 64
    overflows, eoss = [(0, 0)] * n, [[0xFF, 0x00][i % 2] for i in range(n)]
    d_in, d_out, d_back = eng.alloc(host_in.size), eng.alloc(out_size), eng.alloc(host_in.size)
    eng.upload(d_in, host_in)
    items = [dict(in_offset=in_offs[i], in_len=int(blobs[i].size), out_offset=out_offs[i], out_capacity=caps[i],
                  eos_padding=eoss[i]) for i in range(n)]
    plan = eng.encode_plan(items)
    plans, extra = [], []
    try:
        stats = eng.encode_stats(plan)
        if road != "three-kernel":
            assert stats["by_thread"] >= 2 and stats["by_wave"] >= 1 and stats["by_pieces"] >= 2, stats
        else:  # (no bound decides this one but the road: count / scan / pack has no wave's class, the 3000 symbols go by pieces)
            assert stats["by_thread"] >= 2 and stats["by_wave"] == 0 and stats["by_pieces"] >= 3, stats
        label = "%s %r %s" % (shape, (eng.lo, eng.hi), road)
        # the packed launch, then the plain one (whose output the decodes below read)
        pa.check_launch(oracle, fit.ocoder, eng, plan, d_in, blobs, fit.code_lens, overflows, eoss, 1, want_road=want_road,
                        label=label)
        eng.fill(d_out, pa.MARKER, out_size)
        eng.encode_launch(plan, d_in, d_out)
        got = eng.download(d_out, out_size)
        res = eng.encode_results(plan, n)
        assert eng.encode_road(plan) == want_road, (label, eng.encode_road(plan))
        want = np.full(out_size, pa.MARKER, np.uint8)
        streams = []
        for i in range(n):
            rec, enc = pa.oracle_item(oracle, fit.ocoder, blobs[i], (0, 0), eoss[i], caps[i])
            assert res[i] == rec and rec[:2] == (0, 0) and rec[3] == enc_lens[i], (shape, i, res[i], rec)
            want[out_offs[i]:out_offs[i] + caps[i]] = enc
            streams.append((enc[:rec[3]].copy(), 0))
        assert np.array_equal(got, want), (label, int(np.flatnonzero(got != want)[0]))
        if not decode:
            return

        def check_back(dplan, label):
            eng.fill(d_back, pa.MARKER, host_in.size)
            eng.decode_launch(dplan, d_out, d_back)
            back = eng.download(d_back, host_in.size)
            dres = eng.decode_results(dplan, n)
            want_back = np.full(host_in.size, pa.MARKER, np.uint8)
            for i in range(n):
                rec, syms = pda.oracle_item(oracle, fit.ocoder, streams[i][0], 0, int(blobs[i].size))
                assert dres[i] == rec, (shape, label, i, dres[i], rec)
                assert np.array_equal(syms, blobs[i])
                want_back[in_offs[i]:in_offs[i] + blobs[i].size] = syms
            assert np.array_equal(back, want_back), (shape, label, int(np.flatnonzero(back != want_back)[0]))
            # (chunked whatever the code is: the road is the bounds', a flat code in a fitted engine has no road of its own)
            dstats = eng.decode_stats(dplan)
            assert dstats["by_pieces"] > 0 and dstats["by_blocks"] == 0, (shape, label, dstats)

        # decode: a plan of host items, a plan chained to the encode plan, a packed launch over offsets and lengths
        dplan = eng.decode_plan([dict(in_offset=out_offs[i], in_len=int(enc_lens[i]), out_offset=in_offs[i],
                                      out_capacity=int(blobs[i].size)) for i in range(n)])
        plans.append(dplan)
        check_back(dplan, "plain")
        chained = eng.empty_decode_plan()
        plans.append(chained)
        assert eng.decode_plan_from_encode(chained, plan)
        check_back(chained, "from encode")
        packed = eng.empty_decode_plan()
        plans.append(packed)
        d_offs, d_lens = pda.upload_u64(eng, out_offs + [out_offs[-1] + caps[-1]]), pda.upload_u64(eng, enc_lens)
        extra += [d_offs, d_lens]
        assert pda.reset_packed_input(eng, packed, d_offs, d_lens, n) == (0, 0)
        expect = pda.Expect(oracle, fit.ocoder, streams, min(fit.lengths))
        for i in range(n):
            assert np.array_equal(expect.full[i][1][:blobs[i].size], blobs[i]), (shape, i)
        pda.check_launch(eng, packed, d_out, expect, 1, label=shape + " packed decode")

        # arbitrary bytes, and a valid stream with one byte overwritten: the oracle's results and symbols
        arbitrary = harness.splitmix64_bytes(43, 40000)
        broken = streams[-1][0].copy()
        broken[broken.size // 3] ^= 0x5D
        for label, enc in (("arbitrary", arbitrary), ("broken", broken)):
            cap = decode_room(enc.size, fit.lengths)
            d_e, d_s = eng.alloc(enc.size), eng.alloc(cap + 64)
            extra += [d_e, d_s]
            eng.upload(d_e, enc)
            eng.fill(d_s, pa.MARKER, cap + 64)
            one = eng.decode_plan([dict(in_offset=0, in_len=int(enc.size), out_offset=0, out_capacity=cap)])
            plans.append(one)
            eng.decode_launch(one, d_e, d_s)
            out = eng.download(d_s, cap + 64)
            rec, syms = pda.oracle_item(oracle, fit.ocoder, enc, 0, cap)
            assert eng.decode_results(one, 1)[0] == rec, (shape, label, rec)
            assert np.array_equal(out[:cap], syms) and np.all(out[cap:] == pa.MARKER), (shape, label)
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        for p in plans:
            lib.aws_huffman_amd_decode_plan_destroy(p)
        for d in [d_in, d_out, d_back] + extra:
            eng.free(d)


def run_refit_between_launches(lib, oracle, eng, n_bytes):
    """test_refit_between_launches_of_one_plan: fit(A), launch, fit(B), launch on one stream with no host wait between the
    steps -- each buffer is what the oracle makes with its own fit's coder; then the same for one decode plan."""
    a, b = shape_bytes("printable", n_bytes, 61), shape_bytes("geometric", n_bytes, 62)
    data = np.concatenate([a[:n_bytes // 2], b[:n_bytes - n_bytes // 2]])  # (either coder has something to do)
    counts = [ba.bincount(a), ba.bincount(b)]
    lengths = [host_lengths(lib, c, eng.lo, eng.hi) for c in counts]
    ocoders = [oracle_coder(oracle, host_rows(lib, l)) for l in lengths]
    sizes = [n_bytes - 300 - 4097, 300, 4097]
    cuts = np.cumsum([0] + sizes)
    blobs = [data[x:y] for x, y in zip(cuts[:-1], cuts[1:])]
    n = len(blobs)
    caps = [int(s) * eng.hi // 8 + 8 for s in sizes]
    out_offs = [int(o) for o in np.cumsum([0] + caps)[:-1]]
    out_size = sum(caps)
    d_in, d_counts = eng.alloc(n_bytes), [eng.alloc(256 * 8), eng.alloc(256 * 8)]
    d_out, d_back = [eng.alloc(out_size), eng.alloc(out_size)], [eng.alloc(n_bytes), eng.alloc(n_bytes)]
    eng.upload(d_in, data)
    for k in range(2):
        eng.upload(d_counts[k], counts[k].view(np.uint8))
        eng.fill(d_out[k], pa.MARKER, out_size)
        eng.fill(d_back[k], pa.MARKER, n_bytes)
    items = [dict(in_offset=int(cuts[i]), in_len=sizes[i], out_offset=out_offs[i], out_capacity=caps[i]) for i in range(n)]
    plan = eng.encode_plan(items)
    # (one decode plan for both buffers: every item's input is its whole room, its output as many symbols as went in)
    dplan = eng.decode_plan([dict(in_offset=out_offs[i], in_len=caps[i], out_offset=int(cuts[i]), out_capacity=sizes[i])
                             for i in range(n)])
    try:
        st = eng.stream
        # (plans depend on the bounds alone: what they report is the same behind either fit)
        estats, dstats = [eng.encode_stats(plan)], [eng.decode_stats(dplan)]
        for k in range(2):
            assert eng.fit_counts_async(d_counts[k], st) == (0, 0)
            assert lib.aws_huffman_amd_encode_plan_launch(plan, d_in, d_out[k], False, st) == 0
            estats.append(eng.encode_stats(plan))
        eng.sync()
        res = eng.encode_results(plan, n)
        estats.append(eng.encode_stats(plan))
        assert all(e == estats[0] for e in estats), estats
        bufs = [eng.download(d_out[k], out_size) for k in range(2)]
        for k in range(2):
            for i in range(n):
                rec, enc = pa.oracle_item(oracle, ocoders[k], blobs[i], (0, 0), 0xFF, caps[i])
                assert rec[:2] == (0, 0)
                assert np.array_equal(bufs[k][out_offs[i]:out_offs[i] + caps[i]], enc), ("encode", k, i)
                if k == 1:
                    assert res[i] == rec, (i, res[i], rec)
        assert not np.array_equal(bufs[0], bufs[1])
        for k in range(2):
            assert eng.fit_counts_async(d_counts[k], st) == (0, 0)
            assert lib.aws_huffman_amd_decode_plan_launch(dplan, d_out[k], d_back[k], st) == 0
            dstats.append(eng.decode_stats(dplan))
        eng.sync()
        dres = eng.decode_results(dplan, n)
        dstats.append(eng.decode_stats(dplan))
        assert all(d == dstats[0] for d in dstats), dstats
        for k in range(2):
            back = eng.download(d_back[k], n_bytes)
            assert np.array_equal(back, data), ("decode", k, int(np.flatnonzero(back != data)[0]))
        for i in range(n):
            rec, _ = pda.oracle_item(oracle, ocoders[1], bufs[1][out_offs[i]:out_offs[i] + caps[i]], 0, sizes[i])
            assert dres[i] == rec, (i, dres[i], rec)
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        lib.aws_huffman_amd_decode_plan_destroy(dplan)
        for d in [d_in] + d_counts + d_out + d_back:
            eng.free(d)


# ----------------------------------------------------------------------------- a receiver's code, whatever lengths it was sent
RECEIVER_CODES = [  # (bounds, 256 lengths): Kraft sum at most 1 by arithmetic, most of them below 1 (windows without a code)
    ((8, 12), [9] * 256), ((4, 10), [8] * 255 + [9]), ((4, 12), [9] * 256), ((8, 12), [8] * 255 + [12]),
    ((4, 12), [5] * 16 + [9] * 240), ((4, 8), [8] * 256),
    ((4, 11), [11] * 256), ((7, 9), [7] * 64 + [9] * 192), ((6, 11), [6] * 32 + [11] * 224)]


def receiver_id(case):
    (lo, hi), lengths = case
    runs = []
    for l in lengths:
        if runs and runs[-1][0] == l:
            runs[-1][1] += 1
        else:
            runs.append([l, 1])
    return "%d..%d:" % (lo, hi) + "+".join("%dx%d" % (c, l) for l, c in runs)


def run_receiver_codes(lib, oracle, bounds, lengths, kinds=("matched", "uniform"), enc_bytes=120_000):
    """An engine within `bounds` fitted by aws_huffman_amd_engine_fit_lengths from `lengths` (any the interface takes: the
    Kraft sum may be below 1, the decode table then has windows without a code).  Symbols drawn by 2^-length ("matched") and evenly
    ("uniform"), about enc_bytes encoded (three to four decode chunks): one plan encode against the oracle's table coder of the
    canonical rows; the stream whole, damaged, overwritten with ones and with zeros, cut, short of room, its first bytes,
    entered inside a byte, and arbitrary bytes through three decode roads, every record and byte the oracle's; both
    tables against the rows."""
    lo, hi = bounds
    assert len(lengths) == 256 and all(lo <= l <= hi for l in lengths), bounds
    assert sum(1 << (hi - l) for l in lengths) <= 1 << hi, "Kraft sum above 1"
    shortest = min(lengths)
    rows = host_rows(lib, lengths)
    ocoder = oracle_coder(oracle, rows)
    w = types.SimpleNamespace(oracle=oracle)  # (all that parity_cases.decode_items_like_the_oracle asks of a World)
    eng = FittedEngine(lib, lo, hi)
    try:
        assert eng.fit_lengths(lengths) == FIT_OK
        for kind in kinds:
            rng = np.random.default_rng([601, lo, hi, ("matched", "uniform").index(kind)])
            data = pc.shape_data(rng, lengths, kind, enc_bytes)
            n = int(data.size)
            enc = oracle.encode_all(ocoder, data, eos_padding=0xFF)
            # ---- encode: a plan of one item
            cap = int(enc.size) + 8
            d_in, d_out = eng.alloc(n), eng.alloc(cap + 8)
            plan = eng.encode_plan([dict(in_offset=0, in_len=n, out_offset=3, out_capacity=cap, eos_padding=0xFF)])
            try:
                eng.upload(d_in, data)
                eng.fill(d_out, pa.MARKER, cap + 8)
                eng.encode_launch(plan, d_in, d_out)
                rec, want = pa.oracle_item(oracle, ocoder, data, (0, 0), 0xFF, cap)
                assert rec[:4] == (0, 0, n, enc.size) and np.array_equal(want[:enc.size], enc)
                assert eng.encode_results(plan, 1) == [rec], (bounds, kind)
                out = eng.download(d_out, cap + 8)
                assert np.array_equal(out[3:3 + cap], want) and np.all(out[:3] == pa.MARKER) and np.all(out[3 + cap:] == pa.MARKER)
            finally:
                lib.aws_huffman_amd_encode_plan_destroy(plan)
                eng.free(d_in)
                eng.free(d_out)
            # ---- decode
            third, half = enc.size // 3, enc.size // 2
            damaged, ones, zeros = enc.copy(), enc.copy(), enc.copy()
            damaged[half:half + 4] ^= 0xA5
            ones[third:third + 6] = 0xFF
            zeros[third:third + 6] = 0x00
            inside = enc[5:5 + 70000]
            noise = rng.integers(0, 256, 40000).astype(np.uint8)
            streams = [(enc, 0, n), (damaged, 0, n), (ones, 0, n), (zeros, 0, n), (enc[:third + 5], 0, n), (enc, 0, n // 2 + 3),
                       (enc[:700], 0, 700 * 8 // shortest + 8), (inside, 3, inside.size * 8 // shortest + 8),
                       (noise, 0, noise.size * 8 // shortest + 8)]
            pc.decode_items_like_the_oracle(w, eng, ocoder, streams, rng, "receiver %r, %s data" % (bounds, kind),
                                            modes=(None, "long-way", "tails-apart"), kinds=2)
        enc_table, lut = eng.tables()
        want_enc, want_lut = expected_tables(rows, hi)
        assert np.array_equal(enc_table, want_enc) and np.array_equal(lut, want_lut), bounds
    finally:
        eng.close()
        oracle.lib.oracle_table_coder_destroy(ocoder)


# ----------------------------------------------------------------------------- chains on one stream (the GPU tests)
class Hip(pa.HipGraphs):
    """packed_api.HipGraphs and the one more runtime call a chain needs: a memset that is a command of the stream."""

    def __init__(self):
        super().__init__()
        self.hip.hipMemsetAsync.restype = C.c_int
        self.hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]

    def memset_async(self, dptr, byte, size, stream):
        self.call("hipMemsetAsync", dptr, byte, size, stream)


def enqueue_chain(hip, eng, plan, d_in, length, d_out, capacity, d_off, stream, align=1):
    """zero the counts, count, fit, packed encode: four steps on `stream`, nothing waited for."""
    lib = eng.lib
    hip.memset_async(eng.d_counts, 0, 256 * 8, stream)
    assert lib.aws_huffman_amd_symbol_counts(-1, d_in, length, eng.d_counts, stream) == 0
    assert eng.fit_counts_async(None, stream) == (0, 0)
    assert pa.launch_packed(eng, plan, d_in, d_out, capacity, d_off, align, stream) == (0, 0)


def check_chain_output(lib, oracle, eng, plan, data, blobs, d_out, d_off, capacity):
    """Behind a chain over `data` whose plan's items are `blobs`: the fetched lengths are the host's for the data's counts,
    and offsets, records and bytes are the oracle's with the coder of those lengths.  Returns (lengths, offsets)."""
    n = len(blobs)
    assert eng.status() == FIT_OK
    lengths = host_lengths(lib, ba.bincount(data), eng.lo, eng.hi)
    assert eng.bits() == lengths
    ocoder = oracle_coder(oracle, host_rows(lib, lengths))
    code_lens = np.asarray(lengths, dtype=np.int64)
    offsets, reserved = pa.expected_offsets(pa.encoded_lengths(code_lens, blobs, [0] * n), 1)
    assert int(offsets[-1]) <= capacity
    assert np.array_equal(pa.download_u64(eng, d_off, n + 1), offsets)
    got = eng.download(d_out, int(offsets[-1]))
    res = pa.results_array(eng, plan, n)
    assert eng.encode_road(plan) == ROAD_ONE_PASS
    assert np.all(res["rc"] == 0) and np.array_equal(res["produced"].astype(np.int64), reserved)
    assert np.array_equal(res["consumed"].astype(np.int64), [b.size for b in blobs])
    for i, blob in enumerate(blobs):
        want = oracle.encode_all(ocoder, blob, eos_padding=0xFF)
        mine = got[int(offsets[i]):int(offsets[i + 1])]
        assert np.array_equal(mine, want), (i, blob.size)
    return lengths, offsets
