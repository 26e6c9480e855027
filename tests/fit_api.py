"""ctypes face of include/aws/compression/huffman_amd_fit.h (coders fitted on the device) and what its tests share: the
count vectors, the host's lengths and the tables written out in Python from the canonical rows, one check of a fit against
both, and the oracle's coder of a fit.  Used by tests/test_emulated_fit.py (emulator build) and tests/test_gpu_fit.py
(MI355X).  Nothing here asks a second engine what a table should hold."""
import ctypes as C

import numpy as np

import build_api as ba
import harness
import packed_api as pa
import packed_decode_api as pda

AWS_ERROR_INVALID_STATE = 38
FIT_OK, FIT_COUNTS_TOO_LARGE, FIT_LENGTH_ZERO, FIT_LENGTH_OUT_OF_BOUNDS, FIT_KRAFT_ABOVE_ONE = 0, 1, 2, 3, 4
BOUNDS = [(4, 12), (4, 10), (5, 9), (7, 8), (4, 8), (8, 12)]
ROAD_ONE_PASS = 1


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


def run_parity(lib, oracle, eng, shape):
    """test_fitted_engine_parity for one data shape on one fitted engine: the batch through every encode and decode launch,
    record for record and byte for byte against the oracle's table coder of the canonical rows."""
    rng = np.random.default_rng(SHAPES.index(shape) + 500)
    data = shape_bytes(shape, sum(PARITY_SIZES), 41)
    cuts = np.cumsum([0] + PARITY_SIZES)
    blobs = [data[a:b].copy() for a, b in zip(cuts[:-1], cuts[1:])]
    n = len(blobs)
    fit = Fit(lib, oracle, eng, ba.bincount(data), shape)
    assert is_flat(fit.lengths) == (shape == "uniform"), sorted(set(fit.lengths))
    assert lib.aws_huffman_amd_engine_encodes_in_one_pass(eng.h)
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
        assert stats["by_thread"] >= 2 and stats["by_wave"] >= 1 and stats["by_pieces"] >= 2, stats
        # the packed launch, then the plain one (whose output the decodes below read)
        pa.check_launch(oracle, fit.ocoder, eng, plan, d_in, blobs, fit.code_lens, overflows, eoss, 1, want_road=ROAD_ONE_PASS,
                        label=shape)
        eng.fill(d_out, pa.MARKER, out_size)
        eng.encode_launch(plan, d_in, d_out)
        got = eng.download(d_out, out_size)
        res = eng.encode_results(plan, n)
        assert eng.encode_road(plan) == ROAD_ONE_PASS
        want = np.full(out_size, pa.MARKER, np.uint8)
        streams = []
        for i in range(n):
            rec, enc = pa.oracle_item(oracle, fit.ocoder, blobs[i], (0, 0), eoss[i], caps[i])
            assert res[i] == rec and rec[:2] == (0, 0) and rec[3] == enc_lens[i], (shape, i, res[i], rec)
            want[out_offs[i]:out_offs[i] + caps[i]] = enc
            streams.append((enc[:rec[3]].copy(), 0))
        assert np.array_equal(got, want), (shape, int(np.flatnonzero(got != want)[0]))

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
            dstats = eng.decode_stats(dplan)
            if not is_flat(fit.lengths):
                assert dstats["by_pieces"] > 0, (shape, label, dstats)

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
        for k in range(2):
            assert eng.fit_counts_async(d_counts[k], st) == (0, 0)
            assert lib.aws_huffman_amd_encode_plan_launch(plan, d_in, d_out[k], False, st) == 0
        eng.sync()
        res = eng.encode_results(plan, n)
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
        eng.sync()
        dres = eng.decode_results(dplan, n)
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
