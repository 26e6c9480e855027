"""ctypes face of include/aws/compression/huffman_amd_batch_index.h (one block index over the items of an encode plan) and
what its tests share.  Used by tests/test_emulated_batch_index.py (emulator build) and tests/test_gpu_batch_index.py
(MI355X): every run_* scenario below is called by both, at the same sizes.

Expected values never come from the library under test: the directory is the running sum of ceil(len / B) over the items;
the index is numpy's cumsum of the coder's code lengths per item, taken at the item's block edges and chained over the batch
(and pinned to the oracle's length query at the first, a middle and the last item); launches behind an index call are
checked against the oracle by packed_api.check_launch."""
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
import ranges_api as ra

INDEX_OK, INDEX_SYMBOL_WITHOUT_CODE, INDEX_TOO_SMALL = 0, 1, 2
INVALID, UNSUPPORTED, STATE = ia.INVALID, ia.UNSUPPORTED, ia.STATE
GUARD_WORDS = 4  # uint64 words behind the directory and behind the index that a call must leave alone
EE = 0xEEEEEEEEEEEEEEEE
WAVE_RULE = 4096  # items shorter than this are a wave's work (BATCH_INDEX_WAVE_BYTES)
ALL_WAVES, ALL_TILES = 1 << 16, 1  # what the testing switch takes for "every item a wave's" / "every item in tiles"
HEADER = os.path.join(harness.REPO, "include", "aws", "compression", "huffman_amd_batch_index.h")


def bind(lib):
    """Declares the entry points of huffman_amd_batch_index.h (and of the headers in front of it) on a loaded library."""
    ra.bind(lib)
    pda.bind(lib)
    V, U = C.c_void_p, C.c_uint64
    lib.aws_huffman_amd_decode_plan_reset_item_block_ranges.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_reset_item_block_ranges.argtypes = [V, V, V, U, U, U, V, V, U, U, V, C.c_size_t, V]
    lib.aws_huffman_amd_decode_plan_reset_item_symbol_ranges.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_reset_item_symbol_ranges.argtypes = [V, V, V, V, U, U, U, V, V, U, U, V, C.c_size_t, V]
    lib.aws_huffman_amd_locate_item_symbols.restype = C.c_int
    lib.aws_huffman_amd_locate_item_symbols.argtypes = [V, V, U, V, V, U, U, U, V, V, V, V, C.c_size_t, V, V, V]
    lib.aws_huffman_amd_encode_plan_block_index.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_block_index.argtypes = [V, V, C.c_uint64, V, V, C.c_uint64, V, V]
    lib.aws_huffman_amd_encode_plan_block_index_size.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_block_index_size.argtypes = [V, C.POINTER(C.c_uint64), V]
    lib.aws_huffman_amd_testing_set_batch_index_wave_bytes.restype = None
    lib.aws_huffman_amd_testing_set_batch_index_wave_bytes.argtypes = [C.c_uint64]
    return lib


class wave_bytes:
    """with wave_bytes(lib, ALL_TILES): batch index calls inside cut every item into tiles (restored to the rule behind it)."""

    def __init__(self, lib, limit):
        self.lib, self.limit = lib, limit

    def __enter__(self):
        self.lib.aws_huffman_amd_testing_set_batch_index_wave_bytes(self.limit)

    def __exit__(self, *exc):
        self.lib.aws_huffman_amd_testing_set_batch_index_wave_bytes(0)


def plan_block_index(eng, plan, d_in, block_symbols, d_dir, d_index, capacity, d_status, stream=None):
    """(rc, error) of the enqueue."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_encode_plan_block_index(plan, d_in, int(block_symbols), d_dir, d_index, int(capacity), d_status,
                                                         stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def index_size(eng, plan, stream=None):
    """(rc, error, entries)."""
    entries = C.c_uint64(0xEE)
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_encode_plan_block_index_size(plan, C.byref(entries), stream)
    return rc, eng.lib.aws_last_error() if rc else 0, entries.value


def expected(code_lens, blobs, block_symbols):
    """(directory as int64[n + 1][2], index as int64[total_blocks + 1]) from the definition."""
    code_lens = np.asarray(code_lens, dtype=np.int64)
    directory = np.zeros((len(blobs) + 1, 2), np.int64)
    parts, base, first = [np.zeros(1, np.int64)], 0, 0
    for i, blob in enumerate(blobs):
        directory[i] = (first, blob.size)
        own = ia.expected_index(code_lens, blob, block_symbols)  # own[0] = 0 .. own[nb] = the item's bits
        parts.append(base + own[1:])
        base += int(own[-1])
        first += own.size - 1
    directory[len(blobs)] = (first, 0)
    return directory, np.concatenate(parts)


def pin_to_oracle(oracle, ocoder, blobs, directory, index):
    """ceil(bits of an item / 8) from the index against aws_huffman_get_encoded_length, for the first, a middle and the last item."""
    n = len(blobs)
    for i in sorted({0, n // 2, n - 1}) if n else []:
        bits = int(index[directory[i + 1][0]] - index[directory[i][0]])
        want = oracle.encoded_length(oracle.new_encoder(ocoder), blobs[i])
        assert (bits + 7) // 8 == want, (i, bits, want)


class Arrays:
    """The three outputs of a call, at the END of their allocations' useful part: 0xEE everywhere before the call, guard
    words behind the directory and behind `capacity` entries of the index."""

    def __init__(self, eng, n_items, capacity):
        self.eng, self.n, self.capacity = eng, n_items, int(capacity)
        self.dir_bytes = 16 * (n_items + 1) + 8 * GUARD_WORDS
        self.index_bytes = 8 * (self.capacity + GUARD_WORDS)
        self.d_dir, self.d_index, self.d_status = eng.alloc(self.dir_bytes), eng.alloc(self.index_bytes), eng.alloc(8)
        self.refill()

    def refill(self):
        self.eng.fill(self.d_dir, 0xEE, self.dir_bytes)
        self.eng.fill(self.d_index, 0xEE, self.index_bytes)
        self.eng.fill(self.d_status, 0xEE, 8)

    def read(self):
        """(directory int64[n + 1][2], the `capacity` index words as uint64, status); the guards are checked here."""
        eng = self.eng
        d = eng.download(self.d_dir, self.dir_bytes).view(np.uint64)
        x = eng.download(self.d_index, self.index_bytes).view(np.uint64)
        s = eng.download(self.d_status, 8).view(np.uint32)
        assert np.all(d[2 * (self.n + 1):] == EE), "words behind the directory were written"
        assert np.all(x[self.capacity:] == EE), "words behind the index's capacity were written"
        assert s[1] == 0xEEEEEEEE, "the word behind the status was written"
        return d[:2 * (self.n + 1)].astype(np.int64).reshape(-1, 2), x[:self.capacity], int(s[0])

    def close(self):
        for d in (self.d_dir, self.d_index, self.d_status):
            self.eng.free(d)


def device_index(eng, plan, d_in, n_items, block_symbols, capacity, stream=None):
    """One call into fresh arrays of `capacity` entries: (directory, index words, status)."""
    a = Arrays(eng, n_items, capacity)
    try:
        assert plan_block_index(eng, plan, d_in, block_symbols, a.d_dir, a.d_index, capacity, a.d_status, stream) == (0, 0)
        eng.sync()
        return a.read()
    finally:
        a.close()


def check_batch(sc, eng, plan, d_in, blobs, code_lens, ocoder, block_symbols, want_status=INDEX_OK, label="", slack=0):
    """A call with capacity total_blocks + 1 + slack against the definition; returns (directory, index) as expected."""
    want_dir, want_index = expected(code_lens, blobs, block_symbols)
    pin_to_oracle(sc.oracle, ocoder, blobs, want_dir, want_index)
    got_dir, got_index, status = device_index(eng, plan, d_in, len(blobs), block_symbols, want_index.size + slack)
    assert np.array_equal(got_dir, want_dir), (label, "first wrong directory record %d" % int(np.flatnonzero(got_dir != want_dir)[0] // 2))
    assert status == want_status, (label, status)
    bad = np.flatnonzero(got_index[:want_index.size].astype(np.int64) != want_index)
    assert bad.size == 0, (label, block_symbols, "first wrong entry %d of %d" % (int(bad[0]), want_index.size), int(got_index[bad[0]]),
                           int(want_index[bad[0]]))
    assert np.all(got_index[want_index.size:] == EE), (label, "entries behind index[total_blocks] were written")
    assert index_size(eng, plan) == (0, 0, want_index.size), label
    return want_dir, want_index


class Placed:
    """Items placed by hand in one input buffer: (offset, symbols) each -- any order, any overlap."""

    def __init__(self, eng, host, spans):
        self.eng, self.host = eng, host
        self.blobs = [host[o:o + n] for o, n in spans]
        self.items = [dict(in_offset=o, in_len=n, out_offset=0, out_capacity=0) for o, n in spans]
        self.d_in = eng.alloc(host.size)
        eng.upload(self.d_in, host)

    def close(self):
        self.eng.free(self.d_in)


# ----------------------------------------------------------------------------- 1: edges
EDGE_LENGTHS = [0, 1, 63, 64, 65, 64 * 7 + 17, 40_001]


def edge_batch(sc, eng):
    """Empty items first, last and side by side; every edge length at offsets 0, 1, 3 and 15 bytes off a 16-byte boundary;
    the items listed against their address order; two items that share input bytes."""
    rng = np.random.default_rng(901)
    host = pc.inputs(rng, 4 * 41_000 + 4096, "uniform")
    spans, at = [], 0
    for k, n in enumerate(EDGE_LENGTHS[1:]):
        for m in (0, 1, 3, 15)[k % 4:] + (0, 1, 3, 15)[:k % 4]:
            if n == 40_001 and m not in (0, 15):
                continue  # (the long item twice is enough)
            at = (at + 15) // 16 * 16
            spans.append((at + m, n))
            at += m + n
    assert at <= host.size
    long_at = next(o for o, n in spans if n == 40_001)
    spans.append((long_at + 777, 5_000))  # inside the long item: shared bytes
    spans = spans[::-1]                   # against the address order
    spans = [(0, 0), (17, 0)] + spans[:5] + [(99, 0), (99, 0)] + spans[5:] + [(host.size, 0)]
    return Placed(eng, host, spans)


def run_edges(sc):
    eng = sc.eng
    b = edge_batch(sc, eng)
    plan = eng.encode_plan(b.items)
    try:
        assert {x.size for x in b.blobs} >= set(EDGE_LENGTHS)
        assert {int(it["in_offset"]) % 16 for it in b.items if it["in_len"]} >= {0, 1, 3, 15}
        for limit, label in ((ALL_WAVES, "every item a wave's"), (ALL_TILES, "every item in tiles"), (0, "the rule")):
            with wave_bytes(sc.lib, limit):
                d, x = check_batch(sc, eng, plan, b.d_in, b.blobs, sc.lens, sc.w.ocoder, 64, label=label)
            assert x[0] == 0 and d[0][0] == 0 and d[1][0] == 0 and d[-1][1] == 0
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 2: block sizes and data
BLOCK_SIZES = ia.BLOCK_SIZES
DATA_KINDS = ia.DATA_KINDS
N_ITEMS = 37


def seeded_lengths(seed=907):
    """37 lengths, about 200 KB, on both sides of the road limit and at it."""
    rng = np.random.default_rng(seed)
    lens = [int(v) for v in rng.integers(0, 2 * WAVE_RULE, N_ITEMS - 9)]
    lens += [WAVE_RULE - 1, WAVE_RULE, WAVE_RULE + 1, 0, 16_384, 16_385, 33_000, 15, 20_011]
    order = rng.permutation(len(lens))
    return [lens[i] for i in order]


def batch_of(sc, eng, kind, lengths, seed=911, gap=True):
    """The lengths cut one after the other (3 bytes between two items) out of data of one kind."""
    total = sum(lengths) + 3 * len(lengths) + 64
    host = ia.data_of(sc, kind, total, seed=seed)
    spans, at = [], 1
    for n in lengths:
        spans.append((at, n))
        at += n + (3 if gap else 0)
    return Placed(eng, host, spans)


def run_block_sizes(sc, block_symbols, kind):
    eng = sc.eng
    lengths = seeded_lengths()
    assert len(lengths) == N_ITEMS and 150_000 < sum(lengths) < 260_000
    b = batch_of(sc, eng, kind, lengths)
    plan = eng.encode_plan(b.items)
    try:
        check_batch(sc, eng, plan, b.d_in, b.blobs, sc.lens, sc.w.ocoder, block_symbols, label=kind)
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 3: scan boundaries
INDEX_TILES = [1, 3, 256]
PACK_TILES = [1, 3]


def small_batch(sc, eng, seed=919):
    """41 items, some 330 blocks of 64: emulator-sized for scans of one entry a workgroup."""
    rng = np.random.default_rng(seed)
    lengths = [int(v) for v in rng.integers(0, 900, 38)] + [0, 64, 5_000]
    return batch_of(sc, eng, "uniform", lengths, seed=seed)


def run_index_tiles(sc, tile):
    eng = sc.eng
    b = small_batch(sc, eng)
    plan = eng.encode_plan(b.items)
    try:
        with ia.index_tile_blocks(sc.lib, tile):
            check_batch(sc, eng, plan, b.d_in, b.blobs, sc.lens, sc.w.ocoder, 64, label="index tile %d" % tile)
            check_batch(sc, eng, plan, b.d_in, b.blobs, sc.lens, sc.w.ocoder, 64, label="index tile %d, roomy" % tile, slack=150)
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


def run_pack_tiles(sc, tile):
    eng = sc.eng
    b = small_batch(sc, eng, seed=929)
    plan = eng.encode_plan(b.items)
    try:
        with pa.pack_tile_items(sc.lib, tile):
            for limit in (0, ALL_TILES):
                with wave_bytes(sc.lib, limit):
                    check_batch(sc, eng, plan, b.d_in, b.blobs, sc.lens, sc.w.ocoder, 64, label="pack tile %d" % tile)
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 4: fill kinds
def run_fill_kinds(sc):
    """Twelve equal items a stride apart through a host reset, a strided reset and a reset from device items: the same
    directory and index; then the plan's packed launch and its plain launch against the oracle."""
    eng, lib = sc.eng, sc.lib
    n, size, stride = 12, 3_000, 3_011
    rng = np.random.default_rng(937)
    host = pc.inputs(rng, n * stride + 64, "uniform")
    spans = [(5 + i * stride, size) for i in range(n)]
    b = Placed(eng, host, spans)
    room = 2 * size
    for i, it in enumerate(b.items):
        it["out_offset"], it["out_capacity"], it["eos_padding"] = i * room, room, 0xFF
    plan = eng.empty_encode_plan()
    d_items = None
    d_out = eng.alloc(n * room + 64)
    try:
        seen = []
        for kind in ("host", "strided", "device"):
            if kind == "host":
                arr = eng._encode_item_array(b.items)
                assert lib.aws_huffman_amd_encode_plan_reset(plan, arr, n) == 0
            elif kind == "strided":
                eng.plan_strided(True, plan=plan, count=n, in_offset=5, in_stride=stride, in_len=size, out_offset=0,
                                 out_stride=room, out_capacity=room, first_bit=0, eos_padding=0xFF)
            else:
                _, d_items = eng.encode_plan_from_device_items(b.items, plan=plan)
            # (behind a fill no size is known)
            assert index_size(eng, plan)[:2] == INVALID
            seen.append(check_batch(sc, eng, plan, b.d_in, b.blobs, sc.lens, sc.w.ocoder, 512, label=kind))
            # the call is not a launch: the packed launch and the plain one behind it are the oracle's
            pa.check_launch(sc.oracle, sc.w.ocoder, eng, plan, b.d_in, b.blobs, sc.lens, [(0, 0)] * n, [0xFF] * n, 1, label=kind)
            check_batch(sc, eng, plan, b.d_in, b.blobs, sc.lens, sc.w.ocoder, 64, label=kind + " behind a packed launch")
            assert pa.packed_size(eng, plan)[:2] == (0, 0)  # (the packed state is as the launch left it)
            eng.fill(d_out, pa.MARKER, n * room + 64)
            eng.encode_launch(plan, b.d_in, d_out)
            got = eng.download(d_out, n * room + 64)
            res = eng.encode_results(plan, n)
            for i, blob in enumerate(b.blobs):
                rec, data = pa.oracle_item(sc.oracle, sc.w.ocoder, blob, (0, 0), 0xFF, room)
                assert res[i] == rec and np.array_equal(got[i * room:(i + 1) * room], data), (kind, i)
        for d, x in seen[1:]:
            assert np.array_equal(d, seen[0][0]) and np.array_equal(x, seen[0][1])
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        if d_items:
            eng.free(d_items)
        eng.free(d_out)
        b.close()


def run_thread_plan(sc):
    """5 000 items of 16 to 80 bytes: the plan of items that are all a thread's work, from host records and from device
    records -- the same directory and index; the packed launch behind it against the oracle."""
    eng, lib = sc.eng, sc.lib
    rng = np.random.default_rng(941)
    n = 5_000
    blobs = [pc.inputs(rng, int(rng.integers(16, 81)), pc.KINDS[i % 4]) for i in range(n)]
    b = pa.Batch(eng, blobs, rng, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    d_items = None
    try:
        assert eng.encode_stats(plan)["by_thread"] == n
        first = check_batch(sc, eng, plan, b.d_in, blobs, sc.lens, sc.w.ocoder, 64, label="threads")
        pa.check_launch(sc.oracle, sc.w.ocoder, eng, plan, b.d_in, blobs, sc.lens, b.overflows, b.eoss, 1,
                        sample=list(range(0, n, 97)) + [n - 1], label="threads")
        _, d_items = eng.encode_plan_from_device_items(b.items, plan=plan)
        second = check_batch(sc, eng, plan, b.d_in, blobs, sc.lens, sc.w.ocoder, 64, label="threads, device records")
        assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        if d_items:
            eng.free(d_items)
        b.close()


# ----------------------------------------------------------------------------- 5, 6: one item; the packed launch
def run_one_item(sc):
    """A batch of a single item is aws_huffman_amd_block_index of the same bytes, entry for entry -- on either road."""
    eng = sc.eng
    for n, B in ((3_001, 64), (70_001, 512)):
        data = ia.data_of(sc, "uniform", n + 9, seed=947)
        b = Placed(eng, data, [(9, n)])
        plan = eng.encode_plan(b.items)
        try:
            single, status = ia.device_index(eng, b.blobs[0], B, d_data=b.d_in + 9)
            assert status == INDEX_OK
            for limit in (ALL_TILES, ALL_WAVES):
                with wave_bytes(sc.lib, limit):
                    d, x, status = device_index(eng, plan, b.d_in, 1, B, single.size)
                assert status == INDEX_OK and np.array_equal(x.astype(np.int64), single), (n, B, limit)
                assert d.tolist() == [[0, n], [single.size - 1, 0]]
        finally:
            sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
            b.close()


def run_against_packed_launch(sc):
    """For a coder that codes every symbol: offsets[i + 1] - offsets[i] of the packed launch at align 1 is ceil(item bits / 8)
    from the index."""
    eng = sc.eng
    b = batch_of(sc, eng, "printable", seeded_lengths(953), seed=953)
    n = len(b.blobs)
    plan = eng.encode_plan(b.items)
    d_out, d_off = eng.alloc(400_000), eng.alloc(8 * (n + 1))
    try:
        want_dir, want_index = expected(sc.lens, b.blobs, 512)
        d, x, status = device_index(eng, plan, b.d_in, n, 512, want_index.size)
        assert status == INDEX_OK
        assert pa.launch_packed(eng, plan, b.d_in, d_out, 400_000, d_off, 1) == (0, 0)
        eng.sync()
        offsets = pa.download_u64(eng, d_off, n + 1)
        x = x.astype(np.int64)
        bits = x[d[1:, 0]] - x[d[:-1, 0]]
        assert np.array_equal(offsets[1:] - offsets[:-1], (bits + 7) // 8)
    finally:
        eng.free(d_out)
        eng.free(d_off)
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 7: coders
OTHER_CODERS = ia.OTHER_CODERS


def run_other_coders(sc, name):
    """HPACK's lengths (30-bit codes), codes of 4 .. 15 bits, and the test coder less symbols 7 and 200: there the status
    says so (and is clear for a batch that meets neither)."""
    if name == "holes":
        eng, coder = sc.engine(holes=True)
        code_lens, ocoder, want_status = sc.lens_holes, sc.w.ocoder_holes, INDEX_SYMBOL_WITHOUT_CODE
    else:
        ocoder, coder, lengths = pc.profile_coders(sc.w, name)
        eng, code_lens, want_status = harness.Engine(sc.lib, coder), np.asarray(lengths, dtype=np.int64), INDEX_OK
    b = batch_of(sc, eng, "uniform", seeded_lengths(967)[:20] + [20_011, 9, 70], seed=967)
    plan = eng.encode_plan(b.items)
    try:
        if name == "holes":
            # the two symbols in one long item (tiles) and in the short last one (a wave) only
            for blob in b.blobs:
                blob[blob == 7] = 8
                blob[blob == 200] = 201
            longest = max(range(len(b.blobs)), key=lambda i: b.blobs[i].size)
            b.blobs[longest][5_000] = 7
            b.blobs[-1][3] = 200
            eng.upload(b.d_in, b.host)
        for B in (64, 4096):
            check_batch(sc, eng, plan, b.d_in, b.blobs, code_lens, ocoder, B, want_status=want_status, label=name)
        if name == "holes":
            b.blobs[-1][3] = 201  # the wave's hole gone: the tile's still speaks
            eng.upload(b.d_in, b.host)
            check_batch(sc, eng, plan, b.d_in, b.blobs, code_lens, ocoder, 64, want_status=want_status, label="holes, one left")
            b.blobs[longest][5_000] = 8
            eng.upload(b.d_in, b.host)
            check_batch(sc, eng, plan, b.d_in, b.blobs, code_lens, ocoder, 64, label="holes, none met")
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        sc.done(eng, coder)


def fitted_batch(data, rng):
    """Items of a few sizes cut out of `data`, not in address order."""
    spans, at = [], 3
    for size in (300, 0, 5_000, 70, 20_000, 4_096, 33, 9_000):
        spans.append((at, size))
        at += size + int(rng.integers(0, 5))
    assert at <= data.size
    return spans[::-1]


def enqueue_fit_index_encode(eng, clear, plan, d_in, length, B, a, d_out, capacity, d_off, stream):
    """clear the counts, count, fit, batch index, packed encode: five steps on `stream`, nothing waited for in between."""
    clear(eng, eng.d_counts, 256 * 8, stream)
    assert eng.lib.aws_huffman_amd_symbol_counts(-1, d_in, length, eng.d_counts, stream) == 0
    assert eng.fit_counts_async(None, stream) == (0, 0)
    assert plan_block_index(eng, plan, d_in, B, a.d_dir, a.d_index, a.capacity, a.d_status, stream) == (0, 0)
    assert pa.launch_packed(eng, plan, d_in, d_out, capacity, d_off, 1, stream) == (0, 0)


def check_fitted_chain(lib, oracle, eng, plan, data, blobs, B, a, d_out, d_off, capacity):
    """Behind such a chain: the packed output is the oracle's under the fitted lengths (fit_api.check_chain_output), and the
    directory and index are the definition's under the same lengths."""
    lengths, offsets = fa.check_chain_output(lib, oracle, eng, plan, data, blobs, d_out, d_off, capacity)
    want_dir, want_index = expected(lengths, blobs, B)
    d, x, status = a.read()
    assert status == INDEX_OK and np.array_equal(d, want_dir)
    assert np.array_equal(x[:want_index.size].astype(np.int64), want_index)
    bits = want_index[want_dir[1:, 0]] - want_index[want_dir[:-1, 0]]
    assert np.array_equal(offsets[1:] - offsets[:-1], (bits + 7) // 8)
    return lengths


def run_fitted_engine(lib, oracle, clear, B=512, n_bytes=60_000):
    """A (4, 12) engine: never fitted, the call is refused and writes nothing; then count, fit, batch index and packed encode
    enqueued back to back on the engine's stream."""
    eng = fa.FittedEngine(lib, 4, 12)
    rng = np.random.default_rng(971)
    data = fa.shape_bytes("printable", n_bytes, 973)
    spans = fitted_batch(data, rng)
    blobs = [data[o:o + s] for o, s in spans]
    items = [dict(in_offset=o, in_len=s, out_offset=0, out_capacity=0) for o, s in spans]
    n = len(items)
    capacity = n_bytes * 2
    d_in, d_out, d_off = eng.alloc(n_bytes), eng.alloc(capacity), eng.alloc(8 * (n + 1))
    plan = eng.encode_plan(items)
    a = Arrays(eng, n, sum(ia.n_blocks_of(s, B) for _, s in spans) + 1)
    try:
        eng.upload(d_in, data)
        assert plan_block_index(eng, plan, d_in, B, a.d_dir, a.d_index, a.capacity, a.d_status) == STATE
        eng.sync()
        d, x, status = a.read()
        assert np.all(d.view(np.uint64) == EE) and np.all(x == EE) and status == 0xEEEEEEEE
        eng.fill(d_out, pa.MARKER, capacity)
        enqueue_fit_index_encode(eng, clear, plan, d_in, n_bytes, B, a, d_out, capacity, d_off, C.c_void_p(eng.stream))
        eng.sync()
        lengths = check_fitted_chain(lib, oracle, eng, plan, data, blobs, B, a, d_out, d_off, capacity)
        assert not fa.is_flat(lengths)
    finally:
        a.close()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        for d in (d_in, d_out, d_off):
            eng.free(d)
        eng.close()


# ----------------------------------------------------------------------------- 8: capacity, refusals, no GPU, exports
def run_capacity(sc):
    """Exact capacity; one entry short (TOO_SMALL, the directory whole, the index untouched); the NULL query with the size
    call; a batch of empty items; a plan without items."""
    eng, lib = sc.eng, sc.lib
    b = batch_of(sc, eng, "uniform", seeded_lengths(977)[:15], seed=977)
    n, B = len(b.blobs), 64
    plan = eng.encode_plan(b.items)
    try:
        want_dir, want_index = check_batch(sc, eng, plan, b.d_in, b.blobs, sc.lens, sc.w.ocoder, B, label="exact")
        entries = want_index.size
        for capacity in (entries - 1, 1, 7):
            d, x, status = device_index(eng, plan, b.d_in, n, B, capacity)
            assert status == INDEX_TOO_SMALL and np.array_equal(d, want_dir) and np.all(x == EE), capacity
            assert d[n][0] + 1 == entries and index_size(eng, plan) == (0, 0, entries)
        # the size query: no index at all
        a = Arrays(eng, n, 0)
        try:
            assert plan_block_index(eng, plan, b.d_in, B, a.d_dir, None, 0, a.d_status) == (0, 0)
            assert index_size(eng, plan) == (0, 0, entries)
            d, _, status = a.read()
            assert status == INDEX_TOO_SMALL and np.array_equal(d, want_dir)
            # ... and without a status
            a.refill()
            assert plan_block_index(eng, plan, b.d_in, B, a.d_dir, None, 0, None) == (0, 0)
            eng.sync()
            d, _, status = a.read()
            assert status == 0xEEEEEEEE and np.array_equal(d, want_dir)
        finally:
            a.close()
        # empty items only: no block, index[0] = 0, OK
        empty = eng.encode_plan([dict(in_offset=3, in_len=0, out_offset=0, out_capacity=0)] * 3)
        try:
            d, x, status = device_index(eng, empty, b.d_in, 3, B, 2)
            assert status == INDEX_OK and d.tolist() == [[0, 0]] * 4 and x[0] == 0 and x[1] == EE
            assert index_size(eng, empty) == (0, 0, 1)
        finally:
            lib.aws_huffman_amd_encode_plan_destroy(empty)
        # no items at all (and no input)
        none = eng.empty_encode_plan()
        try:
            d, x, status = device_index(eng, none, None, 0, B, 1)
            assert status == INDEX_OK and d.tolist() == [[0, 0]] and x[0] == 0
            a = Arrays(eng, 0, 0)
            try:
                assert plan_block_index(eng, none, None, B, a.d_dir, None, 0, a.d_status) == (0, 0)
                eng.sync()
                d, _, status = a.read()
                assert status == INDEX_TOO_SMALL and d.tolist() == [[0, 0]]
            finally:
                a.close()
        finally:
            lib.aws_huffman_amd_encode_plan_destroy(none)
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


def run_refusals(sc):
    """The argument refusals: nothing is written, and the plan works behind them."""
    eng, lib = sc.eng, sc.lib
    b = batch_of(sc, eng, "uniform", [100, 0, 3_000], seed=983)
    n, B = 3, 64
    plan = eng.encode_plan(b.items)
    a = Arrays(eng, n, 60)
    try:
        call = lambda **kw: plan_block_index(eng, kw.get("plan", plan), kw.get("d_in", b.d_in), kw.get("B", B), kw.get("d_dir", a.d_dir),
                                             kw.get("d_index", a.d_index), kw.get("capacity", 60), kw.get("d_status", a.d_status))
        assert call(plan=None) == INVALID
        assert call(d_dir=None) == INVALID
        assert call(d_dir=a.d_dir + 4) == INVALID
        assert call(d_index=a.d_index + 4) == INVALID
        assert call(d_status=a.d_status + 2) == INVALID
        assert call(d_index=None) == INVALID            # a capacity without an index
        assert call(capacity=0) == INVALID              # an index without a capacity
        assert call(d_in=None) == INVALID
        for bad in (0, 63, 96, 1 << 25):
            assert call(B=bad) == INVALID, bad
        lib.aws_reset_error()
        assert lib.aws_huffman_amd_encode_plan_block_index_size(None, C.byref(C.c_uint64()), None) == -1
        assert lib.aws_last_error() == harness.AWS_ERROR_INVALID_ARGUMENT
        assert index_size(eng, plan)[:2] == INVALID     # (no call was made yet)
        eng.sync()
        d, x, status = a.read()
        assert np.all(d.view(np.uint64) == EE) and np.all(x == EE) and status == 0xEEEEEEEE
        # the status is optional, the largest block is taken
        assert call(d_status=None) == (0, 0)
        eng.sync()
        assert a.read()[2] == 0xEEEEEEEE
        a.refill()
        assert call(B=1 << 24) == (0, 0)
        eng.sync()
        d, x, status = a.read()
        bits = [int(sc.lens[blob].sum()) for blob in b.blobs]
        assert status == INDEX_OK and d.tolist() == [[0, 100], [1, 0], [1, 3_000], [2, 0]]
        assert x[:3].astype(np.int64).tolist() == [0, bits[0], bits[0] + bits[2]] and x[3] == EE
    finally:
        a.close()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


def run_product_without_a_gpu(product):
    """Against the product library on a machine without a GPU: the call raises AWS_ERROR_UNSUPPORTED_OPERATION and touches
    nothing it was handed.  (With a GPU present this has nothing to say: tests/test_gpu_batch_index.py speaks there.)"""
    if product.aws_huffman_amd_device_count() > 0:
        return
    handle = np.full(4096, 0x11, np.uint8)  # (stands for the plan: there is none without a GPU)
    memory = np.full(4096, 0xEE, np.uint8)
    h, m = handle.ctypes.data, memory.ctypes.data
    product.aws_reset_error()
    assert product.aws_huffman_amd_encode_plan_block_index(h, m + 1024, 64, m, m + 512, 8, m + 768, None) == -1
    assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    assert np.all(handle == 0x11) and np.all(memory == 0xEE)


def header_api_names():
    text = open(HEADER).read()
    return re.findall(r"AWS_COMPRESSION_API\s+[\w\s\*]*?\b(aws_\w+)\s*\(", text)


def run_exports(so_path):
    names = header_api_names()
    assert set(names) == {"aws_huffman_amd_encode_plan_block_index", "aws_huffman_amd_encode_plan_block_index_size",
                          "aws_huffman_amd_decode_plan_reset_item_block_ranges",
                          "aws_huffman_amd_decode_plan_reset_item_symbol_ranges", "aws_huffman_amd_locate_item_symbols",
                          "aws_huffman_amd_testing_set_batch_index_wave_bytes"}, names
    listing = subprocess.check_output(["nm", "-D", "--defined-only", so_path], text=True)
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported], [n for n in names if n not in exported]


# ----------------------------------------------------------------------------- 9 .. 12: ranges of blocks addressed by item
MARKER = pa.MARKER


class PackedBatch:
    """A batch as its receiver has it, all of it made by the device and checked against the definition before anything is
    built on it: the packed buffer a packed encode launch wrote (`enc_offset` bytes into a larger one), its offsets, and the
    directory and index of aws_huffman_amd_encode_plan_block_index."""

    def __init__(self, sc, eng, code_lens, ocoder, lengths, B, align=1, enc_offset=0, seed=1009):
        self.sc, self.eng, self.ocoder, self.B, self.enc_offset = sc, eng, ocoder, B, enc_offset
        self.code_lens = np.asarray(code_lens, dtype=np.int64)
        b = batch_of(sc, eng, "uniform", lengths, seed=seed)
        self.blobs, self.n = b.blobs, len(b.blobs)
        plan = eng.encode_plan(b.items)
        self.owned = []
        try:
            self.dir, self.index = expected(self.code_lens, self.blobs, B)
            self.entries = self.index.size
            a = Arrays(eng, self.n, self.entries)
            self.owned += [a.d_dir, a.d_index, a.d_status]
            assert plan_block_index(eng, plan, b.d_in, B, a.d_dir, a.d_index, self.entries, a.d_status) == (0, 0)
            eng.sync()
            d, x, status = a.read()
            assert status == INDEX_OK and np.array_equal(d, self.dir) and np.array_equal(x.astype(np.int64), self.index)
            self.d_dir, self.d_index = a.d_dir, a.d_index
            bits = self.index[self.dir[1:, 0]] - self.index[self.dir[:-1, 0]]
            self.enc_lens = (bits + 7) // 8
            self.offsets, _ = pa.expected_offsets(self.enc_lens, align)
            self.total = int(self.offsets[-1])
            self.size = enc_offset + self.total
            self.d_enc, self.d_off = eng.alloc(self.size + 64), eng.alloc(8 * (self.n + 1))
            self.owned += [self.d_enc, self.d_off]
            eng.fill(self.d_enc, 0x5A, self.size + 64)
            assert pa.launch_packed(eng, plan, b.d_in, self.d_enc + enc_offset, self.total, self.d_off, align) == (0, 0)
            eng.sync()
            assert np.array_equal(pa.download_u64(eng, self.d_off, self.n + 1), self.offsets)
            self.enc_host = eng.download(self.d_enc, self.size + 64)
            self.d_lens = pda.upload_u64(eng, self.enc_lens)
            self.owned.append(self.d_lens)
            self.encs = {}
        finally:
            sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
            b.close()

    def close(self):
        for d in self.owned:
            self.eng.free(d)

    def upload(self, values):
        d = pda.upload_u64(self.eng, values)
        self.owned.append(d)
        return d

    def reset(self, plan, ranges, **kw):
        """(rc, error); any argument can be replaced by name."""
        eng = self.eng
        flat = np.asarray([v & ((1 << 64) - 1) for r in ranges for v in r], dtype=np.uint64)
        d_ranges = self.upload(flat) if "d_ranges" not in kw else kw["d_ranges"]
        eng.lib.aws_reset_error()
        rc = eng.lib.aws_huffman_amd_decode_plan_reset_item_block_ranges(
            kw.get("plan", plan), kw.get("d_dir", self.d_dir), kw.get("d_index", self.d_index), kw.get("entries", self.entries),
            kw.get("items", self.n), kw.get("B", self.B), kw.get("d_off", self.d_off), kw.get("d_lens", None),
            kw.get("enc_offset", self.enc_offset), kw.get("enc_length", self.total), d_ranges, len(ranges), None)
        return rc, eng.lib.aws_last_error() if rc else 0

    def enc_of(self, item):
        """The oracle's encode of the item alone; the packed buffer holds exactly that at the item's offset."""
        if item not in self.encs:
            enc = self.sc.oracle.encode_all(self.ocoder, self.blobs[item], eos_padding=0xFF)
            at = self.enc_offset + int(self.offsets[item])
            assert enc.size == self.enc_lens[item] and np.array_equal(self.enc_host[at:at + enc.size], enc), item
            self.encs[item] = enc
        return self.encs[item]

    def item(self, item, first_block, count):
        """What a range comes to, from the definition: (encoded slice, first bit, capacity, symbols)."""
        blob, enc = self.blobs[item], self.enc_of(item)
        if count == 0:
            return enc[:0], 0, 0, blob[:0]
        own = ia.expected_index(self.code_lens, blob, self.B)
        b1 = first_block + count
        i0, i1 = int(own[first_block]), int(own[b1])
        lo, hi = first_block * self.B, min(b1 * self.B, blob.size)
        return enc[i0 // 8:(i1 + 7) // 8], i0 % 8, hi - lo, blob[lo:hi]

    def check_launch(self, plan, ranges, out_size, label="", symbols=False):
        """A plain launch of the plan: every byte of the output (MARKER where no range writes), every record the oracle's for
        the range's own encoded bytes; produced == out_capacity either way.  symbols: the ranges count symbols, not blocks."""
        eng = self.eng
        want = np.full(out_size, MARKER, np.uint8)
        recs = []
        for item, first, count, out_off in ranges:
            enc, first_bit, cap, syms = (self.symbol_item if symbols else self.item)(item, first, count)
            rec, out = pda.oracle_item(self.sc.oracle, self.ocoder, enc, first_bit, cap)
            assert rec[:2] in ((0, 0), pda.SHORT) and rec[2] == cap, (label, item, first, count, rec)
            assert np.array_equal(out, syms), (label, item, first, count)
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

    def n_blocks(self, item):
        return int(self.dir[item + 1][0] - self.dir[item][0])

    # ---- symbols addressed by item
    def symbol_bits(self, item):
        """bits[s] = where symbol s of the item starts, counted from the packed buffer's first byte, s = 0 .. len."""
        return ra.symbol_bits(self.code_lens, self.blobs[item]) + np.uint64(8 * int(self.offsets[item]))

    def locate(self, items, symbols, **kw):
        """One aws_huffman_amd_locate_item_symbols call: (bits as uint64[count], status); guards checked."""
        eng, n = self.eng, len(items)
        d_items, d_syms = self.upload(np.asarray(items, dtype=np.uint64)), self.upload(np.asarray(symbols, dtype=np.uint64))
        d_bits, d_status = eng.alloc(8 * (n + GUARD_WORDS)), eng.alloc(8)
        self.owned += [d_bits, d_status]
        eng.fill(d_bits, 0xEE, 8 * (n + GUARD_WORDS))
        eng.fill(d_status, 0xEE, 8)
        eng.lib.aws_reset_error()
        rc = eng.lib.aws_huffman_amd_locate_item_symbols(
            eng.h, self.d_enc + self.enc_offset, kw.get("enc_length", self.total), kw.get("d_dir", self.d_dir),
            kw.get("d_index", self.d_index), kw.get("entries", self.entries), kw.get("items", self.n), kw.get("B", self.B),
            kw.get("d_off", self.d_off), kw.get("d_lens", None), d_items, d_syms, n, d_bits, d_status, None)
        assert rc == 0, eng.lib.aws_last_error()
        eng.sync()
        got = eng.download(d_bits, 8 * (n + GUARD_WORDS)).view(np.uint64)
        status = eng.download(d_status, 8).view(np.uint32)
        assert np.all(got[n:] == EE) and status[1] == 0xEEEEEEEE
        return got[:n].copy(), int(status[0])

    def reset_symbols(self, plan, ranges, **kw):
        """aws_huffman_amd_decode_plan_reset_item_symbol_ranges over (item, first_symbol, symbol_count, out_offset): (rc, error)."""
        eng = self.eng
        flat = np.asarray([v & ((1 << 64) - 1) for r in ranges for v in r], dtype=np.uint64)
        d_ranges = self.upload(flat) if "d_ranges" not in kw else kw["d_ranges"]
        eng.lib.aws_reset_error()
        rc = eng.lib.aws_huffman_amd_decode_plan_reset_item_symbol_ranges(
            kw.get("plan", plan), kw.get("d_input", self.d_enc), kw.get("d_dir", self.d_dir), kw.get("d_index", self.d_index),
            kw.get("entries", self.entries), kw.get("items", self.n), kw.get("B", self.B), kw.get("d_off", self.d_off),
            kw.get("d_lens", None), kw.get("enc_offset", self.enc_offset), kw.get("enc_length", self.total), d_ranges, len(ranges), None)
        return rc, eng.lib.aws_last_error() if rc else 0

    def symbol_item(self, item, s0, count):
        """What a range of symbols comes to, from the definition: (encoded slice, first bit, capacity, symbols)."""
        blob, enc = self.blobs[item], self.enc_of(item)
        if count == 0:
            return enc[:0], 0, 0, blob[:0]
        bits = ra.symbol_bits(self.code_lens, blob)
        i0, i1 = int(bits[s0]), int(bits[s0 + count])
        return enc[i0 // 8:(i1 + 7) // 8], i0 % 8, count, blob[s0:s0 + count]


def seeded_ranges(pb, rng, count=60):
    """Empty ranges, whole items, the ragged last block, single blocks, repeats and overlaps, in any order: (ranges with
    their out_offsets one behind the other, 3 bytes between; the output size)."""
    spans = []
    with_blocks = [i for i in range(pb.n) if pb.n_blocks(i)]
    for i in with_blocks[:8]:
        spans.append((i, 0, pb.n_blocks(i)))                 # a whole item
        spans.append((i, pb.n_blocks(i) - 1, 1))             # its last block (ragged for most)
    spans.append((next(i for i in range(pb.n) if pb.n_blocks(i) == 0), 0, 0))   # an empty item's nothing
    while len(spans) < count:
        i = int(rng.choice(with_blocks))
        nb = pb.n_blocks(i)
        b0 = int(rng.integers(0, nb + 1))
        spans.append((i, b0, int(rng.integers(0, nb - b0 + 1))))
    spans += spans[3:6]                                      # repeats
    order = rng.permutation(len(spans))
    ranges, at = [], 3
    for k in order:
        i, b0, c = spans[k]
        ranges.append((i, b0, c, at))
        at += pb.item(i, b0, c)[2] + 3
    return ranges, at + 64


RANGE_CODERS = ["test", "hpack_lengths"]  # (the second: a coder whose plans the host lays out, dec_items_to_host)
RANGE_BLOCKS = [64, 512]


def coder_of(sc, name):
    """(engine, code lengths, oracle coder, what to hand sc.done or None)."""
    if name == "test":
        return sc.eng, sc.lens, sc.w.ocoder, None
    ocoder, coder, lengths = pc.profile_coders(sc.w, name)
    return harness.Engine(sc.lib, coder), np.asarray(lengths, dtype=np.int64), ocoder, coder


def run_item_block_ranges(sc, name, B):
    """Seeded ranges over the batch of scenario 2, decoded by a plain launch from the packed buffer the packed launch wrote,
    5 bytes into a larger one; then the lengths-array form over a buffer packed at align 16; then, for three items, the plan
    is the plan aws_huffman_amd_decode_plan_reset_block_ranges makes of the item's own index, in records and statistics."""
    eng, code_lens, ocoder, coder = coder_of(sc, name)
    rng = np.random.default_rng(1013)
    plan = eng.empty_decode_plan()
    other = eng.empty_decode_plan()
    pbs = []
    try:
        pb = PackedBatch(sc, eng, code_lens, ocoder, seeded_lengths(), B, align=1, enc_offset=5)
        pbs.append(pb)
        ranges, out_size = seeded_ranges(pb, rng)
        assert pb.reset(plan, ranges) == (0, 0)
        assert not eng.decode_plan_is_quiet(plan)
        stats = eng.decode_stats(plan)
        assert stats["items"] == len(ranges) and stats["empty"] >= 1, stats
        pb.check_launch(plan, ranges, out_size, label="%s, B %d" % (name, B))
        # one item against the single stream's call over that item's own index
        for item in sorted(range(pb.n), key=lambda i: -pb.n_blocks(i))[:3]:
            mine, at = [], 7  # (outputs one behind the other again: no two ranges may write one byte)
            for r in [r for r in ranges if r[0] == item] + [(item, 0, pb.n_blocks(item), 0)]:
                mine.append((item, r[1], r[2], at))
                at += pb.item(*r[:3])[2] + 3
            assert pb.reset(plan, mine) == (0, 0)
            own = ia.expected_index(code_lens, pb.blobs[item], B)
            d_own = pb.upload(own)
            flat = np.asarray([v for r in mine for v in r[1:]], dtype=np.uint64)
            assert ia.reset_block_ranges(eng, other, d_own, pb.blobs[item].size, B, pb.enc_offset + int(pb.offsets[item]),
                                         int(pb.enc_lens[item]), pb.upload(flat), len(mine)) == (0, 0)
            assert eng.decode_stats(plan) == eng.decode_stats(other), item
            size = max(r[3] + pb.item(*r[:3])[2] for r in mine) + 64
            recs = pb.check_launch(plan, mine, size, label="item %d" % item)
            d_out = eng.alloc(size)
            try:
                eng.fill(d_out, MARKER, size)
                eng.decode_launch(other, pb.d_enc, d_out)
                assert eng.decode_results(other, len(mine)) == recs, item
            finally:
                eng.free(d_out)
        # lengths beside the offsets, items 16-byte aligned
        pb16 = PackedBatch(sc, eng, code_lens, ocoder, seeded_lengths(1019), B, align=16, enc_offset=0, seed=1021)
        pbs.append(pb16)
        ranges, out_size = seeded_ranges(pb16, rng, count=30)
        assert pb16.reset(plan, ranges, d_lens=pb16.d_lens) == (0, 0)
        pb16.check_launch(plan, ranges, out_size, label="%s, lengths, align 16" % name)
    finally:
        for p in pbs:
            p.close()
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        sc.lib.aws_huffman_amd_decode_plan_destroy(other)
        if coder is not None:
            sc.done(eng, coder)


def run_item_range_damage(sc, name):
    """Every row of the header's refusal list, one at a time: AWS_ERROR_INVALID_ARGUMENT and a plan without items, whose
    launch writes nothing; the same plan then takes a good fill and matches the oracle."""
    eng, code_lens, ocoder, coder = coder_of(sc, name)
    B = 64
    lengths = [700, 0, 3_000, 64, 129, 5_000]
    pb = PackedBatch(sc, eng, code_lens, ocoder, lengths, B, align=1, enc_offset=3, seed=1031)
    plan = eng.empty_decode_plan()
    n = pb.n
    good = [(i, 0, pb.n_blocks(i), 8_000 * i) for i in range(n)]
    out_size = 8_000 * n + 64
    d_out = eng.alloc(out_size)
    try:
        def refused(label, ranges=good, **kw):
            assert pb.reset(plan, good) == (0, 0) and eng.decode_stats(plan)["items"] == n, label
            assert pb.reset(plan, ranges, **kw) == INVALID, label
            assert eng.decode_stats(plan)["items"] == 0, label
            eng.fill(d_out, MARKER, out_size)
            assert sc.lib.aws_huffman_amd_decode_plan_launch(plan, pb.d_enc, d_out, None) == 0, label
            eng.sync()
            assert np.all(eng.download(d_out, out_size) == MARKER), label

        def damaged(array, at, value):
            out = np.asarray(array, dtype=np.int64).copy().reshape(-1)
            out[at] = value
            return pb.upload(out.astype(np.uint64))

        top = (1 << 64) - 1
        refused("item == item_count", good + [(n, 0, 0, 0)])
        refused("item far past", [(top, 0, 1, 0)] + good)
        refused("a directory that decreases", d_dir=damaged(pb.dir, 2 * 3, int(pb.dir[2][0]) - 1))  # record 3 below record 2
        refused("a directory past the index", d_dir=damaged(pb.dir, 2 * n, pb.entries))
        refused("the same, by fewer entries", entries=int(pb.dir[n][0]))
        refused("blocks that are not the symbols'", d_dir=damaged(pb.dir, 2 * 2 + 1, 3_000 + 64))
        refused("a range that starts past the item's blocks", good + [(0, pb.n_blocks(0) + 1, 0, 0)])
        refused("a range that ends past the item's blocks", [(2, 1, pb.n_blocks(2), 0)] + good)
        refused("first_block + block_count overflows", [(2, 1, top, 0)])
        refused("first_block + block_count overflows", [(2, top, 2, 0)])
        first2 = int(pb.dir[2][0])
        refused("an entry lowered inside the item", d_index=damaged(pb.index, first2 + 5, int(pb.index[first2 + 4]) - 1),
                ranges=[(2, 4, 1, 0)])
        refused("the item's first entry above the range's", d_index=damaged(pb.index, first2, int(pb.index[first2 + 1]) + 1),
                ranges=[(2, 1, 1, 0)])
        short = pb.enc_lens.copy()
        short[5] -= 1
        refused("bits beyond the item's encoded length", d_lens=pb.upload(short))
        assert pb.reset(plan, good[:5], d_lens=pb.upload(short)) == (0, 0)   # (the items that are whole)
        refused("offsets that decrease", d_off=damaged(pb.offsets, 3, int(pb.offsets[4]) + 1))
        refused("the item's bytes beyond encoded_length", enc_length=pb.total - 1)
        assert pb.reset(plan, good[:5], enc_length=int(pb.offsets[5])) == (0, 0)
        # an item of 4 GiB: entries, a length and a buffer size that all say so (nothing of it is read by the fill)
        giant_index = damaged(pb.index, int(pb.dir[1][0]), int(pb.index[0]) + (1 << 35))
        giant_lens = pb.enc_lens.copy()
        giant_lens[0] = 1 << 33
        refused("an item of 4 GiB", ranges=[(0, 0, pb.n_blocks(0), 0)], d_index=giant_index, d_lens=pb.upload(giant_lens),
                d_off=pb.upload(np.zeros(n + 1, np.int64)), enc_length=1 << 34, enc_offset=0)
        for bad in (0, 63, 1 << 25):
            refused("block_symbols %d" % bad, B=bad)
        refused("NULL directory", d_dir=None)
        refused("NULL index", d_index=None)
        refused("no entries", entries=0)
        refused("NULL offsets", d_off=None)
        refused("NULL ranges", d_ranges=None)
        refused("misaligned index", d_index=pb.d_index + 4)
        assert pb.reset(None, good) == INVALID
        # a later good fill of the same plan works; no ranges at all is a plan without items, success
        assert pb.reset(plan, good) == (0, 0)
        pb.check_launch(plan, good, out_size, label="behind the refusals")
        assert pb.reset(plan, []) == (0, 0) and eng.decode_stats(plan)["items"] == 0
    finally:
        eng.free(d_out)
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        pb.close()
        if coder is not None:
            sc.done(eng, coder)


SYMBOL_CODERS = ["test", "hpack_lengths", "len8"]  # (the last: codes of one length, located in closed form)


def item_positions(pb, rng, limit):
    """(items, symbols): per item with symbols k = 0 at the first, a middle and the last block, s = the item's length,
    k in {1, limit - 1, limit, limit + 1, B - 1} of a middle block, and random positions; an empty item's s = 0."""
    items, syms = [], []
    for i in range(pb.n):
        n, nb = pb.blobs[i].size, pb.n_blocks(i)
        mine = [0, n]
        if nb:
            mid = nb // 2
            mine += [mid * pb.B, (nb - 1) * pb.B, n - 1] + [mid * pb.B + k for k in (1, limit - 1, limit, limit + 1, pb.B - 1)]
            mine += [int(v) for v in rng.integers(0, n + 1, 12)]
        for s in mine:
            if 0 <= s <= n:
                items.append(i)
                syms.append(s)
    return items, syms


def run_item_symbols(sc, name):
    """Scenario 10: positions addressed by item on both locate roads against numpy; what is not there is not found; seeded
    ranges of symbols decoded from the packed buffer against the oracle; a range of whole blocks is the block-range item."""
    if name == "len8":
        ocoder, coder, lengths = pc.profile_coders(sc.w, name)
        eng, code_lens = harness.Engine(sc.lib, coder), np.asarray(lengths, dtype=np.int64)
    else:
        eng, code_lens, ocoder, coder = coder_of(sc, name)
    rng = np.random.default_rng(1061)
    B = 64
    lengths = [700, 0, 3_000, 64, 129, 9_001, 1, 0, 4_096]
    pb = PackedBatch(sc, eng, code_lens, ocoder, lengths, B, align=1, enc_offset=5, seed=1063)
    plan, other = eng.empty_decode_plan(), eng.empty_decode_plan()
    try:
        seen = []
        for limit in (1, 20, B + 1):  # a workgroup for every walk of two codes and more; both roads; a lane for every walk
            with ra.lone_symbols(sc.lib, limit):
                items, syms = item_positions(pb, rng if not seen else np.random.default_rng(1067), 20)
                if not seen:
                    fixed = (items, syms)
                items, syms = fixed
                got, status = pb.locate(items, syms)
                want = np.asarray([pb.symbol_bits(i)[s] for i, s in zip(items, syms)], dtype=np.uint64)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (name, limit, items[bad[0]], syms[bad[0]], int(got[bad[0]]), int(want[bad[0]]))
                assert status == ra.LOCATE_OK
                seen.append(got)
        assert np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], seen[2])
        # what is not there
        got, status = pb.locate([0, pb.n, 2, (1 << 64) - 1, 1], [701, 0, 5, 0, 1])
        assert [int(g) for g in got] == [ra.NO_BIT, ra.NO_BIT, int(pb.symbol_bits(2)[5]), ra.NO_BIT, ra.NO_BIT]
        assert status == ra.LOCATE_NOT_FOUND
        got, status = pb.locate([], [])
        assert got.size == 0 and status == ra.LOCATE_OK
        # the lengths-array form
        got, status = pb.locate([5, 5], [9_001, 77], d_lens=pb.d_lens)
        assert [int(g) for g in got] == [int(pb.symbol_bits(5)[9_001]), int(pb.symbol_bits(5)[77])] and status == ra.LOCATE_OK
        # ranges of symbols
        spans = [(5, 0, 9_001), (2, 100, 1), (2, 2_999, 1), (1, 0, 0), (0, 63, 2), (8, 64, 4_032), (6, 0, 1), (3, 0, 64), (5, 8_000, 0)]
        for _ in range(20):
            i = int(rng.choice([0, 2, 4, 5, 8]))
            s0 = int(rng.integers(0, pb.blobs[i].size + 1))
            spans.append((i, s0, int(rng.integers(0, min(pb.blobs[i].size - s0, 700) + 1))))
        ranges, at = [], 3
        for k in rng.permutation(len(spans)):
            i, s0, c = spans[k]
            ranges.append((i, s0, c, at))
            at += c + 3
        for limit in (1, 0):
            with ra.lone_symbols(sc.lib, limit):
                assert pb.reset_symbols(plan, ranges) == (0, 0)
            assert not eng.decode_plan_is_quiet(plan)
            pb.check_launch(plan, ranges, at + 64, label="%s, symbols, limit %d" % (name, limit), symbols=True)
        assert pb.reset_symbols(plan, ranges[:9], d_lens=pb.d_lens) == (0, 0)
        pb.check_launch(plan, ranges[:9], at + 64, label="%s, symbols, lengths" % name, symbols=True)
        # whole blocks: the block-range item
        blocks = [(5, 3, 7, 0), (2, 40, 7, 600), (8, 0, 64, 1_200), (4, 2, 1, 5_400), (1, 0, 0, 0)]
        as_symbols = [(i, b0 * B, min(c * B, pb.blobs[i].size - b0 * B), out) for i, b0, c, out in blocks]
        assert pb.reset_symbols(plan, as_symbols) == (0, 0) and pb.reset(other, blocks) == (0, 0)
        assert eng.decode_stats(plan) == eng.decode_stats(other)
        recs = pb.check_launch(plan, as_symbols, 6_000, label="whole blocks as symbols", symbols=True)
        assert pb.check_launch(other, blocks, 6_000, label="whole blocks") == recs
    finally:
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        sc.lib.aws_huffman_amd_decode_plan_destroy(other)
        pb.close()
        if coder is not None:
            sc.done(eng, coder)


def run_item_symbol_range_damage(sc):
    """The refusal list through the symbol-range fill, with its own row: an end that was not located."""
    eng = sc.eng
    B = 64
    pb = PackedBatch(sc, eng, sc.lens, sc.w.ocoder, [700, 0, 3_000, 64, 129, 5_000], B, align=1, enc_offset=3, seed=1069)
    plan = eng.empty_decode_plan()
    n = pb.n
    good = [(i, 1 if pb.blobs[i].size else 0, max(pb.blobs[i].size - 2, 0), 8_000 * i) for i in range(n)]
    out_size = 8_000 * n + 64
    d_out = eng.alloc(out_size)
    try:
        def refused(label, ranges=good, **kw):
            assert pb.reset_symbols(plan, good) == (0, 0) and eng.decode_stats(plan)["items"] == n, label
            assert pb.reset_symbols(plan, ranges, **kw) == INVALID, label
            assert eng.decode_stats(plan)["items"] == 0, label
            eng.fill(d_out, MARKER, out_size)
            assert sc.lib.aws_huffman_amd_decode_plan_launch(plan, pb.d_enc, d_out, None) == 0, label
            eng.sync()
            assert np.all(eng.download(d_out, out_size) == MARKER), label

        def damaged(array, at, value):
            out = np.asarray(array, dtype=np.int64).copy().reshape(-1)
            out[at] = value
            return pb.upload(out.astype(np.uint64))

        top = (1 << 64) - 1
        first2 = int(pb.dir[2][0])
        # block 4 of item 2 made 100 bits shorter than its codes: the walk to its 60th symbol is cut by the span's end
        cut = damaged(pb.index, first2 + 5, int(pb.index[first2 + 5]) - 100)
        assert int(pb.index[first2 + 5]) - 100 > int(pb.index[first2 + 4])
        for limit in (1, 0):
            with ra.lone_symbols(sc.lib, limit):
                refused("an end that was not located", ranges=[(2, 4 * B + 60, 2, 0)], d_index=cut)
        got, status = pb.locate([2, 2], [4 * B + 60, 4 * B + 3], d_index=cut)
        assert int(got[0]) == ra.NO_BIT and int(got[1]) == int(pb.symbol_bits(2)[4 * B + 3]) and status == ra.LOCATE_NOT_FOUND
        refused("item == item_count", good + [(n, 0, 0, 0)])
        refused("a range past the item's symbols", [(0, 700, 1, 0)] + good)
        refused("first_symbol + symbol_count overflows", [(2, 1, top, 0)])
        refused("first_symbol + symbol_count overflows", [(2, top, 2, 0)])
        refused("a directory that decreases", d_dir=damaged(pb.dir, 2 * 3, int(pb.dir[2][0]) - 1))
        refused("a directory past the index", entries=int(pb.dir[n][0]))
        refused("blocks that are not the symbols'", d_dir=damaged(pb.dir, 2 * 2 + 1, 3_000 + 64))
        refused("an entry lowered below the item's first", d_index=damaged(pb.index, first2 + 1, int(pb.index[first2]) - 1),
                ranges=[(2, B, 1, 0)])
        short = pb.enc_lens.copy()
        short[5] -= 1
        refused("bits beyond the item's encoded length", d_lens=pb.upload(short))
        refused("offsets that decrease", d_off=damaged(pb.offsets, 3, int(pb.offsets[4]) + 1))
        refused("the item's bytes beyond encoded_length", enc_length=pb.total - 1)
        refused("block_symbols 63", B=63)
        refused("NULL directory", d_dir=None)
        refused("NULL input", d_input=None)
        refused("NULL ranges", d_ranges=None)
        assert pb.reset_symbols(None, good) == INVALID
        assert pb.reset_symbols(plan, good) == (0, 0)
        pb.check_launch(plan, good, out_size, label="behind the refusals", symbols=True)
        assert pb.reset_symbols(plan, []) == (0, 0) and eng.decode_stats(plan)["items"] == 0
    finally:
        eng.free(d_out)
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        pb.close()


def run_one_plan_several_fills(sc):
    """One plan: item block ranges of a large batch, a packed-input fill of the same buffer (a packed launch), block ranges
    of a single stream, item symbol ranges of the large batch, symbol ranges of the single stream, item symbol ranges and
    item block ranges of a small batch, a strided fill, item block ranges again.  Every launch against the oracle;
    aws_huffman_amd_decode_plan_is_quiet is false behind every new fill."""
    eng, lib = sc.eng, sc.lib
    rng = np.random.default_rng(1033)
    big = PackedBatch(sc, eng, sc.lens, sc.w.ocoder, seeded_lengths(1039), 512, seed=1039)
    small = PackedBatch(sc, eng, sc.lens, sc.w.ocoder, [100, 0, 70_000], 64, seed=1049)
    data = ia.data_of(sc, "uniform", 120_000, seed=1051)
    st = ia.Stream(sc, eng, sc.lens, sc.w.ocoder, data, 4_096)
    plan = eng.empty_decode_plan()
    try:
        ranges, out_size = seeded_ranges(big, rng, count=40)
        assert big.reset(plan, ranges) == (0, 0) and not eng.decode_plan_is_quiet(plan)
        big.check_launch(plan, ranges, out_size, label="tour: big")
        # the same buffer as a packed input, decoded whole by a packed launch
        assert pda.reset_packed_input(eng, plan, big.d_off, None, big.n) == (0, 0)
        total = sum(b.size for b in big.blobs)
        d_out, d_sym = eng.alloc(total + 64), eng.alloc(8 * (big.n + 1))
        try:
            eng.fill(d_out, MARKER, total + 64)
            assert pda.launch_packed(eng, plan, big.d_enc, d_out, total, d_sym, 1) == (0, 0)
            got = eng.download(d_out, total + 64)
            want = np.concatenate(big.blobs + [np.full(64, MARKER, np.uint8)])
            assert np.array_equal(got, want), "tour: packed input"
        finally:
            eng.free(d_out)
            eng.free(d_sym)
        single = [(k, 2, 9_000 * k) for k in range(0, st.nb - 1, 3)]
        assert st.reset(plan, single) == (0, 0)
        st.check_launch(plan, single, 9_000 * st.nb + 64, label="tour: one stream")
        # symbols of items (many ranges: the located bits' array grows), then symbols of the single stream (fewer), then of items
        by_symbol, at = [], 1
        for i in range(big.n):
            size = big.blobs[i].size
            for s0, c in ((size // 3, min(90, size - size // 3)), (0, min(size, 7))):
                by_symbol.append((i, s0, c, at))
                at += c + 2
        assert big.reset_symbols(plan, by_symbol) == (0, 0) and not eng.decode_plan_is_quiet(plan)
        big.check_launch(plan, by_symbol, at + 64, label="tour: symbols of items", symbols=True)
        rs = ra.Ranges(st)
        rs.bits = ra.symbol_bits(sc.lens, data)
        stream_ranges = [(100_000, 300, 0), (5, 4_100, 400), (st.n - 1, 1, 5_000)]
        assert rs.reset(plan, stream_ranges) == (0, 0)
        rs.check_launch(plan, stream_ranges, 6_000, label="tour: symbols of one stream")
        assert small.reset_symbols(plan, [(2, 69_000, 1_000, 0), (0, 1, 98, 2_000)]) == (0, 0) and not eng.decode_plan_is_quiet(plan)
        small.check_launch(plan, [(2, 69_000, 1_000, 0), (0, 1, 98, 2_000)], 3_000, label="tour: symbols of few items", symbols=True)
        few = [(2, 1, small.n_blocks(2) - 1, 5), (0, 0, 2, 80_000), (1, 0, 0, 0)]
        assert small.reset(plan, few) == (0, 0) and not eng.decode_plan_is_quiet(plan)
        small.check_launch(plan, few, 81_000, label="tour: small")
        eng.plan_strided(False, plan=plan, count=2, in_offset=int(small.offsets[2]), in_stride=0, in_len=int(small.enc_lens[2]),
                         out_offset=3, out_stride=70_010, out_capacity=70_000, first_bit=0)
        d_out = eng.alloc(141_000)
        try:
            eng.fill(d_out, MARKER, 141_000)
            eng.decode_launch(plan, small.d_enc, d_out)
            got = eng.download(d_out, 141_000)
            res = eng.decode_results(plan, 2)
            rec, _ = pda.oracle_item(sc.oracle, sc.w.ocoder, small.enc_of(2), 0, 70_000)
            assert res == [rec, rec] and np.array_equal(got[3:70_003], small.blobs[2]) and np.array_equal(got[70_013:140_013], small.blobs[2])
        finally:
            eng.free(d_out)
        ranges, out_size = seeded_ranges(big, rng, count=25)
        assert big.reset(plan, ranges) == (0, 0) and not eng.decode_plan_is_quiet(plan)
        big.check_launch(plan, ranges, out_size, label="tour: big again")
    finally:
        lib.aws_huffman_amd_decode_plan_destroy(plan)
        big.close()
        small.close()
        st.close()


def run_ranges_without_a_gpu(product):
    if product.aws_huffman_amd_device_count() > 0:
        return
    handle = np.full(4096, 0x11, np.uint8)
    memory = np.full(4096, 0xEE, np.uint8)
    h, m = handle.ctypes.data, memory.ctypes.data
    product.aws_reset_error()
    assert product.aws_huffman_amd_decode_plan_reset_item_block_ranges(h, m, m + 512, 8, 1, 64, m + 1024, None, 0, 600, m + 2048, 1,
                                                                       None) == -1
    assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    product.aws_reset_error()
    assert product.aws_huffman_amd_decode_plan_reset_item_symbol_ranges(h, m + 3072, m, m + 512, 8, 1, 64, m + 1024, None, 0, 600,
                                                                        m + 2048, 1, None) == -1
    assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    product.aws_reset_error()
    assert product.aws_huffman_amd_locate_item_symbols(h, m + 3072, 600, m, m + 512, 8, 1, 64, m + 1024, None, m + 2048, m + 2056, 1,
                                                       m + 2064, m + 2072, None) == -1
    assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    assert np.all(handle == 0x11) and np.all(memory == 0xEE)
