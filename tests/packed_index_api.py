"""ctypes face of include/aws/compression/huffman_amd_packed_index.h (a packed encode launch that makes the batch's block
index in its length pass) and what its tests share.  Used by tests/test_emulated_packed_index.py (emulator build) and
tests/test_gpu_packed_index.py (MI355X): every run_* scenario below is called by both, at the same sizes.

Expected values never come from the library under test: directory and index are batch_index_api.expected (numpy's cumsum of
the code lengths, pinned to the oracle's length query), the offsets are packed_api.encoded_lengths and expected_offsets, and
every item's record and bytes are the oracle's encode into the room that layout gives it (packed_api.oracle_item)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import batch_index_api as bi
import fit_api as fa
import harness
import index_api as ia
import packed_api as pa
import parity_cases as pc

INDEX_OK, INDEX_SYMBOL_WITHOUT_CODE, INDEX_TOO_SMALL = bi.INDEX_OK, bi.INDEX_SYMBOL_WITHOUT_CODE, bi.INDEX_TOO_SMALL
INVALID, UNSUPPORTED, STATE = bi.INVALID, bi.UNSUPPORTED, bi.STATE
EE, MARKER = bi.EE, pa.MARKER
HEADER = os.path.join(harness.REPO, "include", "aws", "compression", "huffman_amd_packed_index.h")
SHORT = (-1, harness.AWS_ERROR_SHORT_BUFFER)
UNKNOWN = (-1, harness.AWS_ERROR_COMPRESSION_UNKNOWN_SYMBOL)


def bind(lib):
    """Declares the entry points of huffman_amd_packed_index.h (and of the headers in front of it) on a loaded library."""
    bi.bind(lib)
    pa.bind(lib)
    V, U = C.c_void_p, C.c_uint64
    lib.aws_huffman_amd_encode_plan_launch_packed_indexed.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_launch_packed_indexed.argtypes = [V, V, V, U, V, C.c_uint32, U, V, V, U, V, V]
    return lib


def restore_switches(lib):
    """Every testing switch a scenario here may have set, as a fresh process has it."""
    lib.aws_huffman_amd_testing_set_index_tile_blocks(0)
    lib.aws_huffman_amd_testing_set_batch_index_wave_bytes(0)
    lib.aws_huffman_amd_testing_set_pack_tile_items(0)


def launch_indexed(eng, plan, d_in, d_out, capacity, d_off, align, B, d_dir, d_index, index_capacity, d_status, stream=None):
    """(rc, error) of the enqueue."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_encode_plan_launch_packed_indexed(
        plan, d_in, d_out, int(capacity), d_off, int(align), int(B), d_dir, d_index, int(index_capacity), d_status, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def check_arrays(a, want_dir, want_index, want_status, label=""):
    """bi.Arrays behind a call against the definition; an index that did not fit is untouched."""
    d, x, status = a.read()
    assert np.array_equal(d, want_dir), (label, "first wrong directory record %d" % int(np.flatnonzero(d != want_dir)[0] // 2))
    assert status == want_status, (label, status, want_status)
    if a.capacity < want_index.size:
        assert np.all(x == EE), (label, "an index that does not fit was written")
        return
    bad = np.flatnonzero(x[:want_index.size].astype(np.int64) != want_index)
    assert bad.size == 0, (label, "first wrong entry %d of %d" % (int(bad[0]), want_index.size), int(x[bad[0]]), int(want_index[bad[0]]))
    assert np.all(x[want_index.size:] == EE), (label, "entries behind index[total_blocks] were written")


def check_indexed_launch(sc, eng, plan, d_in, blobs, code_lens, ocoder, overflows, eoss, align, B, capacity=None,
                         index_capacity=None, slack=0, sample=None, want_road=None, want_status=INDEX_OK, label=""):
    """One aws_huffman_amd_encode_plan_launch_packed_indexed of `plan` against the definitions: what packed_api.check_launch
    checks of a packed launch -- the offsets, the total and the longest reserved length; every item of `sample` (default:
    all) record for record and byte for byte against the oracle's encode into the room the layout gives it; MARKER in the
    gaps, behind the total and behind the capacity -- and then the directory, the index and the status (guard words behind
    both arrays).  capacity None: exactly the total.  index_capacity None: total_blocks + 1 + slack; one that is too small
    expects the header's answer: TOO_SMALL, no index word, every length 0.  Returns (offsets, total, got bytes, records)."""
    n = len(blobs)
    want_dir, want_index = bi.expected(code_lens, blobs, B)
    bi.pin_to_oracle(sc.oracle, ocoder, blobs, want_dir, want_index)
    entries = want_index.size
    icap = entries + slack if index_capacity is None else int(index_capacity)
    fits = icap >= entries
    lens = pa.encoded_lengths(code_lens, blobs, [ov[1] for ov in overflows]) if fits else np.zeros(n, np.int64)
    offsets, reserved = pa.expected_offsets(lens, align)
    total = int(offsets[-1])
    cap = total if capacity is None else int(capacity)
    size = max(total, cap) + 64
    d_out, d_off = eng.alloc(size), eng.alloc(8 * (n + 1))
    a = bi.Arrays(eng, n, icap)
    try:
        eng.fill(d_out, MARKER, size)
        eng.fill(d_off, 0xEE, 8 * (n + 1))
        assert launch_indexed(eng, plan, d_in, d_out, cap, d_off, align, B, a.d_dir, a.d_index, icap, a.d_status) == (0, 0), label
        got = eng.download(d_out, size)  # (behind the launch on the stream, before any record is read)
        res = eng.encode_results(plan, n)
        if want_road is not None:
            assert eng.encode_road(plan) == want_road, (label, eng.encode_road(plan))
        got_offsets = pa.download_u64(eng, d_off, n + 1)
        assert np.array_equal(got_offsets, offsets), (label, align, int(np.flatnonzero(got_offsets != offsets)[0]))
        assert pa.packed_size(eng, plan) == (0, 0, total, int(reserved.max()) if n else 0), (label, pa.packed_size(eng, plan), total)
        want = np.full(size, MARKER, np.uint8)
        every = sample is None
        for i in (range(n) if every else sample):
            off = int(offsets[i])
            room = max(0, min(int(reserved[i]), cap - off))
            rec, data = pa.oracle_item(sc.oracle, ocoder, blobs[i], overflows[i], eoss[i], room)
            assert res[i] == rec, (label, align, cap, i, off, room, res[i], rec)
            want[off:off + room] = data
            if not every:
                mine = got[off:off + int(reserved[i])]
                theirs = np.concatenate([data, np.full(int(reserved[i]) - room, MARKER, np.uint8)])
                assert np.array_equal(mine, theirs), (label, align, i)
        if every:
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (label, align, cap, "first wrong byte at %d" % int(bad[0]))
        assert np.all(got[min(cap, total):] == MARKER), (label, "bytes behind the total or the capacity were written")
        check_arrays(a, want_dir, want_index, want_status if fits else INDEX_TOO_SMALL, label)
        assert bi.index_size(eng, plan) == (0, 0, entries), label
        return offsets, total, got, res
    finally:
        a.close()
        eng.free(d_out)
        eng.free(d_off)


def plain(n):
    """(overflows, paddings) of n items without carried bits, padded with ones: what batch_index_api's batches are."""
    return [(0, 0)] * n, [0xFF] * n


# ----------------------------------------------------------------------------- 1: edges
def run_edges(sc, B, align):
    eng = sc.eng
    b = bi.edge_batch(sc, eng)
    plan = eng.encode_plan(b.items)
    ovs, eoss = plain(len(b.blobs))
    try:
        assert {x.size for x in b.blobs} >= set(bi.EDGE_LENGTHS)
        for limit, label in ((bi.ALL_WAVES, "every item a wave's"), (bi.ALL_TILES, "every item in tiles"), (0, "the rule")):
            with bi.wave_bytes(sc.lib, limit):
                check_indexed_launch(sc, eng, plan, b.d_in, b.blobs, sc.lens, sc.w.ocoder, ovs, eoss, align, B, label=label)
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 2: carried bits
def seeded_blobs(seed, lengths=None):
    rng = np.random.default_rng(seed)
    lengths = bi.seeded_lengths() if lengths is None else lengths
    return rng, [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(lengths)]


def run_carried_bits(sc):
    """The carried bits count towards an item's length -- so towards every offset behind it -- and not towards the index."""
    eng = sc.eng
    rng, blobs = seeded_blobs(1201)
    n = len(blobs)
    b = pa.Batch(eng, blobs, rng, overflows=pa.carried(rng, n))
    plan = eng.encode_plan(b.items)
    try:
        assert len({e for e in b.eoss}) == 2 and sum(1 for ov in b.overflows if ov[1]) >= 9
        bare = pa.encoded_lengths(sc.lens, blobs, [0] * n)
        with_carried = pa.encoded_lengths(sc.lens, blobs, [ov[1] for ov in b.overflows])
        assert np.any(bare != with_carried)  # (the two definitions differ on this batch: the check can tell them apart)
        for align, B in ((1, 512), (4, 64)):
            check_indexed_launch(sc, eng, plan, b.d_in, blobs, sc.lens, sc.w.ocoder, b.overflows, b.eoss, align, B, label="carried")
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 3: the output's capacity
def run_capacity(sc, align):
    """Exact, nothing, at an item's boundary, one byte into an item, one byte short of the total: the items in front of the
    edge as without one, the one across it the oracle's SHORT_BUFFER record, the ones behind it with no room."""
    eng = sc.eng
    rng = np.random.default_rng(1213)
    sizes = [40, 0, 700, pa.TILE + 9, 300, pa.SEG + 1, 17, 90, 1]
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    b = pa.Batch(eng, blobs, rng, overflows=pa.carried(rng, len(blobs), every=3))
    plan = eng.encode_plan(b.items)
    try:
        lens = pa.encoded_lengths(sc.lens, blobs, [ov[1] for ov in b.overflows])
        offsets, reserved = pa.expected_offsets(lens, align)
        total = int(offsets[-1])
        caps = [total, 0, int(offsets[3]), int(offsets[5]), int(offsets[3]) + 1, int(offsets[5]) + 1, total - 1]
        for cap in caps:
            _, _, _, res = check_indexed_launch(sc, eng, plan, b.d_in, blobs, sc.lens, sc.w.ocoder, b.overflows, b.eoss, align, 512,
                                                capacity=cap, label="capacity %d" % cap)
            # an item is short where its room -- what of its reserved length lies in front of the capacity -- is less than its length
            rooms = np.clip(np.minimum(reserved, cap - offsets[:-1]), 0, None)
            assert [r[:2] == SHORT for r in res] == (lens > rooms).tolist(), (cap, res)
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 4: an index that does not fit
def run_index_too_small(sc):
    """One entry short and a single entry: the status says so, the directory is whole, no index word, every offset 0, no
    output byte, every record the oracle's for no room, a packed size of nothing; the size call says what was needed.  Then
    the same plan with enough room, nothing reset in between."""
    eng = sc.eng
    rng, blobs = seeded_blobs(1217, bi.seeded_lengths(1217)[:15])
    n, B = len(blobs), 64
    b = pa.Batch(eng, blobs, rng, overflows=pa.carried(rng, n))
    plan = eng.encode_plan(b.items)
    try:
        entries = bi.expected(sc.lens, blobs, B)[1].size
        for icap in (entries - 1, 1):
            offsets, total, got, res = check_indexed_launch(sc, eng, plan, b.d_in, blobs, sc.lens, sc.w.ocoder, b.overflows, b.eoss, 16,
                                                            B, capacity=100_000, index_capacity=icap, label="index capacity %d" % icap)
            assert total == 0 and not offsets.any() and np.all(got == MARKER)
            assert pa.packed_size(eng, plan) == (0, 0, 0, 0)
            assert bi.index_size(eng, plan) == (0, 0, entries)
            assert all(r[3] == 0 for r in res) and SHORT in {r[:2] for r in res}  # (the oracle's records for no room)
        _, total, _, res = check_indexed_launch(sc, eng, plan, b.d_in, blobs, sc.lens, sc.w.ocoder, b.overflows, b.eoss, 16, B,
                                                label="behind the short ones")
        assert total > 0 and all(r[:2] == (0, 0) for r in res)
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 5: scan boundaries
PACK_TILES = [1, 3]
INDEX_TILES = [1, 3, 256]


def run_pack_tiles(sc, tile):
    eng = sc.eng
    rng, blobs = seeded_blobs(1223)
    n = len(blobs)
    b = pa.Batch(eng, blobs, rng, overflows=pa.carried(rng, n))
    plan = eng.encode_plan(b.items)
    try:
        assert n == bi.N_ITEMS
        with pa.pack_tile_items(sc.lib, tile):
            for align in (1, 16):
                check_indexed_launch(sc, eng, plan, b.d_in, blobs, sc.lens, sc.w.ocoder, b.overflows, b.eoss, align, 512,
                                     label="pack tile %d" % tile)
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


def run_index_tiles(sc, tile):
    eng = sc.eng
    b = bi.small_batch(sc, eng, seed=1229)
    plan = eng.encode_plan(b.items)
    ovs, eoss = plain(len(b.blobs))
    try:
        with ia.index_tile_blocks(sc.lib, tile):
            check_indexed_launch(sc, eng, plan, b.d_in, b.blobs, sc.lens, sc.w.ocoder, ovs, eoss, 1, 64, label="index tile %d" % tile)
            check_indexed_launch(sc, eng, plan, b.d_in, b.blobs, sc.lens, sc.w.ocoder, ovs, eoss, 1, 64, slack=150,
                                 label="index tile %d, roomy" % tile)
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


def run_built_in_tile(sc):
    """1 025 items at the built-in tile of 1 024: the offsets' scan crosses one tile boundary."""
    eng = sc.eng
    rng = np.random.default_rng(1231)
    n = 1_025
    blobs = [pc.inputs(rng, int(rng.integers(0, 100)), pc.KINDS[i % 4]) for i in range(n)]
    b = pa.Batch(eng, blobs, rng, overflows=pa.carried(rng, n, every=5))
    plan = eng.encode_plan(b.items)
    try:
        for align in (1, 16):
            check_indexed_launch(sc, eng, plan, b.d_in, blobs, sc.lens, sc.w.ocoder, b.overflows, b.eoss, align, 64,
                                 sample=list(range(0, n, 13)) + [1_023, 1_024], label="1 025 items")
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 6: fill kinds and roads
def run_plan_kinds_and_roads(sc, kind, road, want_road):
    """packed_api.every_plan_and_road through the new call; the plan of thread items is made on the device."""
    rng = np.random.default_rng(1237)
    eng, coder = sc.engine(road)
    d_items = None
    if kind == "strided":
        blobs = [pc.inputs(rng, 20000, "uniform") for _ in range(12)]
        b = pa.Batch(eng, blobs, None, eoss=[0x00] * 12)
        plan = eng.plan_strided(True, count=12, in_offset=b.in_offs[0], in_stride=20000, in_len=20000, out_offset=0,
                                out_stride=0, out_capacity=0, first_bit=0, eos_padding=0x00)
    elif kind == "threads":
        blobs = [pc.inputs(rng, int(rng.integers(16, 81)), pc.KINDS[i % 4]) for i in range(4_200)]
        b = pa.Batch(eng, blobs, rng, overflows=pa.carried(rng, len(blobs), every=9))
        plan, d_items = eng.encode_plan_from_device_items(b.items)
        assert eng.encode_stats(plan)["by_thread"] == len(blobs) >= 4_096
    else:
        blobs = pa.mixed_blobs(rng, with_large=False)
        b = pa.Batch(eng, blobs, rng, overflows=pa.carried(rng, len(blobs)))
        if kind == "host":
            plan = eng.encode_plan(b.items)
        else:
            plan, d_items = eng.encode_plan_from_device_items(b.items)
    try:
        stats = eng.encode_stats(plan)
        # (a plan of items that are all one thread's work has no kernel of the one-pass road to report)
        want = want_road if stats["by_wave"] + stats["by_pieces"] else pc.ROAD_TWO_PASS
        sample = None if len(blobs) < 100 else list(range(0, len(blobs), 7)) + [len(blobs) - 1]
        for align, B in ((1, 64), (8, 4096)):
            check_indexed_launch(sc, eng, plan, b.d_in, blobs, sc.lens, sc.w.ocoder, b.overflows, b.eoss, align, B, sample=sample,
                                 want_road=want, label="%s/%s" % (kind, road))
    finally:
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        if d_items:
            eng.free(d_items)
        b.close()
        sc.done(eng, coder)


# ----------------------------------------------------------------------------- 7: coders
OTHER_CODERS = ["holes", "hpack_lengths", "len4to15", "len8"]


def run_other_coders(sc, name):
    """The test coder less symbols 7 and 200 -- one hole in an item the tiles take, one in an item a wave takes: the status
    says so, those items stop at the symbol as in the oracle, and the offsets are the length query's (0 bits for such a
    symbol) -- and coders of other shapes."""
    if name == "holes":
        eng, coder = sc.engine(holes=True)
        code_lens, ocoder, want_status = sc.lens_holes, sc.w.ocoder_holes, INDEX_SYMBOL_WITHOUT_CODE
    else:
        ocoder, coder, lengths = pc.profile_coders(sc.w, name)
        eng, code_lens, want_status = harness.Engine(sc.lib, coder), np.asarray(lengths, dtype=np.int64), INDEX_OK
    b = bi.batch_of(sc, eng, "uniform", bi.seeded_lengths(1249)[:20] + [20_011, 9, 70], seed=1249)
    plan = eng.encode_plan(b.items)
    ovs, eoss = plain(len(b.blobs))
    try:
        if name == "holes":
            for blob in b.blobs:
                blob[blob == 7] = 8
                blob[blob == 200] = 201
            longest = max(range(len(b.blobs)), key=lambda i: b.blobs[i].size)
            b.blobs[longest][5_000] = 7
            b.blobs[-1][3] = 200
            eng.upload(b.d_in, b.host)
        for B, align in ((64, 1), (4096, 4)):
            _, _, _, res = check_indexed_launch(sc, eng, plan, b.d_in, b.blobs, code_lens, ocoder, ovs, eoss, align, B,
                                                want_status=want_status, label=name)
            if name == "holes":
                assert [i for i, r in enumerate(res) if r[:2] == UNKNOWN] == sorted([longest, len(b.blobs) - 1])
            else:
                assert all(r[:2] == (0, 0) for r in res)
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        sc.done(eng, coder)


# ----------------------------------------------------------------------------- 8: the same as the two calls
def run_same_as_the_two_calls(sc):
    """One plan, one input: the index call then the packed launch into one set of buffers, the new call into another --
    every buffer and every record equal; and the plan's own layout (roomy and too short in turn) survives both."""
    rng = np.random.default_rng(1259)
    sizes = [40, 700, pa.TILE + 9, pa.SEG + 1, 0, 2 * pa.SEG + 500, 17]
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    n, B, align = len(blobs), 512, 4
    eng, coder = sc.engine()
    own, pos = [], 5
    for i, blob in enumerate(blobs):
        cap = [2 * blob.size + 8, blob.size // 3][i % 2]
        own.append((pos, cap))
        pos += cap + 3
    b = pa.Batch(eng, blobs, rng, overflows=pa.carried(rng, n), own=own)
    plan = eng.encode_plan(b.items)
    d_own = eng.alloc(pos + 64)
    size = 4 * sum(sizes) + 64
    entries = bi.expected(sc.lens, blobs, B)[1].size

    def plain_launch():
        eng.fill(d_own, MARKER, pos + 64)
        eng.encode_launch(plan, b.d_in, d_own)
        return eng.download(d_own, pos + 64), eng.encode_results(plan, n)

    def one_set(call):
        d_out, d_off, a = eng.alloc(size), eng.alloc(8 * (n + 1)), bi.Arrays(eng, n, entries + 5)
        try:
            eng.fill(d_out, MARKER, size)
            eng.fill(d_off, 0xEE, 8 * (n + 1))
            call(d_out, d_off, a)
            eng.sync()
            return (eng.download(d_out, size), pa.download_u64(eng, d_off, n + 1), a.read(), eng.encode_results(plan, n),
                    pa.packed_size(eng, plan), bi.index_size(eng, plan), eng.encode_road(plan))
        finally:
            a.close()
            eng.free(d_out)
            eng.free(d_off)

    def two_calls(d_out, d_off, a):
        assert bi.plan_block_index(eng, plan, b.d_in, B, a.d_dir, a.d_index, a.capacity, a.d_status) == (0, 0)
        assert pa.launch_packed(eng, plan, b.d_in, d_out, size - 64, d_off, align) == (0, 0)

    def new_call(d_out, d_off, a):
        assert launch_indexed(eng, plan, b.d_in, d_out, size - 64, d_off, align, B, a.d_dir, a.d_index, a.capacity, a.d_status) == (0, 0)

    try:
        first_bytes, first_res = plain_launch()
        for i, blob in enumerate(blobs):  # (the plain launch itself, against the oracle)
            rec, data = pa.oracle_item(sc.oracle, sc.w.ocoder, blob, b.overflows[i], b.eoss[i], own[i][1])
            assert first_res[i] == rec and np.array_equal(first_bytes[own[i][0]:own[i][0] + own[i][1]], data), i
        theirs = one_set(two_calls)
        mine = one_set(new_call)
        for k, (x, y) in enumerate(zip(mine, theirs)):
            if k == 2:
                assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2] == INDEX_OK
            elif k < 2:
                assert np.array_equal(x, y), k
            else:
                assert x == y, (k, x, y)
        assert np.any(mine[0] != MARKER) and mine[4][2] > 0
        third_bytes, third_res = plain_launch()
        assert third_res == first_res and np.array_equal(third_bytes, first_bytes)
    finally:
        eng.free(d_own)
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        sc.done(eng, coder)


# ----------------------------------------------------------------------------- 9: the receiver
def run_receiver(sc):
    """Behind the new call, with nothing fetched: a decode plan chained to the encode plan decodes every item; and a dozen
    (item, block) ranges over the produced buffer, offsets, directory and index decode to the data's slices."""
    eng, lib = sc.eng, sc.lib
    rng, blobs = seeded_blobs(1277)
    n, B = len(blobs), 512
    b = pa.Batch(eng, blobs, rng, eoss=[0xFF] * n)
    plan = eng.encode_plan(b.items)
    dplan, rplan = eng.empty_decode_plan(), eng.empty_decode_plan()
    want_dir, want_index = bi.expected(sc.lens, blobs, B)
    entries = want_index.size
    lens = pa.encoded_lengths(sc.lens, blobs, [0] * n)
    offsets, _ = pa.expected_offsets(lens, 1)
    total = int(offsets[-1])
    d_out, d_off, d_back = eng.alloc(total + 64), eng.alloc(8 * (n + 1)), eng.alloc(b.host_in.size)
    a = bi.Arrays(eng, n, entries)
    d_ranges = None
    try:
        eng.fill(d_out, MARKER, total + 64)
        assert launch_indexed(eng, plan, b.d_in, d_out, total, d_off, 1, B, a.d_dir, a.d_index, entries, a.d_status) == (0, 0)
        assert eng.decode_plan_from_encode(dplan, plan)
        eng.fill(d_back, MARKER, b.host_in.size)
        eng.decode_launch(dplan, d_out, d_back)
        res = eng.decode_results(dplan, n)
        back = eng.download(d_back, b.host_in.size)
        want = np.full(b.host_in.size, MARKER, np.uint8)
        for i, blob in enumerate(blobs):
            want[b.in_offs[i]:b.in_offs[i] + blob.size] = blob
            assert res[i][:3] == (0, 0, blob.size), (i, res[i])
        assert np.array_equal(back, want)
        # ranges of whole blocks, straight from the device arrays the call left
        with_blocks = [i for i in range(n) if blobs[i].size > B]
        ranges, at = [], 3
        for k in range(12):
            i = with_blocks[int(rng.integers(0, len(with_blocks)))] if k else max(range(n), key=lambda j: blobs[j].size)
            nb = int(want_dir[i + 1][0] - want_dir[i][0])
            b0 = int(rng.integers(0, nb)) if k > 1 else [0, nb - 1][k]
            c = int(rng.integers(1, nb - b0 + 1)) if k else nb
            ranges.append((i, b0, c, at))
            at += min((b0 + c) * B, blobs[i].size) - b0 * B + 3
        flat = np.asarray([v for r in ranges for v in r], dtype=np.uint64)
        d_ranges = eng.alloc(flat.nbytes)
        eng.upload(d_ranges, flat.view(np.uint8))
        lib.aws_reset_error()
        assert lib.aws_huffman_amd_decode_plan_reset_item_block_ranges(
            rplan, a.d_dir, a.d_index, entries, n, B, d_off, None, 0, total, d_ranges, len(ranges), None) == 0, lib.aws_last_error()
        d_sym = eng.alloc(at + 64)
        try:
            eng.fill(d_sym, MARKER, at + 64)
            eng.decode_launch(rplan, d_out, d_sym)
            got = eng.download(d_sym, at + 64)
            res = eng.decode_results(rplan, len(ranges))
        finally:
            eng.free(d_sym)
        want = np.full(at + 64, MARKER, np.uint8)
        for k, (i, b0, c, o) in enumerate(ranges):
            piece = blobs[i][b0 * B:min((b0 + c) * B, blobs[i].size)]
            want[o:o + piece.size] = piece
            assert res[k][2] == piece.size and res[k][:2] in ((0, 0), SHORT), (k, res[k])
        assert np.array_equal(got, want)
        check_arrays(a, want_dir, want_index, INDEX_OK, "receiver")
    finally:
        if d_ranges:
            eng.free(d_ranges)
        a.close()
        for d in (d_out, d_off, d_back):
            eng.free(d)
        lib.aws_huffman_amd_decode_plan_destroy(dplan)
        lib.aws_huffman_amd_decode_plan_destroy(rplan)
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 10: a fitted engine
def enqueue_fit_indexed_encode(eng, clear, plan, d_in, length, B, a, d_out, capacity, d_off, stream):
    """clear the counts, count, fit, the indexed packed launch: four steps on `stream`, nothing waited for in between."""
    clear(eng, eng.d_counts, 256 * 8, stream)
    assert eng.lib.aws_huffman_amd_symbol_counts(-1, d_in, length, eng.d_counts, stream) == 0
    assert eng.fit_counts_async(None, stream) == (0, 0)
    assert launch_indexed(eng, plan, d_in, d_out, capacity, d_off, 1, B, a.d_dir, a.d_index, a.capacity, a.d_status, stream) == (0, 0)


def run_fitted_engine(lib, oracle, clear, B=512, n_bytes=60_000):
    """A (4, 12) engine: never fitted, the call is refused and writes nothing; then clear, count, fit and the new call
    enqueued back to back on the engine's stream."""
    eng = fa.FittedEngine(lib, 4, 12)
    rng = np.random.default_rng(1279)
    data = fa.shape_bytes("printable", n_bytes, 1283)
    spans = bi.fitted_batch(data, rng)
    blobs = [data[o:o + s] for o, s in spans]
    items = [dict(in_offset=o, in_len=s, out_offset=0, out_capacity=0) for o, s in spans]
    n = len(items)
    capacity = n_bytes * 2
    d_in, d_out, d_off = eng.alloc(n_bytes), eng.alloc(capacity), eng.alloc(8 * (n + 1))
    plan = eng.encode_plan(items)
    a = bi.Arrays(eng, n, sum(ia.n_blocks_of(s, B) for _, s in spans) + 1)
    try:
        eng.upload(d_in, data)
        eng.fill(d_out, MARKER, capacity)
        eng.fill(d_off, 0xEE, 8 * (n + 1))
        assert launch_indexed(eng, plan, d_in, d_out, capacity, d_off, 1, B, a.d_dir, a.d_index, a.capacity, a.d_status) == STATE
        eng.sync()
        d, x, status = a.read()
        assert np.all(d.view(np.uint64) == EE) and np.all(x == EE) and status == 0xEEEEEEEE
        assert np.all(eng.download(d_out, capacity) == MARKER) and np.all(eng.download(d_off, 8 * (n + 1)) == 0xEE)
        enqueue_fit_indexed_encode(eng, clear, plan, d_in, n_bytes, B, a, d_out, capacity, d_off, C.c_void_p(eng.stream))
        eng.sync()
        lengths = bi.check_fitted_chain(lib, oracle, eng, plan, data, blobs, B, a, d_out, d_off, capacity)
        assert not fa.is_flat(lengths)
    finally:
        a.close()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        for d in (d_in, d_out, d_off):
            eng.free(d)
        eng.close()


# ----------------------------------------------------------------------------- 11: refusals, no GPU, exports
def run_refusals(sc):
    """Every argument refusal of the two calls and the new call's own: nothing is written, and the plan works behind them."""
    eng, lib = sc.eng, sc.lib
    b = bi.batch_of(sc, eng, "uniform", [100, 0, 3_000], seed=1289)
    n, B = 3, 64
    plan = eng.encode_plan(b.items)
    none = eng.empty_encode_plan()
    a = bi.Arrays(eng, n, 60)
    d_out, d_off = eng.alloc(8_000), eng.alloc(8 * (n + 1) + 8)
    try:
        eng.fill(d_out, MARKER, 8_000)
        eng.fill(d_off, 0xEE, 8 * (n + 1) + 8)
        call = lambda **kw: launch_indexed(
            eng, kw.get("plan", plan), kw.get("d_in", b.d_in), kw.get("d_out", d_out), kw.get("cap", 8_000), kw.get("d_off", d_off),
            kw.get("align", 1), kw.get("B", B), kw.get("d_dir", a.d_dir), kw.get("d_index", a.d_index), kw.get("capacity", 60),
            kw.get("d_status", a.d_status))
        assert call(plan=None) == INVALID
        for bad in (0, 3, 24, 8192):
            assert call(align=bad) == INVALID, bad
        assert call(d_off=None) == INVALID
        assert call(d_off=d_off + 4) == INVALID
        assert call(d_out=None) == INVALID                  # no output with a capacity
        assert call(d_dir=None) == INVALID
        assert call(d_dir=a.d_dir + 4) == INVALID
        assert call(d_index=a.d_index + 4) == INVALID
        assert call(d_status=a.d_status + 2) == INVALID
        assert call(d_index=None) == INVALID                # a capacity without an index
        assert call(capacity=0) == INVALID                  # an index without a capacity
        assert call(d_index=None, capacity=0) == INVALID    # the index call's size query is not this call's
        assert call(plan=none, d_index=None, capacity=0) == INVALID
        assert call(d_in=None) == INVALID
        for bad in (0, 63, 96, 1 << 25):
            assert call(B=bad) == INVALID, bad
        assert bi.index_size(eng, plan)[:2] == INVALID and pa.packed_size(eng, plan)[:2] == INVALID  # (no call was made yet)
        eng.sync()
        d, x, status = a.read()
        assert np.all(d.view(np.uint64) == EE) and np.all(x == EE) and status == 0xEEEEEEEE
        assert np.all(eng.download(d_out, 8_000) == MARKER) and np.all(eng.download(d_off, 8 * (n + 1) + 8) == 0xEE)
        # the status and the output are optional; a plan without items
        assert call(d_status=None, d_out=None, cap=0) == (0, 0)
        eng.sync()
        d, x, status = a.read()
        want_dir, want_index = bi.expected(sc.lens, b.blobs, B)
        assert status == 0xEEEEEEEE and np.array_equal(d, want_dir)
        assert np.array_equal(x[:want_index.size].astype(np.int64), want_index)
        assert np.all(eng.download(d_out, 8_000) == MARKER)
        lens = pa.encoded_lengths(sc.lens, b.blobs, [0] * n)
        assert np.array_equal(pa.download_u64(eng, d_off, n + 1), pa.expected_offsets(lens, 1)[0])
        a0 = bi.Arrays(eng, 0, 1)
        try:
            eng.fill(d_off, 0xEE, 16)
            assert launch_indexed(eng, none, None, None, 0, d_off, 1, B, a0.d_dir, a0.d_index, 1, a0.d_status) == (0, 0)
            eng.sync()
            d, x, status = a0.read()
            assert status == INDEX_OK and d.tolist() == [[0, 0]] and x[0] == 0
            off = eng.download(d_off, 16).view(np.uint64)
            assert off[0] == 0 and off[1] == EE
            assert pa.packed_size(eng, none) == (0, 0, 0, 0) and bi.index_size(eng, none) == (0, 0, 1)
        finally:
            a0.close()
        ovs, eoss = plain(n)
        check_indexed_launch(sc, eng, plan, b.d_in, b.blobs, sc.lens, sc.w.ocoder, ovs, eoss, 1, 1 << 24, label="behind the refusals")
    finally:
        a.close()
        eng.free(d_out)
        eng.free(d_off)
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        lib.aws_huffman_amd_encode_plan_destroy(none)
        b.close()


def run_product_without_a_gpu(product):
    """Against the product library on a machine without a GPU: the call raises AWS_ERROR_UNSUPPORTED_OPERATION and touches
    nothing it was handed.  (With a GPU present this has nothing to say: tests/test_gpu_packed_index.py speaks there.)"""
    if product.aws_huffman_amd_device_count() > 0:
        return
    handle = np.full(4096, 0x11, np.uint8)  # (stands for the plan: there is none without a GPU)
    memory = np.full(8192, 0xEE, np.uint8)
    h, m = handle.ctypes.data, memory.ctypes.data
    product.aws_reset_error()
    assert product.aws_huffman_amd_encode_plan_launch_packed_indexed(h, m + 1024, m + 4096, 2048, m + 2048, 1, 64, m, m + 512, 8,
                                                                     m + 768, None) == -1
    assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    assert np.all(handle == 0x11) and np.all(memory == 0xEE)


def header_api_names():
    text = open(HEADER).read()
    return re.findall(r"AWS_COMPRESSION_API\s+[\w\s\*]*?\b(aws_\w+)\s*\(", text)


def run_exports(so_path):
    names = header_api_names()
    assert names == ["aws_huffman_amd_encode_plan_launch_packed_indexed"], names
    listing = subprocess.check_output(["nm", "-D", "--defined-only", so_path], text=True)
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported], [n for n in names if n not in exported]


# ----------------------------------------------------------------------------- 12: one plan through everything in turn
def run_lifecycle(sc):
    """One plan: the new call, a reset to fewer items, the new call, a packed launch, the new call with another block size, a
    reset to more items than ever (which allocates), the new call -- each step checked in full."""
    eng, lib = sc.eng, sc.lib
    rng = np.random.default_rng(1291)
    sizes = [int(v) for v in rng.integers(0, 6_000, 50)] + [20_011, 0, 64]
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    b = pa.Batch(eng, blobs, rng, overflows=pa.carried(rng, len(blobs)))
    plan = eng.encode_plan(b.items[:20])

    def check(k, align, B, label):
        check_indexed_launch(sc, eng, plan, b.d_in, blobs[:k], sc.lens, sc.w.ocoder, b.overflows[:k], b.eoss[:k], align, B, label=label)

    def reset(k):
        assert lib.aws_huffman_amd_encode_plan_reset(plan, eng._encode_item_array(b.items[:k]), k) == 0
        assert bi.index_size(eng, plan)[:2] == INVALID and pa.packed_size(eng, plan)[:2] == INVALID  # (behind a fill no size is known)

    try:
        check(20, 1, 512, "first")
        reset(7)
        check(7, 16, 512, "fewer items")
        pa.check_launch(sc.oracle, sc.w.ocoder, eng, plan, b.d_in, blobs[:7], sc.lens, b.overflows[:7], b.eoss[:7], 4, label="packed")
        check(7, 1, 64, "another block size")
        reset(len(blobs))
        check(len(blobs), 4, 128, "more items than ever")
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
