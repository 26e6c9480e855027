"""CPU logic tests of the packed batch encode (huffman_amd_packed.h: pack_kernels.hip between a length pass and an encode
pass) through the fiber emulator (tests/emu, UBSan): offsets against the length rule, every item's record and bytes
against the oracle's encode into the room the layout gives it, untouched bytes everywhere else.  The claim at size is
tests/test_gpu_packed.py's, on an MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import harness
import packed_api as pa
import parity_cases as pc

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")

SEG = 16384   # HUFD_ENC_SEG_BYTES
TILE = 4096   # HUFD_ENC_SOLO_BYTES: one tile of the one-pass encoder
LARGE = 64    # HUFD_SCAN_SMALL_MAX segments: above it the workgroup scan


class Emu:
    def __init__(self, oracle):
        self.oracle = oracle
        self.lib = pa.bind(harness.load_product(EMU_SO))
        self.w = pc.World(oracle, harness.Codec(self.lib, "aws_"))
        self.lens = pa.code_lengths(self.w.table[1])
        self.lens_holes = pa.code_lengths(self.w.table[1], holes=(7, 200))

    def engine(self, road=None, holes=False):
        """A fresh coder, so a fresh engine that reads the road switch.  (engine, coder): both the caller's to free."""
        table = self.w.table
        if holes:
            lens = (C.c_uint8 * 256)(*table[1])
            lens[7] = lens[200] = 0
            table = (table[0], lens)
        with harness.encode_road(self.lib, road):
            coder = self.lib.aws_huffman_amd_table_coder_new(*table)
            return harness.Engine(self.lib, coder), coder

    def done(self, eng, coder):
        eng.close()
        self.lib.aws_huffman_amd_table_coder_destroy(coder)


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = Emu(oracle)
    yield e
    e.lib.aws_huffman_amd_testing_set_pack_tile_items(0)
    e.lib.aws_huffman_amd_testing_set_encode_road(0)


class Batch:
    """Items in device memory.  The items' own out_offset / out_capacity are whatever `own` says (default: no room at
    all -- a packed launch must not look at them)."""

    def __init__(self, eng, blobs, rng, overflows=None, eoss=None, own=None):
        self.eng, self.blobs = eng, blobs
        n = len(blobs)
        self.overflows = overflows or [(0, 0)] * n
        self.eoss = eoss or [[0xFF, 0x00][i % 2] for i in range(n)]
        self.host_in, self.in_offs = pa.lay_out(blobs, rng, first=1)
        self.d_in = eng.alloc(self.host_in.size)
        eng.upload(self.d_in, self.host_in)
        own = own or [(0, 0)] * n
        self.items = [dict(in_offset=self.in_offs[i], in_len=int(blobs[i].size), out_offset=own[i][0], out_capacity=own[i][1],
                           overflow_in=self.overflows[i], eos_padding=self.eoss[i]) for i in range(n)]

    def close(self):
        self.eng.free(self.d_in)


def carried(rng, n, every=4):
    out = []
    for i in range(n):
        if i % every == 1:
            nb = int(rng.integers(1, 33))
            out.append((int(rng.integers(0, 1 << nb)), nb))
        else:
            out.append((0, 0))
    return out


def mixed_blobs(rng, with_large=True):
    sizes = [0, 1, 15, 16, 17, 300, 700, TILE - 1, TILE, TILE + 1, SEG - 1, SEG, SEG + 1, 3 * SEG + 77, 0, 5 * SEG]
    if with_large:
        sizes.append((LARGE + 1) * SEG + 5)
    return [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]


def test_offsets_and_bytes(emu):
    rng = np.random.default_rng(301)
    blobs = mixed_blobs(rng)
    eng, coder = emu.engine()
    b = Batch(eng, blobs, rng, overflows=carried(rng, len(blobs)))
    plan = eng.encode_plan(b.items)
    try:
        # the length rule against the reference's own query where nothing is carried
        lens = pa.encoded_lengths(emu.lens, blobs, [ov[1] for ov in b.overflows])
        for i, blob in enumerate(blobs):
            if b.overflows[i][1] == 0:
                assert emu.oracle.encoded_length(emu.oracle.new_encoder(emu.w.ocoder), blob) == lens[i]
        for align in (1, 4, 16):
            _, total, _, res = pa.check_launch(emu.oracle, emu.w.ocoder, eng, plan, b.d_in, blobs, emu.lens, b.overflows, b.eoss,
                                               align, want_road=pc.ROAD_ONE_PASS, label="mixed")
            for i, r in enumerate(res):
                assert r[:2] == (0, 0) and r[3] == lens[i] and r[2] == blobs[i].size, (align, i, r)
    finally:
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        emu.done(eng, coder)


@pytest.mark.parametrize("road,want_road", [(None, pc.ROAD_ONE_PASS), ("three-kernel", pc.ROAD_TWO_PASS),
                                            ("one-pass-fails", pc.ROAD_GAVE_UP)])
@pytest.mark.parametrize("kind", ["host", "strided", "device", "threads"])
def test_every_plan_and_road(emu, kind, road, want_road):
    rng = np.random.default_rng(311)
    eng, coder = emu.engine(road)
    d_items = None
    if kind == "strided":
        blobs = [pc.inputs(rng, 20000, "uniform") for _ in range(12)]
        b = Batch(eng, blobs, None, eoss=[0x00] * 12)
        plan = eng.plan_strided(True, count=12, in_offset=b.in_offs[0], in_stride=20000, in_len=20000, out_offset=0,
                                out_stride=0, out_capacity=0, first_bit=0, eos_padding=0x00)
    elif kind == "threads":
        blobs = [pc.inputs(rng, int(rng.integers(1, 100)), pc.KINDS[i % 4]) for i in range(4200)]
        b = Batch(eng, blobs, rng, overflows=carried(rng, len(blobs), every=9))
        plan = eng.encode_plan(b.items)
        stats = eng.encode_stats(plan)
        assert stats["by_thread"] == len(blobs), stats
    else:
        blobs = mixed_blobs(rng, with_large=False)
        b = Batch(eng, blobs, rng, overflows=carried(rng, len(blobs)))
        if kind == "host":
            plan = eng.encode_plan(b.items)
        else:
            plan, d_items = eng.encode_plan_from_device_items(b.items)
    try:
        stats = eng.encode_stats(plan)
        # (a plan of items that are all one thread's work has no kernel of the one-pass road to report)
        want = want_road if stats["by_wave"] + stats["by_pieces"] else pc.ROAD_TWO_PASS
        sample = None if len(blobs) < 100 else list(range(0, len(blobs), 7)) + [len(blobs) - 1]
        for align in (1, 8):
            pa.check_launch(emu.oracle, emu.w.ocoder, eng, plan, b.d_in, blobs, emu.lens, b.overflows, b.eoss, align,
                            sample=sample, want_road=want, label="%s/%s" % (kind, road))
    finally:
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        if d_items:
            eng.free(d_items)
        b.close()
        emu.done(eng, coder)


@pytest.mark.parametrize("tile,counts", [(4096, (4095, 4096, 4097)), (300, (29999, 30000, 30001)), (64, (23457,)), (1, (301,))])
def test_scan_boundaries(emu, tile, counts):
    """The offset scan in tiles of a few items: item counts of exactly a tile (or a whole number of them), one more, one
    less, a number that is no multiple, more tiles than a workgroup has threads; against numpy's cumulative sum."""
    rng = np.random.default_rng(317 + tile)
    eng, coder = emu.engine()
    most = max(counts)
    blobs = [pc.inputs(rng, int(rng.integers(1, 40)), pc.KINDS[i % 4]) for i in range(most)]
    b = Batch(eng, blobs, None, overflows=carried(rng, most, every=5))
    try:
        with pa.pack_tile_items(emu.lib, tile):
            for n in counts:
                plan = eng.encode_plan(b.items[:n])
                ovs = b.overflows[:n]
                lens = pa.encoded_lengths(emu.lens, blobs[:n], [ov[1] for ov in ovs])
                for align in (1, 16):
                    offsets, total, _, _ = pa.check_launch(
                        emu.oracle, emu.w.ocoder, eng, plan, b.d_in, blobs[:n], emu.lens, ovs, b.eoss[:n], align,
                        sample=list(range(0, n, 97)) + [n - 1], label="tile %d, %d items" % (tile, n))
                    rounded = (lens + align - 1) // align * align
                    assert np.array_equal(offsets[1:], np.cumsum(rounded)) and total == int(rounded.sum())
                eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
    finally:
        b.close()
        emu.done(eng, coder)


@pytest.mark.parametrize("road", [None, "three-kernel"])
def test_capacity_clipping(emu, road):
    rng = np.random.default_rng(331)
    sizes = [40, 0, 700, TILE + 9, 300, SEG + 1, 2 * SEG + 500, 17, 3 * SEG, 90, 1]
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    eng, coder = emu.engine(road)
    b = Batch(eng, blobs, rng, overflows=carried(rng, len(blobs), every=3))
    plan = eng.encode_plan(b.items)
    try:
        for align in (1, 16):
            lens = pa.encoded_lengths(emu.lens, blobs, [ov[1] for ov in b.overflows])
            offsets, reserved = pa.expected_offsets(lens, align)
            total = int(offsets[-1])
            caps = [0, total - 1, total + 5]
            for k in (0, 2, 3, 5, 6, 8, 10):
                caps += [int(offsets[k]), int(offsets[k]) + 1, int(offsets[k] + reserved[k] // 2), int(offsets[k] + lens[k]) - 1]
            for cap in sorted(set(c for c in caps if c >= 0)):
                _, _, _, res = pa.check_launch(emu.oracle, emu.w.ocoder, eng, plan, b.d_in, blobs, emu.lens, b.overflows, b.eoss,
                                               align, capacity=cap, label="clip/%s" % road)
                kinds = {r[:2] for r in res}
                if cap < total - 16:
                    assert (-1, harness.AWS_ERROR_SHORT_BUFFER) in kinds, (cap, kinds)
    finally:
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        emu.done(eng, coder)


def test_coder_with_holes(emu):
    """Symbols 7 and 200 have no code: an item that meets one stops there as in the oracle; the offsets follow the length
    query (0 bits for such a symbol).  Among the items: one whose coded bits fill its room exactly in front of the
    symbol without a code (the reference then asks for room first)."""
    rng = np.random.default_rng(337)
    sizes = [30, 0, 600, TILE + 3, 100, SEG + 40, 2 * SEG + 9, 55, 4000, 12]
    blobs = []
    for i, n in enumerate(sizes):
        blob = pc.inputs(rng, n, pc.KINDS[i % 4])
        blob[blob == 7] = 8
        blob[blob == 200] = 201
        if n and i % 2 == 0:
            blob[int(rng.integers(0, n))] = 7 if i % 4 else 200
        blobs.append(blob)
    eight = int(np.flatnonzero(emu.lens_holes == 8)[0])
    blobs.append(np.asarray([eight, eight, eight, 7], np.uint8))
    blobs.append(np.asarray([200], np.uint8))
    eng, coder = emu.engine(holes=True)
    b = Batch(eng, blobs, rng, overflows=carried(rng, len(blobs), every=5))
    plan = eng.encode_plan(b.items)
    try:
        for align in (1, 4):
            _, _, _, res = pa.check_launch(emu.oracle, emu.w.ocoder_holes, eng, plan, b.d_in, blobs, emu.lens_holes, b.overflows,
                                           b.eoss, align, want_road=pc.ROAD_TWO_PASS, label="holes")
            kinds = {r[:2] for r in res}
            assert (-1, harness.AWS_ERROR_COMPRESSION_UNKNOWN_SYMBOL) in kinds and (0, 0) in kinds, kinds
    finally:
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        emu.done(eng, coder)


def test_the_plans_own_layout_survives(emu):
    rng = np.random.default_rng(347)
    sizes = [40, 700, TILE + 9, SEG + 1, 0, 2 * SEG + 500, 17]
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    eng, coder = emu.engine()
    own, pos = [], 5
    for i, blob in enumerate(blobs):
        cap = [2 * blob.size + 8, blob.size // 3][i % 2]  # roomy, and too short
        own.append((pos, cap))
        pos += cap + 3
    b = Batch(eng, blobs, rng, overflows=carried(rng, len(blobs)), own=own)
    plan = eng.encode_plan(b.items)
    d_out = eng.alloc(pos + 64)

    def plain():
        eng.fill(d_out, pa.MARKER, pos + 64)
        eng.encode_launch(plan, b.d_in, d_out)
        return eng.download(d_out, pos + 64), eng.encode_results(plan, len(blobs))

    try:
        first_bytes, first_res = plain()
        for i, blob in enumerate(blobs):  # (the plain launch itself, against the oracle)
            rec, data = pa.oracle_item(emu.oracle, emu.w.ocoder, blob, b.overflows[i], b.eoss[i], own[i][1])
            assert first_res[i] == rec and np.array_equal(first_bytes[own[i][0]:own[i][0] + own[i][1]], data), i
        pa.check_launch(emu.oracle, emu.w.ocoder, eng, plan, b.d_in, blobs, emu.lens, b.overflows, b.eoss, 4, label="between")
        third_bytes, third_res = plain()
        assert third_res == first_res and np.array_equal(third_bytes, first_bytes)
    finally:
        eng.free(d_out)
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        emu.done(eng, coder)


@pytest.mark.parametrize("shape", ["threads", "chunks"])
def test_round_trip_through_a_chained_decode(emu, shape):
    """decode_plan_from_encode behind a packed launch reads at the offsets that launch made, as many bytes as were
    produced -- whatever the items' own out_capacity fields say (here: one byte each, less than anything encodes to)."""
    rng = np.random.default_rng(353)
    if shape == "threads":
        blobs = [pc.inputs(rng, int(rng.integers(1, 90)), pc.KINDS[i % 4]) for i in range(5000)]
    else:
        blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate([70000, 300, 20000, SEG, 1, 140000, 900])]
    n = len(blobs)
    eng, coder = emu.engine()
    b = Batch(eng, blobs, rng, own=[(0, 1)] * n)
    plan = eng.encode_plan(b.items)
    dplan = eng.empty_decode_plan()
    d_back = eng.alloc(b.host_in.size)
    try:
        for align in (1, 16):
            offsets, total, got, _ = pa.check_launch(emu.oracle, emu.w.ocoder, eng, plan, b.d_in, blobs, emu.lens, b.overflows,
                                                     b.eoss, align, sample=list(range(0, n, 53)), label="round trip")
            # (check_launch freed its output: encode again into a buffer that stays, then chain the decode to it)
            d_out, d_off = eng.alloc(total + 64), eng.alloc(8 * (n + 1))
            try:
                assert pa.launch_packed(eng, plan, b.d_in, d_out, total, d_off, align) == (0, 0)
                assert eng.decode_plan_from_encode(dplan, plan)
                stats = eng.decode_stats(dplan)
                assert stats["items"] == n and (stats["by_thread"] == n) == (shape == "threads"), stats
                eng.fill(d_back, pa.MARKER, b.host_in.size)
                eng.decode_launch(dplan, d_out, d_back)
                res = eng.decode_results(dplan, n)
                back = eng.download(d_back, b.host_in.size)
                want = np.full(b.host_in.size, pa.MARKER, np.uint8)
                for i, blob in enumerate(blobs):
                    want[b.in_offs[i]:b.in_offs[i] + blob.size] = blob
                    assert res[i][:3] == (0, 0, blob.size), (i, res[i])
                assert np.array_equal(back, want)
            finally:
                eng.free(d_out)
                eng.free(d_off)
    finally:
        eng.free(d_back)
        eng.lib.aws_huffman_amd_decode_plan_destroy(dplan)
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        emu.done(eng, coder)


def test_arguments(emu):
    rng = np.random.default_rng(359)
    blobs = [pc.inputs(rng, n, "uniform") for n in (50, 5000)]
    eng, coder = emu.engine()
    b = Batch(eng, blobs, rng)
    plan = eng.encode_plan(b.items)
    d_out, d_off = eng.alloc(8192), eng.alloc(8 * 3)
    INVALID = (-1, harness.AWS_ERROR_INVALID_ARGUMENT)
    try:
        assert pa.packed_size(eng, plan)[:2] == INVALID  # (no packed launch yet)
        assert pa.launch_packed(eng, plan, b.d_in, d_out, 8192, None, 1) == INVALID
        for align in (0, 3, 8192):
            assert pa.launch_packed(eng, plan, b.d_in, d_out, 8192, d_off, align) == INVALID
        assert pa.launch_packed(eng, plan, b.d_in, None, 8192, d_off, 1) == INVALID
        assert pa.packed_size(eng, plan)[:2] == INVALID  # (none of those was one)
        # NULL output with no capacity: the offsets and the sizes, nothing written
        assert pa.launch_packed(eng, plan, b.d_in, None, 0, d_off, 4096) == (0, 0)
        lens = pa.encoded_lengths(emu.lens, blobs, [0, 0])
        offsets, reserved = pa.expected_offsets(lens, 4096)
        assert np.array_equal(pa.download_u64(eng, d_off, 3), offsets)
        assert pa.packed_size(eng, plan) == (0, 0, int(offsets[-1]), int(reserved.max()))
        # a reset: the sizes of the items before say nothing about these
        arr = eng._encode_item_array(b.items[:1])
        assert eng.lib.aws_huffman_amd_encode_plan_reset(plan, arr, 1) == 0
        assert pa.packed_size(eng, plan)[:2] == INVALID
        # a plan without items: success, offsets[0] = 0 written, sizes 0
        empty = eng.empty_encode_plan()
        eng.fill(d_off, 0xEE, 24)
        assert pa.launch_packed(eng, empty, None, None, 0, d_off, 1) == (0, 0)
        eng.sync()
        got = eng.download(d_off, 24).view(np.uint64)
        assert got[0] == 0 and got[1] == 0xEEEEEEEEEEEEEEEE
        assert pa.packed_size(eng, empty) == (0, 0, 0, 0)
        eng.lib.aws_huffman_amd_encode_plan_destroy(empty)
    finally:
        eng.free(d_out)
        eng.free(d_off)
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        emu.done(eng, coder)
