"""CPU logic tests of the packed batch encode (huffman_amd_packed.h: pack_kernels.hip between a length pass and an encode
pass) through the fiber emulator (tests/emu, UBSan): offsets against the length rule, every item's record and bytes
against the oracle's encode into the room the layout gives it, untouched bytes everywhere else.  The claim at size is
tests/test_gpu_packed.py's, on an MI355X."""
import os
import subprocess

import numpy as np
import pytest

import harness
import packed_api as pa
import parity_cases as pc

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = pa.Scene(oracle, pa.bind(harness.load_product(EMU_SO)))
    yield e
    e.close()


def test_offsets_and_bytes(emu):
    pa.offsets_and_bytes(emu)


@pytest.mark.parametrize("road,want_road", pa.ENCODE_ROADS)
@pytest.mark.parametrize("kind", pa.ENCODE_PLAN_KINDS)
def test_every_plan_and_road(emu, kind, road, want_road):
    pa.every_plan_and_road(emu, kind, road, want_road)


@pytest.mark.parametrize("tile,counts", pa.SCAN_TILES)
def test_scan_boundaries(emu, tile, counts):
    pa.scan_boundaries(emu, tile, counts)


@pytest.mark.parametrize("road", [None, "three-kernel"])
def test_capacity_clipping(emu, road):
    pa.capacity_clipping(emu, road)


def test_coder_with_holes(emu):
    pa.coder_with_holes(emu)


def test_the_plans_own_layout_survives(emu):
    pa.the_plans_own_layout_survives(emu)


@pytest.mark.parametrize("shape", ["threads", "chunks"])
def test_round_trip_through_a_chained_decode(emu, shape):
    pa.round_trip_through_a_chained_decode(emu, shape)


def test_arguments(emu):
    rng = np.random.default_rng(359)
    blobs = [pc.inputs(rng, n, "uniform") for n in (50, 5000)]
    eng, coder = emu.engine()
    b = pa.Batch(eng, blobs, rng)
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
