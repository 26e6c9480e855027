"""CPU logic tests of packed batches with items stored raw (huffman_amd_stored.h) through the fiber emulator (tests/emu,
UBSan): the scenarios of tests/stored_api.py, every expectation the oracle's and numpy's.  The claim on the chip is
tests/test_gpu_stored.py's, at the same sizes.  Beside them: the registers of the two pack kernels, which host none of the
new scan kinds, and of unpack_records_kernel, which hosts them and the copy."""
import os
import re
import subprocess

import pytest

import harness
import packed_api as pa
import stored_api as sa

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = pa.Scene(oracle, sa.bind(harness.load_product(EMU_SO)))
    yield e
    e.close()


def clear(eng, dptr, size, stream):
    """(every emulated launch has run when its call returns: a fill is in order with whatever stream)"""
    eng.fill(dptr, 0, size)


@pytest.mark.parametrize("fill", ["host", "strided", "device"])
def test_mixed_batch(emu, fill):
    sa.run_mixed(emu, fill)


def test_ties_are_stored(emu):
    sa.run_ties(emu)


def test_never_stored(emu):
    sa.run_never_stored(emu)


def test_alignment_sweep(emu):
    sa.run_alignment_sweep(emu)


def test_capacity_clipping(emu):
    sa.run_capacity_clipping(emu)


@pytest.mark.parametrize("tile,counts", pa.SCAN_TILES)
def test_scan_boundaries(emu, tile, counts):
    sa.run_scan_boundaries(emu, tile, counts)


@pytest.mark.parametrize("with_lengths", [False, True])
def test_round_trip(emu, with_lengths):
    sa.run_round_trip(emu, with_lengths=with_lengths)


def test_receiver_checks(emu):
    sa.run_receiver_checks(emu)


def test_fitted_engine(emu):
    sa.run_fitted(emu, clear)


def test_exports():
    sa.run_exports(harness.PRODUCT_SO)


def test_pack_kernels_keep_their_registers(tmp_path):
    """pack_tile_sums_kernel and pack_offsets_kernel, compiled for gfx950 beside the builds of the new kinds: the registers
    they had (38 / 19 and 80 / 60 scalar / vector; 80 scalar registers are the most that admit eight workgroups a CU), no
    scratch."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(harness.REPO, "aws-c-compression_amd", "csrc", "hip", "pack_kernels.hip")
    asm = tmp_path / "pack_kernels.s"
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                           "-I" + os.path.join(harness.REPO, "include"), "-I" + os.path.join(harness.REPO, "include", "compat"),
                           src, "-o", str(asm)], stderr=subprocess.DEVNULL)
    listing = open(asm).read()
    found = {}
    for block in listing.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
        found[name] = (field("sgpr_count"), field("vgpr_count"), field("private_segment_fixed_size"))
    sums = [v for k, v in found.items() if "pack_tile_sums_kernel" in k]
    offsets = [v for k, v in found.items() if "pack_offsets_kernel" in k]
    assert len(sums) == 1 and len(offsets) == 1, sorted(found)
    assert sums[0][0] <= 38 and sums[0][1] <= 19 and sums[0][2] == 0, sums
    assert offsets[0][0] <= 80 and offsets[0][1] <= 60 and offsets[0][2] == 0, offsets
    # their host: 106 scalar registers as before (800 / (112 + 16): six waves a SIMD), so vector registers up to
    # 512 / 6 = 85, in granules of 8 at most 80, cost it no wave (the parent commit's build has 63, this one 65); no scratch
    host = [v for k, v in found.items() if "unpack_records_kernel" in k]
    assert len(host) == 1 and host[0][0] <= 106 and host[0][1] <= 80 and host[0][2] == 0, host
