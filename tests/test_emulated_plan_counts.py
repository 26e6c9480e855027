"""CPU logic tests of the symbol counts of an encode plan's items (huffman_amd_plan_counts.h) through the fiber emulator
(tests/emu, UBSan): the scenarios of tests/plan_counts_api.py, every expectation numpy's.  The claim on the chip is
tests/test_gpu_plan_counts.py's, at the same sizes.  Beside them: the registers of the kernel the new body shares."""
import os
import re
import subprocess

import pytest

import harness
import packed_api as pa
import plan_counts_api as pk

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = pa.Scene(oracle, pk.bind(harness.load_product(EMU_SO)))
    yield e
    pk.restore_switches(e.lib)
    e.close()


def clear(eng, dptr, size, stream):
    """(every emulated launch has run when its call returns: a fill is in order with whatever stream)"""
    eng.fill(dptr, 0, size)


def test_edges(emu):
    pk.run_edges(emu)


def test_overlap_and_repeats(emu):
    pk.run_overlap_and_repeats(emu)


@pytest.mark.parametrize("kind", pa.ENCODE_PLAN_KINDS)
def test_plan_kinds(emu, kind):
    pk.run_plan_kind(emu, kind)


@pytest.mark.parametrize("name", pk.ENGINES)
def test_engines(emu, name):
    pk.run_engine(emu, name)


def test_add_semantics(emu):
    pk.run_add_semantics(emu)


def test_same_as_the_range_count(emu):
    pk.run_same_as_the_range_count(emu)


def test_flush(emu):
    pk.run_flush(emu)


def test_lifecycle(emu):
    pk.run_lifecycle(emu)


def test_count_changes_nothing(emu):
    pk.run_count_changes_nothing(emu)


@pytest.mark.parametrize("kind", pk.CHAIN_KINDS)
def test_chain(emu, kind):
    pk.run_chain(emu.lib, emu.oracle, clear, kind)


def test_refusals(emu):
    pk.run_refusals(emu)


def test_product_without_a_gpu_fails_loudly():
    pk.run_product_without_a_gpu(pk.bind(harness.load_product()))


def test_exports():
    pk.run_exports(harness.PRODUCT_SO)


def test_count_kernel_keeps_its_registers(tmp_path):
    """count_kernel with its fourth body, compiled for gfx950: at most 64 vector registers (eight waves a SIMD, as with three
    bodies), no scratch, no spill, and at most 80 scalar registers (the band of residency the three bodies had at 75)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(harness.REPO, "aws-c-compression_amd", "csrc", "hip", "count_kernels.hip")
    asm = tmp_path / "count_kernels.s"
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                           "-I" + os.path.join(harness.REPO, "include"), "-I" + os.path.join(harness.REPO, "include", "compat"),
                           src, "-o", str(asm)], stderr=subprocess.DEVNULL)
    listing = open(asm).read()
    names = [n for n in re.findall(r"\.name:\s+(\S+)", listing) if not n.endswith(".kd") and "count_kernel" in n]
    assert len(names) == 1, names  # (a body, not a kernel)
    field = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, listing).group(1))
    assert field("vgpr_count") <= 64, field("vgpr_count")
    assert field("sgpr_count") <= 80, field("sgpr_count")
    assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0
