"""CPU logic tests of the byte planes of differences in runs (huffman_amd_planes_delta.h) through the fiber emulator
(tests/emu, UBSan): the scenarios of tests/planes_delta_api.py, every expectation numpy's or the oracle's.  The claim on the
chip is tests/test_gpu_planes_delta.py's, at the same sizes."""
import os
import subprocess

import pytest

import harness
import packed_api as pa
import planes_delta_api as pd

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = pa.Scene(oracle, pd.bind(harness.load_product(EMU_SO)))
    yield e
    pd.restore_switches(e.lib)
    e.close()


def clear(eng, dptr, size, stream):
    """(every emulated launch has run when its call returns: a fill is in order with whatever stream)"""
    eng.fill(dptr, 0, size)


@pytest.mark.parametrize("run_elements", pd.RUNS)
@pytest.mark.parametrize("element_bytes", pd.SIZES)
def test_edges(emu, element_bytes, run_elements):
    pd.run_edges(emu, element_bytes, run_elements)


@pytest.mark.parametrize("regime", list(pd.REGIMES))
def test_scan_regime(emu, regime):
    pd.run_regime(emu, regime)


@pytest.mark.parametrize("cap", pd.GRID_CAPS)
def test_grid(emu, cap):
    pd.run_grid(emu, cap)


def test_add_semantics(emu):
    pd.run_add_semantics(emu)


@pytest.mark.parametrize("kind", pd.CODER_KINDS)
def test_with_coder(emu, kind):
    pd.run_with_coder(emu, kind, clear)


def test_refusals(emu):
    pd.run_refusals(emu)


def test_product_without_a_gpu_fails_loudly():
    pd.run_product_without_a_gpu(pd.bind(harness.load_product()))


def test_exports():
    pd.run_exports(harness.PRODUCT_SO)
