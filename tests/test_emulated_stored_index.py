"""CPU logic tests of indexed packed batches with stored items (huffman_amd_stored_index.h) through the fiber emulator
(tests/emu, UBSan): the scenarios of tests/stored_index_api.py, every expectation the oracle's and numpy's.  The claim on the
chip is tests/test_gpu_stored_index.py's, at the same sizes."""
import os
import subprocess

import pytest

import batch_index_api as bi
import harness
import packed_api as pa
import stored_index_api as si

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = pa.Scene(oracle, si.bind(harness.load_product(EMU_SO)))
    yield e
    e.close()


def clear(eng, dptr, size, stream):
    """(every emulated launch has run when its call returns: a fill is in order with whatever stream)"""
    eng.fill(dptr, 0, size)


# ---- the sender
@pytest.mark.parametrize("fill", ["host", "strided", "device"])
def test_one_call_is_the_two_calls(emu, fill):
    si.run_mixed(emu, fill)


def test_ties_are_stored(emu):
    si.run_ties(emu)


def test_never_stored(emu):
    si.run_never_stored(emu)


def test_capacity_clipping(emu):
    si.run_capacity_clipping(emu)


@pytest.mark.parametrize("tile,counts", pa.SCAN_TILES)
def test_scan_boundaries(emu, tile, counts):
    si.run_scan_boundaries(emu, tile, counts)


def test_index_too_small(emu):
    si.run_index_too_small(emu)


def test_other_states(emu):
    si.run_other_states(emu)


def test_fitted_engine(emu):
    si.run_fitted(emu, clear)


# ---- the receiver
@pytest.mark.parametrize("B", bi.RANGE_BLOCKS)
@pytest.mark.parametrize("name", bi.RANGE_CODERS)
def test_ranges(emu, name, B):
    si.run_ranges(emu, name, B)


def test_range_copy_alignment_sweep(emu):
    si.run_alignment_sweep(emu)


def test_the_index_of_a_stored_item_is_not_read(emu):
    si.run_ranges(emu, "test", 64, poison=True)


@pytest.mark.parametrize("name", ["test", "len8"])
def test_locate(emu, name):
    si.run_locate(emu, name)


@pytest.mark.parametrize("name", bi.RANGE_CODERS)
def test_damage(emu, name):
    si.run_damage(emu, name)


def test_plan_lifecycle(emu):
    si.run_lifecycle(emu)


# ---- the library's face
def test_exports():
    si.run_exports(harness.PRODUCT_SO)


def test_product_without_a_gpu():
    si.run_product_without_a_gpu(si.bind(harness.load_product()))
