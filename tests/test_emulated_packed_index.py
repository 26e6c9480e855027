"""CPU logic tests of the packed encode launch that makes the batch's block index (huffman_amd_packed_index.h) through the
fiber emulator (tests/emu, UBSan): the scenarios of tests/packed_index_api.py, every expectation numpy's or the oracle's.
The claim on the chip is tests/test_gpu_packed_index.py's, at the same sizes."""
import os
import subprocess

import pytest

import harness
import packed_api as pa
import packed_index_api as pi

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = pa.Scene(oracle, pi.bind(harness.load_product(EMU_SO)))
    yield e
    pi.restore_switches(e.lib)
    e.close()


def clear(eng, dptr, size, stream):
    """(every emulated launch has run when its call returns: a fill is in order with whatever stream)"""
    eng.fill(dptr, 0, size)


@pytest.mark.parametrize("align", [1, 16])
@pytest.mark.parametrize("block_symbols", [64, 4096])
def test_edges(emu, block_symbols, align):
    pi.run_edges(emu, block_symbols, align)


def test_carried_bits(emu):
    pi.run_carried_bits(emu)


@pytest.mark.parametrize("align", [1, 16])
def test_output_capacity(emu, align):
    pi.run_capacity(emu, align)


def test_index_too_small(emu):
    pi.run_index_too_small(emu)


@pytest.mark.parametrize("tile", pi.PACK_TILES)
def test_offset_scan_tiles(emu, tile):
    pi.run_pack_tiles(emu, tile)


@pytest.mark.parametrize("tile", pi.INDEX_TILES)
def test_index_scan_tiles(emu, tile):
    pi.run_index_tiles(emu, tile)


def test_built_in_tile_boundary(emu):
    pi.run_built_in_tile(emu)


@pytest.mark.parametrize("road,want_road", pa.ENCODE_ROADS)
@pytest.mark.parametrize("kind", pa.ENCODE_PLAN_KINDS)
def test_plan_kinds_and_roads(emu, kind, road, want_road):
    pi.run_plan_kinds_and_roads(emu, kind, road, want_road)


@pytest.mark.parametrize("name", pi.OTHER_CODERS)
def test_other_coders(emu, name):
    pi.run_other_coders(emu, name)


def test_same_as_the_two_calls(emu):
    pi.run_same_as_the_two_calls(emu)


def test_receiver(emu):
    pi.run_receiver(emu)


def test_fitted_engine(emu):
    pi.run_fitted_engine(emu.lib, emu.oracle, clear)


def test_refusals(emu):
    pi.run_refusals(emu)


def test_product_without_a_gpu_fails_loudly():
    pi.run_product_without_a_gpu(pi.bind(harness.load_product()))


def test_exports():
    pi.run_exports(harness.PRODUCT_SO)


def test_lifecycle(emu):
    pi.run_lifecycle(emu)
