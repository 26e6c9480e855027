"""CPU logic tests of the block index and the range plans (huffman_amd_index.h, index_kernels.hip) through the fiber
emulator (tests/emu, UBSan): the scenarios of tests/index_api.py, every expectation numpy's or the oracle's.  The claim on
the chip is tests/test_gpu_index.py's, at the same sizes."""
import os
import subprocess

import pytest

import harness
import index_api as ia
import packed_api as pa

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = pa.Scene(oracle, ia.bind(harness.load_product(EMU_SO)))
    yield e
    e.lib.aws_huffman_amd_testing_set_index_tile_blocks(0)
    e.close()


def clear(eng, dptr, size, stream):
    """(every emulated launch has run when its call returns: a fill is in order with whatever stream)"""
    eng.fill(dptr, 0, size)


def test_index_edges(emu):
    ia.run_index_edges(emu)


@pytest.mark.parametrize("kind", ia.DATA_KINDS)
@pytest.mark.parametrize("block_symbols", ia.BLOCK_SIZES)
def test_block_sizes_and_data(emu, block_symbols, kind):
    ia.run_block_sizes(emu, block_symbols, kind)


@pytest.mark.parametrize("tile", ia.SCAN_TILES)
def test_scan_tiles(emu, tile):
    ia.run_scan_tiles(emu, tile)


@pytest.mark.parametrize("name", ia.OTHER_CODERS)
def test_other_coders(emu, name):
    ia.run_other_coders(emu, name)


def test_fitted_engine(emu):
    ia.run_fitted_engine(emu.lib, clear)


@pytest.mark.parametrize("block_symbols", ia.BLOCK_SIZES)
def test_every_block_as_its_own_range(emu, block_symbols):
    ia.run_every_block(emu, block_symbols)


@pytest.mark.parametrize("enc_offset", ia.RANGES_ENC_OFFSETS)
def test_ranges(emu, enc_offset):
    ia.run_ranges(emu, enc_offset)


def test_printable_text_under_a_fitted_coder(emu):
    ia.run_printable_fitted(emu, clear)


def test_refusals(emu):
    ia.run_refusals(emu)


def test_product_without_a_gpu_fails_loudly():
    ia.run_product_without_a_gpu(ia.bind(harness.load_product()))


def test_exports():
    ia.run_exports(harness.PRODUCT_SO)
