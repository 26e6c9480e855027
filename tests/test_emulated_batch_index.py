"""CPU logic tests of the block index over the items of an encode plan (huffman_amd_batch_index.h) through the fiber
emulator (tests/emu, UBSan): the scenarios of tests/batch_index_api.py, every expectation numpy's or the oracle's.  The claim
on the chip is tests/test_gpu_batch_index.py's, at the same sizes."""
import os
import subprocess

import pytest

import batch_index_api as bi
import harness
import packed_api as pa

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = pa.Scene(oracle, bi.bind(harness.load_product(EMU_SO)))
    yield e
    e.lib.aws_huffman_amd_testing_set_index_tile_blocks(0)
    e.lib.aws_huffman_amd_testing_set_batch_index_wave_bytes(0)
    e.close()


def clear(eng, dptr, size, stream):
    """(every emulated launch has run when its call returns: a fill is in order with whatever stream)"""
    eng.fill(dptr, 0, size)


def test_edges(emu):
    bi.run_edges(emu)


@pytest.mark.parametrize("kind", bi.DATA_KINDS)
@pytest.mark.parametrize("block_symbols", bi.BLOCK_SIZES)
def test_block_sizes_and_data(emu, block_symbols, kind):
    bi.run_block_sizes(emu, block_symbols, kind)


@pytest.mark.parametrize("tile", bi.INDEX_TILES)
def test_index_scan_tiles(emu, tile):
    bi.run_index_tiles(emu, tile)


@pytest.mark.parametrize("tile", bi.PACK_TILES)
def test_directory_scan_tiles(emu, tile):
    bi.run_pack_tiles(emu, tile)


def test_fill_kinds(emu):
    bi.run_fill_kinds(emu)


def test_plan_of_thread_items(emu):
    bi.run_thread_plan(emu)


def test_one_item_is_the_single_stream_index(emu):
    bi.run_one_item(emu)


def test_against_the_packed_launch(emu):
    bi.run_against_packed_launch(emu)


@pytest.mark.parametrize("name", bi.OTHER_CODERS)
def test_other_coders(emu, name):
    bi.run_other_coders(emu, name)


def test_fitted_engine(emu):
    bi.run_fitted_engine(emu.lib, emu.oracle, clear)


def test_capacity(emu):
    bi.run_capacity(emu)


def test_refusals(emu):
    bi.run_refusals(emu)


def test_product_without_a_gpu_fails_loudly():
    product = bi.bind(harness.load_product())
    bi.run_product_without_a_gpu(product)
    bi.run_ranges_without_a_gpu(product)


@pytest.mark.parametrize("block_symbols", bi.RANGE_BLOCKS)
@pytest.mark.parametrize("name", bi.RANGE_CODERS)
def test_item_block_ranges(emu, name, block_symbols):
    bi.run_item_block_ranges(emu, name, block_symbols)


@pytest.mark.parametrize("name", bi.RANGE_CODERS)
def test_item_range_damage(emu, name):
    bi.run_item_range_damage(emu, name)


@pytest.mark.parametrize("name", bi.SYMBOL_CODERS)
def test_item_symbols(emu, name):
    bi.run_item_symbols(emu, name)


def test_item_symbol_range_damage(emu):
    bi.run_item_symbol_range_damage(emu)


def test_one_plan_several_fills(emu):
    bi.run_one_plan_several_fills(emu)


def test_exports():
    bi.run_exports(harness.PRODUCT_SO)
