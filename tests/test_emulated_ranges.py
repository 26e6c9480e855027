"""CPU logic tests of the locate walk and the symbol-range plans (huffman_amd_ranges.h, decode_locate_body.inc) through the
fiber emulator (tests/emu, UBSan): the scenarios of tests/ranges_api.py, every expectation numpy's or the oracle's.  The
claim on the chip is tests/test_gpu_ranges.py's, at the same sizes."""
import os
import subprocess

import pytest

import harness
import index_api as ia
import packed_api as pa
import ranges_api as ra

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = pa.Scene(oracle, ra.bind(harness.load_product(EMU_SO)))
    yield e
    e.lib.aws_huffman_amd_testing_set_locate_lone_symbols(0)
    e.close()


@pytest.fixture(scope="module")
def road_results():
    return {}


def clear(eng, dptr, size, stream):
    """(every emulated launch has run when its call returns: a fill is in order with whatever stream)"""
    eng.fill(dptr, 0, size)


@pytest.mark.parametrize("kind", ia.DATA_KINDS)
def test_locate_edges(emu, kind):
    ra.run_locate_edges(emu, kind)


@pytest.mark.parametrize("limit", ra.ROADS_LIMITS)
@pytest.mark.parametrize("block_symbols", ra.ROADS_BLOCKS)
def test_both_roads_and_their_boundary(emu, road_results, block_symbols, limit):
    ra.run_roads(emu, block_symbols, limit, road_results)


@pytest.mark.parametrize("name", ["hpack_lengths", "len4to15", "len8"])
def test_other_coders(emu, name):
    ra.run_other_coder(emu, name)


def test_never_in_step(emu):
    ra.run_never_in_step(emu)


def test_a_walk_that_stops(emu):
    ra.run_walk_that_stops(emu)


@pytest.mark.parametrize("enc_offset", ia.RANGES_ENC_OFFSETS)
def test_range_plans(emu, enc_offset):
    ra.run_range_plans(emu, enc_offset)


def test_a_stream_cut_into_odd_pieces(emu):
    ra.run_odd_pieces(emu)


def test_fitted_engines(emu):
    ra.run_fitted(emu, clear)


def test_refusals(emu):
    ra.run_refusals(emu)


def test_product_without_a_gpu_fails_loudly():
    ra.run_product_without_a_gpu(ra.bind(harness.load_product()))


def test_exports():
    ra.run_exports(harness.PRODUCT_SO)
