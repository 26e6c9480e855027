"""CPU logic tests of the byte planes of multi-byte elements (huffman_amd_planes.h) through the fiber emulator (tests/emu,
UBSan): the scenarios of tests/planes_api.py, every expectation numpy's or the oracle's.  The claim on the chip is
tests/test_gpu_planes.py's, at the same sizes."""
import os
import subprocess

import pytest

import harness
import packed_api as pa
import planes_api as pl

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = pa.Scene(oracle, pl.bind(harness.load_product(EMU_SO)))
    yield e
    pl.restore_switches(e.lib)
    e.close()


def clear(eng, dptr, size, stream):
    """(every emulated launch has run when its call returns: a fill is in order with whatever stream)"""
    eng.fill(dptr, 0, size)


@pytest.mark.parametrize("element_bytes", pl.SIZES)
def test_edges(emu, element_bytes):
    pl.run_edges(emu, element_bytes)


def test_grid(emu):
    pl.run_grid(emu)


def test_flush(emu):
    pl.run_flush(emu)


def test_add_semantics(emu):
    pl.run_add_semantics(emu)


@pytest.mark.parametrize("kind", pl.ROUND_TRIP_KINDS)
def test_round_trip(emu, kind):
    pl.run_round_trip(emu, kind, clear)


def test_refusals(emu):
    pl.run_refusals(emu)


def test_product_without_a_gpu_fails_loudly():
    pl.run_product_without_a_gpu(pl.bind(harness.load_product()))


def test_exports():
    pl.run_exports(harness.PRODUCT_SO)
