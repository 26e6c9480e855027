"""CPU logic tests of the sub-chunk records (struct hufd_lane_rec) through the fiber emulator (tests/emu, UBSan): the scenarios
of tests/lane_record_cases.py.  The claim on the chip is tests/test_gpu_lane_record.py's, at the same sizes."""
import os
import subprocess

import pytest

import harness
import lane_record_cases as lr
import packed_api as pa
import ranges_api as ra

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def sc(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    scene = pa.Scene(oracle, ra.bind(harness.load_product(EMU_SO)))
    yield scene
    scene.close()


def test_one_chunk_plus_8(sc):
    lr.one_chunk_plus_8(sc)


@pytest.mark.parametrize("tail", lr.TAILS)
def test_two_chunks_and_a_tail(sc, tail):
    lr.two_chunks_and_a_tail(sc, tail)


def test_entered_inside_a_byte(sc):
    lr.entered_inside_a_byte(sc)


def test_seventy_items_and_a_long_one(sc):
    lr.seventy_items_and_a_long_one(sc)


def test_one_repeated_symbol(sc):
    lr.one_repeated_symbol(sc)


def test_damaged_and_cut(sc):
    lr.damaged_and_cut(sc)


def test_ranges_and_locate(sc):
    lr.ranges_and_locate(sc)
