"""The sub-chunk records (struct hufd_lane_rec) on an MI355X (`pytest -m gpu`): the scenarios of tests/lane_record_cases.py,
which tests/test_emulated_lane_record.py runs on the emulator at the same sizes."""
import pytest

import harness
import lane_record_cases as lr
import packed_api as pa
import ranges_api as ra

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc(oracle):
    lib = ra.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    scene = pa.Scene(oracle, lib)
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
