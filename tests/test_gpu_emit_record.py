"""The per-chunk emit record of the scan stage (struct hufd_emit_rec) on an MI355X (`pytest -m gpu`): the scenarios of
tests/emit_record_cases.py, which tests/test_emulated_emit_record.py runs on the emulator at the same sizes."""
import pytest

import emit_record_cases as er
import harness
import parity_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(oracle):
    lib = harness.load_product()
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    return pc.World(oracle, harness.Codec(lib, "aws_"))


@pytest.fixture(scope="module")
def engine(world):
    eng = harness.Engine(world.product.lib, world.pcoder)
    yield eng
    eng.close()


def test_every_entry_state_of_a_chunk_inside_a_stream(world, engine):
    er.every_entry_state(world, engine)


@pytest.mark.parametrize("name", er.LISTED)
def test_chunks_that_leave_the_common_path(world, engine, name):
    er.the_lists(world, engine, name)


def test_stream_scanned_in_runs(world, engine):
    er.stream_scanned_in_runs(world, engine)


def test_three_streams_and_a_refill(world, engine):
    er.three_streams_and_a_refill(world, engine)
