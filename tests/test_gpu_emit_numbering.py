"""dec_emit_fast's quarter-first thread numbering on an MI355X (`pytest -m gpu`): the scenarios of
tests/emit_numbering_cases.py, which tests/test_emulated_emit_numbering.py runs on the emulator at the same sizes."""
import pytest

import emit_numbering_cases as en
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


def test_source_and_output_offsets(world, engine):
    en.source_and_output_offsets(world, engine)


def test_entered_inside_a_byte(world, engine):
    en.entered_inside_a_byte(world, engine)


def test_sub_chunk_0_without_its_first_checkpoint(world, engine):
    en.missing_first_checkpoint(world, engine)


def test_lanes_that_never_meet_their_guessed_walk(world, engine):
    en.lanes_that_never_meet(world, engine)


def test_short_codes_over_the_stage(world):
    en.short_codes_over_the_stage(world)


def test_long_item_among_short_ones(world, engine):
    en.long_item_among_short_ones(world, engine)
