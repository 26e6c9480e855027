"""CPU logic tests of dec_emit_fast's quarter-first thread numbering through the fiber emulator (tests/emu, UBSan): the
scenarios of tests/emit_numbering_cases.py.  The claim on the chip is tests/test_gpu_emit_numbering.py's, at the same sizes."""
import os
import subprocess

import pytest

import emit_numbering_cases as en
import harness
import parity_cases as pc

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def world(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return pc.World(oracle, harness.Codec(harness.load_product(EMU_SO), "aws_"))


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
