"""CPU logic tests of what a plan carries from one fill to the next (csrc/host/engine.c, the kernels behind it) through the
fiber emulator (tests/emu, UBSan): the scenarios of tests/plan_lifecycle.py -- one decode plan through every ordered pair of
its seven fill kinds, its launch kinds and roads, what aws_huffman_amd_decode_plan_is_quiet may say, one encode plan through
its fills, launches and roads with the segment count going up and down --, every expectation the oracle's or numpy's.  A
look-back word left behind by an earlier, larger fill is a spin that never ends in the one-pass encoder's way back: it shows
here, under a time limit, before it can on a chip.  The claim on the chip is tests/test_gpu_plan_lifecycle.py's, at the same
sizes."""
import faulthandler
import os
import subprocess

import pytest

import harness
import packed_api as pa
import plan_lifecycle as pl
import ranges_api as ra

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def life(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    scene = pa.Scene(oracle, ra.bind(harness.load_product(EMU_SO)))
    one = pl.Life(scene)
    yield one
    one.close()
    scene.close()


@pytest.fixture(autouse=True)
def a_spin_ends_the_run():
    """A look-back word that is never written is a wait without end inside one emulated launch, which no Python exception can
    leave: after ten minutes in one test (the longest takes about one) the process says where it stands and exits."""
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def test_every_ordered_pair_of_fill_kinds_first_half(life):
    """(the tour is one plan's, fifty steps in order; here in two tests, each within a minute of emulation)"""
    pl.run_decode_tour(life, 0, 25)


def test_every_ordered_pair_of_fill_kinds_second_half(life):
    """(one test with the one above, in two parts: run alone, or behind a first half that failed, it takes the whole tour.
    Every test of this module works on the ONE plan of `life`, as the scenarios mean it to: a failure in one changes what the
    later ones start from, so read the first failure first)"""
    pl.run_decode_tour(life, 25, None)


def test_launch_kinds_between_fills(life):
    pl.run_launch_kinds(life)


@pytest.mark.parametrize("road", ["long-way", "tails-apart", "lean-sync", "all-kernels"])
def test_roads_between_fills(life, road):
    pl.run_roads(life, road)


@pytest.mark.parametrize("kind", pl.QUIET_VARIANTS)
def test_streams_that_list_chunks_then_clean_ones(life, kind):
    pl.run_listed_then_clean(life, kind)


@pytest.mark.parametrize("kind", pl.FILL_KINDS)
def test_what_is_quiet_may_say(life, kind):
    pl.run_is_quiet(life, kind)


@pytest.mark.parametrize("engine", pl.ENC_ENGINES)
def test_encode_plan_life(life, engine):
    pl.run_encode_life(life, engine)


def test_decode_tour_without_waits(life):
    """(every emulated launch has run when its call returns: this passes wherever the tour does)"""
    pl.run_decode_tour_without_waits(life)


def test_encode_life_without_waits(life):
    pl.run_encode_life_without_waits(life)
