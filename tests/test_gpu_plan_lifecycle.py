"""What a plan carries from one fill to the next, on an MI355X (`pytest -m gpu`): the scenarios of tests/plan_lifecycle.py
that tests/test_emulated_plan_lifecycle.py runs on the emulator, here at the same sizes -- and the two tours once more with
no host wait between a launch and the next reset, which only a chip can get wrong."""
import pytest

import harness
import packed_api as pa
import plan_lifecycle as pl
import ranges_api as ra

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def life(oracle):
    lib = ra.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    scene = pa.Scene(oracle, lib)
    one = pl.Life(scene)
    yield one
    one.close()
    scene.close()


def test_every_ordered_pair_of_fill_kinds(life):
    pl.run_decode_tour(life)


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
    pl.run_decode_tour_without_waits(life)


def test_encode_life_without_waits(life):
    pl.run_encode_life_without_waits(life)
