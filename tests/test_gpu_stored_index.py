"""Indexed packed batches with stored items (huffman_amd_stored_index.h) on an MI355X (`pytest -m gpu`): the scenarios of
tests/stored_index_api.py that tests/test_emulated_stored_index.py runs on the emulator, here at the same sizes, and the
sender's call replayed from a captured graph."""
import pytest

import batch_index_api as bi
import fit_api as fa
import harness
import packed_api as pa
import stored_index_api as si

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(oracle):
    lib = si.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    sc = pa.Scene(oracle, lib)
    yield sc
    sc.close()


# ---- the sender
@pytest.mark.parametrize("fill", ["host", "strided", "device"])
def test_one_call_is_the_two_calls(scene, fill):
    si.run_mixed(scene, fill)


def test_ties_are_stored(scene):
    si.run_ties(scene)


def test_never_stored(scene):
    si.run_never_stored(scene)


def test_capacity_clipping(scene):
    si.run_capacity_clipping(scene)


@pytest.mark.parametrize("tile,counts", pa.SCAN_TILES)
def test_scan_boundaries(scene, tile, counts):
    si.run_scan_boundaries(scene, tile, counts)


def test_index_too_small(scene):
    si.run_index_too_small(scene)


def test_other_states(scene):
    si.run_other_states(scene)


def test_fitted_engine(scene):
    hip = fa.Hip()
    si.run_fitted(scene, lambda eng, dptr, size, stream: hip.memset_async(dptr, 0, size, stream))


def test_replayed_from_a_graph(scene):
    si.run_replayed(scene, pa.HipGraphs())


# ---- the receiver
@pytest.mark.parametrize("B", bi.RANGE_BLOCKS)
@pytest.mark.parametrize("name", bi.RANGE_CODERS)
def test_ranges(scene, name, B):
    si.run_ranges(scene, name, B)


def test_range_copy_alignment_sweep(scene):
    si.run_alignment_sweep(scene)


def test_the_index_of_a_stored_item_is_not_read(scene):
    si.run_ranges(scene, "test", 64, poison=True)


@pytest.mark.parametrize("name", ["test", "len8"])
def test_locate(scene, name):
    si.run_locate(scene, name)


@pytest.mark.parametrize("name", bi.RANGE_CODERS)
def test_damage(scene, name):
    si.run_damage(scene, name)


def test_plan_lifecycle(scene):
    si.run_lifecycle(scene)
