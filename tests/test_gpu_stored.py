"""Packed batches with items stored raw (huffman_amd_stored.h) on an MI355X (`pytest -m gpu`): the scenarios of
tests/stored_api.py that tests/test_emulated_stored.py runs on the emulator, here at the same sizes, and the round trip
replayed from captured graphs."""
import pytest

import fit_api as fa
import harness
import packed_api as pa
import stored_api as sa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(oracle):
    lib = sa.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    sc = pa.Scene(oracle, lib)
    yield sc
    sc.close()


@pytest.mark.parametrize("fill", ["host", "strided", "device"])
def test_mixed_batch(scene, fill):
    sa.run_mixed(scene, fill)


def test_ties_are_stored(scene):
    sa.run_ties(scene)


def test_never_stored(scene):
    sa.run_never_stored(scene)


def test_alignment_sweep(scene):
    sa.run_alignment_sweep(scene)


def test_capacity_clipping(scene):
    sa.run_capacity_clipping(scene)


@pytest.mark.parametrize("tile,counts", pa.SCAN_TILES)
def test_scan_boundaries(scene, tile, counts):
    sa.run_scan_boundaries(scene, tile, counts)


@pytest.mark.parametrize("with_lengths", [False, True])
def test_round_trip(scene, with_lengths):
    sa.run_round_trip(scene, with_lengths=with_lengths)


def test_round_trip_replayed_from_graphs(scene):
    sa.run_round_trip(scene, graphs=pa.HipGraphs())


def test_receiver_checks(scene):
    sa.run_receiver_checks(scene)


def test_fitted_engine(scene):
    hip = fa.Hip()
    sa.run_fitted(scene, lambda eng, dptr, size, stream: hip.memset_async(dptr, 0, size, stream))
