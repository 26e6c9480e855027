"""Packed batches with constant items (huffman_amd_constant.h) on an MI355X (`pytest -m gpu`): the scenarios of
tests/constant_api.py that tests/test_emulated_constant.py runs on the emulator, here at the same sizes, and the sender's
launch captured once and replayed over different data."""
import pytest

import constant_api as ca
import fit_api as fa
import harness
import packed_api as pa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(oracle):
    lib = ca.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    sc = pa.Scene(oracle, lib)
    yield sc
    sc.close()


def test_rule_boundaries(scene):
    ca.run_rule_boundaries(scene)


def test_one_byte_changed_is_the_old_rule(scene):
    ca.run_one_byte_changed(scene)


def test_value_with_a_one_bit_code(scene):
    ca.run_one_bit_value(scene)


def test_hole_at_the_value(scene):
    ca.run_hole_at_the_value(scene)


def test_carried_bits_are_never_constant(scene):
    ca.run_carried_bits(scene)


@pytest.mark.parametrize("fill", ["host", "strided", "device"])
def test_mixed_batch(scene, fill):
    ca.run_mixed(scene, fill)


@pytest.mark.parametrize("road", ["three-kernel", "one-pass-fails"])
def test_mixed_batch_by_road(scene, road):
    ca.run_mixed(scene, "host", road)


@pytest.mark.parametrize("tile,counts", pa.SCAN_TILES)
def test_scan_boundaries(scene, tile, counts):
    ca.run_scan_boundaries(scene, tile, counts)


def test_capacity(scene):
    ca.run_capacity(scene)


@pytest.mark.parametrize("with_lengths", [False, True])
def test_round_trip(scene, with_lengths):
    ca.run_round_trip(scene, with_lengths=with_lengths)


def test_checks(scene):
    ca.run_checks(scene)


def test_host_laid_decode_plan(scene):
    ca.run_host_laid_plan(scene)


def test_fitted_engine(scene):
    hip = fa.Hip()
    ca.run_fitted(scene, lambda eng, dptr, size, stream: hip.memset_async(dptr, 0, size, stream))


def test_sender_replayed_from_a_graph(scene):
    ca.run_replays(scene, pa.HipGraphs())
