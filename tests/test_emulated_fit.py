"""CPU logic tests of the coder fitted on the device (huffman_amd_fit.h, fit_kernels.hip) through the fiber emulator
(tests/emu, UBSan): the device's lengths against the host function's, both tables against the canonical coder of those
lengths, and engines whose tables a kernel wrote against the oracle on every encode and decode road.  The claim on the
chip is tests/test_gpu_fit.py's."""
import ctypes as C
import os
import subprocess

import pytest

import fit_api as fa
import harness

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")

OTHER_BOUNDS = [b for b in fa.BOUNDS if b != (4, 12)]  # ((4, 12): test_fitted_engine_parity)


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return fa.bind(harness.load_product(EMU_SO))


@pytest.fixture(scope="module")
def engines(lib):
    """One fitted engine for each pair of bounds."""
    made = [fa.FittedEngine(lib, lo, hi) for lo, hi in fa.BOUNDS]
    yield made
    for e in made:
        e.close()


def test_device_lengths_equal_host_lengths(lib, engines):
    fa.run_lengths_equal_host(lib, engines)


def test_device_tables_equal_host_engine_tables(lib, engines):
    fa.run_tables_equal_host(lib, engines)


def test_fit_lengths(lib, engines):
    fa.run_fit_lengths(lib, engines[0])  # (4, 12)


@pytest.mark.parametrize("shape", fa.SHAPES)
def test_fitted_engine_parity(lib, oracle, shape):
    fa.run_parity(lib, oracle, (4, 12), shape)


@pytest.mark.parametrize("shape", fa.SHAPES)
@pytest.mark.parametrize("bounds", OTHER_BOUNDS, ids=lambda b: "%d..%d" % b)
def test_fitted_engine_parity_within_other_bounds(lib, oracle, bounds, shape):
    """The same under every other pair of fit_api.BOUNDS: plans, capacities, stage sizes and the 10- or 12-bit kernel builds
    follow the bounds."""
    fa.run_parity(lib, oracle, bounds, shape)


def test_the_sweep_saw_a_spread_of_lengths(lib):
    fa.run_sweep_saw_a_spread(lib, [((4, 12), s) for s in fa.SHAPES] + [(b, s) for b in OTHER_BOUNDS for s in fa.SHAPES])


@pytest.mark.parametrize("shape", ["printable", "one byte"])
@pytest.mark.parametrize("road", ["three-kernel", "one-pass-fails"])
def test_fitted_engine_made_under_an_encode_road(lib, oracle, road, shape):
    """aws_huffman_amd_engine_new_fitted reads the road switch: the encode half of the parity run, packed and plain launch."""
    fa.run_parity(lib, oracle, (4, 12), shape, road=road, decode=False)


@pytest.mark.parametrize("kind", ["matched", "uniform"])
@pytest.mark.parametrize("case", fa.RECEIVER_CODES, ids=fa.receiver_id)
def test_receiver_codes(lib, oracle, case, kind):
    fa.run_receiver_codes(lib, oracle, *case, kinds=(kind,))


def test_refit_between_launches_of_one_plan(lib, oracle):
    eng = fa.FittedEngine(lib, 4, 12)
    try:
        fa.run_refit_between_launches(lib, oracle, eng, 120_001)
    finally:
        eng.close()


def test_interface_errors(lib):
    fa.run_interface_errors(lib)


def test_product_without_a_gpu_fails_loudly():
    """Against the product library (not the emulator): without a GPU there is no fitted engine, and the caller's pointer is
    as it was.  (With a GPU present this machine has nothing to say here: tests/test_gpu_fit.py speaks there.)"""
    product = fa.bind(harness.load_product())
    if product.aws_huffman_amd_device_count() > 0:
        return
    h = C.c_void_p(0x1234)
    product.aws_reset_error()
    assert product.aws_huffman_amd_engine_new_fitted(C.byref(h), -1, 4, 12) == -1
    assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION and h.value == 0x1234
