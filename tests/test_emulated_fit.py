"""CPU logic tests of the coder fitted on the device (huffman_amd_fit.h, fit_kernels.hip) through the fiber emulator
(tests/emu, UBSan): the device's lengths against the host function's, both tables against the canonical coder of those
lengths, and engines whose tables a kernel wrote against the oracle on every encode and decode road.  The claim on the
chip is tests/test_gpu_fit.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fit_api as fa
import harness

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")

INVALID = (-1, harness.AWS_ERROR_INVALID_ARGUMENT)


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
    first = engines[0]  # (4, 12)
    lengths = fa.check_fit(lib, first, fa.printable_counts(), "printable")
    enc, lut = first.tables()
    second = fa.FittedEngine(lib, 4, 12)
    narrow = fa.FittedEngine(lib, 4, 10)
    try:
        # the receiver's half, from the first engine's own 256 bytes in device memory
        second.fill(second.d_status, 0xEE, 4)
        assert second.fit_lengths_async(first.d_bits) == (0, 0)
        assert second.status() == fa.FIT_OK
        enc2, lut2 = second.tables()
        assert np.array_equal(enc, enc2) and np.array_equal(lut, lut2)
        # refused, the tables as they were
        for bad, why in (([0] + lengths[1:], fa.FIT_LENGTH_ZERO), ([3] + lengths[1:], fa.FIT_LENGTH_OUT_OF_BOUNDS),
                         (lengths[:200] + [13] + lengths[201:], fa.FIT_LENGTH_OUT_OF_BOUNDS), ([7] * 256, fa.FIT_KRAFT_ABOVE_ONE)):
            assert second.fit_lengths(bad) == why, (bad[:4], why)
            enc2, lut2 = second.tables()
            assert np.array_equal(enc, enc2) and np.array_equal(lut, lut2), why
        # Kraft below 1: accepted, and the windows nobody owns say "no code" -- here one pair of 10-bit windows, behind
        # the 9-bit code
        short = [8] * 255 + [9]
        assert narrow.fit_lengths(short) == fa.FIT_OK
        enc3, lut3 = narrow.tables()
        want_enc, want_lut = fa.expected_tables(fa.host_rows(lib, short), 10)
        assert np.array_equal(enc3, want_enc) and np.array_equal(lut3, want_lut)
        assert list(np.flatnonzero(lut3 == 0)) == [1022, 1023]
        # a length the (4, 10) engine did not declare
        assert narrow.fit_lengths([8] * 254 + [7, 11]) == fa.FIT_LENGTH_OUT_OF_BOUNDS
        assert np.array_equal(narrow.tables()[1], want_lut)
    finally:
        second.close()
        narrow.close()


@pytest.mark.parametrize("shape", fa.SHAPES)
def test_fitted_engine_parity(lib, oracle, shape):
    eng = fa.FittedEngine(lib, 4, 12)
    try:
        fa.run_parity(lib, oracle, eng, shape)
    finally:
        eng.close()


def test_refit_between_launches_of_one_plan(lib, oracle):
    eng = fa.FittedEngine(lib, 4, 12)
    try:
        fa.run_refit_between_launches(lib, oracle, eng, 120_001)
    finally:
        eng.close()


def test_interface_errors(lib):
    h = C.c_void_p(0x1234)
    for lo, hi in ((3, 12), (4, 13), (8, 8), (9, 12), (4, 7)):
        lib.aws_reset_error()
        assert lib.aws_huffman_amd_engine_new_fitted(C.byref(h), -1, lo, hi) == -1, (lo, hi)
        assert lib.aws_last_error() == harness.AWS_ERROR_INVALID_ARGUMENT and h.value == 0x1234, (lo, hi)
    assert fa.new_fitted(lib, 4, 12, device=7)[:2] == INVALID
    lib.aws_reset_error()
    assert lib.aws_huffman_amd_engine_new_fitted(None, -1, 4, 12) == -1
    assert lib.aws_last_error() == harness.AWS_ERROR_INVALID_ARGUMENT

    eng = fa.FittedEngine(lib, 5, 11)
    patterns, lens = harness.load_table()
    coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    plain = harness.Engine(lib, coder)
    d_in, d_out, d_off = eng.alloc(4096), eng.alloc(4096), eng.alloc(64)
    try:
        assert lib.aws_huffman_amd_engine_is_fitted(eng.h) and not lib.aws_huffman_amd_engine_is_fitted(plain.h)
        assert lib.aws_huffman_amd_engine_max_code_bits(eng.h) == 11
        assert lib.aws_huffman_amd_engine_can_decode(eng.h) and lib.aws_huffman_amd_engine_encodes_in_one_pass(eng.h)

        def error_of(call, *args):
            lib.aws_reset_error()
            rc = call(*args)
            return rc, lib.aws_last_error() if rc else 0

        # NULL arguments, an engine with a coder
        fit_counts, fit_lengths = lib.aws_huffman_amd_engine_fit_counts, lib.aws_huffman_amd_engine_fit_lengths
        assert error_of(fit_counts, None, eng.d_counts, eng.d_bits, eng.d_status, None) == INVALID
        assert error_of(fit_counts, eng.h, None, eng.d_bits, eng.d_status, None) == INVALID
        assert error_of(fit_lengths, None, eng.d_bits, eng.d_status, None) == INVALID
        assert error_of(fit_lengths, eng.h, None, eng.d_status, None) == INVALID
        assert error_of(fit_counts, plain.h, eng.d_counts, eng.d_bits, eng.d_status, None) == INVALID
        assert error_of(fit_lengths, plain.h, eng.d_bits, eng.d_status, None) == INVALID
        assert error_of(lib.aws_huffman_amd_testing_engine_tables, eng.h, None, None, 1 << 11) == INVALID

        # never fitted: plans are made (their geometry is the bounds'), no launch is taken, nothing is written
        eng.fill(d_out, 0xC3, 4096)
        eng.fill(d_off, 0xEE, 64)
        plan = eng.encode_plan([dict(in_offset=0, in_len=1000, out_offset=0, out_capacity=2000)])
        dplan = eng.decode_plan([dict(in_offset=0, in_len=1000, out_offset=0, out_capacity=2000)])
        state = (-1, fa.AWS_ERROR_INVALID_STATE)
        assert error_of(lib.aws_huffman_amd_encode_plan_launch, plan, d_in, d_out, False, None) == state
        assert error_of(lib.aws_huffman_amd_encode_plan_launch, plan, d_in, d_out, True, None) == state
        assert error_of(lib.aws_huffman_amd_encode_plan_launch_packed, plan, d_in, d_out, 4096, d_off, 1, None) == state
        assert error_of(lib.aws_huffman_amd_decode_plan_launch, dplan, d_in, d_out, None) == state
        assert error_of(lib.aws_huffman_amd_decode_plan_launch_packed, dplan, d_in, d_out, 4096, d_off, 1, None) == state
        eng.sync()
        assert np.all(eng.download(d_out, 4096) == 0xC3) and np.all(eng.download(d_off, 64) == 0xEE)
        # ... and behind the first fit the same plans are
        status, _ = eng.fit_counts(fa.printable_counts())
        assert status == fa.FIT_OK
        assert error_of(lib.aws_huffman_amd_encode_plan_launch, plan, d_in, d_out, False, None) == (0, 0)
        eng.sync()
        # the status and the lengths are optional
        assert error_of(fit_counts, eng.h, eng.d_counts, None, None, None) == (0, 0)
        assert error_of(fit_lengths, eng.h, eng.d_bits, None, None) == (0, 0)
        eng.sync()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        lib.aws_huffman_amd_decode_plan_destroy(dplan)
    finally:
        for d in (d_in, d_out, d_off):
            eng.free(d)
        eng.close()
        plain.close()
        lib.aws_huffman_amd_table_coder_destroy(coder)


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
