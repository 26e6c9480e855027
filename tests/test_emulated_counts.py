"""CPU logic tests of the symbol-count kernel (count_kernels.hip) through the fiber emulator (tests/emu): exact counts
at every head / tail alignment, input shapes, accumulation into the caller's array, and the flushes a workgroup makes
inside a launch.  The parity claim at size is tests/test_gpu_coder_from_data.py's, on an MI355X."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import build_api as ba
import harness

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    lib = ba.bind(harness.load_product(EMU_SO))
    patterns, lens = harness.load_table()
    coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    eng = harness.Engine(lib, coder)
    yield lib, eng
    lib.aws_huffman_amd_testing_set_count_flush_bytes(0)
    eng.close()


def device_counts(lib, eng, d_counts, d_in, offset, length, zero=True):
    if zero:
        eng.fill(d_counts, 0, 256 * 8)
    assert lib.aws_huffman_amd_symbol_counts(-1, d_in + offset if length or d_in else None, length, d_counts, None) == 0
    eng.sync()
    return eng.download(d_counts, 256 * 8).view(np.uint64)


def test_exact_counts_every_alignment(emu):
    lib, eng = emu
    data = harness.splitmix64_bytes(5, 64 * 1024)
    d_in, d_counts = eng.alloc(data.size + 64), eng.alloc(256 * 8)
    eng.upload(d_in, data)
    try:
        for offset in range(18):
            for length in (0, 1, 15, 16, 17, 255, 4097):
                got = device_counts(lib, eng, d_counts, d_in, offset, length)
                want = ba.bincount(data[offset:offset + length])
                assert np.array_equal(got, want), (offset, length)
    finally:
        eng.free(d_in)
        eng.free(d_counts)


@pytest.mark.parametrize("shape", ["uniform", "printable", "one_byte", "two_symbols"])
def test_input_shapes(emu, shape):
    lib, eng = emu
    n = 3 * 1024 * 1024 + 3
    raw = harness.splitmix64_bytes(9, n)
    data = {"uniform": raw, "printable": harness.printable_map(raw), "one_byte": np.full(n, 0xA7, np.uint8),
            "two_symbols": np.where(raw & 1, 0x41, 0x00).astype(np.uint8)}[shape]
    d_in, d_counts = eng.alloc(n + 16), eng.alloc(256 * 8)
    eng.upload(d_in, data, offset=5)
    try:
        got = device_counts(lib, eng, d_counts, d_in, 5, n)
        assert np.array_equal(got, ba.bincount(data)), shape
        assert int(got.sum()) == n
    finally:
        eng.free(d_in)
        eng.free(d_counts)


def test_calls_add_up(emu):
    lib, eng = emu
    a = harness.printable_map(harness.splitmix64_bytes(1, 100_003))
    b = harness.splitmix64_bytes(2, 70_001)
    d_a, d_b, d_counts = eng.alloc(a.size), eng.alloc(b.size), eng.alloc(256 * 8)
    eng.upload(d_a, a)
    eng.upload(d_b, b)
    try:
        device_counts(lib, eng, d_counts, d_a, 0, a.size)
        got = device_counts(lib, eng, d_counts, d_b, 0, b.size, zero=False)
        assert np.array_equal(got, ba.bincount(a) + ba.bincount(b))
        # length 0: nothing enqueued, the counts as they were (a NULL input too)
        assert lib.aws_huffman_amd_symbol_counts(-1, None, 0, d_counts, None) == 0
        assert lib.aws_huffman_amd_symbol_counts(-1, d_a, 0, None, None) == 0
        got = device_counts(lib, eng, d_counts, d_b, 0, 0, zero=False)
        assert np.array_equal(got, ba.bincount(a) + ba.bincount(b))
        # NULL pointers with a length, a device that does not exist
        for args in ((-1, None, 5, d_counts, None), (-1, d_a, 5, None, None), (7, d_a, 5, d_counts, None)):
            lib.aws_reset_error()
            assert lib.aws_huffman_amd_symbol_counts(*args) == -1
            assert lib.aws_last_error() == harness.AWS_ERROR_INVALID_ARGUMENT
    finally:
        for p in (d_a, d_b, d_counts):
            eng.free(p)


def test_flushes_inside_a_launch(emu):
    """A workgroup flushes its LDS counts after every 32 KiB here (instead of 1 GiB): many flushes a launch, the last
    step partly full, the head and the tail of workgroup 0 in the first flush."""
    lib, eng = emu
    n = 1024 * 1024 + 77
    raw = harness.splitmix64_bytes(3, n)
    shapes = [raw, np.full(n, 0x00, np.uint8), np.where(raw < 200, 0xFF, raw).astype(np.uint8)]
    d_in, d_counts = eng.alloc(n + 16), eng.alloc(256 * 8)
    try:
        for bytes_ in (1, 32 * 1024, 100 * 1024):
            lib.aws_huffman_amd_testing_set_count_flush_bytes(bytes_)
            for data in shapes:
                eng.upload(d_in, data, offset=3)
                got = device_counts(lib, eng, d_counts, d_in, 3, n)
                assert np.array_equal(got, ba.bincount(data)), bytes_
    finally:
        lib.aws_huffman_amd_testing_set_count_flush_bytes(0)
        eng.free(d_in)
        eng.free(d_counts)
