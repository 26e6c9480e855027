"""CPU logic tests of packed batches with constant items (huffman_amd_constant.h) through the fiber emulator (tests/emu,
UBSan): the scenarios of tests/constant_api.py, every expectation the oracle's and numpy's.  The claim on the chip is
tests/test_gpu_constant.py's, at the same sizes.  Beside them: what the kind buys, by the oracle alone."""
import os
import subprocess

import numpy as np
import pytest

import constant_api as ca
import fit_api as fa
import harness
import packed_api as pa

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = pa.Scene(oracle, ca.bind(harness.load_product(EMU_SO)))
    yield e
    e.close()


def clear(eng, dptr, size, stream):
    """(every emulated launch has run when its call returns: a fill is in order with whatever stream)"""
    eng.fill(dptr, 0, size)


def test_rule_boundaries(emu):
    ca.run_rule_boundaries(emu)


def test_one_byte_changed_is_the_old_rule(emu):
    ca.run_one_byte_changed(emu)


def test_value_with_a_one_bit_code(emu):
    ca.run_one_bit_value(emu)


def test_hole_at_the_value(emu):
    ca.run_hole_at_the_value(emu)


def test_carried_bits_are_never_constant(emu):
    ca.run_carried_bits(emu)


@pytest.mark.parametrize("fill", ["host", "strided", "device"])
def test_mixed_batch(emu, fill):
    ca.run_mixed(emu, fill)


@pytest.mark.parametrize("road", ["three-kernel", "one-pass-fails"])
def test_mixed_batch_by_road(emu, road):
    ca.run_mixed(emu, "host", road)


@pytest.mark.parametrize("tile,counts", pa.SCAN_TILES)
def test_scan_boundaries(emu, tile, counts):
    ca.run_scan_boundaries(emu, tile, counts)


def test_capacity(emu):
    ca.run_capacity(emu)


@pytest.mark.parametrize("with_lengths", [False, True])
def test_round_trip(emu, with_lengths):
    ca.run_round_trip(emu, with_lengths=with_lengths)


def test_checks(emu):
    ca.run_checks(emu)


def test_host_laid_decode_plan(emu):
    ca.run_host_laid_plan(emu)


def test_fitted_engine(emu):
    ca.run_fitted(emu, clear)


def test_exports():
    ca.run_exports(harness.PRODUCT_SO)


# ----------------------------------------------------------------------------- what it buys, by the oracle
ITEM = 4096
ELEMENTS = 40_000


def plane_sizes(oracle, lib, plane):
    """(packed bytes without the kind, with it) of one byte plane in items of 4 KiB under a (4, 12) coder fitted to the plane:
    the stored rule alone, and the constant rule in front of it."""
    lengths = np.asarray(fa.host_lengths(lib, np.bincount(plane, minlength=256).astype(np.uint64), 4, 12), dtype=np.int64)
    without = with_kind = 0
    for at in range(0, plane.size, ITEM):
        item = plane[at:at + ITEM]
        coded = (int(lengths[item].sum()) + 7) // 8
        old = item.size if coded >= item.size else coded
        without += old
        with_kind += ca.HEAD if item.size > ca.HEAD and coded > ca.HEAD and np.all(item == item[0]) else old
    return without, with_kind


def planes_ratio(oracle, lib, elements):
    planes = elements.view(np.uint8).reshape(-1, elements.dtype.itemsize).T
    sizes = [plane_sizes(oracle, lib, np.ascontiguousarray(p)) for p in planes]
    return sum(s[0] for s in sizes) / elements.nbytes, sum(s[1] for s in sizes) / elements.nbytes


def test_what_the_kind_buys(oracle, emu, capsys):
    """int64 below 2^24: planes 3 to 7 are zeros whatever the seed, (3 * 1.0 + 5 * 0.5) / 8 = 0.69 without the kind and
    (3 + 5 * 9 / 4096) / 8 = 0.376 with it.  The offsets of a packed batch (planes_delta_api's example): planes with the kind
    below planes of differences without it."""
    lib = emu.lib  # (the host's package-merge: the lengths a fit gives)
    rng = np.random.default_rng(1601)
    ids = rng.integers(0, 1 << 24, ELEMENTS, dtype=np.int64)
    without, with_kind = planes_ratio(oracle, lib, ids)
    offsets = np.concatenate([[0], np.cumsum(rng.integers(16, 81, ELEMENTS - 1))]).astype(np.int64)
    plain = planes_ratio(oracle, lib, offsets)
    run = 256
    deltas = offsets.copy()
    deltas[1:] -= offsets[:-1]
    deltas[::run] = offsets[::run]  # (a run's first element is kept whole: huffman_amd_planes_delta.h)
    delta = planes_ratio(oracle, lib, deltas)
    with capsys.disabled():
        print("\nint64 ids below 2^24: %.3f without the kind, %.3f with it" % (without, with_kind))
        print("offsets: planes %.3f / %.3f with the kind, planes of differences %.3f / %.3f with the kind" % (plain + delta))
    assert with_kind <= 0.38 and without >= 0.65, (without, with_kind)
    assert plain[1] < delta[0], (plain, delta)
