"""CPU logic tests of the per-chunk emit record of the scan stage (struct hufd_emit_rec: dec_scan_small, dec_scan_apply,
dec_sync_true write it, dec_emit_fast and dec_emit_big decide from it) through the fiber emulator (tests/emu, UBSan; runs of
32 chunks): the scenarios of tests/emit_record_cases.py.  The claim on the chip is tests/test_gpu_emit_record.py's, at the
same sizes.  And the bound on a chunk's symbol count that the record's fields rest on, from the constants alone."""
import os
import re
import subprocess

import numpy as np
import pytest

import emit_record_cases as er
import harness
import parity_cases as pc

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")
DEVICE_TYPES = os.path.join(harness.REPO, "aws-c-compression_amd", "csrc", "hip", "device_types.h")


@pytest.fixture(scope="module")
def world(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    return pc.World(oracle, harness.Codec(harness.load_product(EMU_SO), "aws_"))


@pytest.fixture(scope="module")
def engine(world):
    eng = harness.Engine(world.product.lib, world.pcoder)
    yield eng
    eng.close()


def test_every_entry_state_of_a_chunk_inside_a_stream(world, engine):
    er.every_entry_state(world, engine)


@pytest.mark.parametrize("name", er.LISTED)
def test_chunks_that_leave_the_common_path(world, engine, name):
    er.the_lists(world, engine, name)


def test_stream_scanned_in_runs(world, engine):
    er.stream_scanned_in_runs(world, engine)


def test_three_streams_and_a_refill(world, engine):
    er.three_streams_and_a_refill(world, engine)


def constant(name):
    text = open(DEVICE_TYPES).read()
    m = re.search(r"#define\s+%s\s+\(?\s*(\d+)u?\s*\)?\s*(?:/\*|$)" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def test_symbols_of_a_chunk_inside_a_stream_stay_below_65000():
    """A chunk inside a stream is HUFD_DEC_CHUNK_BYTES of whole codes and at most one cut at either end: with a shortest code
    of m bits, at most chunk bits / m + 1 codes START in it.  For the test coder (shortest code 5 bits) that is 52 429: counts
    of 65 000 and more cannot occur.  The bound is the coder's, not the format's: at 4 bits it is 65 537, at 3 bits 87 382 --
    a coder with such codes breaks it, so nothing that has to hold for every coder may keep a chunk's count, or a sum of
    lane counts, in sixteen bits.  The emit record keeps the scan's own count (26 bits, enough for codes of one bit)."""
    chunk = constant("HUFD_DEC_SUB_BYTES") * constant("HUFD_DEC_LANES")
    assert chunk == er.CHUNK
    _, table_lens = harness.load_table()
    lens = np.array([table_lens[i] for i in range(256)], dtype=np.int64)
    shortest = int(lens[lens > 0].min())

    def most(bits):
        return chunk * 8 // bits + 1

    assert most(shortest) < 65_000, (shortest, most(shortest))
    assert [most(b) for b in (5, 4, 3)] == [52_429, 65_537, 87_382]
    assert most(1) < 1 << 26  # (wide_count's field, which the record copies)
