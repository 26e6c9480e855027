"""CPU logic tests of the packed batch decode (huffman_amd_packed.h: the offset kernels of pack_kernels.hip between the scan
and the emit stage of a decode launch) through the fiber emulator (tests/emu, UBSan).  Every expectation is the oracle's:
sym_i from its decode of the item with room for everything -- symbols the padding bits spell included --, records and
bytes from its decode into the room the layout gives the item.  The claim at size is tests/test_gpu_packed_decode.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import build_api as ba
import harness
import packed_api as pa
import packed_decode_api as pd
import parity_cases as pc

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = pa.Scene(oracle, ba.bind(pd.bind(harness.load_product(EMU_SO))))
    yield e
    e.close()


def test_mixed_batch(emu):
    pd.mixed_batch(emu)


def test_padding_adds_symbols_or_not(emu):
    """The premise of the layout: sym_i is not the length of the text.  The test coder has no code of all ones or all
    zeros, so paddings 0xFF and 0x00 spell nothing; 0x20 starts with its five-bit code 00100 and spells a symbol more
    wherever five bits or more are padding.  The canonical coder of 4 .. 12 bits has the code 0000: there 0x00 does."""
    rng = np.random.default_rng(503)
    oc, pcoder, lengths = pd.shaped_coders(emu, "from_lengths 4..12")
    coded = np.flatnonzero(np.asarray(lengths))
    more = {}
    for i in range(60):
        plain = pc.inputs(rng, int(rng.integers(1, 300)), "uniform")
        other = coded[rng.integers(0, coded.size, plain.size)].astype(np.uint8)
        for name, coder, data, eos in (("test 0x00", emu.w.ocoder, plain, 0x00), ("test 0xFF", emu.w.ocoder, plain, 0xFF),
                                       ("test 0x20", emu.w.ocoder, plain, 0x20), ("4..12 0x00", oc, other, 0x00),
                                       ("4..12 0xFF", oc, other, 0xFF)):
            enc = emu.oracle.encode_all(coder, data, eos_padding=eos)
            rec, _ = pd.oracle_item(emu.oracle, coder, enc, 0, data.size + 16)
            assert rec[:2] == (0, 0) and rec[2] >= data.size
            more[name] = more.get(name, 0) + (rec[2] > data.size)
    emu.lib.aws_huffman_amd_table_coder_destroy(pcoder)
    assert more["test 0x00"] == 0 and more["test 0xFF"] == 0 and more["4..12 0xFF"] == 0, more
    assert 5 < more["test 0x20"] < 55 and 5 < more["4..12 0x00"] < 55, more


@pytest.mark.parametrize("kind", pd.DECODE_PLAN_KINDS)
def test_every_way_a_plan_is_made(emu, kind):
    pd.every_way_a_plan_is_made(emu, kind)


@pytest.mark.parametrize("road", pd.DECODE_ROADS)
def test_decode_road_switches(emu, road):
    pd.decode_road_switches(emu, road)


@pytest.mark.parametrize("tile,counts", pa.SCAN_TILES)
def test_scan_boundaries(emu, tile, counts):
    pd.scan_boundaries(emu, tile, counts)


def test_streams_that_stop_early(emu):
    pd.streams_that_stop_early(emu)


@pytest.mark.parametrize("road", [None, "long-way"])
def test_capacity_clipping(emu, road):
    pd.capacity_clipping(emu, road)


@pytest.mark.parametrize("name", pd.OTHER_CODERS)
def test_other_coders(emu, name):
    pd.other_coders(emu, name)


def test_the_plans_own_layout_survives(emu):
    pd.the_plans_own_layout_survives(emu)


def test_arguments(emu):
    rng = np.random.default_rng(569)
    eng = emu.eng
    streams = [(emu.encoded(t, 0x00, rng), 0) for t in (50, 5000, 40_000)]
    b = pd.Batch(emu, streams, None)
    plan = eng.decode_plan(b.items)
    n = len(streams)
    d_out, d_off = eng.alloc(200_000), eng.alloc(8 * (n + 1))
    d_extra = []
    try:
        assert pd.packed_size(eng, plan)[:2] == pd.INVALID  # (no packed launch yet)
        assert pd.launch_packed(eng, plan, b.d_in, d_out, 8192, None, 1) == pd.INVALID
        for align in (0, 3, 8192):
            assert pd.launch_packed(eng, plan, b.d_in, d_out, 8192, d_off, align) == pd.INVALID
        assert pd.launch_packed(eng, plan, b.d_in, None, 8192, d_off, 1) == pd.INVALID
        assert pd.packed_size(eng, plan)[:2] == pd.INVALID  # (none of those was one)
        # NULL output with no capacity: the offsets and the sizes, nothing written
        assert pd.launch_packed(eng, plan, b.d_in, None, 0, d_off, 4096) == (0, 0)
        syms = b.expect.syms()
        offsets, reserved = pd.expected_offsets(syms, 4096)
        assert np.array_equal(pa.download_u64(eng, d_off, n + 1), offsets)
        assert pd.packed_size(eng, plan) == (0, 0, int(offsets[-1]), int(reserved.max()))
        assert eng.decode_results(plan, n) == [pd.SHORT + (0, 0)] * n
        total, longest = C.c_uint64(), C.c_uint64()
        assert emu.lib.aws_huffman_amd_decode_plan_packed_size(plan, None, C.byref(longest), None) == 0 and longest.value == reserved.max()
        assert emu.lib.aws_huffman_amd_decode_plan_packed_size(plan, C.byref(total), None, None) == 0 and total.value == offsets[-1]
        # a reset: the sizes of the items before say nothing about these
        arr = eng._decode_item_array(b.items[:1])
        assert emu.lib.aws_huffman_amd_decode_plan_reset(plan, arr, 1) == 0
        assert pd.packed_size(eng, plan)[:2] == pd.INVALID
        # a packed input whose offsets decrease, with and without lengths: refused, a plan without items
        good = b.in_offs + [b.in_offs[-1] + streams[-1][0].size]
        d_good, d_bad = pd.upload_u64(eng, good), pd.upload_u64(eng, [good[0], good[2], good[1], good[3]])
        d_lens = pd.upload_u64(eng, [s[0].size for s in streams])
        d_extra += [d_good, d_bad, d_lens]
        for lens in (None, d_lens):
            assert pd.reset_packed_input(eng, plan, d_good, lens, n) == (0, 0)
            assert eng.decode_stats(plan)["items"] == n
            assert pd.reset_packed_input(eng, plan, d_bad, lens, n) == pd.INVALID
            assert eng.decode_stats(plan)["items"] == 0
            assert pd.packed_size(eng, plan)[:2] == pd.INVALID
        assert pd.reset_packed_input(eng, plan, None, None, n) == pd.INVALID
        # ... an item of 4 GiB: refused as well
        d_huge = pd.upload_u64(eng, [0, 1 << 32])
        d_extra.append(d_huge)
        assert pd.reset_packed_input(eng, plan, d_huge, None, 1) == pd.INVALID
        # a plan without items: success, offsets[0] = 0 written, sizes 0
        for make_empty in ("new", "packed-input"):
            empty = eng.empty_decode_plan()
            if make_empty == "packed-input":
                assert pd.reset_packed_input(eng, empty, d_good, None, 0) == (0, 0)
            eng.fill(d_off, 0xEE, 8 * (n + 1))
            assert pd.launch_packed(eng, empty, None, None, 0, d_off, 1) == (0, 0)
            eng.sync()
            got = eng.download(d_off, 16).view(np.uint64)
            assert got[0] == 0 and got[1] == 0xEEEEEEEEEEEEEEEE
            assert pd.packed_size(eng, empty) == (0, 0, 0, 0)
            emu.lib.aws_huffman_amd_decode_plan_destroy(empty)
    finally:
        eng.free(d_out)
        eng.free(d_off)
        for d in d_extra:
            eng.free(d)
        emu.lib.aws_huffman_amd_decode_plan_destroy(plan)
        b.close()
