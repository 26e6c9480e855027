"""Packed batch decode on an MI355X (`pytest -m gpu`): a receiver's view of what a packed encode launch wrote.  The
BASELINE batch of 65 536 x 16 KiB, a million header-sized items and one 1 GiB item at full size -- the plan made from the
packed buffer's offsets on the device, the output laid out by the device, symbol counts of a sample against the oracle,
every item's symbols against the original --, odd lengths at align 1 with every output byte against the oracle, and a
packed launch captured in a graph and replayed on new input.  Then the edge scenarios of tests/packed_decode_api.py that
tests/test_emulated_packed_decode.py runs on the emulator, here at the same sizes: other coders, streams that stop early,
clipped capacities, the decode roads and every way a plan is made under a packed launch."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import build_api as ba
import harness
import packed_api as pa
import packed_decode_api as pd
import parity_cases as pc

pytestmark = pytest.mark.gpu

PROBE = harness.load_json("survey_probe_records.json")
STEP = 256 << 20


@pytest.fixture(scope="module")
def lib():
    lib = pd.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    return lib


@pytest.fixture(scope="module")
def world(oracle, lib):
    return pc.World(oracle, harness.Codec(lib, "aws_"))


@pytest.fixture(scope="module")
def eng(world):
    e = harness.Engine(world.product.lib, world.pcoder)
    yield e
    e.close()


def min_bits(world):
    return min(int(l) for l in world.table[1] if l)


def received_batch(world, eng, data, in_offs, in_lens, align, sample, eos=0xFF):
    """The items data[in_offs[i] : + in_lens[i]] through a packed encode launch at `align`, then as a receiver has them:
    the packed buffer, its offsets (and, with an alignment, the lengths) in device memory.  The decode plan is made from
    those by aws_huffman_amd_decode_plan_reset_packed_input; a size query, then the packed decode launch into exactly the
    total.  The sample's symbol counts and records against the oracle's decode of the encoded bytes, every item's first
    in_len symbols against the original, the total against the sum of the records' `produced`."""
    n = len(in_lens)
    in_lens, in_offs = np.asarray(in_lens, np.int64), np.asarray(in_offs, np.int64)
    d_in = eng.alloc(data.size)
    eng.upload(d_in, data)
    eplan, d_items = pa.plan_from_records(eng, in_offs, in_lens, eos=eos)
    d_enc_off, d_off = eng.alloc(8 * (n + 1)), eng.alloc(8 * (n + 1))
    assert pa.launch_packed(eng, eplan, d_in, None, 0, d_enc_off, align) == (0, 0)
    enc_total = pa.packed_size(eng, eplan)[2]
    d_enc = eng.alloc(enc_total + 64)
    dplan = eng.empty_decode_plan()
    d_lens, d_out = None, None
    try:
        assert pa.launch_packed(eng, eplan, d_in, d_enc, enc_total, d_enc_off, align) == (0, 0)
        enc_res = pa.results_array(eng, eplan, n)
        assert np.all(enc_res["rc"] == 0)
        enc_offs = pa.download_u64(eng, d_enc_off, n + 1)
        enc_lens = enc_res["produced"].astype(np.int64)
        if align > 1:  # (the gap bytes were never written: the sender ships the lengths)
            d_lens = pd.upload_u64(eng, enc_lens)
        else:
            assert np.array_equal(np.diff(enc_offs), enc_lens)
        assert pd.reset_packed_input(eng, dplan, d_enc_off, d_lens, n) == (0, 0)
        assert eng.decode_stats(dplan)["items"] == n
        # how much room: a size query
        eng.fill(d_off, 0xEE, 8 * (n + 1))
        assert pd.launch_packed(eng, dplan, d_enc, None, 0, d_off, align) == (0, 0)
        rc, err, total, longest = pd.packed_size(eng, dplan)
        assert (rc, err) == (0, 0)
        query_offsets = pa.download_u64(eng, d_off, n + 1)
        d_out = eng.alloc(total + 64)
        eng.fill(d_out, pd.MARKER, total + 64)
        assert pd.launch_packed(eng, dplan, d_enc, d_out, total, d_off, align) == (0, 0)
        res = pd.results_array(eng, dplan, n)
        offsets = pa.download_u64(eng, d_off, n + 1)
        assert np.array_equal(offsets, query_offsets) and pd.packed_size(eng, dplan) == (0, 0, total, longest)
        assert offsets[0] == 0 and offsets[-1] == total and np.all(offsets % align == 0)
        produced = res["produced"].astype(np.int64)
        reserved = (produced + align - 1) // align * align
        assert np.all(res["rc"] == 0), int(np.flatnonzero(res["rc"])[0])
        assert np.array_equal(np.diff(offsets), reserved) and total == int(reserved.sum()) and longest == int(reserved.max())
        if align == 1:
            assert total == int(produced.sum())
        assert np.all(produced >= in_lens)
        # the sample: symbol count, record and bytes as the oracle decodes the encoded bytes with room for everything
        for i in sample:
            enc = eng.download(d_enc, int(enc_lens[i]), offset=int(enc_offs[i]))
            rec, want = pd.oracle_item(world.oracle, world.ocoder, enc, 0, int(enc_lens[i]) * 8 // min_bits(world) + 8)
            assert rec[:2] == (0, 0)
            assert int(offsets[i + 1] - offsets[i]) == (rec[2] + align - 1) // align * align, (i, rec)
            assert tuple(res[i]) == rec, (i, tuple(res[i]), rec)
            got = eng.download(d_out, int(offsets[i + 1] - offsets[i]), offset=int(offsets[i]))
            assert np.array_equal(got[:rec[2]], want[:rec[2]]) and np.all(got[rec[2]:] == pd.MARKER), i
        # every item: the first in_len symbols at its offset are the original
        uniform = np.all(produced == in_lens) and align == 1
        for lo in range(0, n, 65536):
            hi = min(lo + 65536, n)
            got = eng.download(d_out, int(offsets[hi] - offsets[lo]), offset=int(offsets[lo]))
            if uniform:
                assert np.array_equal(got, data[in_offs[lo]:in_offs[hi - 1] + in_lens[hi - 1]]), lo
                continue
            # (the originals lie back to back: symbol k of item i is output byte offsets[i] + k)
            first = in_offs[lo]
            assert np.array_equal(in_offs[lo:hi] + in_lens[lo:hi], np.append(in_offs[lo + 1:hi], in_offs[hi - 1] + in_lens[hi - 1]))
            shift = (offsets[lo:hi] - offsets[lo]) - (in_offs[lo:hi] - first)
            index = np.repeat(shift, in_lens[lo:hi]) + np.arange(int(in_lens[lo:hi].sum()), dtype=np.int64)
            assert np.array_equal(got[index], data[first:first + index.size]), lo
        assert np.all(eng.download(d_out, 64, offset=total) == pd.MARKER)
        return produced, in_lens
    finally:
        eng.lib.aws_huffman_amd_decode_plan_destroy(dplan)
        eng.lib.aws_huffman_amd_encode_plan_destroy(eplan)
        for p in (d_in, d_items, d_enc_off, d_off, d_enc, d_lens, d_out):
            if p:
                eng.free(p)


def test_batch_of_65536_buffers_of_16k(world, eng):
    """BASELINE configs[3]: 65 536 x 16 KiB of splitmix64 seed 5, packed encode at align 1, the plan from the device
    offsets without lengths."""
    count, size = 65536, 16384
    data = harness.splitmix64_bytes(5, count * size)
    in_offs = np.arange(count, dtype=np.int64) * size
    rng = np.random.default_rng(5)
    sample = [0, 1, count - 1] + [int(x) for x in rng.integers(0, count, 37)]
    received_batch(world, eng, data, in_offs, np.full(count, size, np.int64), 1, sample)


@pytest.mark.parametrize("align,eos", [(1, 0xFF), (8, 0x20)])
def test_a_million_header_sized_items(world, eng, align, eos):
    """16 to 80 bytes of printable text each.  Padding 0x20 starts with a five-bit code of the test coder: wherever five
    bits or more are padding the item decodes to a symbol more than was encoded, and the layout must say so."""
    count = 1_000_000
    rng = np.random.default_rng(7)
    in_lens = rng.integers(16, 81, count).astype(np.int64)
    in_offs = np.concatenate([[0], np.cumsum(in_lens)[:-1]]).astype(np.int64)
    data = harness.printable_map(harness.splitmix64_bytes(9, int(in_lens.sum())))
    sample = [0, 1, count - 1] + [int(x) for x in rng.integers(0, count, 60)]
    produced, lens = received_batch(world, eng, data, in_offs, in_lens, align, sample, eos=eos)
    more = int((produced > lens).sum())
    assert (more == 0) if eos == 0xFF else (count // 8 < more < count * 7 // 8), more


def test_one_item_of_1gib(world, eng):
    """The 1 GiB stream of BASELINE configs[1] as one item: offsets [0, sym] with sym the oracle's count for the encoded
    stream, and the output's digest equal to the input's."""
    rec = PROBE["streams"]["G1G"]
    n, e = rec["len"], rec["encoded_len"]
    d_in, d_enc, d_off, d_enc_off = eng.alloc(n), eng.alloc(e + 64), eng.alloc(16), pd.upload_u64(eng, [0, e])
    eplan = eng.encode_plan([dict(in_offset=0, in_len=n, out_offset=0, out_capacity=e + 64)])
    dplan = eng.empty_decode_plan()
    d_out = None
    try:
        eng.fill_splitmix64(d_in, n, rec["seed"])
        eng.encode_launch(eplan, d_in, d_enc)
        assert eng.encode_results(eplan, 1)[0][:4] == (0, 0, n, e)
        eng.free(d_in)
        d_in = None
        # the oracle's word on the encoded stream, with room for everything
        enc = np.empty(e, np.uint8)
        for off in range(0, e, STEP):
            enc[off:off + STEP] = eng.download(d_enc, min(STEP, e - off), offset=off)
        assert hashlib.sha256(memoryview(enc)).hexdigest() == rec["sha256_encoded"]
        want_rec, want = pd.oracle_item(world.oracle, world.ocoder, enc, 0, n + 64)
        del enc
        sym = want_rec[2]
        assert want_rec[:2] == (0, 0) and sym >= n
        assert hashlib.sha256(memoryview(np.ascontiguousarray(want[:n]))).hexdigest() == rec["sha256_input"]
        assert pd.reset_packed_input(eng, dplan, d_enc_off, None, 1) == (0, 0)
        assert eng.decode_stats(dplan)["by_pieces"] == 1
        d_out = eng.alloc(sym + 64)
        eng.fill(d_out, pd.MARKER, sym + 64)
        assert pd.launch_packed(eng, dplan, d_enc, d_out, sym, d_off, 1) == (0, 0)
        assert eng.decode_results(dplan, 1) == [want_rec]
        assert list(pa.download_u64(eng, d_off, 2)) == [0, sym]
        assert pd.packed_size(eng, dplan) == (0, 0, sym, sym)
        h = hashlib.sha256()
        for off in range(0, n, STEP):
            h.update(eng.download(d_out, min(STEP, n - off), offset=off).tobytes())
        assert h.hexdigest() == rec["sha256_input"]
        assert np.array_equal(eng.download(d_out, sym - n + 64, offset=n), np.concatenate([want[n:sym], np.full(64, pd.MARKER, np.uint8)]))
    finally:
        eng.lib.aws_huffman_amd_decode_plan_destroy(dplan)
        eng.lib.aws_huffman_amd_encode_plan_destroy(eplan)
        for p in (d_in, d_enc, d_off, d_enc_off, d_out):
            if p:
                eng.free(p)


def odd_streams(world, rng, sizes):
    """Whole streams of so many symbols each; paddings 0x00, 0xFF and 0x20 (which spells a symbol) in turn."""
    eos = (0x00, 0xFF, 0x20)
    return [(pc.oracle_encode(world, pc.inputs(rng, n, pc.KINDS[i % 4]), eos=eos[i % 3]), 0) for i, n in enumerate(sizes)]


def test_align_1_over_many_odd_lengths(world, eng):
    """Neighbouring items share dwords and cache lines: 3000 items of odd lengths from 1 to 40 000 symbols (some entered
    inside their first byte), their outputs back to back; offsets, records and every output byte against the oracle."""
    rng = np.random.default_rng(11)
    sizes = [1, 3, 5, 511, 513, 4095, 4097, 16383, 16385] + [int(x) | 1 for x in rng.integers(1, 40000, 2991)]
    streams = odd_streams(world, rng, sizes)
    streams = [(enc, int(rng.integers(1, 8)) if i % 6 == 4 else 0) for i, (enc, _) in enumerate(streams)]
    host_in, in_offs = pd.lay_out(streams, rng, first=1)
    d_in = eng.alloc(host_in.size)
    eng.upload(d_in, host_in)
    items = [dict(in_offset=in_offs[i], in_len=int(enc.size), first_bit=fb, out_offset=0, out_capacity=0)
             for i, (enc, fb) in enumerate(streams)]
    expect = pd.Expect(world.oracle, world.ocoder, streams, min_bits(world))
    assert np.any(expect.syms() % 2 == 0) and np.any(expect.syms() % 2 == 1)
    plan = eng.decode_plan(items)
    try:
        pd.check_launch(eng, plan, d_in, expect, 1, label="odd lengths", launches=2)
        total = int(expect.syms().sum())
        pd.check_launch(eng, plan, d_in, expect, 1, capacity=total // 2 + 1, label="odd lengths, half the room")
    finally:
        eng.lib.aws_huffman_amd_decode_plan_destroy(plan)
        eng.free(d_in)


def test_captured_graph(world, eng):
    """A packed decode launch captured on the engine's stream (after a first one outside the capture, which allocates the
    plan's second record arrays) and replayed on new input: the same slots of encoded bytes filled with streams of other
    text, which decode to other lengths.  Offsets, records and bytes of every replay against the oracle."""
    hip = pa.HipGraphs()
    rng = np.random.default_rng(13)
    slots = [200, 5000, 16384, 70000, 33, 40000, 900, 100000, 600, 0] * 6
    n = len(slots)

    def fill(kinds):
        """Every slot full of a stream of text of one kind, cut at the slot's end."""
        out = []
        for i, s in enumerate(slots):
            plain = pc.inputs(rng, s * 8 // min_bits(world) + 8, kinds[i % len(kinds)])
            out.append((pc.oracle_encode(world, plain)[:s].copy(), 0))
        return out

    first, second = fill(["printable"]), fill(["uniform", "short", "long", "printable"])
    host_in, in_offs = pd.lay_out(first, None)
    d_offs, d_lens = pd.upload_u64(eng, in_offs), pd.upload_u64(eng, slots)
    room = sum(slots) * 8 // min_bits(world) + 64
    d_in, d_out, d_off = eng.alloc(host_in.size), eng.alloc(room + 64), eng.alloc(8 * (n + 1))
    plan = eng.empty_decode_plan()
    stream = C.c_void_p(eng.stream)
    graph_exec = None
    try:
        assert pd.reset_packed_input(eng, plan, d_offs, d_lens, n) == (0, 0)
        eng.upload(d_in, host_in)
        assert pd.launch_packed(eng, plan, d_in, d_out, room, d_off, 4, stream) == (0, 0)
        hip.call("hipStreamSynchronize", stream)
        graph_exec = hip.capture(stream, lambda: pd.launch_packed(eng, plan, d_in, d_out, room, d_off, 4, stream))
        totals = []
        for streams in (second, first, second):
            host, _ = pd.lay_out(streams, None)
            eng.upload(d_in, host)
            eng.fill(d_out, pd.MARKER, room + 64)
            eng.fill(d_off, 0xEE, 8 * (n + 1))
            eng.sync()
            hip.call("hipGraphLaunch", graph_exec, stream)
            hip.call("hipStreamSynchronize", stream)
            expect = pd.Expect(world.oracle, world.ocoder, streams, min_bits(world))
            syms = expect.syms()
            offsets, reserved = pd.expected_offsets(syms, 4)
            assert np.array_equal(pa.download_u64(eng, d_off, n + 1), offsets)
            got = eng.download(d_out, room + 64)
            res = eng.decode_results(plan, n)
            want = np.full(room + 64, pd.MARKER, np.uint8)
            for i in range(n):
                rec, data = expect.item(i, int(syms[i]))
                assert res[i] == rec, (i, res[i], rec)
                want[int(offsets[i]):int(offsets[i]) + int(syms[i])] = data
            assert np.array_equal(got, want)
            assert pd.packed_size(eng, plan, stream)[2:] == (int(offsets[-1]), int(reserved.max()))
            totals.append(int(offsets[-1]))
        assert totals[0] != totals[1] and totals[0] == totals[2], totals
    finally:
        if graph_exec is not None:
            hip.call("hipGraphExecDestroy", graph_exec)
        eng.lib.aws_huffman_amd_decode_plan_destroy(plan)
        for p in (d_in, d_out, d_off, d_offs, d_lens):
            eng.free(p)


# ----------------------------------------------------------------------------- the emulator's scenarios, on the chip
@pytest.fixture(scope="module")
def scene(oracle, lib):
    s = pa.Scene(oracle, ba.bind(lib))
    yield s
    s.close()


def test_mixed_batch(scene):
    pd.mixed_batch(scene)


def test_streams_that_stop_early(scene):
    pd.streams_that_stop_early(scene)


@pytest.mark.parametrize("align", [1, 16])
@pytest.mark.parametrize("road", [None, "long-way"])
def test_capacity_clipping(scene, road, align):
    pd.capacity_clipping(scene, road, aligns=(align,))


@pytest.mark.parametrize("name", pd.OTHER_CODERS)
def test_other_coders(scene, name):
    pd.other_coders(scene, name)


@pytest.mark.parametrize("kind", pd.DECODE_PLAN_KINDS)
def test_every_way_a_plan_is_made(scene, kind):
    pd.every_way_a_plan_is_made(scene, kind)


@pytest.mark.parametrize("road", pd.DECODE_ROADS)
def test_decode_road_switches(scene, road):
    pd.decode_road_switches(scene, road)


@pytest.mark.parametrize("tile,count", [(tile, n) for tile, counts in pa.SCAN_TILES for n in counts])
def test_scan_boundaries(scene, tile, count):
    pd.scan_boundaries(scene, tile, (count,))


def test_the_plans_own_layout_survives(scene):
    pd.the_plans_own_layout_survives(scene)
