"""Packed batch encode on an MI355X (`pytest -m gpu`): the BASELINE batch of 65 536 x 16 KiB, a million header-sized
items and one 1 GiB item at full size -- offsets against a numpy table sum of the code lengths, a sample of items byte
for byte against the oracle, everything round-tripped through the chained decode --, odd lengths at align 1 on both
encode roads, and a packed launch captured in a graph and replayed on new input.  Then the edge scenarios of
tests/packed_api.py that tests/test_emulated_packed.py runs on the emulator, here at the same sizes."""
import hashlib

import numpy as np
import pytest

import harness
import packed_api as pa
import parity_cases as pc

pytestmark = pytest.mark.gpu

PROBE = harness.load_json("survey_probe_records.json")
GiB = 1 << 30


@pytest.fixture(scope="module")
def lib():
    lib = pa.bind(harness.load_product())
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


def big_batch(world, eng, data, in_offs, in_lens, align, sample):
    """A packed launch of the items data[in_offs[i] : + in_lens[i]] (already in device memory at d_in = the first
    return value's owner): offsets and total against numpy, the sample against the oracle, then all of it decoded back
    through aws_huffman_amd_decode_plan_from_encode and compared with the input."""
    n = len(in_lens)
    code_lens = pa.code_lengths(world.table[1]).astype(np.uint8)
    d_in = eng.alloc(data.size)
    eng.upload(d_in, data)
    bits = np.add.reduceat(code_lens[data], in_offs, dtype=np.int64)  # (the items lie back to back)
    lens = (bits + 7) // 8
    offsets, reserved = pa.expected_offsets(lens, align)
    total = int(offsets[-1])
    plan, d_items = pa.plan_from_records(eng, in_offs, in_lens)
    d_out, d_off, d_back = eng.alloc(total + 64), eng.alloc(8 * (n + 1)), eng.alloc(data.size)
    dplan = eng.empty_decode_plan()
    try:
        eng.fill(d_out, pa.MARKER, total + 64)
        assert pa.launch_packed(eng, plan, d_in, d_out, total, d_off, align) == (0, 0)
        res = pa.results_array(eng, plan, n)
        got_offsets = pa.download_u64(eng, d_off, n + 1)
        assert np.array_equal(got_offsets, offsets), int(np.flatnonzero(got_offsets != offsets)[0])
        assert pa.packed_size(eng, plan) == (0, 0, total, int(reserved.max()))
        assert total == int(reserved.sum())
        assert np.all(res["rc"] == 0) and np.array_equal(res["produced"].astype(np.int64), lens)
        assert np.array_equal(res["consumed"].astype(np.int64), np.asarray(in_lens, np.int64)) and np.all(res["num_bits"] == 0)
        for i in sample:
            blob = data[in_offs[i]:in_offs[i] + in_lens[i]]
            rec, want = pa.oracle_item(world.oracle, world.ocoder, blob, (0, 0), 0xFF, int(reserved[i]))
            assert rec[:4] == (0, 0, blob.size, int(lens[i])), (i, rec)
            got = eng.download(d_out, int(reserved[i]), offset=int(offsets[i]))
            assert np.array_equal(got, want), i
        assert np.all(eng.download(d_out, 64, offset=total) == pa.MARKER)
        # the chained decode: reads at the offsets, the lengths never come to the host
        assert eng.decode_plan_from_encode(dplan, plan)
        eng.fill(d_back, pa.MARKER, data.size)
        eng.decode_launch(dplan, d_out, d_back)
        assert all(r[0] == 0 and r[2] == m for r, m in zip(eng.decode_results(dplan, n), in_lens))
        step = 256 << 20
        for off in range(0, data.size, step):
            assert np.array_equal(eng.download(d_back, min(step, data.size - off), offset=off), data[off:off + step]), off
    finally:
        eng.lib.aws_huffman_amd_decode_plan_destroy(dplan)
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        for p in (d_in, d_items, d_out, d_off, d_back):
            eng.free(p)


def test_batch_of_65536_buffers_of_16k(world, eng):
    count, size = 65536, 16384
    data = harness.splitmix64_bytes(5, count * size)
    in_offs = np.arange(count, dtype=np.int64) * size
    rng = np.random.default_rng(5)
    sample = [0, 1, count - 1] + [int(x) for x in rng.integers(0, count, 36)]
    big_batch(world, eng, data, in_offs, np.full(count, size, np.int64), 1, sample)


def test_a_million_header_sized_items(world, eng):
    count = 1_000_000
    rng = np.random.default_rng(7)
    in_lens = rng.integers(16, 81, count).astype(np.int64)
    in_offs = np.concatenate([[0], np.cumsum(in_lens)[:-1]]).astype(np.int64)
    data = harness.printable_map(harness.splitmix64_bytes(9, int(in_lens.sum())))
    sample = [0, 1, count - 1] + [int(x) for x in rng.integers(0, count, 60)]
    for align in (1, 8):
        big_batch(world, eng, data, in_offs, in_lens, align, sample)


def test_one_item_of_1gib(world, eng):
    """The 1 GiB stream of BASELINE configs[1]: offsets [0, len], and the output's digest equal to the pinned record the
    plain launch is checked against (tests/test_gpu_parity.py)."""
    rec = PROBE["streams"]["G1G"]
    n, e = rec["len"], rec["encoded_len"]
    d_in, d_out, d_off = eng.alloc(n), eng.alloc(e + 64), eng.alloc(16)
    plan, d_items = pa.plan_from_records(eng, [0], [n])
    try:
        eng.fill_splitmix64(d_in, n, rec["seed"])
        eng.fill(d_out, pa.MARKER, e + 64)
        assert pa.launch_packed(eng, plan, d_in, d_out, e, d_off, 1) == (0, 0)
        (rc, err, consumed, produced, ob, _), = eng.encode_results(plan, 1)
        assert (rc, err, consumed, produced, ob) == (0, 0, n, e, 0)
        assert eng.encode_road(plan) == pc.ROAD_ONE_PASS
        assert list(pa.download_u64(eng, d_off, 2)) == [0, e]
        assert pa.packed_size(eng, plan) == (0, 0, e, e)
        h = hashlib.sha256()
        step = 256 << 20
        for off in range(0, e, step):
            h.update(eng.download(d_out, min(step, e - off), offset=off).tobytes())
        assert h.hexdigest() == rec["sha256_encoded"]
        assert np.all(eng.download(d_out, 64, offset=e) == pa.MARKER)
    finally:
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        for p in (d_in, d_out, d_off, d_items):
            eng.free(p)


@pytest.mark.parametrize("road,want_road", [(None, pc.ROAD_ONE_PASS), ("three-kernel", pc.ROAD_TWO_PASS)])
def test_align_1_over_many_odd_lengths(world, road, want_road):
    """Neighbouring items share dwords and cache lines: 3000 items of odd lengths from 1 to 40 000 symbols back to back,
    every byte of the output against the oracle."""
    rng = np.random.default_rng(11)
    lib = world.product.lib
    with harness.encode_road(lib, road):
        coder = lib.aws_huffman_amd_table_coder_new(*world.table)
        eng = harness.Engine(lib, coder)
    sizes = [1, 3, 5, 511, 513, 4095, 4097, 16383, 16385] + [int(x) | 1 for x in rng.integers(1, 40000, 2991)]
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    host_in, in_offs = pa.lay_out(blobs, rng, first=1)
    d_in = eng.alloc(host_in.size)
    eng.upload(d_in, host_in)
    n = len(blobs)
    overflows = [((int(rng.integers(0, 1 << 7)), 7) if i % 5 == 2 else (0, 0)) for i in range(n)]
    eoss = [[0xFF, 0x00][i % 2] for i in range(n)]
    items = [dict(in_offset=in_offs[i], in_len=sizes[i], out_offset=0, out_capacity=0, overflow_in=overflows[i],
                  eos_padding=eoss[i]) for i in range(n)]
    plan = eng.encode_plan(items)
    try:
        pa.check_launch(world.oracle, world.ocoder, eng, plan, d_in, blobs, pa.code_lengths(world.table[1]), overflows, eoss, 1,
                        want_road=want_road, label="odd lengths")
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        eng.free(d_in)
        eng.close()
        lib.aws_huffman_amd_table_coder_destroy(coder)


def test_captured_graph(world, eng):
    """A packed launch captured on the engine's stream (after a first one outside the capture, which allocates the plan's
    second record array) and replayed on new input of other lengths: offsets, records and bytes of the replay against the
    oracle."""
    import ctypes as C

    hip = pa.HipGraphs()
    rng = np.random.default_rng(13)
    sizes = [200, 5000, 16384, 70000, 33, 16385, 900, 40000] * 8
    n = len(sizes)
    code_lens = pa.code_lengths(world.table[1])
    first = [pc.inputs(rng, s, "printable") for s in sizes]
    second = [pc.inputs(rng, s, pc.KINDS[i % 4]) for i, s in enumerate(sizes)]
    host_in, in_offs = pa.lay_out(first, None)
    items = [dict(in_offset=in_offs[i], in_len=sizes[i], out_offset=0, out_capacity=0) for i in range(n)]
    room = sum(sizes) * 2
    d_in, d_out, d_off = eng.alloc(host_in.size), eng.alloc(room + 64), eng.alloc(8 * (n + 1))
    plan = eng.encode_plan(items)
    stream = C.c_void_p(eng.stream)
    graph_exec = None
    try:
        eng.upload(d_in, host_in)
        assert pa.launch_packed(eng, plan, d_in, d_out, room, d_off, 4, stream) == (0, 0)
        hip.call("hipStreamSynchronize", stream)
        graph_exec = hip.capture(stream, lambda: pa.launch_packed(eng, plan, d_in, d_out, room, d_off, 4, stream))
        for blobs in (second, first):
            host, _ = pa.lay_out(blobs, None)
            eng.upload(d_in, host)
            eng.fill(d_out, pa.MARKER, room + 64)
            eng.fill(d_off, 0xEE, 8 * (n + 1))
            eng.sync()
            hip.call("hipGraphLaunch", graph_exec, stream)
            hip.call("hipStreamSynchronize", stream)
            lens = pa.encoded_lengths(code_lens, blobs, [0] * n)
            offsets, reserved = pa.expected_offsets(lens, 4)
            assert np.array_equal(pa.download_u64(eng, d_off, n + 1), offsets)
            got = eng.download(d_out, room + 64)
            res = eng.encode_results(plan, n)
            want = np.full(room + 64, pa.MARKER, np.uint8)
            for i, blob in enumerate(blobs):
                rec, data = pa.oracle_item(world.oracle, world.ocoder, blob, (0, 0), 0xFF, int(reserved[i]))
                assert res[i] == rec, (i, res[i], rec)
                want[int(offsets[i]):int(offsets[i]) + int(reserved[i])] = data
            assert np.array_equal(got, want)
            assert pa.packed_size(eng, plan, stream)[2] == int(offsets[-1])
    finally:
        if graph_exec is not None:
            hip.call("hipGraphExecDestroy", graph_exec)
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        for p in (d_in, d_out, d_off):
            eng.free(p)


# ----------------------------------------------------------------------------- the emulator's scenarios, on the chip
@pytest.fixture(scope="module")
def scene(oracle, lib):
    s = pa.Scene(oracle, lib)
    yield s
    s.close()


def test_offsets_and_bytes(scene):
    pa.offsets_and_bytes(scene)


@pytest.mark.parametrize("road,want_road", pa.ENCODE_ROADS)
@pytest.mark.parametrize("kind", pa.ENCODE_PLAN_KINDS)
def test_every_plan_and_road(scene, kind, road, want_road):
    pa.every_plan_and_road(scene, kind, road, want_road)


@pytest.mark.parametrize("tile,count", [(tile, n) for tile, counts in pa.SCAN_TILES for n in counts])
def test_scan_boundaries(scene, tile, count):
    pa.scan_boundaries(scene, tile, (count,))


@pytest.mark.parametrize("align", [1, 16])
@pytest.mark.parametrize("road", [None, "three-kernel"])
def test_capacity_clipping(scene, road, align):
    pa.capacity_clipping(scene, road, aligns=(align,))


def test_coder_with_holes(scene):
    pa.coder_with_holes(scene)


def test_the_plans_own_layout_survives(scene):
    pa.the_plans_own_layout_survives(scene)


@pytest.mark.parametrize("shape", ["threads", "chunks"])
def test_round_trip_through_a_chained_decode(scene, shape):
    pa.round_trip_through_a_chained_decode(scene, shape)
