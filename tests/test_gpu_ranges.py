"""The locate walk and the symbol-range plans (huffman_amd_ranges.h, decode_locate_body.inc) on an MI355X (`pytest -m gpu`):
the scenarios of tests/ranges_api.py that tests/test_emulated_ranges.py runs on the emulator, here at the same sizes, and a
locate captured in a graph and replayed over two streams."""
import ctypes as C

import numpy as np
import pytest

import fit_api as fa
import harness
import index_api as ia
import packed_api as pa
import packed_decode_api as pda
import ranges_api as ra

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc(oracle):
    lib = ra.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    scene = pa.Scene(oracle, lib)
    yield scene
    lib.aws_huffman_amd_testing_set_locate_lone_symbols(0)
    scene.close()


@pytest.fixture(scope="module")
def hip():
    return fa.Hip()


@pytest.fixture(scope="module")
def clear(hip):
    return lambda eng, dptr, size, stream: hip.memset_async(dptr, 0, size, stream)


@pytest.fixture(scope="module")
def road_results():
    return {}


@pytest.mark.parametrize("kind", ia.DATA_KINDS)
def test_locate_edges(sc, kind):
    ra.run_locate_edges(sc, kind)


@pytest.mark.parametrize("limit", ra.ROADS_LIMITS)
@pytest.mark.parametrize("block_symbols", ra.ROADS_BLOCKS)
def test_both_roads_and_their_boundary(sc, road_results, block_symbols, limit):
    ra.run_roads(sc, block_symbols, limit, road_results)


@pytest.mark.parametrize("name", ["hpack_lengths", "len4to15", "len8"])
def test_other_coders(sc, name):
    ra.run_other_coder(sc, name)


def test_never_in_step(sc):
    ra.run_never_in_step(sc)


def test_a_walk_that_stops(sc):
    ra.run_walk_that_stops(sc)


@pytest.mark.parametrize("enc_offset", ia.RANGES_ENC_OFFSETS)
def test_range_plans(sc, enc_offset):
    ra.run_range_plans(sc, enc_offset)


def test_a_stream_cut_into_odd_pieces(sc):
    ra.run_odd_pieces(sc)


def test_fitted_engines(sc, clear):
    ra.run_fitted(sc, clear)


def test_captured_graph(sc, hip):
    """locate_symbols as a graph (captured after a first call outside the capture), replayed over two streams and their
    indexes held in the same buffers: each replay is numpy's, on both roads (the limit is 100 at the capture), and the two
    differ."""
    n, B, eng = 200_003, 512, sc.eng
    datas = [ia.data_of(sc, "uniform", n, seed=951), ia.data_of(sc, "printable", n, seed=953)]
    pos = np.random.default_rng(955).integers(0, n + 1, 3000).astype(np.uint64)
    room = 2 * n + 64  # (codes of at most 10 bits)
    d_enc, d_index = eng.alloc(room), eng.alloc(8 * (ia.n_blocks_of(n, B) + 1))
    d_pos, d_bits, d_status = pda.upload_u64(eng, pos), eng.alloc(8 * pos.size), eng.alloc(4)
    stream = C.c_void_p(eng.stream)
    graph_exec = None

    def load(data):
        enc = sc.oracle.encode_all(sc.w.ocoder, data, eos_padding=0xFF)
        assert enc.size <= room
        eng.upload(d_enc, enc)
        eng.upload(d_index, np.ascontiguousarray(ia.expected_index(sc.lens, data, B).astype(np.uint64)).view(np.uint8))
        return enc.size

    try:
        sizes = [load(d) for d in datas]
        enc_length = max(sizes)  # (one call for both: the bytes behind the shorter stream are the buffer's, never looked at)
        load(datas[0])
        with ra.lone_symbols(sc.lib, 100):
            call = lambda: ra.locate_call(eng, d_enc, enc_length, d_index, n, B, d_pos, pos.size, d_bits, d_status, stream)
            assert call() == (0, 0)
            hip.call("hipStreamSynchronize", stream)
            graph_exec = hip.capture(stream, lambda: call() == (0, 0) or pytest.fail("refused inside the capture"))
        seen = []
        for data in datas:
            load(data)
            eng.fill(d_bits, 0xEE, 8 * pos.size)
            eng.fill(d_status, 0xEE, 4)
            eng.sync()
            hip.call("hipGraphLaunch", graph_exec, stream)
            hip.call("hipStreamSynchronize", stream)
            got = pa.download_u64(eng, d_bits, pos.size).astype(np.uint64)
            assert np.array_equal(got, ra.symbol_bits(sc.lens, data)[pos.astype(np.int64)])
            assert int(eng.download(d_status, 4).view(np.uint32)[0]) == ra.LOCATE_OK
            seen.append(got)
        assert not np.array_equal(seen[0], seen[1])
    finally:
        if graph_exec:
            hip.call("hipGraphExecDestroy", graph_exec)
        for d in (d_enc, d_index, d_pos, d_bits, d_status):
            eng.free(d)


def test_refusals(sc):
    ra.run_refusals(sc)


def test_exports():
    ra.run_exports(harness.PRODUCT_SO)
