"""The packed encode launch that makes the batch's block index (huffman_amd_packed_index.h) on an MI355X (`pytest -m gpu`):
the scenarios of tests/packed_index_api.py that tests/test_emulated_packed_index.py runs on the emulator, here at the same
sizes, and (clear, count, fit, the new call) captured in one
graph and replayed over changed input bytes."""
import ctypes as C

import numpy as np
import pytest

import batch_index_api as bi
import fit_api as fa
import harness
import packed_api as pa
import packed_index_api as pi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc(oracle):
    lib = pi.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    scene = pa.Scene(oracle, lib)
    yield scene
    pi.restore_switches(lib)
    scene.close()


@pytest.fixture(scope="module")
def hip():
    return fa.Hip()


@pytest.fixture(scope="module")
def clear(hip):
    return lambda eng, dptr, size, stream: hip.memset_async(dptr, 0, size, stream)


@pytest.mark.parametrize("align", [1, 16])
@pytest.mark.parametrize("block_symbols", [64, 4096])
def test_edges(sc, block_symbols, align):
    pi.run_edges(sc, block_symbols, align)


def test_carried_bits(sc):
    pi.run_carried_bits(sc)


@pytest.mark.parametrize("align", [1, 16])
def test_output_capacity(sc, align):
    pi.run_capacity(sc, align)


def test_index_too_small(sc):
    pi.run_index_too_small(sc)


@pytest.mark.parametrize("tile", pi.PACK_TILES)
def test_offset_scan_tiles(sc, tile):
    pi.run_pack_tiles(sc, tile)


@pytest.mark.parametrize("tile", pi.INDEX_TILES)
def test_index_scan_tiles(sc, tile):
    pi.run_index_tiles(sc, tile)


def test_built_in_tile_boundary(sc):
    pi.run_built_in_tile(sc)


@pytest.mark.parametrize("road,want_road", pa.ENCODE_ROADS)
@pytest.mark.parametrize("kind", pa.ENCODE_PLAN_KINDS)
def test_plan_kinds_and_roads(sc, kind, road, want_road):
    pi.run_plan_kinds_and_roads(sc, kind, road, want_road)


@pytest.mark.parametrize("name", pi.OTHER_CODERS)
def test_other_coders(sc, name):
    pi.run_other_coders(sc, name)


def test_same_as_the_two_calls(sc):
    pi.run_same_as_the_two_calls(sc)


def test_receiver(sc):
    pi.run_receiver(sc)


def test_fitted_engine(sc, clear):
    pi.run_fitted_engine(sc.lib, sc.oracle, clear)


def test_captured_graph(sc, hip, clear):
    """clear the counts, count, fit and the indexed packed launch as ONE graph (captured after a first run outside the
    capture, which makes the plan's and the engine's scratch), replayed over two kinds of data in one input buffer."""
    lib, B, n_bytes = sc.lib, 512, 60_000
    datas = [fa.shape_bytes("printable", n_bytes, 1311), fa.shape_bytes("geometric", n_bytes, 1313)]
    spans = bi.fitted_batch(datas[0], np.random.default_rng(1319))
    items = [dict(in_offset=o, in_len=s, out_offset=0, out_capacity=0) for o, s in spans]
    n, capacity = len(items), 2 * n_bytes
    eng = fa.FittedEngine(lib, 4, 12)
    d_in, d_out, d_off = eng.alloc(n_bytes), eng.alloc(capacity), eng.alloc(8 * (n + 1))
    plan = eng.encode_plan(items)
    a = bi.Arrays(eng, n, sum((s + B - 1) // B for _, s in spans) + 1)
    stream = C.c_void_p(eng.stream)
    graph_exec = None
    try:
        eng.upload(d_in, datas[0])
        chain = lambda: pi.enqueue_fit_indexed_encode(eng, clear, plan, d_in, n_bytes, B, a, d_out, capacity, d_off, stream)
        chain()
        hip.call("hipStreamSynchronize", stream)
        graph_exec = hip.capture(stream, chain)
        seen = []
        for data in datas:
            eng.upload(d_in, data)
            a.refill()
            eng.fill(d_out, pa.MARKER, capacity)
            eng.fill(d_off, 0xEE, 8 * (n + 1))
            eng.fill(eng.d_bits, 0, 256)
            eng.fill(eng.d_status, 0xEE, 4)
            eng.sync()
            hip.call("hipGraphLaunch", graph_exec, stream)
            hip.call("hipStreamSynchronize", stream)
            blobs = [data[o:o + s] for o, s in spans]
            seen.append(bi.check_fitted_chain(lib, sc.oracle, eng, plan, data, blobs, B, a, d_out, d_off, capacity))
        assert seen[0] != seen[1]
    finally:
        if graph_exec:
            hip.call("hipGraphExecDestroy", graph_exec)
        a.close()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        for d in (d_in, d_out, d_off):
            eng.free(d)
        eng.close()


def test_refusals(sc):
    pi.run_refusals(sc)


def test_exports():
    pi.run_exports(harness.PRODUCT_SO)


def test_lifecycle(sc):
    pi.run_lifecycle(sc)
