"""The block index over the items of an encode plan (huffman_amd_batch_index.h) on an MI355X (`pytest -m gpu`): the
scenarios of tests/batch_index_api.py that tests/test_emulated_batch_index.py runs on the emulator, here at the same sizes,
and (batch index, packed encode) captured in one graph and replayed over changed input bytes."""
import ctypes as C

import numpy as np
import pytest

import batch_index_api as bi
import fit_api as fa
import harness
import packed_api as pa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc(oracle):
    lib = bi.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    scene = pa.Scene(oracle, lib)
    yield scene
    lib.aws_huffman_amd_testing_set_index_tile_blocks(0)
    lib.aws_huffman_amd_testing_set_batch_index_wave_bytes(0)
    scene.close()


@pytest.fixture(scope="module")
def hip():
    return fa.Hip()


@pytest.fixture(scope="module")
def clear(hip):
    return lambda eng, dptr, size, stream: hip.memset_async(dptr, 0, size, stream)


def test_edges(sc):
    bi.run_edges(sc)


@pytest.mark.parametrize("kind", bi.DATA_KINDS)
@pytest.mark.parametrize("block_symbols", bi.BLOCK_SIZES)
def test_block_sizes_and_data(sc, block_symbols, kind):
    bi.run_block_sizes(sc, block_symbols, kind)


@pytest.mark.parametrize("tile", bi.INDEX_TILES)
def test_index_scan_tiles(sc, tile):
    bi.run_index_tiles(sc, tile)


@pytest.mark.parametrize("tile", bi.PACK_TILES)
def test_directory_scan_tiles(sc, tile):
    bi.run_pack_tiles(sc, tile)


def test_fill_kinds(sc):
    bi.run_fill_kinds(sc)


def test_plan_of_thread_items(sc):
    bi.run_thread_plan(sc)


def test_one_item_is_the_single_stream_index(sc):
    bi.run_one_item(sc)


def test_against_the_packed_launch(sc):
    bi.run_against_packed_launch(sc)


@pytest.mark.parametrize("name", bi.OTHER_CODERS)
def test_other_coders(sc, name):
    bi.run_other_coders(sc, name)


def test_fitted_engine(sc, clear):
    bi.run_fitted_engine(sc.lib, sc.oracle, clear)


def test_capacity(sc):
    bi.run_capacity(sc)


def test_refusals(sc):
    bi.run_refusals(sc)


def test_many_workgroups(sc):
    """More tiles and more short items than one resident grid has workgroups and waves: 3 000 items of 0 .. 40 KB (24 MB)
    among 30 000 of 0 .. 99 bytes, in blocks of 64 -- every workgroup searches tile_first[] many times."""
    eng = sc.eng
    rng = np.random.default_rng(991)
    long_ones = rng.integers(0, 40_000, 3_000)
    lengths = rng.integers(0, 100, 33_000)
    lengths[rng.choice(33_000, 3_000, replace=False)] = long_ones
    offsets = np.concatenate([[0], np.cumsum(lengths + 1)])[:-1] + 7
    total = int(offsets[-1] + lengths[-1]) + 64
    host = harness.splitmix64_bytes(993, total)
    d_in = eng.alloc(total)
    eng.upload(d_in, host)
    plan, d_items = pa.plan_from_records(eng, offsets, lengths)
    try:
        blobs = [host[o:o + n] for o, n in zip(offsets.tolist(), lengths.tolist())]
        bi.check_batch(sc, eng, plan, d_in, blobs, sc.lens, sc.w.ocoder, 64, label="many workgroups")
    finally:
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        eng.free(d_items)
        eng.free(d_in)


def test_captured_graph(sc, hip, clear):
    """clear the counts, count, fit, batch index, packed encode as ONE graph (captured after a first run outside the
    capture, which makes the plan's and the engine's scratch), replayed over two kinds of data in one input buffer."""
    lib, B, n_bytes = sc.lib, 512, 60_000
    datas = [fa.shape_bytes("printable", n_bytes, 995), fa.shape_bytes("geometric", n_bytes, 996)]
    spans = bi.fitted_batch(datas[0], np.random.default_rng(997))
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
        chain = lambda: bi.enqueue_fit_index_encode(eng, clear, plan, d_in, n_bytes, B, a, d_out, capacity, d_off, stream)
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


@pytest.mark.parametrize("block_symbols", bi.RANGE_BLOCKS)
@pytest.mark.parametrize("name", bi.RANGE_CODERS)
def test_item_block_ranges(sc, name, block_symbols):
    bi.run_item_block_ranges(sc, name, block_symbols)


@pytest.mark.parametrize("name", bi.RANGE_CODERS)
def test_item_range_damage(sc, name):
    bi.run_item_range_damage(sc, name)


@pytest.mark.parametrize("name", bi.SYMBOL_CODERS)
def test_item_symbols(sc, name):
    bi.run_item_symbols(sc, name)


def test_item_symbol_range_damage(sc):
    bi.run_item_symbol_range_damage(sc)


def test_one_plan_several_fills(sc):
    bi.run_one_plan_several_fills(sc)


def test_exports():
    bi.run_exports(harness.PRODUCT_SO)
