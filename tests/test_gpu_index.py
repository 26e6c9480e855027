"""The block index and the range plans (huffman_amd_index.h, index_kernels.hip) on an MI355X (`pytest -m gpu`): the
scenarios of tests/index_api.py that tests/test_emulated_index.py runs on the emulator, here at the same sizes, and clear,
count, fit, index captured in one graph and replayed over two inputs."""
import ctypes as C

import numpy as np
import pytest

import fit_api as fa
import harness
import index_api as ia
import packed_api as pa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc(oracle):
    lib = ia.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    scene = pa.Scene(oracle, lib)
    yield scene
    lib.aws_huffman_amd_testing_set_index_tile_blocks(0)
    scene.close()


@pytest.fixture(scope="module")
def hip():
    return fa.Hip()


@pytest.fixture(scope="module")
def clear(hip):
    return lambda eng, dptr, size, stream: hip.memset_async(dptr, 0, size, stream)


def test_index_edges(sc):
    ia.run_index_edges(sc)


@pytest.mark.parametrize("kind", ia.DATA_KINDS)
@pytest.mark.parametrize("block_symbols", ia.BLOCK_SIZES)
def test_block_sizes_and_data(sc, block_symbols, kind):
    ia.run_block_sizes(sc, block_symbols, kind)


@pytest.mark.parametrize("tile", ia.SCAN_TILES)
def test_scan_tiles(sc, tile):
    ia.run_scan_tiles(sc, tile)


@pytest.mark.parametrize("name", ia.OTHER_CODERS)
def test_other_coders(sc, name):
    ia.run_other_coders(sc, name)


def test_fitted_engine(sc, clear):
    ia.run_fitted_engine(sc.lib, clear)


def test_captured_graph(sc, hip, clear):
    """clear the counts, count, fit, index as ONE graph (captured after a first run outside the capture, which makes the
    engine's scratch), replayed over two kinds of data in one input buffer: every replay indexes under its own fit."""
    n, B = ia.N_SYMBOLS, 512
    nb = ia.n_blocks_of(n, B)
    datas = [fa.shape_bytes("printable", n, 91), fa.shape_bytes("geometric", n, 92)]
    eng = fa.FittedEngine(sc.lib, 4, 12)
    d_in, d_index, d_status = eng.alloc(n), eng.alloc(8 * (nb + 1)), eng.alloc(4)
    stream = C.c_void_p(eng.stream)
    graph_exec = None
    try:
        eng.upload(d_in, datas[0])
        chain = lambda: ia.enqueue_fit_and_index(eng, clear, d_in, n, B, d_index, d_status, stream)
        chain()
        hip.call("hipStreamSynchronize", stream)
        graph_exec = hip.capture(stream, chain)
        seen = []
        for data in datas:
            eng.upload(d_in, data)
            eng.fill(d_index, 0xEE, 8 * (nb + 1))
            eng.fill(d_status, 0xEE, 4)
            eng.fill(eng.d_bits, 0, 256)
            eng.fill(eng.d_status, 0xEE, 4)
            eng.sync()
            hip.call("hipGraphLaunch", graph_exec, stream)
            hip.call("hipStreamSynchronize", stream)
            lengths, want = ia.check_fitted_index(eng, data, B, d_index, d_status)
            seen.append((lengths, int(want[-1])))
        assert seen[0] != seen[1]
    finally:
        if graph_exec:
            hip.call("hipGraphExecDestroy", graph_exec)
        for d in (d_in, d_index, d_status):
            eng.free(d)
        eng.close()


@pytest.mark.parametrize("block_symbols", ia.BLOCK_SIZES)
def test_every_block_as_its_own_range(sc, block_symbols):
    ia.run_every_block(sc, block_symbols)


@pytest.mark.parametrize("enc_offset", ia.RANGES_ENC_OFFSETS)
def test_ranges(sc, enc_offset):
    ia.run_ranges(sc, enc_offset)


def test_printable_text_under_a_fitted_coder(sc, clear):
    ia.run_printable_fitted(sc, clear)


def test_refusals(sc):
    ia.run_refusals(sc)


def test_exports():
    ia.run_exports(harness.PRODUCT_SO)
