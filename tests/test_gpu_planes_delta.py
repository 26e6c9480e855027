"""Byte planes of differences in runs (huffman_amd_planes_delta.h) on an MI355X (`pytest -m gpu`): the scenarios of
tests/planes_delta_api.py that tests/test_emulated_planes_delta.py runs on the emulator, here at the same sizes, and (clear,
counted split of differences, fit of the low plane, packed stored launch of that plane) captured in one graph and replayed
over changed elements."""
import ctypes as C

import numpy as np
import pytest

import fit_api as fa
import harness
import packed_api as pa
import planes_api as pl
import planes_delta_api as pd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc(oracle):
    lib = pd.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    scene = pa.Scene(oracle, lib)
    yield scene
    pd.restore_switches(lib)
    scene.close()


@pytest.fixture(scope="module")
def hip():
    return fa.Hip()


@pytest.fixture(scope="module")
def clear(hip):
    return lambda eng, dptr, size, stream: hip.memset_async(dptr, 0, size, stream)


@pytest.mark.parametrize("run_elements", pd.RUNS)
@pytest.mark.parametrize("element_bytes", pd.SIZES)
def test_edges(sc, element_bytes, run_elements):
    pd.run_edges(sc, element_bytes, run_elements)


@pytest.mark.parametrize("regime", list(pd.REGIMES))
def test_scan_regime(sc, regime):
    pd.run_regime(sc, regime)


@pytest.mark.parametrize("cap", pd.GRID_CAPS)
def test_grid(sc, cap):
    pd.run_grid(sc, cap)


def test_add_semantics(sc):
    pd.run_add_semantics(sc)


@pytest.mark.parametrize("kind", pd.CODER_KINDS)
def test_with_coder(sc, clear, kind):
    pd.run_with_coder(sc, kind, clear)


def test_captured_graph(sc, hip, clear):
    """Clear, counted split of differences, fit of the low plane and the packed stored launch of that plane as ONE graph,
    captured after one uncaptured run (which makes the plan's scratch; the split needs none), replayed over two fillings of
    one input buffer: u64 offsets of items of 16 to 80 bytes and of 16 to 200, whose low plane of differences is another.
    Each against numpy and the oracle."""
    lib, eng = sc.lib, sc.eng
    n, r = pd.CODER_ELEMENTS, pd.CODER_RUN
    fillings = [pd.coder_data("u64 offsets", seed=1643)[1], pd.coder_data("u64 offsets", seed=1657, longest=200)[1]]
    e, low = 8, 0
    stride = (n + pl.ITEM - 1) // pl.ITEM * pl.ITEM
    d_in, d_planes, d_counts = eng.alloc(n * e), eng.alloc(e * stride), eng.alloc(256 * 8 * e)
    stream = C.c_void_p(eng.stream)
    sender = pl.PlaneSender(lib, d_planes + low * stride, stride)
    graph_exec = None

    def chain():
        clear(eng, d_counts, 256 * 8 * e, stream)
        assert pd.split_delta(eng, d_in, n, e, r, d_planes, stride, d_counts, stream) == (0, 0)
        sender.enqueue(d_counts + 256 * 8 * low, stream)

    try:
        eng.upload(d_in, fillings[0])
        eng.fill(d_planes, pl.PlaneSender.FILL, e * stride)
        sender.prepare()
        chain()
        hip.call("hipStreamSynchronize", stream)
        graph_exec = hip.capture(stream, chain)
        seen = []
        for a in fillings:
            eng.upload(d_in, a)
            eng.fill(d_planes, pl.PlaneSender.FILL, e * stride)
            eng.fill(d_counts, 0xEE, 256 * 8 * e)
            sender.prepare()
            eng.sync()
            hip.call("hipGraphLaunch", graph_exec, stream)
            hip.call("hipStreamSynchronize", stream)
            d = pd.differences(a, e, r)
            assert np.array_equal(eng.download(d_counts, 256 * 8 * e).view(np.uint64), pl.plane_counts(d, n, e))
            want = np.full(e * stride, pl.PlaneSender.FILL, np.uint8)
            for p in range(e):
                want[p * stride:p * stride + n] = d.reshape(n, e)[:, p]
            assert np.array_equal(eng.download(d_planes, e * stride), want)
            sent = sender.check(sc.oracle, want[low * stride:(low + 1) * stride], n, "replayed")
            assert sent.total < stride, (sent.total, stride)
            seen.append((sender.lengths, eng.download(sender.bufs.d_out, sent.total).tobytes()))
        assert seen[0][0] != seen[1][0] and seen[0][1] != seen[1][1]
    finally:
        if graph_exec:
            hip.call("hipGraphExecDestroy", graph_exec)
        sender.close()
        for d in (d_in, d_planes, d_counts):
            eng.free(d)


def test_refusals(sc):
    pd.run_refusals(sc)


def test_exports():
    pd.run_exports(harness.PRODUCT_SO)
