"""Byte planes of multi-byte elements (huffman_amd_planes.h) on an MI355X (`pytest -m gpu`): the scenarios of
tests/planes_api.py that tests/test_emulated_planes.py runs on the emulator, here at the same sizes, and (clear, counted
split, fit of the top plane, packed stored launch of that plane) captured in one graph and replayed over changed elements."""
import ctypes as C

import numpy as np
import pytest

import fit_api as fa
import harness
import packed_api as pa
import planes_api as pl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc(oracle):
    lib = pl.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    scene = pa.Scene(oracle, lib)
    yield scene
    pl.restore_switches(lib)
    scene.close()


@pytest.fixture(scope="module")
def hip():
    return fa.Hip()


@pytest.fixture(scope="module")
def clear(hip):
    return lambda eng, dptr, size, stream: hip.memset_async(dptr, 0, size, stream)


@pytest.mark.parametrize("element_bytes", pl.SIZES)
def test_edges(sc, element_bytes):
    pl.run_edges(sc, element_bytes)


def test_grid(sc):
    pl.run_grid(sc)


def test_flush(sc):
    pl.run_flush(sc)


def test_add_semantics(sc):
    pl.run_add_semantics(sc)


@pytest.mark.parametrize("kind", pl.ROUND_TRIP_KINDS)
def test_round_trip(sc, clear, kind):
    pl.run_round_trip(sc, kind, clear)


def test_captured_graph(sc, hip, clear):
    """Clear, counted split, fit of the top plane and the packed stored launch of that plane as ONE graph, captured after one
    uncaptured run (which makes the plan's scratch; the split needs none), replayed over two fillings of one input buffer:
    bf16 of N(0, 1) and of N(0, 1) scaled by 1 000, whose exponents are others.  Each against numpy and the oracle."""
    lib, eng = sc.lib, sc.eng
    n = pl.ROUND_TRIP_ELEMENTS
    fillings = [pl.round_trip_data("bf16", seed=1549)[1], pl.round_trip_data("bf16", seed=1553, scale=1000.0)[1]]
    e, top = 2, 1
    stride = (n + pl.ITEM - 1) // pl.ITEM * pl.ITEM
    d_in, d_planes, d_counts = eng.alloc(n * e), eng.alloc(e * stride), eng.alloc(256 * 8 * e)
    stream = C.c_void_p(eng.stream)
    sender = pl.PlaneSender(lib, d_planes + top * stride, stride)
    graph_exec = None

    def chain():
        clear(eng, d_counts, 256 * 8 * e, stream)
        assert pl.split(eng, d_in, n, e, d_planes, stride, d_counts, stream) == (0, 0)
        sender.enqueue(d_counts + 256 * 8 * top, stream)

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
            assert np.array_equal(eng.download(d_counts, 256 * 8 * e).view(np.uint64), pl.plane_counts(a, n, e))
            plane = np.full(stride, pl.PlaneSender.FILL, np.uint8)
            plane[:n] = a.reshape(n, e)[:, top]
            assert np.array_equal(eng.download(d_planes + top * stride, stride), plane)
            sent = sender.check(sc.oracle, plane, n, "replayed")
            assert sent.total <= pl.BF16_TOP_PLANE_CAP * stride, (sent.total, stride)
            seen.append((sender.lengths, eng.download(sender.bufs.d_out, sent.total).tobytes()))
        assert seen[0][0] != seen[1][0] and seen[0][1] != seen[1][1]
    finally:
        if graph_exec:
            hip.call("hipGraphExecDestroy", graph_exec)
        sender.close()
        for d in (d_in, d_planes, d_counts):
            eng.free(d)


def test_refusals(sc):
    pl.run_refusals(sc)


def test_exports():
    pl.run_exports(harness.PRODUCT_SO)
