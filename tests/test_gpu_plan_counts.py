"""Symbol counts of an encode plan's items (huffman_amd_plan_counts.h) on an MI355X (`pytest -m gpu`): the scenarios of
tests/plan_counts_api.py that tests/test_emulated_plan_counts.py runs on the emulator, here at the same sizes, and (clear,
plan count, fit, packed launch) captured in one graph and replayed over changed input bytes."""
import ctypes as C

import numpy as np
import pytest

import fit_api as fa
import harness
import packed_api as pa
import plan_counts_api as pk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc(oracle):
    lib = pk.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    scene = pa.Scene(oracle, lib)
    yield scene
    pk.restore_switches(lib)
    scene.close()


@pytest.fixture(scope="module")
def hip():
    return fa.Hip()


@pytest.fixture(scope="module")
def clear(hip):
    return lambda eng, dptr, size, stream: hip.memset_async(dptr, 0, size, stream)


def test_edges(sc):
    pk.run_edges(sc)


def test_overlap_and_repeats(sc):
    pk.run_overlap_and_repeats(sc)


@pytest.mark.parametrize("kind", pa.ENCODE_PLAN_KINDS)
def test_plan_kinds(sc, kind):
    pk.run_plan_kind(sc, kind)


@pytest.mark.parametrize("name", pk.ENGINES)
def test_engines(sc, name):
    pk.run_engine(sc, name)


def test_add_semantics(sc):
    pk.run_add_semantics(sc)


def test_same_as_the_range_count(sc):
    pk.run_same_as_the_range_count(sc)


def test_flush(sc):
    pk.run_flush(sc)


def test_lifecycle(sc):
    pk.run_lifecycle(sc)


def test_count_changes_nothing(sc):
    pk.run_count_changes_nothing(sc)


@pytest.mark.parametrize("kind", pk.CHAIN_KINDS)
def test_chain(sc, clear, kind):
    pk.run_chain(sc.lib, sc.oracle, clear, kind)


@pytest.mark.parametrize("kind", pk.CHAIN_KINDS)
def test_captured_graph(sc, hip, clear, kind):
    """The chain as ONE graph, captured after one uncaptured packed launch (which makes the plan's scratch; the count itself
    needs none), replayed over two fillings of one input buffer: other text in the items, the gaps still 0x00."""
    lib = sc.lib
    fillings = [pk.chain_data(1399), pk.chain_data(1409)]
    fillings[1][0][fillings[1][0] == ord("e")] = ord("#")  # (other counts, so another code)
    spans = fillings[0][1]
    n, n_bytes = len(spans), fillings[0][0].size
    capacity = 2 * n_bytes
    eng = fa.FittedEngine(lib, 4, 12)
    d_in, d_out, d_off = eng.alloc(n_bytes), eng.alloc(capacity), eng.alloc(8 * (n + 1))
    plan, d_items = pk.chain_plan(eng, kind, spans)
    stream = C.c_void_p(eng.stream)
    graph_exec = None
    try:
        eng.upload(d_in, fillings[0][0])
        chain = lambda: pk.enqueue_chain(eng, clear, plan, d_in, d_out, capacity, d_off, stream)
        chain()
        hip.call("hipStreamSynchronize", stream)
        graph_exec = hip.capture(stream, chain)
        seen = []
        for host, _ in fillings:
            eng.upload(d_in, host)
            eng.fill(d_out, pa.MARKER, capacity)
            eng.fill(d_off, 0xEE, 8 * (n + 1))
            eng.fill(eng.d_bits, 0, 256)
            eng.fill(eng.d_status, 0xEE, 4)
            eng.sync()
            hip.call("hipGraphLaunch", graph_exec, stream)
            hip.call("hipStreamSynchronize", stream)
            seen.append(pk.check_chain(lib, sc.oracle, eng, plan, host, spans, d_out, d_off, capacity))
        assert seen[0] != seen[1]
    finally:
        if graph_exec:
            hip.call("hipGraphExecDestroy", graph_exec)
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        if d_items:
            eng.free(d_items)
        for d in (d_in, d_out, d_off):
            eng.free(d)
        eng.close()


def test_refusals(sc):
    pk.run_refusals(sc)


def test_exports():
    pk.run_exports(harness.PRODUCT_SO)
