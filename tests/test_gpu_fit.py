"""The coder fitted on the device (huffman_amd_fit.h, fit_kernels.hip) on an MI355X (`pytest -m gpu`): lengths and tables
against the host's, count -> fit -> packed encode chained on one stream and captured in a graph against the oracle, a
receiver fitted from the 256 lengths, and a refit between two launches of one plan with no host wait.  Then the scenarios
of tests/fit_api.py that tests/test_emulated_fit.py runs on the emulator, here at the same sizes: a fitted engine against
the oracle within every pair of bounds, under the encode roads, receivers of codes with windows without a code, the
refusals of a fit and the never-fitted state."""
import ctypes as C

import numpy as np
import pytest

import build_api as ba
import fit_api as fa
import harness
import packed_api as pa
import packed_decode_api as pda

pytestmark = pytest.mark.gpu

MiB = 1 << 20


@pytest.fixture(scope="module")
def lib():
    lib = fa.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    return lib


def test_lengths_and_tables_on_the_chip(lib):
    engines = [fa.FittedEngine(lib, lo, hi) for lo, hi in fa.BOUNDS]
    try:
        fa.run_lengths_equal_host(lib, engines)
        fa.run_tables_equal_host(lib, engines)
    finally:
        for e in engines:
            e.close()


def batch_of(data, rng, n_items=2000):
    """The whole of `data` as one stream, and n_items items of 16 .. 6 000 bytes from its front: (blobs, item records)."""
    sizes = [int(s) for s in rng.integers(16, 6001, n_items)]
    starts = np.cumsum([0] + sizes)[:-1]
    spans = [(0, data.size)] + [(int(a), s) for a, s in zip(starts, sizes)]
    blobs = [data[a:a + s] for a, s in spans]
    items = [dict(in_offset=a, in_len=s, out_offset=0, out_capacity=0) for a, s in spans]
    return blobs, items


@pytest.mark.parametrize("shape", ["printable", "geometric", "uniform"])
def test_count_fit_encode_decode(lib, oracle, shape):
    hip = fa.Hip()
    n_bytes = 8 * MiB
    data = fa.shape_bytes(shape, n_bytes, 71)
    blobs, items = batch_of(data, np.random.default_rng(72))
    n = len(blobs)
    total_in = sum(b.size for b in blobs)
    capacity = total_in * 12 // 8 + n
    eng, receiver = fa.FittedEngine(lib, 4, 12), fa.FittedEngine(lib, 4, 12)
    d_in, d_out, d_off = eng.alloc(n_bytes), eng.alloc(capacity), eng.alloc(8 * (n + 1))
    d_back, d_back_off = eng.alloc(total_in + 64), eng.alloc(8 * (n + 1))
    plan = eng.encode_plan(items)
    dplan = receiver.empty_decode_plan()
    stream = C.c_void_p(eng.stream)
    try:
        eng.upload(d_in, data)
        eng.fill(eng.d_status, 0xEE, 4)
        fa.enqueue_chain(hip, eng, plan, d_in, n_bytes, d_out, capacity, d_off, stream)
        hip.call("hipStreamSynchronize", stream)
        lengths, offsets = fa.check_chain_output(lib, oracle, eng, plan, data, blobs, d_out, d_off, capacity)
        assert fa.is_flat(lengths) == (shape == "uniform")
        stats = eng.encode_stats(plan)
        assert stats["by_pieces"] >= 1 and stats["by_wave"] + stats["by_thread"] >= 1, stats
        # the receiver: the 256 lengths beside the packed buffer and its offsets
        assert receiver.fit_lengths_async(eng.d_bits) == (0, 0)
        assert receiver.status() == fa.FIT_OK
        assert pda.reset_packed_input(receiver, dplan, d_off, None, n) == (0, 0)
        receiver.fill(d_back, pa.MARKER, total_in + 64)
        assert pda.launch_packed(receiver, dplan, d_out, d_back, total_in, d_back_off, 1) == (0, 0)
        back = receiver.download(d_back, total_in + 64)
        res = pda.results_array(receiver, dplan, n)
        assert np.all(res["rc"] == 0) and np.array_equal(res["produced"].astype(np.int64), [b.size for b in blobs])
        assert np.array_equal(pa.download_u64(receiver, d_back_off, n + 1), np.cumsum([0] + [b.size for b in blobs]))
        assert np.array_equal(back[:total_in], np.concatenate(blobs)) and np.all(back[total_in:] == pa.MARKER)
        if not fa.is_flat(lengths):
            assert receiver.decode_stats(dplan)["by_pieces"] > 0, receiver.decode_stats(dplan)
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        lib.aws_huffman_amd_decode_plan_destroy(dplan)
        for d in (d_in, d_out, d_off, d_back, d_back_off):
            eng.free(d)
        eng.close()
        receiver.close()


def test_captured_graph(lib, oracle):
    """clear the counts, count, fit, packed encode as ONE graph (captured after a first run outside the capture, which makes
    the plan's allocations), replayed over three kinds of data in one input buffer: every replay fits its own data."""
    hip = fa.Hip()
    n_bytes = 2 * MiB + 5
    shapes = ["printable", "geometric", "uniform"]
    datas = [fa.shape_bytes(s, n_bytes, 81 + i) for i, s in enumerate(shapes)]
    spans = [(0, n_bytes)] + [(a, s) for a, s in ((7, 300), (1001, 3000), (5000, 40000), (70001, 17), (90000, 100003))]
    items = [dict(in_offset=a, in_len=s, out_offset=0, out_capacity=0) for a, s in spans]
    n = len(spans)
    capacity = sum(s for _, s in spans) * 12 // 8 + n
    eng = fa.FittedEngine(lib, 4, 12)
    d_in, d_out, d_off = eng.alloc(n_bytes), eng.alloc(capacity), eng.alloc(8 * (n + 1))
    plan = eng.encode_plan(items)
    stream = C.c_void_p(eng.stream)
    graph_exec = None
    try:
        eng.upload(d_in, datas[0])
        fa.enqueue_chain(hip, eng, plan, d_in, n_bytes, d_out, capacity, d_off, stream)
        hip.call("hipStreamSynchronize", stream)
        graph_exec = hip.capture(stream, lambda: fa.enqueue_chain(hip, eng, plan, d_in, n_bytes, d_out, capacity, d_off, stream))
        for data in datas:
            eng.upload(d_in, data)
            eng.fill(d_out, pa.MARKER, capacity)
            eng.fill(d_off, 0xEE, 8 * (n + 1))
            eng.fill(eng.d_bits, 0, 256)
            eng.fill(eng.d_status, 0xEE, 4)
            eng.sync()
            hip.call("hipGraphLaunch", graph_exec, stream)
            hip.call("hipStreamSynchronize", stream)
            blobs = [data[a:a + s] for a, s in spans]
            _, offsets = fa.check_chain_output(lib, oracle, eng, plan, data, blobs, d_out, d_off, capacity)
            assert np.all(eng.download(d_out, capacity)[int(offsets[-1]):] == pa.MARKER)
            assert np.array_equal(eng.download(eng.d_counts, 256 * 8).view(np.uint64), ba.bincount(data))
    finally:
        if graph_exec:
            hip.call("hipGraphExecDestroy", graph_exec)
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        for d in (d_in, d_out, d_off):
            eng.free(d)
        eng.close()


def test_refit_between_launches_of_one_plan(lib, oracle):
    eng = fa.FittedEngine(lib, 4, 12)
    try:
        fa.run_refit_between_launches(lib, oracle, eng, 4 * MiB)
    finally:
        eng.close()


# ----------------------------------------------------------------------------- the emulator's scenarios, on the chip
SWEEP = [(b, s) for b in fa.BOUNDS for s in fa.SHAPES]


@pytest.mark.parametrize("bounds,shape", SWEEP, ids=["%d..%d-%s" % (b + (s,)) for b, s in SWEEP])
def test_fitted_engine_parity(lib, oracle, bounds, shape):
    fa.run_parity(lib, oracle, bounds, shape)


def test_the_sweep_saw_a_spread_of_lengths(lib):
    fa.run_sweep_saw_a_spread(lib, SWEEP)


@pytest.mark.parametrize("shape", ["printable", "one byte"])
@pytest.mark.parametrize("road", ["three-kernel", "one-pass-fails"])
def test_fitted_engine_made_under_an_encode_road(lib, oracle, road, shape):
    fa.run_parity(lib, oracle, (4, 12), shape, road=road, decode=False)


@pytest.mark.parametrize("kind", ["matched", "uniform"])
@pytest.mark.parametrize("case", fa.RECEIVER_CODES, ids=fa.receiver_id)
def test_receiver_codes(lib, oracle, case, kind):
    fa.run_receiver_codes(lib, oracle, *case, kinds=(kind,))


def test_fit_lengths(lib):
    first = fa.FittedEngine(lib, 4, 12)
    try:
        fa.run_fit_lengths(lib, first)
    finally:
        first.close()


def test_refit_between_launches_of_one_small_plan(lib, oracle):
    """(the emulator's size: items of a wave's and a chunk's length beside the long one)"""
    eng = fa.FittedEngine(lib, 4, 12)
    try:
        fa.run_refit_between_launches(lib, oracle, eng, 120_001)
    finally:
        eng.close()


def test_interface_errors(lib):
    fa.run_interface_errors(lib)
