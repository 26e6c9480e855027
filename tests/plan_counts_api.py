"""ctypes face of include/aws/compression/huffman_amd_plan_counts.h (symbol counts of the items of an encode plan) and what
its tests share.  Used by tests/test_emulated_plan_counts.py (emulator build) and tests/test_gpu_plan_counts.py (MI355X):
every run_* scenario below is called by both, at the same sizes.

Every expectation is numpy's: all 256 uint64 compared exactly against np.bincount over the concatenation of the items' own
bytes, added to START, the non-zero value the array holds before the call.  Nothing here asks the library what a count
should be."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import build_api as ba
import fit_api as fa
import harness
import packed_api as pa
import packed_index_api as pi
import parity_cases as pc

INVALID = (-1, harness.AWS_ERROR_INVALID_ARGUMENT)
HEADER = os.path.join(harness.REPO, "include", "aws", "compression", "huffman_amd_plan_counts.h")
SEG = pa.SEG
START = (np.arange(256, dtype=np.uint64) * np.uint64(1_000_003) + np.uint64(7)) << np.uint64(20)  # (above 2^32: the adds are 64-bit)
# the thread, wave and segment limits of device_types.h and the edges of a 16-byte load
EDGE_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385,
                2 * 16384 + 500]


def bind(lib):
    """Declares the entry point of huffman_amd_plan_counts.h (and those of the headers its scenarios call) on a loaded
    library.  The symbol is looked up here: on a build without it every test fails."""
    pi.bind(lib)
    fa.bind(lib)
    V = C.c_void_p
    lib.aws_huffman_amd_encode_plan_symbol_counts.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_symbol_counts.argtypes = [V, V, V, V]
    return lib


def restore_switches(lib):
    lib.aws_huffman_amd_testing_set_count_flush_bytes(0)
    lib.aws_huffman_amd_testing_set_items_per_byte(0, 0)


def plan_counts(eng, plan, d_in, d_counts, stream=None):
    """(rc, error) of the enqueue."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_encode_plan_symbol_counts(plan, d_in, d_counts, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


class Counts:
    """256 uint64 in device memory that hold START."""

    def __init__(self, eng):
        self.eng = eng
        self.d = eng.alloc(256 * 8 + 8)
        self.reset()

    def reset(self):
        self.eng.upload(self.d, START.view(np.uint8))
        self.eng.fill(self.d + 256 * 8, 0xEE, 8)

    def read(self):
        raw = self.eng.download(self.d, 256 * 8 + 8).view(np.uint64)
        assert raw[256] == 0xEEEEEEEEEEEEEEEE, "the word behind the counts was written"
        return raw[:256]

    def close(self):
        self.eng.free(self.d)


def bincount(blobs):
    """numpy's counts of the items' own bytes, one after the other."""
    if not len(blobs):
        return np.zeros(256, np.uint64)
    return ba.bincount(np.concatenate([np.asarray(b, dtype=np.uint8) for b in blobs]))


def assert_counts(got, want, label=""):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (label, "first wrong count: byte %d" % int(bad[0]), int(got[bad[0]] - START[bad[0]]),
                           int(want[bad[0]] - START[bad[0]]), "%d wrong" % bad.size)


def check_counts(eng, plan, d_in, blobs, c, label="", times=1, stream=None):
    """`times` calls into START against numpy."""
    c.reset()
    for _ in range(times):
        assert plan_counts(eng, plan, d_in, c.d, stream) == (0, 0), label
    assert_counts(c.read(), START + np.uint64(times) * bincount(blobs), label)


class Placed:
    """Items placed by hand in an input allocation of exactly host.size bytes: (offset, length) each."""

    def __init__(self, eng, host, spans):
        self.eng, self.host, self.spans = eng, host, spans
        self.blobs = [host[o:o + n] for o, n in spans]
        self.items = [dict(in_offset=o, in_len=n, out_offset=0, out_capacity=0) for o, n in spans]
        self.d_in = eng.alloc(host.size)
        eng.upload(self.d_in, host)

    def close(self):
        self.eng.free(self.d_in)


def records_plan(eng, spans, plan=None):
    """A plan (a new one, or `plan` reset) from records that numpy builds and only device memory holds."""
    recs = np.zeros(max(len(spans), 1), pa.ITEM_DTYPE)
    if spans:
        recs["in_offset"][:len(spans)] = [o for o, _ in spans]
        recs["in_len"][:len(spans)] = [n for _, n in spans]
    recs["eos_padding"] = 0xFF
    d_items = eng.alloc(recs.nbytes)
    eng.upload(d_items, recs.view(np.uint8))
    plan = plan or eng.empty_encode_plan()
    assert eng.lib.aws_huffman_amd_encode_plan_reset_device_items(plan, d_items, len(spans), None) == 0, eng.lib.aws_last_error()
    return plan, d_items


# ----------------------------------------------------------------------------- 1: edges
def edge_batch(eng):
    """Every edge length once, and for every in_offset % 16 one short and one long item of those lengths; random bytes in the
    gaps; the items listed in shuffled order; the last item by address ends on the allocation's last byte."""
    rng = np.random.default_rng(1301)
    short = [n for n in EDGE_LENGTHS if 0 < n <= 65]
    long_ = [n for n in EDGE_LENGTHS if 511 <= n <= 4097]
    wanted = [(n, int(rng.integers(0, 16))) for n in EDGE_LENGTHS]
    for m in range(16):
        wanted += [(short[m % len(short)], m), (long_[m % len(long_)], m)]
    spans, at = [], 0
    for n, m in wanted:
        at = (at + 15) // 16 * 16 + 16 + m  # (at least 16 bytes of gap in front of every item)
        spans.append((at, n))
        at += n
    host = pc.inputs(rng, at, "uniform")
    assert spans[-1][0] + spans[-1][1] == host.size and spans[-1][1] > 0
    order = rng.permutation(len(spans))
    assert not np.array_equal(order, np.arange(len(spans)))
    return Placed(eng, host, [spans[i] for i in order])


def run_edges(sc):
    eng = sc.eng
    b = edge_batch(eng)
    plan = eng.encode_plan(b.items)
    c = Counts(eng)
    try:
        assert {n for _, n in b.spans} == set(EDGE_LENGTHS)
        for lo, hi in ((1, 65), (511, 4097)):
            assert {o % 16 for o, n in b.spans if lo <= n <= hi} == set(range(16))
        assert max(o + n for o, n in b.spans) == b.host.size
        stats = eng.encode_stats(plan)
        assert stats["by_thread"] and stats["by_wave"] and stats["by_pieces"] and stats["empty"], stats  # (every kind of unit)
        whole = ba.bincount(b.host[min(o for o, _ in b.spans):])
        assert np.any(whole != bincount(b.blobs))  # (counting the gaps would show)
        check_counts(eng, plan, b.d_in, b.blobs, c, "edges")
    finally:
        c.close()
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 2: overlap and repeats
def run_overlap_and_repeats(sc):
    """Two items over the same bytes, one item inside another, the same item listed three times: each listing counts."""
    eng = sc.eng
    rng = np.random.default_rng(1303)
    host = pc.inputs(rng, 3 * SEG, "uniform")
    spans = [(5, 20_000), (5, 20_000), (3_000, 700), (SEG + 9, 90), (SEG + 9, 90), (SEG + 9, 90), (SEG + 30, 17), (40_000, 5_000),
             (41_000, 5_000)]
    b = Placed(eng, host, spans)
    plan = eng.encode_plan(b.items)
    c = Counts(eng)
    try:
        union = np.zeros(host.size, bool)
        for o, n in spans:
            union[o:o + n] = True
        assert np.any(ba.bincount(host[union]) != bincount(b.blobs))  # (counting a repeated byte once would show)
        check_counts(eng, plan, b.d_in, b.blobs, c, "overlap")
    finally:
        c.close()
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 3: plan kinds
STRIDES = ["gaps", "tiled", "overlapping"]


def run_plan_kind(sc, kind):
    eng = sc.eng
    rng = np.random.default_rng(1307)
    c = Counts(eng)
    d_items = []
    plans = []
    try:
        if kind == "strided":
            in_len, count, first = SEG + 77, 12, 3
            host = pc.inputs(rng, first + count * 20_000 + 64, "uniform")
            d_in = eng.alloc(host.size)
            eng.upload(d_in, host)
            d_items.append(d_in)
            for stride in (20_000, in_len, in_len - 1_000):  # stride > in_len, == in_len, < in_len
                plan = eng.plan_strided(True, count=count, in_offset=first, in_stride=stride, in_len=in_len, out_offset=0,
                                        out_stride=0, out_capacity=0, first_bit=0, eos_padding=0xFF)
                plans.append(plan)
                stats = eng.encode_stats(plan)
                assert stats["items"] == count and stats["by_pieces"] == count and stats["pieces"] == 2 * count, stats
                blobs = [host[first + i * stride:first + i * stride + in_len] for i in range(count)]
                check_counts(eng, plan, d_in, blobs, c, "strided %d" % stride)
            return
        if kind == "threads":
            blobs = [pc.inputs(rng, int(rng.integers(1, 91)), pc.KINDS[i % 4]) for i in range(5_000)]
            b = pa.Batch(eng, blobs, rng)
            plan = eng.encode_plan(b.items)  # (5 000 items that are all a thread's work: made on the device from the records)
            plans.append(plan)
            assert eng.encode_stats(plan)["by_thread"] == len(blobs) >= 4_096
            check_counts(eng, plan, b.d_in, blobs, c, "threads")
            plan, d = records_plan(eng, [(o, x.size) for o, x in zip(b.in_offs, blobs)])
            plans.append(plan)
            d_items.append(d)
            stats = eng.encode_stats(plan)
            assert stats["by_thread"] == len(blobs) and stats["by_wave"] + stats["by_pieces"] == 0, stats
            check_counts(eng, plan, b.d_in, blobs, c, "threads, device records")
            b.close()
            return
        sizes = [0, 1, 15, 16, 17, 300, 700, pa.TILE - 1, pa.TILE, pa.TILE + 1, SEG - 1, SEG, SEG + 1, 2 * SEG + 500, 0, 40, 90, 129]
        blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
        b = pa.Batch(eng, blobs, rng)
        if kind == "host":
            plan = eng.encode_plan(b.items)
        else:
            assert kind == "device"
            plan, d = records_plan(eng, [(o, x.size) for o, x in zip(b.in_offs, blobs)])
            d_items.append(d)
        plans.append(plan)
        stats = eng.encode_stats(plan)
        assert stats["items"] == len(blobs) and stats["by_thread"] and stats["by_wave"] and stats["by_pieces"] and stats["empty"] == 2, stats
        check_counts(eng, plan, b.d_in, blobs, c, kind)
        b.close()
    finally:
        c.close()
        for plan in plans:
            sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        for d in d_items:
            eng.free(d)


# ----------------------------------------------------------------------------- 4: engines
ENGINES = ["test", "fitted", "hpack_lengths", "holes"]
ENGINE_SIZES = [0, 5, 100, 700, 5_000, SEG + 5, 40_000]


def run_engine(sc, name):
    """The call reads no table: the test coder, an engine made to be fitted before any fit (no AWS_ERROR_INVALID_STATE) and
    after one, a coder with 30-bit codes, a coder with symbols without a code."""
    lib = sc.lib
    rng = np.random.default_rng(1319)
    blobs = [pc.inputs(rng, n, "uniform") for n in ENGINE_SIZES]
    coder = None
    if name == "test":
        eng = sc.eng
    elif name == "fitted":
        eng = fa.FittedEngine(lib, 4, 12)
    elif name == "holes":
        eng, coder = sc.engine(holes=True)
    else:
        _, coder, _ = pc.profile_coders(sc.w, name)
        eng = harness.Engine(lib, coder)
    b = pa.Batch(eng, blobs, rng)
    plan = eng.encode_plan(b.items)
    c = Counts(eng)
    try:
        check_counts(eng, plan, b.d_in, blobs, c, name)
        if name == "fitted":
            d_out, d_off = eng.alloc(8), eng.alloc(8 * (len(blobs) + 1))
            try:  # (the engine really has no tables yet: a launch is refused, the count above was not)
                assert pa.launch_packed(eng, plan, b.d_in, d_out, 0, d_off, 1) == (-1, fa.AWS_ERROR_INVALID_STATE)
            finally:
                eng.free(d_out)
                eng.free(d_off)
            status, _ = eng.fit_counts(fa.printable_counts())
            assert status == fa.FIT_OK
            check_counts(eng, plan, b.d_in, blobs, c, "fitted, after a fit")
    finally:
        c.close()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        if name == "fitted":
            eng.close()
        elif coder is not None:
            sc.done(eng, coder)


# ----------------------------------------------------------------------------- 5, 6: add semantics; the range count
def range_counts(eng, d_in, offset, length, d_counts):
    """aws_huffman_amd_symbol_counts on the engine's stream (its own NULL is the null stream, which nothing here waits for)."""
    assert eng.lib.aws_huffman_amd_symbol_counts(-1, d_in + offset, length, d_counts, C.c_void_p(eng.stream)) == 0


def run_add_semantics(sc):
    eng = sc.eng
    rng = np.random.default_rng(1321)
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate([300, 0, 5_000, 70, 20_000, 33])]
    b = pa.Batch(eng, blobs, rng)
    plan = eng.encode_plan(b.items)
    other = eng.encode_plan(b.items[2:5][::-1])
    c = Counts(eng)
    try:
        check_counts(eng, plan, b.d_in, blobs, c, "twice", times=2)
        c.reset()
        assert plan_counts(eng, plan, b.d_in, c.d) == (0, 0) and plan_counts(eng, other, b.d_in, c.d) == (0, 0)
        assert_counts(c.read(), START + bincount(blobs) + bincount(blobs[2:5]), "two plans")
        # a plan's count plus the range count of a disjoint range: the bytes behind the last item
        last = b.in_offs[-1] + blobs[-1].size
        tail = b.host_in[last:]
        assert tail.size >= 64
        c.reset()
        assert plan_counts(eng, plan, b.d_in, c.d) == (0, 0)
        range_counts(eng, b.d_in, last, tail.size, c.d)
        assert_counts(c.read(), START + bincount(blobs) + ba.bincount(tail), "with a range count")
    finally:
        c.close()
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        sc.lib.aws_huffman_amd_encode_plan_destroy(other)
        b.close()


def run_same_as_the_range_count(sc):
    """Items that tile a range, listed in shuffled order: the array is what aws_huffman_amd_symbol_counts leaves for the
    range from the same start value."""
    eng = sc.eng
    rng = np.random.default_rng(1327)
    sizes = [17, 4_096, 1, 0, 700, SEG, 90, 2 * SEG + 500, 5_000, 64]
    first = 13
    host = pc.inputs(rng, first + sum(sizes) + 31, "printable")
    spans, at = [], first
    for n in sizes:
        spans.append((at, n))
        at += n
    b = Placed(eng, host, [spans[i] for i in rng.permutation(len(spans))])
    plan = eng.encode_plan(b.items)
    c = Counts(eng)
    try:
        check_counts(eng, plan, b.d_in, b.blobs, c, "tiling")
        mine = c.read().copy()
        c.reset()
        range_counts(eng, b.d_in, first, sum(sizes), c.d)
        theirs = c.read()
        assert_counts(theirs, START + ba.bincount(host[first:first + sum(sizes)]), "the range count itself")
        assert np.array_equal(mine, theirs)
    finally:
        c.close()
        sc.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 7: flushes inside a launch
def run_flush(sc):
    """67 segments and a few hundred short items with a flush after every 32 KiB a workgroup reads: several flushes a
    workgroup, exact sums.  The switch is restored."""
    eng, lib = sc.eng, sc.lib
    rng = np.random.default_rng(1331)
    sizes = [3 * SEG] * 21 + [2 * SEG] * 2 + [int(v) for v in rng.integers(1, 100, 300)]
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    b = pa.Batch(eng, blobs, rng)
    plan = eng.encode_plan(b.items)
    c = Counts(eng)
    try:
        stats = eng.encode_stats(plan)
        assert stats["pieces"] == 67 and stats["by_thread"] == 300, stats
        lib.aws_huffman_amd_testing_set_count_flush_bytes(32768)
        check_counts(eng, plan, b.d_in, blobs, c, "flush every step")
        lib.aws_huffman_amd_testing_set_count_flush_bytes(5 * 32768)
        check_counts(eng, plan, b.d_in, blobs, c, "flush every five steps")
    finally:
        lib.aws_huffman_amd_testing_set_count_flush_bytes(0)
        c.close()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()


# ----------------------------------------------------------------------------- 8: the life of a plan
LIFE = [(67, "host"), (0, "strided"), (3, "device"), (67, "strided"), (2, "host"), (0, "device"), (67, "device")]


def run_lifecycle(sc):
    """One plan reset to 67, 0, 3, 67, 2, 0 and 67 items across its fill kinds, the count behind each fill."""
    eng, lib = sc.eng, sc.lib
    rng = np.random.default_rng(1361)
    sizes = [int(v) for v in rng.integers(0, 3_000, 64)] + [SEG + 9, 0, 3 * SEG]
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    b = pa.Batch(eng, blobs, rng)
    plan = eng.empty_encode_plan()
    c = Counts(eng)
    d_items = []
    try:
        assert len(blobs) == 67
        for n, kind in LIFE:
            if kind == "host":
                assert lib.aws_huffman_amd_encode_plan_reset(plan, eng._encode_item_array(b.items[:n]), n) == 0
                mine = blobs[:n]
            elif kind == "strided":
                eng.plan_strided(True, plan=plan, count=n, in_offset=2, in_stride=1_000, in_len=900, out_offset=0, out_stride=0,
                                 out_capacity=0, first_bit=0, eos_padding=0xFF)
                mine = [b.host_in[2 + i * 1_000:2 + i * 1_000 + 900] for i in range(n)]
            else:
                _, d = records_plan(eng, [(o, x.size) for o, x in zip(b.in_offs[:n], blobs[:n])], plan=plan)
                d_items.append(d)
                mine = blobs[:n]
            assert eng.encode_stats(plan)["items"] == n
            check_counts(eng, plan, b.d_in, mine, c, "%d items, %s" % (n, kind))
            if n == 0:
                c.reset()
                assert plan_counts(eng, plan, None, c.d) == (0, 0)
                assert np.array_equal(c.read(), START)
    finally:
        c.close()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        for d in d_items:
            eng.free(d)
        b.close()


def run_count_changes_nothing(sc):
    """A count between a packed launch and the fetch of its results: records, road, sizes, statistics and bytes are those of
    a fresh plan that was never counted.  And a count before the first launch leaves aws_huffman_amd_decode_plan_from_encode
    answering as it does without one."""
    eng, lib = sc.eng, sc.lib
    rng = np.random.default_rng(1367)
    sizes = [40, 700, pa.TILE + 9, SEG + 1, 0, 2 * SEG + 500, 17]
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    n = len(blobs)
    b = pa.Batch(eng, blobs, rng, overflows=pa.carried(rng, n))
    c = Counts(eng)
    size = 4 * sum(sizes) + 64

    def one(counted):
        plan = eng.encode_plan(b.items)
        dplan = eng.empty_decode_plan()
        d_out, d_off = eng.alloc(size), eng.alloc(8 * (n + 1))
        try:
            if counted:
                check_counts(eng, plan, b.d_in, blobs, c, "before the first launch")
            lib.aws_reset_error()
            rc = lib.aws_huffman_amd_decode_plan_from_encode(dplan, plan, None)
            before = (rc, lib.aws_last_error() if rc else 0)
            eng.fill(d_out, pa.MARKER, size)
            eng.fill(d_off, 0xEE, 8 * (n + 1))
            assert pa.launch_packed(eng, plan, b.d_in, d_out, size - 64, d_off, 4) == (0, 0)
            if counted:
                c.reset()
                assert plan_counts(eng, plan, b.d_in, c.d) == (0, 0)
            res = eng.encode_results(plan, n)
            if counted:
                assert_counts(c.read(), START + bincount(blobs), "between a launch and its fetch")
            lib.aws_reset_error()
            rc = lib.aws_huffman_amd_decode_plan_from_encode(dplan, plan, None)
            after = (rc, lib.aws_last_error() if rc else 0)
            return (before, res, eng.encode_road(plan), pa.packed_size(eng, plan), bi_size(eng, plan), eng.encode_stats(plan), after,
                    eng.download(d_out, size).tobytes(), eng.download(d_off, 8 * (n + 1)).tobytes())
        finally:
            eng.free(d_out)
            eng.free(d_off)
            lib.aws_huffman_amd_decode_plan_destroy(dplan)
            lib.aws_huffman_amd_encode_plan_destroy(plan)

    try:
        fresh, counted = one(False), one(True)
        for k, (x, y) in enumerate(zip(counted, fresh)):
            assert x == y, (k, x if k < 7 else "bytes", y if k < 7 else "bytes")
        assert fresh[0][0] != 0 and fresh[3][:2] == (0, 0) and fresh[4][:2] == INVALID  # (no launch yet; packed; never indexed)
    finally:
        c.close()
        b.close()


def bi_size(eng, plan):
    import batch_index_api as bi

    return bi.index_size(eng, plan)


# ----------------------------------------------------------------------------- 9: the chain
def enqueue_chain(eng, clear, plan, d_in, d_out, capacity, d_off, stream):
    """clear the counts, count the plan's items, fit, packed encode: four steps on `stream`, nothing waited for in between."""
    clear(eng, eng.d_counts, 256 * 8, stream)
    assert plan_counts(eng, plan, d_in, eng.d_counts, stream) == (0, 0)
    assert eng.fit_counts_async(None, stream) == (0, 0)
    assert pa.launch_packed(eng, plan, d_in, d_out, capacity, d_off, 1, stream) == (0, 0)


CHAIN_ITEM, CHAIN_STRIDE, CHAIN_ITEMS = 2_000, 2_500, 24


def chain_data(seed):
    """Printable items with gaps that hold only the byte 0x00: (the buffer, the items' spans)."""
    host = np.zeros(CHAIN_ITEMS * CHAIN_STRIDE, np.uint8)
    text = fa.shape_bytes("printable", CHAIN_ITEMS * CHAIN_ITEM, seed)
    spans = [(i * CHAIN_STRIDE, CHAIN_ITEM) for i in range(CHAIN_ITEMS)]
    for i, (o, n) in enumerate(spans):
        host[o:o + n] = text[i * n:(i + 1) * n]
    return host, spans


def check_chain(lib, oracle, eng, plan, host, spans, d_out, d_off, capacity):
    """Behind a chain: the lengths on the device are the host's for numpy's counts of the ITEMS -- not those of the whole
    range, which differ -- and offsets, records and bytes are the oracle's under the coder of those lengths
    (fit_api.check_chain_output); every item decodes to its bytes under that coder.  Returns the lengths."""
    blobs = [host[o:o + n] for o, n in spans]
    items_only = np.concatenate(blobs)
    want = fa.host_lengths(lib, ba.bincount(items_only), eng.lo, eng.hi)
    whole = fa.host_lengths(lib, ba.bincount(host), eng.lo, eng.hi)
    assert want != whole  # (a count that took the gaps in would fit another code)
    assert eng.bits() == want
    lengths, offsets = fa.check_chain_output(lib, oracle, eng, plan, items_only, blobs, d_out, d_off, capacity)
    assert lengths == want
    ocoder = fa.oracle_coder(oracle, fa.host_rows(lib, lengths))
    got = eng.download(d_out, int(offsets[-1]))
    for i, blob in enumerate(blobs):
        r, back = oracle.decode_all(ocoder, got[int(offsets[i]):int(offsets[i + 1])], blob.size)
        assert r.rc == 0 and np.array_equal(back, blob), i
    oracle.lib.oracle_table_coder_destroy(ocoder)
    return lengths


CHAIN_KINDS = ["strided", "device"]


def chain_plan(eng, kind, spans):
    """(plan, device records or None)."""
    if kind == "strided":
        return eng.plan_strided(True, count=len(spans), in_offset=0, in_stride=CHAIN_STRIDE, in_len=CHAIN_ITEM, out_offset=0,
                                out_stride=0, out_capacity=0, first_bit=0, eos_padding=0xFF), None
    return records_plan(eng, spans)


def run_chain(lib, oracle, clear, kind):
    """A (4, 12) engine that was never fitted: clear, plan count, fit and packed launch back to back on the engine's stream,
    over a plan WITH gaps."""
    eng = fa.FittedEngine(lib, 4, 12)
    host, spans = chain_data(1373)
    capacity = 2 * host.size
    d_in, d_out, d_off = eng.alloc(host.size), eng.alloc(capacity), eng.alloc(8 * (len(spans) + 1))
    plan, d_items = chain_plan(eng, kind, spans)
    try:
        eng.upload(d_in, host)
        eng.fill(eng.d_bits, 0, 256)
        eng.fill(eng.d_status, 0xEE, 4)
        enqueue_chain(eng, clear, plan, d_in, d_out, capacity, d_off, C.c_void_p(eng.stream))
        eng.sync()
        lengths = check_chain(lib, oracle, eng, plan, host, spans, d_out, d_off, capacity)
        assert not fa.is_flat(lengths)
    finally:
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        if d_items:
            eng.free(d_items)
        for d in (d_in, d_out, d_off):
            eng.free(d)
        eng.close()


# ----------------------------------------------------------------------------- 10: refusals, no GPU, exports
def run_refusals(sc):
    eng, lib = sc.eng, sc.lib
    rng = np.random.default_rng(1381)
    blobs = [pc.inputs(rng, n, "uniform") for n in (100, 0, 3_000)]
    b = pa.Batch(eng, blobs, rng)
    plan = eng.encode_plan(b.items)
    none = eng.empty_encode_plan()
    c = Counts(eng)
    try:
        assert plan_counts(eng, None, b.d_in, c.d) == INVALID
        assert plan_counts(eng, plan, b.d_in, None) == INVALID
        assert plan_counts(eng, none, None, None) == INVALID
        for off in (1, 2, 4, 7):
            assert plan_counts(eng, plan, b.d_in, c.d + off) == INVALID, off
        assert plan_counts(eng, plan, None, c.d) == INVALID
        eng.sync()
        assert np.array_equal(c.read(), START)
        assert plan_counts(eng, none, None, c.d) == (0, 0)  # a plan without items: success, nothing enqueued
        eng.sync()
        assert np.array_equal(c.read(), START)
        check_counts(eng, plan, b.d_in, blobs, c, "behind the refusals")
    finally:
        c.close()
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        lib.aws_huffman_amd_encode_plan_destroy(none)
        b.close()


def run_product_without_a_gpu(product):
    """Against the product library on a machine without a GPU: the call raises AWS_ERROR_UNSUPPORTED_OPERATION and touches
    nothing it was handed.  (With a GPU present this has nothing to say: tests/test_gpu_plan_counts.py speaks there.)"""
    if product.aws_huffman_amd_device_count() > 0:
        return
    handle = np.full(4096, 0x11, np.uint8)  # (stands for the plan: there is none without a GPU)
    memory = np.full(8192, 0xEE, np.uint8)
    product.aws_reset_error()
    assert product.aws_huffman_amd_encode_plan_symbol_counts(handle.ctypes.data, memory.ctypes.data, memory.ctypes.data + 4096, None) == -1
    assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    assert np.all(handle == 0x11) and np.all(memory == 0xEE)


def header_api_names():
    text = open(HEADER).read()
    return re.findall(r"AWS_COMPRESSION_API\s+[\w\s\*]*?\b(aws_\w+)\s*\(", text)


def run_exports(so_path):
    names = header_api_names()
    assert names == ["aws_huffman_amd_encode_plan_symbol_counts"], names
    listing = subprocess.check_output(["nm", "-D", "--defined-only", so_path], text=True)
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported], [n for n in names if n not in exported]
