"""ctypes face of include/aws/compression/huffman_amd_planes.h (byte planes of multi-byte elements: the split with counts, and
the merge) and what its tests share.  Used by tests/test_emulated_planes.py (emulator build) and tests/test_gpu_planes.py
(MI355X): every run_* scenario below is called by both, at the same sizes.

Every expectation is numpy's or the oracle's: a plane is a.reshape(n, E)[:, p], its counts np.bincount of that, a packed
plane what the oracle makes under the host's code lengths for those counts with the stored rule applied
(stored_api.Sent).  Nothing here asks the library what it should have done."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import build_api as ba
import fit_api as fa
import harness
import packed_decode_api as pd
import plan_counts_api as pk
import stored_api as sa

INVALID = (-1, harness.AWS_ERROR_INVALID_ARGUMENT)
HEADER = os.path.join(harness.REPO, "include", "aws", "compression", "huffman_amd_planes.h")
NAMES = ["aws_huffman_amd_planes_split", "aws_huffman_amd_planes_merge", "aws_huffman_amd_testing_set_planes_grid"]
MARKER = 0xC3
STEP = 32768  # bytes of elements a workgroup of the split takes a step (the merge's step is half of it)
SIZES = (1, 2, 4, 8)
EDGE_COUNTS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025]
IN_MISALIGN, PLANE_MISALIGN, OUT_MISALIGN = (0, 1, 3, 15), (0, 5), (0, 7)
CONTENTS = ("uniform", "one element", "constant top byte")


def start(element_bytes):
    """What a counts array of element_bytes planes holds before a call: plan_counts_api.START's pattern (above 2^32: the
    adds are 64-bit), carried on over every plane."""
    return (np.arange(256 * element_bytes, dtype=np.uint64) * np.uint64(1_000_003) + np.uint64(7)) << np.uint64(20)


def bind(lib):
    """Declares the entry points of huffman_amd_planes.h (and those of the headers its scenarios call) on a loaded library.
    The symbols are looked up here: on a build without them every test fails."""
    sa.bind(lib)
    V = C.c_void_p
    lib.aws_huffman_amd_planes_split.restype = C.c_int
    lib.aws_huffman_amd_planes_split.argtypes = [C.c_int, V, C.c_uint64, C.c_uint32, V, C.c_uint64, V, V]
    lib.aws_huffman_amd_planes_merge.restype = C.c_int
    lib.aws_huffman_amd_planes_merge.argtypes = [C.c_int, V, C.c_uint64, C.c_uint64, C.c_uint32, V, V]
    lib.aws_huffman_amd_testing_set_planes_grid.restype = None
    lib.aws_huffman_amd_testing_set_planes_grid.argtypes = [C.c_uint32]
    return lib


def restore_switches(lib):
    lib.aws_huffman_amd_testing_set_planes_grid(0)
    lib.aws_huffman_amd_testing_set_count_flush_bytes(0)


def split(eng, d_in, n, e, d_planes, stride, d_counts, stream=None, device=-1):
    """(rc, error) of the enqueue, on the engine's stream unless told otherwise."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_planes_split(device, d_in, n, e, d_planes, stride, d_counts, stream or C.c_void_p(eng.stream))
    return rc, eng.lib.aws_last_error() if rc else 0


def merge(eng, d_planes, stride, n, e, d_out, stream=None, device=-1):
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_planes_merge(device, d_planes, stride, n, e, d_out, stream or C.c_void_p(eng.stream))
    return rc, eng.lib.aws_last_error() if rc else 0


def elements(rng, n, e, content):
    """n elements of e bytes, as bytes."""
    if content == "uniform":
        return rng.integers(0, 256, n * e, dtype=np.uint8)
    if content == "one element":
        return np.tile(rng.integers(0, 256, e, dtype=np.uint8), n)
    assert content == "constant top byte"
    a = rng.integers(0, 256, (n, e), dtype=np.uint8)
    a[:, e - 1] = 0x3F
    return a.reshape(-1)


def plane_counts(a, n, e):
    """numpy's counts of every plane, one after the other: e * 256 uint64."""
    if n == 0:
        return np.zeros(256 * e, np.uint64)
    return np.concatenate([ba.bincount(a.reshape(n, e)[:, p]) for p in range(e)])


def planes_image(a, n, e, stride, misalign, size):
    """What a planes buffer of `size` marker bytes holds behind a split to its byte `misalign`."""
    want = np.full(size, MARKER, np.uint8)
    for p in range(e):
        want[misalign + p * stride:misalign + p * stride + n] = a.reshape(n, e)[:, p] if n else []
    return want


def first_difference(got, want):
    bad = np.flatnonzero(got != want)
    return "first wrong byte at %d of %d, %d wrong" % (int(bad[0]), got.size, bad.size) if bad.size else None


class Arena:
    """Device memory of one scenario: elements, planes, output (each with room for a misalignment and markers behind it) and
    a counts array with a guard word."""

    def __init__(self, eng, most_bytes, most_plane_bytes, e_most=8):
        self.eng = eng
        self.in_size, self.planes_size = most_bytes + 64, most_plane_bytes + 64
        self.d_in, self.d_planes, self.d_out = eng.alloc(self.in_size), eng.alloc(self.planes_size), eng.alloc(self.in_size)
        self.d_counts = eng.alloc(256 * 8 * e_most + 8)

    def reset_counts(self, e):
        self.eng.upload(self.d_counts, np.concatenate([start(e), np.full(1, 0xEEEEEEEEEEEEEEEE, np.uint64)]).view(np.uint8))

    def counts(self, e):
        raw = self.eng.download(self.d_counts, 256 * 8 * e + 8).view(np.uint64)
        assert raw[256 * e] == 0xEEEEEEEEEEEEEEEE, "the word behind the counts was written"
        return raw[:256 * e]

    def close(self):
        for p in (self.d_in, self.d_planes, self.d_out, self.d_counts):
            self.eng.free(p)


def check_case(eng, ar, a, n, e, stride, in_mis, plane_mis, out_mis, label, counted=True, uploaded=False):
    """One split (counted) and one merge of `a` at these misalignments: every byte of the planes buffer and of the output
    buffer, every count."""
    if not uploaded:
        eng.upload(ar.d_in, a, offset=in_mis)
    span = plane_mis + (e - 1) * stride + n + 48
    assert span <= ar.planes_size and in_mis + a.size <= ar.in_size
    eng.fill(ar.d_planes, MARKER, span)
    if counted:
        ar.reset_counts(e)
    assert split(eng, ar.d_in + in_mis, n, e, ar.d_planes + plane_mis, stride, ar.d_counts if counted else None) == (0, 0), label
    out_span = out_mis + a.size + 48
    eng.fill(ar.d_out, MARKER, out_span)
    assert merge(eng, ar.d_planes + plane_mis, stride, n, e, ar.d_out + out_mis) == (0, 0), label
    eng.sync()
    got = eng.download(ar.d_planes, span)
    assert first_difference(got, planes_image(a, n, e, stride, plane_mis, span)) is None, (
        label, first_difference(got, planes_image(a, n, e, stride, plane_mis, span)))
    if counted:
        got_counts, want = ar.counts(e), start(e) + plane_counts(a, n, e)
        bad = np.flatnonzero(got_counts != want)
        assert bad.size == 0, (label, "first wrong count: plane %d byte %d" % (int(bad[0]) // 256, int(bad[0]) % 256),
                               int(got_counts[bad[0]] - start(e)[bad[0]]), int(want[bad[0]] - start(e)[bad[0]]), "%d wrong" % bad.size)
    back = eng.download(ar.d_out, out_span)
    want_out = np.full(out_span, MARKER, np.uint8)
    want_out[out_mis:out_mis + a.size] = a
    assert first_difference(back, want_out) is None, (label, "merge", first_difference(back, want_out))


# ----------------------------------------------------------------------------- 1: edges
def strides(n):
    return [n, n + 1, n + 13, (n + 4095) // 4096 * 4096]


def run_edges(sc, e):
    """Element size e: every edge count (and one 32 KiB step of elements - 1, + 0, + 1), every content, every misalignment of
    the elements crossed with every misalignment of the planes and every stride; the merge lands at misalignment 0 and 7 in
    turn, so that each (count, content, misalignment of the elements and of the planes) meets both."""
    eng = sc.eng
    counts = EDGE_COUNTS + [STEP // e - 1, STEP // e, STEP // e + 1]
    most = max(counts)
    ar = Arena(eng, most * e + 16, 5 + (e - 1) * ((most + 4095) // 4096 * 4096) + most + 48, e)
    rng = np.random.default_rng(1500 + e)
    try:
        for n in counts:
            for content in CONTENTS:
                a = elements(rng, n, e, content)
                for in_mis in IN_MISALIGN:
                    eng.upload(ar.d_in, a, offset=in_mis)
                    for plane_mis in PLANE_MISALIGN:
                        for k, stride in enumerate(strides(n)):
                            check_case(eng, ar, a, n, e, stride, in_mis, plane_mis, OUT_MISALIGN[k % 2],
                                       "E %d, n %d, %s, in + %d, planes + %d, S %d" % (e, n, content, in_mis, plane_mis, stride),
                                       uploaded=True)
    finally:
        ar.close()


# ----------------------------------------------------------------------------- 2, 3: a workgroup's second and third turn; flushes
GRID_SHAPES = [(e, steps * STEP // e + 5) for e in (2, 8) for steps in (3, 6, 7)]


def run_grid(sc, flush_bytes=(0,)):
    """With at most three workgroups a launch: 3, 6 and 7 steps plus 5 elements, so every workgroup takes exactly one,
    exactly two, or two turns and a bit through its grid-stride loop.  flush_bytes: the flush switch at each of these."""
    eng, lib = sc.eng, sc.lib
    most = max(n * e for e, n in GRID_SHAPES)
    ar = Arena(eng, most + 16, 5 + most + 7 * 13 + 48)
    rng = np.random.default_rng(1511)
    try:
        lib.aws_huffman_amd_testing_set_planes_grid(3)
        for flush in flush_bytes:
            lib.aws_huffman_amd_testing_set_count_flush_bytes(flush)
            for e, n in GRID_SHAPES:
                # (a plane of the constant top byte: 2^17 and more hits on one bin between two flushes)
                a = elements(rng, n, e, "constant top byte" if flush else "uniform")
                check_case(eng, ar, a, n, e, n + 13, 3, 5, 7, "grid 3, flush %d, E %d, n %d" % (flush, e, n))
    finally:
        restore_switches(lib)
        ar.close()


def run_flush(sc):
    """The run_grid shapes with a flush after every 32 KiB and after every five times that a workgroup reads: exact sums."""
    run_grid(sc, flush_bytes=(32768, 5 * 32768))


# ----------------------------------------------------------------------------- 4: add semantics
def run_add_semantics(sc):
    eng = sc.eng
    rng = np.random.default_rng(1523)
    e, n = 4, 5_003
    a, b = elements(rng, n, e, "uniform"), elements(rng, n, e, "constant top byte")
    ar = Arena(eng, n * e, 3 * n + n + 48)
    try:
        # two splits of different data into one counts array
        ar.reset_counts(e)
        for x in (a, b):
            eng.upload(ar.d_in, x)
            assert split(eng, ar.d_in, n, e, ar.d_planes, n, ar.d_counts) == (0, 0)
            eng.sync()
        assert np.array_equal(ar.counts(e), start(e) + plane_counts(a, n, e) + plane_counts(b, n, e))
        # NULL: nothing is counted (the planes are made all the same)
        ar.reset_counts(e)
        eng.fill(ar.d_planes, MARKER, 4 * n + 48)
        assert split(eng, ar.d_in, n, e, ar.d_planes, n, None) == (0, 0)
        eng.sync()
        assert np.array_equal(ar.counts(e), start(e))
        assert first_difference(eng.download(ar.d_planes, 4 * n + 48), planes_image(b, n, e, n, 0, 4 * n + 48)) is None
        # E = 1 over a range: a copy, and the counts aws_huffman_amd_symbol_counts leaves for the range
        span = 4 * n - 29
        ar.reset_counts(1)
        eng.fill(ar.d_planes, MARKER, span + 48)
        assert split(eng, ar.d_in + 13, span, 1, ar.d_planes + 5, span, ar.d_counts) == (0, 0)
        eng.sync()
        mine = ar.counts(1).copy()
        assert first_difference(eng.download(ar.d_planes, span + 48), planes_image(b[13:13 + span], span, 1, span, 5, span + 48)) is None
        ar.reset_counts(1)
        pk.range_counts(eng, ar.d_in, 13, span, ar.d_counts)
        eng.sync()
        theirs = ar.counts(1)
        assert np.array_equal(theirs, start(1) + ba.bincount(b[13:13 + span])) and np.array_equal(mine, theirs)
    finally:
        ar.close()


# ----------------------------------------------------------------------------- 5: the round trip through a coder a plane
ROUND_TRIP_KINDS = ["bf16", "f32", "u32 below 1000"]
ROUND_TRIP_ELEMENTS = 40_000
ITEM = 4096
BF16_TOP_PLANE_CAP = 0.55  # of the plane's bytes: the min-4 cost bound of N(0, 1)'s sign-and-exponent byte is 0.513


def round_trip_data(kind, seed=1531, n=ROUND_TRIP_ELEMENTS, scale=1.0):
    """(element size, the elements as bytes)."""
    rng = np.random.default_rng(seed)
    if kind == "bf16":  # the top 16 bits of the f32
        return 2, ((scale * rng.standard_normal(n)).astype("<f4").view("<u4") >> 16).astype("<u2").view(np.uint8)
    if kind == "f32":
        return 4, rng.standard_normal(n).astype("<f4").view(np.uint8)
    assert kind == "u32 below 1000"
    return 4, rng.integers(0, 1000, n).astype("<u4").view(np.uint8)


class PlaneSender:
    """One plane's sender: a (4, 12) engine fitted from the split's counts of the plane, a strided plan of 4 KiB items over
    the plane, a packed stored launch.  The planes buffer's stride is the elements rounded up to whole items and the buffer
    holds FILL before the split, so the last item ends in bytes the split must leave alone; the fit is from the counts of
    the plane's own n bytes, as the split counts them."""
    FILL = 0x00

    def __init__(self, lib, d_plane, stride):
        self.lib, self.d_plane, self.stride = lib, d_plane, stride
        self.items = stride // ITEM
        self.eng = fa.FittedEngine(lib, 4, 12)
        self.plan = self.eng.plan_strided(True, count=self.items, in_offset=0, in_stride=ITEM, in_len=ITEM, out_offset=0,
                                          out_stride=0, out_capacity=0, first_bit=0, eos_padding=0xFF)
        self.bufs = sa.Buffers(self.eng, self.items, stride + 64, d_plane)

    def prepare(self):
        self.bufs.refill()
        self.eng.fill(self.eng.d_bits, 0, 256)
        self.eng.fill(self.eng.d_status, 0xEE, 4)

    def enqueue(self, d_counts, stream):
        assert self.eng.fit_counts_async(d_counts, stream) == (0, 0)
        assert sa.launch_stored(self.eng, self.plan, self.d_plane, self.bufs.d_out, self.stride, self.bufs.d_off, self.bufs.d_flags,
                                1, stream) == (0, 0)

    def check(self, oracle, plane, n, label):
        """Behind the chain: the fitted lengths are the host's for numpy's counts of the plane, and packed bytes, offsets,
        flags and records are what the oracle makes of the items under them with the stored rule.  Returns the Sent."""
        assert self.eng.status() == fa.FIT_OK, label
        lengths = fa.host_lengths(self.lib, ba.bincount(plane[:n]), 4, 12)
        assert self.eng.bits() == lengths, label
        self.lengths = lengths
        self.ocoder = fa.oracle_coder(oracle, fa.host_rows(self.lib, lengths))
        blobs = [plane[i * ITEM:(i + 1) * ITEM] for i in range(self.items)]
        sent = sa.Sent(oracle, self.ocoder, blobs, np.asarray(lengths, dtype=np.int64), [(0, 0)] * self.items, [0xFF] * self.items, 1)
        sa.check_sent(self.eng, self.plan, sent, self.bufs, self.stride, label, launch=False)
        return sent

    def close(self):
        self.bufs.close()
        self.lib.aws_huffman_amd_encode_plan_destroy(self.plan)
        self.eng.close()


class PlaneReceiver:
    """One plane's receiver: an engine fitted from the sender's 256 lengths, a decode plan reset from the sender's offsets
    and flags, a packed decode launch into the plane's place in the buffer the merge reads."""

    def __init__(self, lib, sender, d_back, room):
        self.lib, self.sender, self.d_back, self.room = lib, sender, d_back, room
        self.eng = fa.FittedEngine(lib, 4, 12)
        self.plan = self.eng.empty_decode_plan()
        self.d_off = self.eng.alloc(8 * (sender.items + 1))

    def prepare(self):
        self.eng.fill(self.d_off, 0xEE, 8 * (self.sender.items + 1))
        self.eng.fill(self.eng.d_status, 0xEE, 4)

    def enqueue(self, stream):
        s = self.sender
        assert self.eng.fit_lengths_async(s.eng.d_bits, stream) == (0, 0)
        assert sa.reset_stored_input(self.eng, self.plan, s.bufs.d_off, None, s.bufs.d_flags, s.items, stream) == (0, 0)
        assert pd.launch_packed(self.eng, self.plan, s.bufs.d_out, self.d_back, s.stride, self.d_off, 1, stream) == (0, 0)

    def check(self, sc, sent, label):
        assert self.eng.status() == fa.FIT_OK, label
        recv = sa.Received(sc, sent, ocoder=self.sender.ocoder, min_bits=min(self.sender.lengths))
        sa.check_received(self.eng, self.plan, self.sender.bufs.d_out, recv, self.sender.stride, self.d_back, self.d_off, self.room,
                          label, launch=False)

    def close(self):
        self.eng.free(self.d_off)
        self.lib.aws_huffman_amd_decode_plan_destroy(self.plan)
        self.eng.close()


def run_round_trip(sc, kind, clear):
    """Counted split, then a plane at a time fit, strided plan and packed stored launch; the receiver's fit from the lengths,
    reset, packed decode; the merge -- all enqueued on one stream, nothing waited for before the checks.  clear(eng, dptr,
    size, stream) zeroes the counts in stream order."""
    lib, eng = sc.lib, sc.eng
    e, a = round_trip_data(kind)
    n = ROUND_TRIP_ELEMENTS
    stride = (n + ITEM - 1) // ITEM * ITEM
    back_stride = stride + 64  # (markers behind every decoded plane)
    d_in, d_planes, d_back, d_out = eng.alloc(n * e), eng.alloc(e * stride), eng.alloc(e * back_stride), eng.alloc(n * e + 64)
    d_counts = eng.alloc(256 * 8 * e)
    stream = C.c_void_p(eng.stream)
    senders = [PlaneSender(lib, d_planes + p * stride, stride) for p in range(e)]
    receivers = [PlaneReceiver(lib, senders[p], d_back + p * back_stride, back_stride) for p in range(e)]
    try:
        eng.upload(d_in, a)
        eng.fill(d_planes, PlaneSender.FILL, e * stride)
        eng.fill(d_back, MARKER, e * back_stride)
        eng.fill(d_out, MARKER, n * e + 64)
        eng.fill(d_counts, 0xEE, 256 * 8 * e)
        for x in senders + receivers:
            x.prepare()
        # ---- the chain: nothing below waits
        clear(eng, d_counts, 256 * 8 * e, stream)
        assert split(eng, d_in, n, e, d_planes, stride, d_counts, stream) == (0, 0)
        for p, s in enumerate(senders):
            s.enqueue(d_counts + 256 * 8 * p, stream)
        for r in receivers:
            r.enqueue(stream)
        assert merge(eng, d_back, back_stride, n, e, d_out, stream) == (0, 0)
        # ---- the checks
        eng.sync()
        back = eng.download(d_out, n * e + 64)
        assert np.array_equal(back[:n * e], a) and np.all(back[n * e:] == MARKER), kind
        counts = eng.download(d_counts, 256 * 8 * e).view(np.uint64)
        assert np.array_equal(counts, plane_counts(a, n, e)), kind
        planes = eng.download(d_planes, e * stride)
        want = np.full(e * stride, PlaneSender.FILL, np.uint8)
        for p in range(e):
            want[p * stride:p * stride + n] = a.reshape(n, e)[:, p]
        assert np.array_equal(planes, want), kind
        packed = 0
        for p in range(e):
            label = "%s, plane %d" % (kind, p)
            sent = senders[p].check(sc.oracle, want[p * stride:(p + 1) * stride], n, label)
            receivers[p].check(sc, sent, label)
            packed += sent.total
            print("%s: %d items stored of %d, packed to %.4f of the plane" % (label, int(sent.stored.sum()), sent.stored.size, sent.total / stride))
            if kind == "bf16" and p == 1:
                assert sent.total <= BF16_TOP_PLANE_CAP * stride, (label, sent.total, stride, sent.total / stride)
                assert not sent.stored.any()
        assert packed < e * stride, (kind, packed, e * stride)
    finally:
        for x in receivers + senders:
            x.close()
        for d in (d_in, d_planes, d_back, d_out, d_counts):
            eng.free(d)


# ----------------------------------------------------------------------------- 6: refusals
def run_refusals(sc):
    """Every refusal of the header; behind each, the planes, the output and the counts are as they were."""
    eng, lib = sc.eng, sc.lib
    rng = np.random.default_rng(1543)
    e, n = 4, 3_000
    a = elements(rng, n, e, "uniform")
    ar = Arena(eng, 8 * n, 8 * n)
    try:
        eng.upload(ar.d_in, a)
        eng.fill(ar.d_planes, MARKER, ar.planes_size)
        eng.fill(ar.d_out, MARKER, ar.in_size)
        ar.reset_counts(8)
        no_device = lib.aws_huffman_amd_device_count()
        for bad in (0, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF):
            assert split(eng, ar.d_in, n, bad, ar.d_planes, n, ar.d_counts) == INVALID, bad
            assert merge(eng, ar.d_planes, n, n, bad, ar.d_out) == INVALID, bad
        assert split(eng, None, n, e, ar.d_planes, n, ar.d_counts) == INVALID
        assert split(eng, ar.d_in, n, e, None, n, ar.d_counts) == INVALID
        assert merge(eng, None, n, n, e, ar.d_out) == INVALID
        assert merge(eng, ar.d_planes, n, n, e, None) == INVALID
        assert split(eng, ar.d_in, n, e, ar.d_planes, n - 1, ar.d_counts) == INVALID
        assert merge(eng, ar.d_planes, n - 1, n, e, ar.d_out) == INVALID
        # n * E, and (E - 1) * S + n, that do not fit 64 bits
        assert split(eng, ar.d_in, 1 << 63, 2, ar.d_planes, 1 << 63, ar.d_counts) == INVALID
        assert merge(eng, ar.d_planes, 1 << 63, 1 << 63, 2, ar.d_out) == INVALID
        assert split(eng, ar.d_in, 1 << 61, 8, ar.d_planes, 1 << 61, ar.d_counts) == INVALID
        assert split(eng, ar.d_in, 1, 8, ar.d_planes, 1 << 62, ar.d_counts) == INVALID
        assert merge(eng, ar.d_planes, 1 << 62, 1, 8, ar.d_out) == INVALID
        assert split(eng, ar.d_in, 16, 2, ar.d_planes, (1 << 64) - 8, ar.d_counts) == INVALID
        # a device that does not exist
        assert split(eng, ar.d_in, n, e, ar.d_planes, n, ar.d_counts, device=no_device) == INVALID
        assert merge(eng, ar.d_planes, n, n, e, ar.d_out, device=no_device) == INVALID
        assert split(eng, ar.d_in, 0, e, ar.d_planes, 0, ar.d_counts, device=no_device) == INVALID
        # counts that are not 8-byte aligned
        for off in (1, 2, 4, 7):
            assert split(eng, ar.d_in, n, e, ar.d_planes, n, ar.d_counts + off) == INVALID, off
        # source and destination that overlap: the planes inside the elements, one byte shared at either end, the last
        # plane alone; the same for the merge
        assert split(eng, ar.d_in, n, e, ar.d_in + 16, n, ar.d_counts) == INVALID
        assert split(eng, ar.d_in, n, e, ar.d_in + n * e - 1, n, ar.d_counts) == INVALID
        assert split(eng, ar.d_in + 3 * n + n - 1, n, e, ar.d_in, n, ar.d_counts) == INVALID
        assert split(eng, ar.d_in + 3 * 4096 + 5, 8, e, ar.d_in, 4096, ar.d_counts) == INVALID
        assert merge(eng, ar.d_planes, n, n, e, ar.d_planes + 16) == INVALID
        assert merge(eng, ar.d_planes, n, n, e, ar.d_planes + 4 * n - 1) == INVALID
        assert merge(eng, ar.d_planes + n * e - 1, n, n, e, ar.d_planes) == INVALID
        eng.sync()
        assert np.all(eng.download(ar.d_planes, ar.planes_size) == MARKER) and np.all(eng.download(ar.d_out, ar.in_size) == MARKER)
        assert np.array_equal(ar.counts(8), start(8))
        assert np.array_equal(eng.download(ar.d_in, a.size), a)
        # ranges that only touch are taken; no elements: success, nothing enqueued, NULL pointers and all
        assert split(eng, ar.d_in, n, e, ar.d_in + n * e, n, None) == (0, 0)
        eng.sync()
        assert np.array_equal(eng.download(ar.d_in, 2 * n * e), np.concatenate([a, a.reshape(n, e).T.reshape(-1)]))
        assert split(eng, None, 0, e, None, 0, None) == (0, 0) and merge(eng, None, 0, 0, e, None) == (0, 0)
        assert split(eng, ar.d_in, 0, e, ar.d_planes, 77, ar.d_counts) == (0, 0) and merge(eng, ar.d_planes, 77, 0, e, ar.d_out) == (0, 0)
        eng.sync()
        assert np.all(eng.download(ar.d_planes, ar.planes_size) == MARKER) and np.all(eng.download(ar.d_out, ar.in_size) == MARKER)
        assert np.array_equal(ar.counts(8), start(8))
        check_case(eng, ar, a, n, e, n, 0, 0, 0, "behind the refusals")
    finally:
        ar.close()


# ----------------------------------------------------------------------------- 7: no GPU, exports
def run_product_without_a_gpu(product):
    """Against the product library on a machine without a GPU: both calls raise AWS_ERROR_UNSUPPORTED_OPERATION and touch
    nothing they were handed.  (With a GPU present this has nothing to say: tests/test_gpu_planes.py speaks there.)"""
    if product.aws_huffman_amd_device_count() > 0:
        return
    memory = np.full(16384, 0xEE, np.uint8)
    base = memory.ctypes.data
    for call in (lambda: product.aws_huffman_amd_planes_split(-1, base, 512, 4, base + 4096, 512, base + 8192, None),
                 lambda: product.aws_huffman_amd_planes_split(-1, base, 512, 3, base + 4096, 12, base + 8193, None),
                 lambda: product.aws_huffman_amd_planes_merge(-1, base + 4096, 512, 512, 4, base, None),
                 lambda: product.aws_huffman_amd_planes_merge(-1, None, 0, 0, 4, None, None)):
        product.aws_reset_error()
        assert call() == -1
        assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    assert np.all(memory == 0xEE)


def header_api_names():
    text = open(HEADER).read()
    return re.findall(r"AWS_COMPRESSION_API\s+[\w\s\*]*?\b(aws_\w+)\s*\(", text)


def run_exports(so_path):
    """The names the header declares are exactly the library's exported names that speak of planes."""
    names = header_api_names()
    assert names == NAMES, names
    listing = subprocess.check_output(["nm", "-D", "--defined-only", so_path], text=True)
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    assert {x for x in exported if "planes" in x} == set(names), sorted(x for x in exported if "planes" in x)
