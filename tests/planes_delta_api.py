"""ctypes face of include/aws/compression/huffman_amd_planes_delta.h (byte planes of differences in runs: the split with
counts, and the merge that sums) and what its tests share.  Used by tests/test_emulated_planes_delta.py (emulator build) and
tests/test_gpu_planes_delta.py (MI355X): every run_* scenario below is called by both, at the same sizes.

Every expectation is numpy's or the oracle's.  With x the elements in their unsigned dtype and R the run,
    d[j] = x[j] where R divides j, x[j] - x[j - 1] elsewhere        (differences)
    out  = np.cumsum of d over every run, in that dtype             (sums)
the planes are those of d, their counts np.bincount of them, a packed plane what the oracle makes of it
(planes_api.PlaneSender).  Nothing here asks the library what it should have done."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import harness
import planes_api as pl

INVALID = pl.INVALID
HEADER = os.path.join(harness.REPO, "include", "aws", "compression", "huffman_amd_planes_delta.h")
NAMES = ["aws_huffman_amd_plane_delta_split", "aws_huffman_amd_plane_delta_merge"]
MARKER = pl.MARKER
SPLIT_STEP, MERGE_STEP = 32768, 16384  # bytes of elements a workgroup takes a step
SIZES = pl.SIZES
RUNS = (16, 512, 1024, 2048)
DTYPE = {1: "<u1", 2: "<u2", 4: "<u4", 8: "<u8"}
CONTENTS = ("uniform", "ramp", "one element", "all-ones differences", "differences below 256")


def bind(lib):
    """Declares the entry points of huffman_amd_planes_delta.h (and of huffman_amd_planes.h and what its scenarios call) on
    a loaded library.  The symbols are looked up here: on a build without them every test fails."""
    pl.bind(lib)
    V = C.c_void_p
    lib.aws_huffman_amd_plane_delta_split.restype = C.c_int
    lib.aws_huffman_amd_plane_delta_split.argtypes = [C.c_int, V, C.c_uint64, C.c_uint32, C.c_uint32, V, C.c_uint64, V, V]
    lib.aws_huffman_amd_plane_delta_merge.restype = C.c_int
    lib.aws_huffman_amd_plane_delta_merge.argtypes = [C.c_int, V, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, V, V]
    return lib


restore_switches = pl.restore_switches


def split_delta(eng, d_in, n, e, r, d_planes, stride, d_counts, stream=None, device=-1):
    """(rc, error) of the enqueue, on the engine's stream unless told otherwise."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_plane_delta_split(device, d_in, n, e, r, d_planes, stride, d_counts, stream or C.c_void_p(eng.stream))
    return rc, eng.lib.aws_last_error() if rc else 0


def merge_delta(eng, d_planes, stride, n, e, r, d_out, stream=None, device=-1):
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_plane_delta_merge(device, d_planes, stride, n, e, r, d_out, stream or C.c_void_p(eng.stream))
    return rc, eng.lib.aws_last_error() if rc else 0


# ----------------------------------------------------------------------------- numpy's side
def differences(a, e, r):
    """The bytes of d for the elements whose bytes are a: the formula of the header, spelled out."""
    x = np.ascontiguousarray(a).view(DTYPE[e])
    d = x.copy()
    d[1:] = x[1:] - x[:-1]  # (unsigned: modulo 2^(8 e))
    d[::r] = x[::r]
    return d.view(np.uint8)


def sums(d_bytes, e, r):
    """The bytes of the elements whose differences' bytes are d_bytes: np.cumsum over every run, in the unsigned dtype."""
    d = np.ascontiguousarray(d_bytes).view(DTYPE[e])
    n = d.size
    whole = np.zeros((n + r - 1) // r * r, DTYPE[e])
    whole[:n] = d
    return np.cumsum(whole.reshape(-1, r), axis=1, dtype=DTYPE[e]).reshape(-1)[:n].view(np.uint8)


def elements(rng, n, e, r, content):
    """n elements of e bytes, as bytes."""
    dt = np.dtype(DTYPE[e])
    j = np.arange(n, dtype=np.uint64)
    if content == "uniform":  # (every difference wraps around)
        return rng.integers(0, 256, n * e, dtype=np.uint8)
    if content == "ramp":
        return (j * np.uint64(3) + np.uint64(1000)).astype(dt).view(np.uint8)
    if content == "one element":
        return np.tile(rng.integers(0, 256, e, dtype=np.uint8), n)
    if content == "all-ones differences":  # x[j] = -(j % r + 1): a borrow through every byte of every difference
        return (np.uint64(0) - (j % np.uint64(r) + np.uint64(1))).astype(dt).view(np.uint8)
    assert content == "differences below 256"
    return np.cumsum(rng.integers(0, 256, n, dtype=np.uint64), dtype=np.uint64).astype(dt).view(np.uint8)


def check_case(eng, ar, rng, a, n, e, r, stride, in_mis, plane_mis, out_mis, label, random_merge=True):
    """Of `a` at these misalignments: the split of differences, counted and not, against the formula -- every byte of the
    planes buffer, every count; the merge of those planes, which gives a back; the merge of random planes against the
    sums over every run -- every byte of the output buffer."""
    d = differences(a, e, r)
    assert np.array_equal(sums(d, e, r), a)  # (numpy's two sides agree)
    eng.upload(ar.d_in, a, offset=in_mis)
    span = plane_mis + (e - 1) * stride + n + 48
    out_span = out_mis + a.size + 48
    assert span <= ar.planes_size and in_mis + a.size <= ar.in_size and out_span <= ar.in_size
    want_planes = pl.planes_image(d, n, e, stride, plane_mis, span)
    for counted in (True, False):
        eng.fill(ar.d_planes, MARKER, span)
        ar.reset_counts(e)
        assert split_delta(eng, ar.d_in + in_mis, n, e, r, ar.d_planes + plane_mis, stride, ar.d_counts if counted else None) == (0, 0), label
        eng.sync()
        got = eng.download(ar.d_planes, span)
        assert pl.first_difference(got, want_planes) is None, (label, "counted" if counted else "not counted", pl.first_difference(got, want_planes))
        got_counts, want = ar.counts(e), pl.start(e) + (pl.plane_counts(d, n, e) if counted else 0)
        bad = np.flatnonzero(got_counts != want)
        assert bad.size == 0, (label, counted, "first wrong count: plane %d byte %d" % (int(bad[0]) // 256, int(bad[0]) % 256),
                               int(got_counts[bad[0]] - pl.start(e)[bad[0]]), int(want[bad[0]] - pl.start(e)[bad[0]]), "%d wrong" % bad.size)
    want_out = np.full(out_span, MARKER, np.uint8)
    want_out[out_mis:out_mis + a.size] = a
    eng.fill(ar.d_out, MARKER, out_span)
    assert merge_delta(eng, ar.d_planes + plane_mis, stride, n, e, r, ar.d_out + out_mis) == (0, 0), label
    eng.sync()
    back = eng.download(ar.d_out, out_span)
    assert pl.first_difference(back, want_out) is None, (label, "merge after split", pl.first_difference(back, want_out))
    if random_merge:
        b = rng.integers(0, 256, n * e, dtype=np.uint8)
        eng.upload(ar.d_planes, pl.planes_image(b, n, e, stride, plane_mis, span))
        want_out[out_mis:out_mis + a.size] = sums(b, e, r)
        eng.fill(ar.d_out, MARKER, out_span)
        assert merge_delta(eng, ar.d_planes + plane_mis, stride, n, e, r, ar.d_out + out_mis) == (0, 0), label
        eng.sync()
        back = eng.download(ar.d_out, out_span)
        assert pl.first_difference(back, want_out) is None, (label, "merge of random planes", pl.first_difference(back, want_out))
        assert np.array_equal(eng.download(ar.d_planes, span), pl.planes_image(b, n, e, stride, plane_mis, span)), (label, "the merge wrote planes")


# ----------------------------------------------------------------------------- 1: edges
def edge_counts(e, r):
    """planes_api's edge counts; a run - 1, + 0, + 1 and two runs and 15; one step - 1, + 0, + 1 of the merge and of the split."""
    counts = pl.EDGE_COUNTS + [r - 1, r, r + 1, 2 * r + 15]
    for step in (MERGE_STEP, SPLIT_STEP):
        counts += [step // e - 1, step // e, step // e + 1]
    return sorted(set(counts))


def run_edges(sc, e, r):
    """Element size e and run r: every edge count with every content; the misalignments of elements, planes and output and
    the stride change from case to case (planes_api's values, with periods 4, 2, 2 and 4 against 5 contents a count), so that
    every count and every content meets every one of them."""
    eng = sc.eng
    counts = edge_counts(e, r)
    most = max(counts)
    ar = pl.Arena(eng, most * e + 16, 5 + (e - 1) * ((most + 4095) // 4096 * 4096) + most + 48, e)
    rng = np.random.default_rng(1600 + 16 * e + r)
    k = 0
    try:
        for n in counts:
            for content in CONTENTS:
                a = elements(rng, n, e, r, content)
                in_mis, plane_mis = pl.IN_MISALIGN[k % 4], pl.PLANE_MISALIGN[(k // 4) % 2]
                out_mis, stride = pl.OUT_MISALIGN[(k // 2) % 2], pl.strides(n)[(k // 3) % 4]
                check_case(eng, ar, rng, a, n, e, r, stride, in_mis, plane_mis, out_mis,
                           "E %d, R %d, n %d, %s, in + %d, planes + %d, out + %d, S %d" % (e, r, n, content, in_mis, plane_mis, out_mis, stride))
                k += 1
    finally:
        ar.close()


# ----------------------------------------------------------------------------- 2: the regimes of the merge's scan
REGIMES = {
    "run of 16, within a lane": [(4, 16, 5_000), (8, 16, 5_000), (1, 16, 5_000)],
    "run of 1024 at E = 4, one wave's span exactly": [(4, 1024, 3 * 1024)],
    "run of 512, part of a wave": [(2, 512, 5 * 512), (8, 256, 9 * 256)],
    "run of 2048 at E = 1, two waves through LDS": [(1, 2048, 5 * 2048)],
    "run of 2048 at E = 2, two waves through LDS": [(2, 2048, 5 * 2048)],
    "run of 2048 at E = 4, two waves through LDS": [(4, 2048, 5 * 2048)],
    "run of 1024 at E = 8, two waves through LDS": [(8, 1024, 5 * 1024)],
    "run of 2048 at E = 8, four waves through LDS": [(8, 2048, 3 * 2048)],
    "a run that ends in the tail, groups of it in front": [(e, r, 2 * r + 16 * 3 + 5) for e in SIZES for r in (64, 2048)],
    "a run that ends in the tail, nothing of it in front": [(e, r, 2 * r + 5) for e in SIZES for r in (64, 2048)],
    "a tail that starts a run": [(e, r, 3 * r + 3) for e in SIZES for r in (16, 1024)],
    "a tail behind all but one group of a run": [(e, 2048, 2 * 2048 - 1) for e in SIZES],
}


def run_regime(sc, name):
    eng = sc.eng
    shapes = REGIMES[name]
    most = max(n for _, _, n in shapes)
    ar = pl.Arena(eng, most * 8 + 16, 5 + 8 * (most + 13) + 48)
    rng = np.random.default_rng(1613)
    try:
        for e, r, n in shapes:
            for content in ("uniform", "all-ones differences"):
                check_case(eng, ar, rng, elements(rng, n, e, r, content), n, e, r, n + 13, 3, 5, 7,
                           "%s: E %d, R %d, n %d, %s" % (name, e, r, n, content))
    finally:
        ar.close()


# ----------------------------------------------------------------------------- 3: a workgroup's further turns; flushes
GRID_SHAPES = [(e, steps * SPLIT_STEP // e + 5) for e in (2, 8) for steps in (3, 6, 7)]
GRID_CAPS = (1, 2, 4)
SMALL_FLUSH = 32768


def run_grid(sc, cap):
    """With at most `cap` workgroups a launch: 3, 6 and 7 steps of the split (twice as many of the merge) plus 5 elements,
    so a workgroup loops and the last step is short, through both calls; the runs in turn.  At two workgroups the counted
    split also flushes its counters after every 32 KiB it reads (differences below 256: planes of one value)."""
    eng, lib = sc.eng, sc.lib
    most = max(n * e for e, n in GRID_SHAPES)
    ar = pl.Arena(eng, most + 16, 5 + most + 7 * 13 + 48)
    rng = np.random.default_rng(1619 + cap)
    try:
        lib.aws_huffman_amd_testing_set_planes_grid(cap)
        for flush in (0, SMALL_FLUSH) if cap == 2 else (0,):
            lib.aws_huffman_amd_testing_set_count_flush_bytes(flush)
            for k, (e, n) in enumerate(GRID_SHAPES):
                r = (2048, 16, 1024)[(k + cap) % 3]
                a = elements(rng, n, e, r, "differences below 256" if flush else "uniform")
                check_case(eng, ar, rng, a, n, e, r, n + 13, 3, 5, 7, "grid %d, flush %d, E %d, R %d, n %d" % (cap, flush, e, r, n),
                           random_merge=False)
    finally:
        restore_switches(lib)
        ar.close()


# ----------------------------------------------------------------------------- 4: add semantics
def run_add_semantics(sc):
    eng = sc.eng
    rng = np.random.default_rng(1621)
    e, r, n = 4, 512, 5_003
    a, b = elements(rng, n, e, r, "uniform"), elements(rng, n, e, r, "differences below 256")
    ar = pl.Arena(eng, n * e, 3 * n + n + 48)
    try:
        # two splits of different data into one counts array, which was not clear (planes_api.start) before the first
        ar.reset_counts(e)
        for x in (a, b):
            eng.upload(ar.d_in, x)
            assert split_delta(eng, ar.d_in, n, e, r, ar.d_planes, n, ar.d_counts) == (0, 0)
            eng.sync()
        want = pl.plane_counts(differences(a, e, r), n, e) + pl.plane_counts(differences(b, e, r), n, e)
        assert np.array_equal(ar.counts(e), pl.start(e) + want)
        assert int(want[256 * 3]) > n  # (the top plane of b's differences is one value but where a run starts)
        # NULL: nothing is counted (the planes are made all the same)
        ar.reset_counts(e)
        eng.fill(ar.d_planes, MARKER, 4 * n + 48)
        assert split_delta(eng, ar.d_in, n, e, r, ar.d_planes, n, None) == (0, 0)
        eng.sync()
        assert np.array_equal(ar.counts(e), pl.start(e))
        assert pl.first_difference(eng.download(ar.d_planes, 4 * n + 48), pl.planes_image(differences(b, e, r), n, e, n, 0, 4 * n + 48)) is None
    finally:
        ar.close()


# ----------------------------------------------------------------------------- 5: with a coder a plane
CODER_KINDS = ["u64 offsets", "sorted u32 ids"]
CODER_ELEMENTS = pl.ROUND_TRIP_ELEMENTS
CODER_RUN = 1024


def coder_data(kind, seed=1627, n=CODER_ELEMENTS, longest=80):
    """(element size, the elements as bytes)."""
    rng = np.random.default_rng(seed)
    if kind == "u64 offsets":  # the running sum of lengths 16 .. longest
        return 8, np.cumsum(rng.integers(16, longest + 1, n, dtype=np.uint64), dtype=np.uint64).astype("<u8").view(np.uint8)
    assert kind == "sorted u32 ids"
    return 4, np.sort(rng.integers(0, 1 << 32, n, dtype=np.uint64)).astype("<u4").view(np.uint8)


def road(sc, a, e, r, clear, label):
    """planes_api.run_round_trip's chain over the elements a with run r (0: the plain split and merge): clear, counted split,
    a plane at a time fit from the counts and packed stored launch; the receiver's fit from the lengths, packed decode; the
    merge -- enqueued on one stream, nothing waited for.  The output is a, the planes and counts numpy's, every plane's
    packed bytes the oracle's.  Returns the packed total of the planes (the oracle's)."""
    lib, eng = sc.lib, sc.eng
    n = a.size // e
    stride = (n + pl.ITEM - 1) // pl.ITEM * pl.ITEM
    back_stride = stride + 64
    d_in, d_planes, d_back, d_out = eng.alloc(n * e), eng.alloc(e * stride), eng.alloc(e * back_stride), eng.alloc(n * e + 64)
    d_counts = eng.alloc(256 * 8 * e)
    stream = C.c_void_p(eng.stream)
    senders = [pl.PlaneSender(lib, d_planes + p * stride, stride) for p in range(e)]
    receivers = [pl.PlaneReceiver(lib, senders[p], d_back + p * back_stride, back_stride) for p in range(e)]
    try:
        eng.upload(d_in, a)
        eng.fill(d_planes, pl.PlaneSender.FILL, e * stride)
        eng.fill(d_back, MARKER, e * back_stride)
        eng.fill(d_out, MARKER, n * e + 64)
        eng.fill(d_counts, 0xEE, 256 * 8 * e)
        for x in senders + receivers:
            x.prepare()
        clear(eng, d_counts, 256 * 8 * e, stream)
        if r:
            assert split_delta(eng, d_in, n, e, r, d_planes, stride, d_counts, stream) == (0, 0)
        else:
            assert pl.split(eng, d_in, n, e, d_planes, stride, d_counts, stream) == (0, 0)
        for p, s in enumerate(senders):
            s.enqueue(d_counts + 256 * 8 * p, stream)
        for x in receivers:
            x.enqueue(stream)
        if r:
            assert merge_delta(eng, d_back, back_stride, n, e, r, d_out, stream) == (0, 0)
        else:
            assert pl.merge(eng, d_back, back_stride, n, e, d_out, stream) == (0, 0)
        eng.sync()
        back = eng.download(d_out, n * e + 64)
        assert np.array_equal(back[:n * e], a) and np.all(back[n * e:] == MARKER), label
        d = differences(a, e, r) if r else a
        assert np.array_equal(eng.download(d_counts, 256 * 8 * e).view(np.uint64), pl.plane_counts(d, n, e)), label
        want = np.full(e * stride, pl.PlaneSender.FILL, np.uint8)
        for p in range(e):
            want[p * stride:p * stride + n] = d.reshape(n, e)[:, p]
        assert np.array_equal(eng.download(d_planes, e * stride), want), label
        packed = 0
        for p in range(e):
            sent = senders[p].check(sc.oracle, want[p * stride:(p + 1) * stride], n, "%s, plane %d" % (label, p))
            receivers[p].check(sc, sent, "%s, plane %d" % (label, p))
            packed += sent.total
            print("%s, plane %d: %d items stored of %d, packed to %.4f of the plane" % (label, p, int(sent.stored.sum()), sent.stored.size, sent.total / stride))
        return packed, e * stride
    finally:
        for x in receivers + senders:
            x.close()
        for dptr in (d_in, d_planes, d_back, d_out, d_counts):
            eng.free(dptr)


def run_with_coder(sc, kind, clear):
    """The plain road and the road of differences in runs of 1024 over one array, each round trip checked plane by plane
    against the oracle; the planes of differences pack to less (the oracle's totals: 0.64 against 0.53 of the raw size
    estimated for the offsets, 1.00 against 0.75 for the ids)."""
    e, a = coder_data(kind)
    plain, raw = road(sc, a, e, 0, clear, kind + ", plain")
    delta, _ = road(sc, a, e, CODER_RUN, clear, kind + ", differences")
    print("%s: planes alone %.4f of the planes' bytes, planes of differences %.4f" % (kind, plain / raw, delta / raw))
    assert delta < plain, (kind, delta, plain, raw)


# ----------------------------------------------------------------------------- 6: refusals
BAD_RUNS = (0, 8, 24, 4096, 1 << 31)


def run_refusals(sc):
    """Every run that is refused, and every refusal of the plain pair through these names; behind each, the planes, the
    output and the counts are as they were."""
    eng, lib = sc.eng, sc.lib
    rng = np.random.default_rng(1637)
    e, r, n = 4, 64, 3_000
    a = elements(rng, n, e, r, "uniform")
    ar = pl.Arena(eng, 8 * n, 8 * n)
    try:
        eng.upload(ar.d_in, a)
        eng.fill(ar.d_planes, MARKER, ar.planes_size)
        eng.fill(ar.d_out, MARKER, ar.in_size)
        ar.reset_counts(8)
        no_device = lib.aws_huffman_amd_device_count()
        for bad in BAD_RUNS + (1, 15, 17, 48, 2047, 2049, 0xFFFFFFFF):
            assert split_delta(eng, ar.d_in, n, e, bad, ar.d_planes, n, ar.d_counts) == INVALID, bad
            assert merge_delta(eng, ar.d_planes, n, n, e, bad, ar.d_out) == INVALID, bad
            assert split_delta(eng, None, 0, e, bad, None, 0, None) == INVALID, bad
        for bad in (0, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF):
            assert split_delta(eng, ar.d_in, n, bad, r, ar.d_planes, n, ar.d_counts) == INVALID, bad
            assert merge_delta(eng, ar.d_planes, n, n, bad, r, ar.d_out) == INVALID, bad
        assert split_delta(eng, None, n, e, r, ar.d_planes, n, ar.d_counts) == INVALID
        assert split_delta(eng, ar.d_in, n, e, r, None, n, ar.d_counts) == INVALID
        assert merge_delta(eng, None, n, n, e, r, ar.d_out) == INVALID
        assert merge_delta(eng, ar.d_planes, n, n, e, r, None) == INVALID
        assert split_delta(eng, ar.d_in, n, e, r, ar.d_planes, n - 1, ar.d_counts) == INVALID
        assert merge_delta(eng, ar.d_planes, n - 1, n, e, r, ar.d_out) == INVALID
        # n * E, and (E - 1) * S + n, that do not fit 64 bits
        assert split_delta(eng, ar.d_in, 1 << 63, 2, r, ar.d_planes, 1 << 63, ar.d_counts) == INVALID
        assert merge_delta(eng, ar.d_planes, 1 << 63, 1 << 63, 2, r, ar.d_out) == INVALID
        assert split_delta(eng, ar.d_in, 1 << 61, 8, r, ar.d_planes, 1 << 61, ar.d_counts) == INVALID
        assert split_delta(eng, ar.d_in, 1, 8, r, ar.d_planes, 1 << 62, ar.d_counts) == INVALID
        assert merge_delta(eng, ar.d_planes, 1 << 62, 1, 8, r, ar.d_out) == INVALID
        assert split_delta(eng, ar.d_in, 16, 2, r, ar.d_planes, (1 << 64) - 8, ar.d_counts) == INVALID
        # a device that does not exist
        assert split_delta(eng, ar.d_in, n, e, r, ar.d_planes, n, ar.d_counts, device=no_device) == INVALID
        assert merge_delta(eng, ar.d_planes, n, n, e, r, ar.d_out, device=no_device) == INVALID
        assert split_delta(eng, ar.d_in, 0, e, r, ar.d_planes, 0, ar.d_counts, device=no_device) == INVALID
        # counts that are not 8-byte aligned
        for off in (1, 2, 4, 7):
            assert split_delta(eng, ar.d_in, n, e, r, ar.d_planes, n, ar.d_counts + off) == INVALID, off
        # source and destination that overlap (in-place use is one such): the planes inside the elements, one byte shared at
        # either end, the last plane alone; the same for the merge
        assert split_delta(eng, ar.d_in, n, e, r, ar.d_in, n, ar.d_counts) == INVALID
        assert split_delta(eng, ar.d_in, n, e, r, ar.d_in + 16, n, ar.d_counts) == INVALID
        assert split_delta(eng, ar.d_in, n, e, r, ar.d_in + n * e - 1, n, ar.d_counts) == INVALID
        assert split_delta(eng, ar.d_in + 3 * n + n - 1, n, e, r, ar.d_in, n, ar.d_counts) == INVALID
        assert split_delta(eng, ar.d_in + 3 * 4096 + 5, 8, e, r, ar.d_in, 4096, ar.d_counts) == INVALID
        assert merge_delta(eng, ar.d_planes, n, n, e, r, ar.d_planes) == INVALID
        assert merge_delta(eng, ar.d_planes, n, n, e, r, ar.d_planes + 16) == INVALID
        assert merge_delta(eng, ar.d_planes, n, n, e, r, ar.d_planes + 4 * n - 1) == INVALID
        assert merge_delta(eng, ar.d_planes + n * e - 1, n, n, e, r, ar.d_planes) == INVALID
        eng.sync()
        assert np.all(eng.download(ar.d_planes, ar.planes_size) == MARKER) and np.all(eng.download(ar.d_out, ar.in_size) == MARKER)
        assert np.array_equal(ar.counts(8), pl.start(8))
        assert np.array_equal(eng.download(ar.d_in, a.size), a)
        # ranges that only touch are taken; no elements: success, nothing enqueued, NULL pointers and all
        assert split_delta(eng, ar.d_in, n, e, r, ar.d_in + n * e, n, None) == (0, 0)
        eng.sync()
        assert np.array_equal(eng.download(ar.d_in, 2 * n * e), np.concatenate([a, differences(a, e, r).reshape(n, e).T.reshape(-1)]))
        assert split_delta(eng, None, 0, e, r, None, 0, None) == (0, 0) and merge_delta(eng, None, 0, 0, e, r, None) == (0, 0)
        assert split_delta(eng, ar.d_in, 0, e, r, ar.d_planes, 77, ar.d_counts) == (0, 0)
        assert merge_delta(eng, ar.d_planes, 77, 0, e, r, ar.d_out) == (0, 0)
        eng.sync()
        assert np.all(eng.download(ar.d_planes, ar.planes_size) == MARKER) and np.all(eng.download(ar.d_out, ar.in_size) == MARKER)
        assert np.array_equal(ar.counts(8), pl.start(8))
        check_case(eng, ar, rng, a, n, e, r, n, 0, 0, 0, "behind the refusals")
    finally:
        ar.close()


# ----------------------------------------------------------------------------- 7: no GPU, exports
def run_product_without_a_gpu(product):
    """Against the product library on a machine without a GPU: both calls raise AWS_ERROR_UNSUPPORTED_OPERATION, whatever
    the run, and touch nothing they were handed.  (With a GPU present tests/test_gpu_planes_delta.py speaks.)"""
    if product.aws_huffman_amd_device_count() > 0:
        return
    memory = np.full(16384, 0xEE, np.uint8)
    base = memory.ctypes.data
    for call in (lambda: product.aws_huffman_amd_plane_delta_split(-1, base, 512, 4, 64, base + 4096, 512, base + 8192, None),
                 lambda: product.aws_huffman_amd_plane_delta_split(-1, base, 512, 3, 24, base + 4096, 12, base + 8193, None),
                 lambda: product.aws_huffman_amd_plane_delta_merge(-1, base + 4096, 512, 512, 4, 64, base, None),
                 lambda: product.aws_huffman_amd_plane_delta_merge(-1, base + 4096, 512, 512, 4, 0, base, None),
                 lambda: product.aws_huffman_amd_plane_delta_merge(-1, None, 0, 0, 4, 64, None, None)):
        product.aws_reset_error()
        assert call() == -1
        assert product.aws_last_error() == harness.AWS_ERROR_UNSUPPORTED_OPERATION
    assert np.all(memory == 0xEE)


def header_api_names():
    text = open(HEADER).read()
    return re.findall(r"AWS_COMPRESSION_API\s+[\w\s\*]*?\b(aws_\w+)\s*\(", text)


def run_exports(so_path):
    """The names the header declares are exported by the library."""
    names = header_api_names()
    assert names == NAMES, names
    listing = subprocess.check_output(["nm", "-D", "--defined-only", so_path], text=True)
    exported = {line.split()[-1] for line in listing.splitlines() if line.strip()}
    assert not [x for x in names if x not in exported], [x for x in names if x not in exported]
