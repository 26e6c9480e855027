"""ctypes face of include/aws/compression/huffman_amd_packed.h (packed batch encode) and what its tests share: the
expected layout of a packed launch from the code lengths, the oracle's encode of one item into the room that layout gives
it, and one check of a launch against both.  Used by tests/test_emulated_packed.py (emulator build) and
tests/test_gpu_packed.py (MI355X).  Below the faces: the Scene the packed scenarios run on and the
encode scenarios themselves, library-agnostic as those of tests/parity_cases.py -- the emulated test file and the GPU one
call the same functions, at the same sizes."""
import ctypes as C

import numpy as np

import harness
import parity_cases as pc

MARKER = 0xC3  # what the output holds before a launch: gaps and everything behind the total must keep it


def bind(lib):
    """Declares the entry points of huffman_amd_packed.h on a loaded product (or emulator) library."""
    V, P = C.c_void_p, C.POINTER
    lib.aws_huffman_amd_encode_plan_launch_packed.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_launch_packed.argtypes = [V, V, V, C.c_uint64, V, C.c_uint32, V]
    lib.aws_huffman_amd_encode_plan_packed_size.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_packed_size.argtypes = [V, P(C.c_uint64), P(C.c_uint64), V]
    lib.aws_huffman_amd_testing_set_pack_tile_items.restype = None
    lib.aws_huffman_amd_testing_set_pack_tile_items.argtypes = [C.c_uint32]
    lib.aws_huffman_amd_encode_plan_reset.restype = C.c_int
    lib.aws_huffman_amd_encode_plan_reset.argtypes = [V, P(harness.AmdEncodeItem), C.c_size_t]
    lib.aws_huffman_amd_decode_plan_from_encode.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_from_encode.argtypes = [V, V, V]
    return lib


class pack_tile_items:
    """with packed_api.pack_tile_items(lib, 96): packed launches inside scan their offsets in tiles of 96 items."""

    def __init__(self, lib, items):
        self.lib, self.items = lib, items

    def __enter__(self):
        self.lib.aws_huffman_amd_testing_set_pack_tile_items(self.items)

    def __exit__(self, *exc):
        self.lib.aws_huffman_amd_testing_set_pack_tile_items(0)


def launch_packed(eng, plan, d_in, d_out, capacity, d_offsets, align, stream=None):
    """(rc, error)."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_encode_plan_launch_packed(plan, d_in, d_out, int(capacity), d_offsets, align, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def packed_size(eng, plan, stream=None):
    """(rc, error, total_bytes, longest_item_bytes)."""
    total, longest = C.c_uint64(), C.c_uint64()
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_encode_plan_packed_size(plan, C.byref(total), C.byref(longest), stream)
    return rc, eng.lib.aws_last_error() if rc else 0, total.value, longest.value


def download_u64(eng, dptr, n):
    return eng.download(dptr, 8 * int(n)).view(np.uint64).astype(np.int64)


def code_lengths(lens_table, holes=()):
    """The coder's code lengths as an int64 array (0: no code)."""
    arr = np.asarray([int(lens_table[b]) for b in range(256)], dtype=np.int64)
    for s in holes:
        arr[s] = 0
    return arr


def encoded_lengths(code_lens, blobs, overflow_bits):
    """len_i: (carried bits + every code bit + 7) // 8 -- the length query's rule, a symbol without a code 0 bits."""
    return np.asarray([(int(ob) + int(code_lens[b].sum()) + 7) // 8 for b, ob in zip(blobs, overflow_bits)], dtype=np.int64)


def expected_offsets(lens, align):
    """offsets[0] = 0, offsets[i + 1] = round_up(offsets[i] + len_i, align) -- the running sum of the rounded lengths --
    and the reserved length of every item."""
    reserved = (np.asarray(lens, dtype=np.int64) + align - 1) // align * align
    return np.concatenate([[0], np.cumsum(reserved)]).astype(np.int64), reserved


def oracle_item(oracle, ocoder, blob, overflow, eos, cap):
    """aws_huffman_encode of one item into a byte_buf of capacity `cap`: (the record as Engine.encode_results gives it,
    the `cap` bytes with MARKER where nothing was written)."""
    e = oracle.new_encoder(ocoder, eos_padding=eos)
    e.overflow_bits.pattern, e.overflow_bits.num_bits = overflow
    dst = np.full(cap + 1, MARKER, np.uint8)
    r = oracle.encode_call(e, np.ascontiguousarray(blob), 0, dst, 0, cap)
    assert dst[cap] == MARKER
    return (r.rc, r.err, r.consumed, r.produced, r.state[0], r.state[1]), dst[:cap]


def lay_out(blobs, rng=None, first=0):
    """The items' symbols one after the other (a few bytes between them with `rng`): (host array, offsets)."""
    offs, pos = [], first
    for b in blobs:
        offs.append(pos)
        pos += b.size + (int(rng.integers(0, 3)) if rng is not None else 0)
    host = np.zeros(pos + 64, np.uint8)
    for b, o in zip(blobs, offs):
        host[o:o + b.size] = b
    return host, offs


def check_launch(oracle, ocoder, eng, plan, d_in, blobs, code_lens, overflows, eoss, align, capacity=None, sample=None,
                 want_road=None, label=""):
    """One packed launch of `plan` (its items are `blobs` with these carried bits and paddings) against the definition:
    the offsets, the total and the longest reserved length; every item of `sample` (default: all) record for record and
    byte for byte against the oracle's encode into the room the layout gives it; MARKER in the gaps, behind the total
    and behind the capacity.  capacity None: exactly the total.  Returns (offsets, total, got bytes, records)."""
    n = len(blobs)
    lens = encoded_lengths(code_lens, blobs, [ov[1] for ov in overflows])
    offsets, reserved = expected_offsets(lens, align)
    total = int(offsets[-1])
    cap = total if capacity is None else int(capacity)
    size = max(total, cap) + 64
    d_out, d_off = eng.alloc(size), eng.alloc(8 * (n + 1))
    try:
        eng.fill(d_out, MARKER, size)
        eng.fill(d_off, 0xEE, 8 * (n + 1))
        assert launch_packed(eng, plan, d_in, d_out, cap, d_off, align) == (0, 0), label
        got = eng.download(d_out, size)  # (behind the launch on the stream, before any record is read)
        res = eng.encode_results(plan, n)
        if want_road is not None:
            assert eng.encode_road(plan) == want_road, (label, eng.encode_road(plan))
        got_offsets = download_u64(eng, d_off, n + 1)
        assert np.array_equal(got_offsets, offsets), (label, align, int(np.flatnonzero(got_offsets != offsets)[0]))
        assert packed_size(eng, plan) == (0, 0, total, int(reserved.max()) if n else 0), (label, packed_size(eng, plan), total)
        want = np.full(size, MARKER, np.uint8)
        every = sample is None
        for i in (range(n) if every else sample):
            off = int(offsets[i])
            room = max(0, min(int(reserved[i]), cap - off))
            rec, data = oracle_item(oracle, ocoder, blobs[i], overflows[i], eoss[i], room)
            assert res[i] == rec, (label, align, cap, i, off, room, res[i], rec)
            want[off:off + room] = data
            if not every:
                mine = got[off:off + int(reserved[i])]
                theirs = np.concatenate([data, np.full(int(reserved[i]) - room, MARKER, np.uint8)])
                assert np.array_equal(mine, theirs), (label, align, i)
        if every:
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (label, align, cap, "first wrong byte at %d" % int(bad[0]))
        assert np.all(got[min(cap, total):] == MARKER), (label, "bytes behind the total or the capacity were written")
        return offsets, total, got, res
    finally:
        eng.free(d_out)
        eng.free(d_off)


# ----------------------------------------------------------------------------- batches too large for Python lists
ITEM_DTYPE = np.dtype([("in_offset", "<u8"), ("in_len", "<u8"), ("out_offset", "<u8"), ("out_capacity", "<u8"),
                       ("pattern", "<u4"), ("num_bits", "u1"), ("pad0", "u1", 3), ("eos_padding", "u1"), ("pad1", "u1", 7)])
RESULT_DTYPE = np.dtype([("rc", "<i4"), ("error", "<i4"), ("consumed", "<u8"), ("produced", "<u8"), ("pattern", "<u4"),
                         ("num_bits", "u1"), ("pad", "u1", 3)])
assert ITEM_DTYPE.itemsize == C.sizeof(harness.AmdEncodeItem) and RESULT_DTYPE.itemsize == C.sizeof(harness.AmdEncodeResult)


def plan_from_records(eng, in_offsets, in_lens, eos=0xFF):
    """An encode plan made on the device from records built with numpy (struct aws_huffman_amd_encode_item; no room of
    their own: out_offset = out_capacity = 0).  (plan, device array of the records: the caller's to free)."""
    recs = np.zeros(len(in_lens), ITEM_DTYPE)
    recs["in_offset"], recs["in_len"], recs["eos_padding"] = in_offsets, in_lens, eos
    d_items = eng.alloc(recs.nbytes)
    eng.upload(d_items, recs.view(np.uint8))
    plan = eng.empty_encode_plan()
    assert eng.lib.aws_huffman_amd_encode_plan_reset_device_items(plan, d_items, len(in_lens), None) == 0, eng.lib.aws_last_error()
    return plan, d_items


def results_array(eng, plan, n):
    """aws_huffman_amd_encode_plan_results as a numpy record array."""
    out = np.zeros(max(n, 1), RESULT_DTYPE)
    assert eng.lib.aws_huffman_amd_encode_plan_results(plan, out.ctypes.data_as(C.POINTER(harness.AmdEncodeResult)), None) == 0
    return out[:n]


# ----------------------------------------------------------------------------- a captured graph (the HIP runtime, through ctypes)
class HipGraphs:
    """The few runtime calls a capture needs: begin / end on a stream, instantiate, launch."""

    def __init__(self):
        self.hip = None
        for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
            try:
                self.hip = C.CDLL(name)
                break
            except OSError:
                continue
        assert self.hip is not None, "the HIP runtime library was not found"
        V, P = C.c_void_p, C.POINTER
        for fn, args in (("hipStreamSynchronize", [V]),
                         ("hipStreamBeginCapture", [V, C.c_int]), ("hipStreamEndCapture", [V, P(V)]),
                         ("hipGraphInstantiate", [P(V), V, V, V, C.c_size_t]), ("hipGraphLaunch", [V, V]),
                         ("hipGraphExecDestroy", [V]), ("hipGraphDestroy", [V])):
            getattr(self.hip, fn).restype = C.c_int
            getattr(self.hip, fn).argtypes = args

    def call(self, fn, *args):
        rc = getattr(self.hip, fn)(*args)
        assert rc == 0, (fn, rc)

    def capture(self, stream, enqueue):
        """What `enqueue()` puts on `stream`, as an executable graph (hipStreamCaptureModeGlobal: a call that may not be
        captured -- an allocation, a wait -- fails it)."""
        graph, graph_exec = C.c_void_p(), C.c_void_p()
        self.call("hipStreamBeginCapture", stream, 0)
        try:
            enqueue()
        finally:
            rc = self.hip.hipStreamEndCapture(stream, C.byref(graph))
        assert rc == 0 and graph, ("hipStreamEndCapture", rc)
        self.call("hipGraphInstantiate", C.byref(graph_exec), graph, None, None, 0)
        self.call("hipGraphDestroy", graph)
        return graph_exec


# ----------------------------------------------------------------------------- what a packed scenario runs on
SEG = 16384   # HUFD_ENC_SEG_BYTES
TILE = 4096   # HUFD_ENC_SOLO_BYTES: one tile of the one-pass encoder
LARGE = 64    # HUFD_SCAN_SMALL_MAX segments (encode) or chunks (decode): above it the workgroup scan


class Scene:
    """The context of a packed scenario (encode here, decode in tests/packed_decode_api.py), whichever build `lib` is: the
    oracle, the bound library, a parity_cases.World of both, an engine of the test coder, its shortest code, and streams
    of a wanted encoded size."""

    def __init__(self, oracle, lib):
        self.oracle, self.lib = oracle, lib
        self.w = pc.World(oracle, harness.Codec(lib, "aws_"))
        self.lens = code_lengths(self.w.table[1])
        self.lens_holes = code_lengths(self.w.table[1], holes=(7, 200))
        self.min_bits = min(int(l) for l in self.w.table[1] if l)
        self.eng = harness.Engine(lib, self.w.pcoder)
        # symbols for a stream of about 3 MB: what the long items are cut from
        self.long_plain = pc.inputs(np.random.default_rng(401), 3_400_000, "uniform")

    def close(self):
        """The testing switches as a fresh process has them (a scenario restores its own; this is the module's end)."""
        self.lib.aws_huffman_amd_testing_set_pack_tile_items(0)
        self.lib.aws_huffman_amd_testing_set_decode_road(0)
        self.lib.aws_huffman_amd_testing_set_wide_min_bytes(0)
        self.lib.aws_huffman_amd_testing_set_encode_road(0)
        self.eng.close()

    def engine(self, road=None, holes=False):
        """A fresh coder, so a fresh engine that reads the road switch.  (engine, coder): both the caller's to free."""
        table = self.w.table
        if holes:
            lens = (C.c_uint8 * 256)(*table[1])
            lens[7] = lens[200] = 0
            table = (table[0], lens)
        with harness.encode_road(self.lib, road):
            coder = self.lib.aws_huffman_amd_table_coder_new(*table)
            return harness.Engine(self.lib, coder), coder

    def done(self, eng, coder):
        eng.close()
        self.lib.aws_huffman_amd_table_coder_destroy(coder)

    def encoded(self, target, eos, rng=None, kind=None):
        """A whole stream of `target` encoded bytes or a few less: as many symbols as encode to that."""
        if rng is not None and target < 100_000:
            plain = pc.inputs(rng, target * 8 // self.min_bits + 8, kind or "uniform")
        else:
            plain = self.long_plain
        enc = self.oracle.new_encoder(self.w.ocoder)
        lo, hi = 0, plain.size
        while lo < hi:  # the longest prefix that encodes to at most `target` bytes
            mid = (lo + hi + 1) // 2
            if self.oracle.encoded_length(enc, plain[:mid]) <= target:
                lo = mid
            else:
                hi = mid - 1
        out = pc.oracle_encode(self.w, plain[:lo], eos=eos)
        assert target - 3 <= out.size <= target, (target, out.size)
        return out


# ----------------------------------------------------------------------------- the encode scenarios (emulator and MI355X alike)
ENCODE_ROADS = [(None, pc.ROAD_ONE_PASS), ("three-kernel", pc.ROAD_TWO_PASS), ("one-pass-fails", pc.ROAD_GAVE_UP)]
ENCODE_PLAN_KINDS = ["host", "strided", "device", "threads"]
SCAN_TILES = [(4096, (4095, 4096, 4097)), (300, (29999, 30000, 30001)), (64, (23457,)), (1, (301,))]  # (tile, item counts)


class Batch:
    """Items in device memory.  The items' own out_offset / out_capacity are whatever `own` says (default: no room at
    all -- a packed launch must not look at them)."""

    def __init__(self, eng, blobs, rng, overflows=None, eoss=None, own=None):
        self.eng, self.blobs = eng, blobs
        n = len(blobs)
        self.overflows = overflows or [(0, 0)] * n
        self.eoss = eoss or [[0xFF, 0x00][i % 2] for i in range(n)]
        self.host_in, self.in_offs = lay_out(blobs, rng, first=1)
        self.d_in = eng.alloc(self.host_in.size)
        eng.upload(self.d_in, self.host_in)
        own = own or [(0, 0)] * n
        self.items = [dict(in_offset=self.in_offs[i], in_len=int(blobs[i].size), out_offset=own[i][0], out_capacity=own[i][1],
                           overflow_in=self.overflows[i], eos_padding=self.eoss[i]) for i in range(n)]

    def close(self):
        self.eng.free(self.d_in)


def carried(rng, n, every=4):
    out = []
    for i in range(n):
        if i % every == 1:
            nb = int(rng.integers(1, 33))
            out.append((int(rng.integers(0, 1 << nb)), nb))
        else:
            out.append((0, 0))
    return out


def mixed_blobs(rng, with_large=True):
    sizes = [0, 1, 15, 16, 17, 300, 700, TILE - 1, TILE, TILE + 1, SEG - 1, SEG, SEG + 1, 3 * SEG + 77, 0, 5 * SEG]
    if with_large:
        sizes.append((LARGE + 1) * SEG + 5)
    return [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]


def offsets_and_bytes(sc):
    """The mixed batch -- items of 0, 1, a thread's and a wave's size, either side of a tile and a segment, several segments,
    one above HUFD_SCAN_SMALL_MAX segments, some with carried bits -- at three alignments, every byte against the oracle."""
    rng = np.random.default_rng(301)
    blobs = mixed_blobs(rng)
    eng, coder = sc.engine()
    b = Batch(eng, blobs, rng, overflows=carried(rng, len(blobs)))
    plan = eng.encode_plan(b.items)
    try:
        # the length rule against the reference's own query where nothing is carried
        lens = encoded_lengths(sc.lens, blobs, [ov[1] for ov in b.overflows])
        for i, blob in enumerate(blobs):
            if b.overflows[i][1] == 0:
                assert sc.oracle.encoded_length(sc.oracle.new_encoder(sc.w.ocoder), blob) == lens[i]
        for align in (1, 4, 16):
            _, total, _, res = check_launch(sc.oracle, sc.w.ocoder, eng, plan, b.d_in, blobs, sc.lens, b.overflows, b.eoss,
                                            align, want_road=pc.ROAD_ONE_PASS, label="mixed")
            for i, r in enumerate(res):
                assert r[:2] == (0, 0) and r[3] == lens[i] and r[2] == blobs[i].size, (align, i, r)
    finally:
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        sc.done(eng, coder)


def every_plan_and_road(sc, kind, road, want_road):
    """A plan made from host items, strided, from device items, or of items that are all a thread's work, on an engine made
    under `road`: the packed launch against the oracle, and the road it reports."""
    rng = np.random.default_rng(311)
    eng, coder = sc.engine(road)
    d_items = None
    if kind == "strided":
        blobs = [pc.inputs(rng, 20000, "uniform") for _ in range(12)]
        b = Batch(eng, blobs, None, eoss=[0x00] * 12)
        plan = eng.plan_strided(True, count=12, in_offset=b.in_offs[0], in_stride=20000, in_len=20000, out_offset=0,
                                out_stride=0, out_capacity=0, first_bit=0, eos_padding=0x00)
    elif kind == "threads":
        blobs = [pc.inputs(rng, int(rng.integers(1, 100)), pc.KINDS[i % 4]) for i in range(4200)]
        b = Batch(eng, blobs, rng, overflows=carried(rng, len(blobs), every=9))
        plan = eng.encode_plan(b.items)
        stats = eng.encode_stats(plan)
        assert stats["by_thread"] == len(blobs), stats
    else:
        blobs = mixed_blobs(rng, with_large=False)
        b = Batch(eng, blobs, rng, overflows=carried(rng, len(blobs)))
        if kind == "host":
            plan = eng.encode_plan(b.items)
        else:
            plan, d_items = eng.encode_plan_from_device_items(b.items)
    try:
        stats = eng.encode_stats(plan)
        # (a plan of items that are all one thread's work has no kernel of the one-pass road to report)
        want = want_road if stats["by_wave"] + stats["by_pieces"] else pc.ROAD_TWO_PASS
        sample = None if len(blobs) < 100 else list(range(0, len(blobs), 7)) + [len(blobs) - 1]
        for align in (1, 8):
            check_launch(sc.oracle, sc.w.ocoder, eng, plan, b.d_in, blobs, sc.lens, b.overflows, b.eoss, align,
                         sample=sample, want_road=want, label="%s/%s" % (kind, road))
    finally:
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        if d_items:
            eng.free(d_items)
        b.close()
        sc.done(eng, coder)


def scan_boundaries(sc, tile, counts):
    """The offset scan in tiles of a few items: item counts of exactly a tile (or a whole number of them), one more, one
    less, a number that is no multiple, more tiles than a workgroup has threads; against numpy's cumulative sum."""
    rng = np.random.default_rng(317 + tile)
    eng, coder = sc.engine()
    most = max(counts)
    blobs = [pc.inputs(rng, int(rng.integers(1, 40)), pc.KINDS[i % 4]) for i in range(most)]
    b = Batch(eng, blobs, None, overflows=carried(rng, most, every=5))
    try:
        with pack_tile_items(sc.lib, tile):
            for n in counts:
                plan = eng.encode_plan(b.items[:n])
                ovs = b.overflows[:n]
                lens = encoded_lengths(sc.lens, blobs[:n], [ov[1] for ov in ovs])
                for align in (1, 16):
                    offsets, total, _, _ = check_launch(
                        sc.oracle, sc.w.ocoder, eng, plan, b.d_in, blobs[:n], sc.lens, ovs, b.eoss[:n], align,
                        sample=list(range(0, n, 97)) + [n - 1], label="tile %d, %d items" % (tile, n))
                    rounded = (lens + align - 1) // align * align
                    assert np.array_equal(offsets[1:], np.cumsum(rounded)) and total == int(rounded.sum())
                eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
    finally:
        b.close()
        sc.done(eng, coder)


def capacity_clipping(sc, road, aligns=(1, 16)):
    """Capacities of nothing, at, just behind and inside every other item's place, one byte short of an item's bytes, and
    around the total: what fits is written as the oracle writes it into that room, the rest reports SHORT_BUFFER."""
    rng = np.random.default_rng(331)
    sizes = [40, 0, 700, TILE + 9, 300, SEG + 1, 2 * SEG + 500, 17, 3 * SEG, 90, 1]
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    eng, coder = sc.engine(road)
    b = Batch(eng, blobs, rng, overflows=carried(rng, len(blobs), every=3))
    plan = eng.encode_plan(b.items)
    try:
        for align in aligns:
            lens = encoded_lengths(sc.lens, blobs, [ov[1] for ov in b.overflows])
            offsets, reserved = expected_offsets(lens, align)
            total = int(offsets[-1])
            caps = [0, total - 1, total + 5]
            for k in (0, 2, 3, 5, 6, 8, 10):
                caps += [int(offsets[k]), int(offsets[k]) + 1, int(offsets[k] + reserved[k] // 2), int(offsets[k] + lens[k]) - 1]
            for cap in sorted(set(c for c in caps if c >= 0)):
                _, _, _, res = check_launch(sc.oracle, sc.w.ocoder, eng, plan, b.d_in, blobs, sc.lens, b.overflows, b.eoss,
                                            align, capacity=cap, label="clip/%s" % road)
                kinds = {r[:2] for r in res}
                if cap < total - 16:
                    assert (-1, harness.AWS_ERROR_SHORT_BUFFER) in kinds, (cap, kinds)
    finally:
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        sc.done(eng, coder)


def coder_with_holes(sc):
    """Symbols 7 and 200 have no code: an item that meets one stops there as in the oracle; the offsets follow the length
    query (0 bits for such a symbol).  Among the items: one whose coded bits fill its room exactly in front of the
    symbol without a code (the reference then asks for room first)."""
    rng = np.random.default_rng(337)
    sizes = [30, 0, 600, TILE + 3, 100, SEG + 40, 2 * SEG + 9, 55, 4000, 12]
    blobs = []
    for i, n in enumerate(sizes):
        blob = pc.inputs(rng, n, pc.KINDS[i % 4])
        blob[blob == 7] = 8
        blob[blob == 200] = 201
        if n and i % 2 == 0:
            blob[int(rng.integers(0, n))] = 7 if i % 4 else 200
        blobs.append(blob)
    eight = int(np.flatnonzero(sc.lens_holes == 8)[0])
    blobs.append(np.asarray([eight, eight, eight, 7], np.uint8))
    blobs.append(np.asarray([200], np.uint8))
    eng, coder = sc.engine(holes=True)
    b = Batch(eng, blobs, rng, overflows=carried(rng, len(blobs), every=5))
    plan = eng.encode_plan(b.items)
    try:
        for align in (1, 4):
            _, _, _, res = check_launch(sc.oracle, sc.w.ocoder_holes, eng, plan, b.d_in, blobs, sc.lens_holes, b.overflows,
                                        b.eoss, align, want_road=pc.ROAD_TWO_PASS, label="holes")
            kinds = {r[:2] for r in res}
            assert (-1, harness.AWS_ERROR_COMPRESSION_UNKNOWN_SYMBOL) in kinds and (0, 0) in kinds, kinds
    finally:
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        sc.done(eng, coder)


def the_plans_own_layout_survives(sc):
    """A plain launch, a packed launch, a plain launch of one plan whose items have room of their own (roomy and too short in
    turn): the third is the first again, record for record and byte for byte."""
    rng = np.random.default_rng(347)
    sizes = [40, 700, TILE + 9, SEG + 1, 0, 2 * SEG + 500, 17]
    blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate(sizes)]
    eng, coder = sc.engine()
    own, pos = [], 5
    for i, blob in enumerate(blobs):
        cap = [2 * blob.size + 8, blob.size // 3][i % 2]  # roomy, and too short
        own.append((pos, cap))
        pos += cap + 3
    b = Batch(eng, blobs, rng, overflows=carried(rng, len(blobs)), own=own)
    plan = eng.encode_plan(b.items)
    d_out = eng.alloc(pos + 64)

    def plain():
        eng.fill(d_out, MARKER, pos + 64)
        eng.encode_launch(plan, b.d_in, d_out)
        return eng.download(d_out, pos + 64), eng.encode_results(plan, len(blobs))

    try:
        first_bytes, first_res = plain()
        for i, blob in enumerate(blobs):  # (the plain launch itself, against the oracle)
            rec, data = oracle_item(sc.oracle, sc.w.ocoder, blob, b.overflows[i], b.eoss[i], own[i][1])
            assert first_res[i] == rec and np.array_equal(first_bytes[own[i][0]:own[i][0] + own[i][1]], data), i
        check_launch(sc.oracle, sc.w.ocoder, eng, plan, b.d_in, blobs, sc.lens, b.overflows, b.eoss, 4, label="between")
        third_bytes, third_res = plain()
        assert third_res == first_res and np.array_equal(third_bytes, first_bytes)
    finally:
        eng.free(d_out)
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        sc.done(eng, coder)


def round_trip_through_a_chained_decode(sc, shape):
    """decode_plan_from_encode behind a packed launch reads at the offsets that launch made, as many bytes as were
    produced -- whatever the items' own out_capacity fields say (here: one byte each, less than anything encodes to)."""
    rng = np.random.default_rng(353)
    if shape == "threads":
        blobs = [pc.inputs(rng, int(rng.integers(1, 90)), pc.KINDS[i % 4]) for i in range(5000)]
    else:
        blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate([70000, 300, 20000, SEG, 1, 140000, 900])]
    n = len(blobs)
    eng, coder = sc.engine()
    b = Batch(eng, blobs, rng, own=[(0, 1)] * n)
    plan = eng.encode_plan(b.items)
    dplan = eng.empty_decode_plan()
    d_back = eng.alloc(b.host_in.size)
    try:
        for align in (1, 16):
            offsets, total, got, _ = check_launch(sc.oracle, sc.w.ocoder, eng, plan, b.d_in, blobs, sc.lens, b.overflows,
                                                  b.eoss, align, sample=list(range(0, n, 53)), label="round trip")
            # (check_launch freed its output: encode again into a buffer that stays, then chain the decode to it)
            d_out, d_off = eng.alloc(total + 64), eng.alloc(8 * (n + 1))
            try:
                assert launch_packed(eng, plan, b.d_in, d_out, total, d_off, align) == (0, 0)
                assert eng.decode_plan_from_encode(dplan, plan)
                stats = eng.decode_stats(dplan)
                assert stats["items"] == n and (stats["by_thread"] == n) == (shape == "threads"), stats
                eng.fill(d_back, MARKER, b.host_in.size)
                eng.decode_launch(dplan, d_out, d_back)
                res = eng.decode_results(dplan, n)
                back = eng.download(d_back, b.host_in.size)
                want = np.full(b.host_in.size, MARKER, np.uint8)
                for i, blob in enumerate(blobs):
                    want[b.in_offs[i]:b.in_offs[i] + blob.size] = blob
                    assert res[i][:3] == (0, 0, blob.size), (i, res[i])
                assert np.array_equal(back, want)
            finally:
                eng.free(d_out)
                eng.free(d_off)
    finally:
        eng.free(d_back)
        eng.lib.aws_huffman_amd_decode_plan_destroy(dplan)
        eng.lib.aws_huffman_amd_encode_plan_destroy(plan)
        b.close()
        sc.done(eng, coder)
