"""ctypes face of include/aws/compression/huffman_amd_packed.h (packed batch encode) and what its tests share: the
expected layout of a packed launch from the code lengths, the oracle's encode of one item into the room that layout gives
it, and one check of a launch against both.  Used by tests/test_emulated_packed.py (emulator build) and
tests/test_gpu_packed.py (MI355X)."""
import ctypes as C

import numpy as np

import harness

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
