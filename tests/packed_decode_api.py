"""ctypes face of the packed batch decode in include/aws/compression/huffman_amd_packed.h and what its tests share: the
oracle's decode of one item with room for everything (sym_i) and into the room a layout gives it, the expected layout, and
one check of a launch against both.  Used by tests/test_emulated_packed_decode.py (emulator build) and
tests/test_gpu_packed_decode.py (MI355X).  Nothing here asks the library under test what an item decodes to."""
import ctypes as C

import numpy as np

import harness
import packed_api as pa

MARKER = pa.MARKER  # what the output holds before a launch: gaps and everything behind the total must keep it

RESULT_DTYPE = np.dtype([("rc", "<i4"), ("error", "<i4"), ("produced", "<u8"), ("bits_consumed", "<u8")])
assert RESULT_DTYPE.itemsize == C.sizeof(harness.AmdDecodeResult)


def bind(lib):
    """Declares the decode entry points of huffman_amd_packed.h (and the encode ones: packed_api.bind)."""
    pa.bind(lib)
    V, P = C.c_void_p, C.POINTER
    lib.aws_huffman_amd_decode_plan_launch_packed.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_launch_packed.argtypes = [V, V, V, C.c_uint64, V, C.c_uint32, V]
    lib.aws_huffman_amd_decode_plan_packed_size.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_packed_size.argtypes = [V, P(C.c_uint64), P(C.c_uint64), V]
    lib.aws_huffman_amd_decode_plan_reset_packed_input.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_reset_packed_input.argtypes = [V, V, V, C.c_size_t, V]
    lib.aws_huffman_amd_decode_plan_reset.restype = C.c_int
    lib.aws_huffman_amd_decode_plan_reset.argtypes = [V, P(harness.AmdDecodeItem), C.c_size_t]
    return lib


def launch_packed(eng, plan, d_in, d_out, capacity, d_offsets, align, stream=None):
    """(rc, error)."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_decode_plan_launch_packed(plan, d_in, d_out, int(capacity), d_offsets, align, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def packed_size(eng, plan, stream=None):
    """(rc, error, total_symbols, longest_item_symbols)."""
    total, longest = C.c_uint64(), C.c_uint64()
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_decode_plan_packed_size(plan, C.byref(total), C.byref(longest), stream)
    return rc, eng.lib.aws_last_error() if rc else 0, total.value, longest.value


def reset_packed_input(eng, plan, d_offsets, d_lengths, n, stream=None):
    """(rc, error)."""
    eng.lib.aws_reset_error()
    rc = eng.lib.aws_huffman_amd_decode_plan_reset_packed_input(plan, d_offsets, d_lengths, n, stream)
    return rc, eng.lib.aws_last_error() if rc else 0


def upload_u64(eng, values):
    """The numbers as uint64 in device memory: the caller's to free."""
    arr = np.ascontiguousarray(np.asarray(values, dtype=np.uint64))
    d = eng.alloc(max(arr.nbytes, 8))
    if arr.size:
        eng.upload(d, arr.view(np.uint8))
    return d


def results_array(eng, plan, n):
    """aws_huffman_amd_decode_plan_results as a numpy record array."""
    out = np.zeros(max(n, 1), RESULT_DTYPE)
    assert eng.lib.aws_huffman_amd_decode_plan_results(plan, out.ctypes.data_as(C.POINTER(harness.AmdDecodeResult)), None) == 0
    return out[:n]


def oracle_item(oracle, ocoder, enc, first_bit, cap):
    """aws_huffman_decode of one item (entered at `first_bit` of its first byte: the bits behind it are what a call before
    left in the decoder) into a byte_buf of capacity `cap`: (the record as Engine.decode_results gives it, the `cap` bytes
    with MARKER where nothing was written)."""
    d = oracle.new_decoder(ocoder)
    start = 0
    if first_bit:
        d.working_bits = (int(enc[0]) & (0xFF >> first_bit)) << (56 + first_bit)
        d.num_bits = 8 - first_bit
        start = 1
    dst = np.full(cap + 1, MARKER, np.uint8)
    r = oracle.decode_call(d, np.ascontiguousarray(enc), start, enc.size, dst, 0, cap)
    assert dst[cap] == MARKER
    bits = (8 - first_bit if first_bit else 0) + r.consumed * 8 - r.state[0]
    return (r.rc, r.err, r.produced, bits), dst[:cap]


class Expect:
    """What the oracle says of a batch of (encoded bytes, first bit) streams: sym_i -- the symbols it writes when it never
    runs out of room (8 * bytes / shortest code + 8 is room for everything) --, and record and bytes for that room."""

    def __init__(self, oracle, ocoder, streams, min_bits, only=None):
        self.oracle, self.ocoder, self.streams = oracle, ocoder, streams
        self.full = {}
        for i in (range(len(streams)) if only is None else only):
            enc, fb = streams[i]
            rec, data = oracle_item(oracle, ocoder, enc, fb, enc.size * 8 // max(min_bits, 1) + 8)
            assert rec[:2] in ((0, 0), (-1, harness.AWS_ERROR_COMPRESSION_UNKNOWN_SYMBOL)), (i, rec)
            self.full[i] = (rec, data[:rec[2]].copy())

    def syms(self):
        return np.asarray([self.full[i][0][2] for i in range(len(self.streams))], dtype=np.int64)

    def first(self, n):
        """The same of the batch's first n streams."""
        part = Expect.__new__(Expect)
        part.oracle, part.ocoder, part.streams, part.full = self.oracle, self.ocoder, self.streams[:n], self.full
        return part

    def item(self, i, room):
        """Record and bytes of item i decoded into `room` symbols: all of its own, or none."""
        rec, data = self.full[i]
        if room == rec[2]:
            return rec, data
        assert room == 0
        enc, fb = self.streams[i]
        rec0, data0 = oracle_item(self.oracle, self.ocoder, enc, fb, 0)
        # (what huffman_amd_packed.h promises of an item without room)
        assert rec0 == (-1, harness.AWS_ERROR_SHORT_BUFFER, 0, 0), (i, rec0)
        return rec0, data0


def expected_offsets(syms, align):
    return pa.expected_offsets(syms, align)


def rooms(offsets, syms, cap):
    """The capacity a launch gives each item: sym_i where [offsets[i], offsets[i] + sym_i) lies in front of cap, else 0."""
    syms = np.asarray(syms, dtype=np.int64)
    return np.where(offsets[:-1] + syms <= cap, syms, 0)


def lay_out(streams, rng=None, first=0, align=1):
    """The encoded streams one after the other (a few bytes between them with `rng`; starts rounded up to `align`):
    (host array, offsets)."""
    offs, pos = [], first
    for enc, _ in streams:
        pos = (pos + align - 1) // align * align
        offs.append(pos)
        pos += enc.size + (int(rng.integers(0, 4)) if rng is not None else 0)
    host = np.zeros(pos + 64, np.uint8)
    for (enc, _), o in zip(streams, offs):
        host[o:o + enc.size] = enc
    return host, offs


def check_launch(eng, plan, d_in, expect, align, capacity=None, label="", launches=1):
    """Packed launches of `plan` (its items are expect.streams) against the definition: the offsets, the total and the
    longest reserved length from the oracle's sym_i; every item record for record and byte for byte against the oracle's
    decode into the room the layout gives it; MARKER in the gaps, behind the total and behind the capacity.  capacity
    None: exactly the total.  Returns (offsets, total, got bytes, records)."""
    n = len(expect.streams)
    syms = expect.syms()
    offsets, reserved = expected_offsets(syms, align)
    total = int(offsets[-1])
    cap = total if capacity is None else int(capacity)
    size = max(total, cap) + 64
    room = rooms(offsets, syms, cap)
    want = np.full(size, MARKER, np.uint8)
    recs = []
    for i in range(n):
        rec, data = expect.item(i, int(room[i]))
        recs.append(rec)
        want[int(offsets[i]):int(offsets[i]) + int(room[i])] = data
    d_out, d_off = eng.alloc(size), eng.alloc(8 * (n + 1))
    try:
        for _ in range(launches):
            eng.fill(d_out, MARKER, size)
            eng.fill(d_off, 0xEE, 8 * (n + 1))
            assert launch_packed(eng, plan, d_in, d_out, cap, d_off, align) == (0, 0), label
            got = eng.download(d_out, size)  # (behind the launch on the stream, before any record is read)
            res = eng.decode_results(plan, n)
            got_offsets = pa.download_u64(eng, d_off, n + 1)
            assert np.array_equal(got_offsets, offsets), (label, align, int(np.flatnonzero(got_offsets != offsets)[0]))
            assert packed_size(eng, plan) == (0, 0, total, int(reserved.max()) if n else 0), (label, packed_size(eng, plan), total)
            for i in range(n):
                assert res[i] == recs[i], (label, align, cap, i, int(offsets[i]), int(room[i]), res[i], recs[i])
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (label, align, cap, "first wrong byte at %d" % int(bad[0]))
            assert np.all(got[min(cap, total):] == MARKER), (label, "bytes behind the total or the capacity were written")
        return offsets, total, got, res
    finally:
        eng.free(d_out)
        eng.free(d_off)
