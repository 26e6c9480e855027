"""ctypes face of the packed batch decode in include/aws/compression/huffman_amd_packed.h and what its tests share: the
oracle's decode of one item with room for everything (sym_i) and into the room a layout gives it, the expected layout, and
one check of a launch against both.  Used by tests/test_emulated_packed_decode.py (emulator build) and
tests/test_gpu_packed_decode.py (MI355X).  Nothing here asks the library under test what an item decodes to.  Below the
faces: the decode scenarios, run alike by both test files on a packed_api.Scene, at the same sizes."""
import ctypes as C

import numpy as np

import coder_shapes as cs
import harness
import packed_api as pa
import parity_cases as pc

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


# ----------------------------------------------------------------------------- the decode scenarios (emulator and MI355X alike)
CHUNK = 32768      # HUFD_DEC_CHUNK_BYTES
LARGE = pa.LARGE   # HUFD_SCAN_SMALL_MAX chunks: above it the workgroup scan
INVALID = (-1, harness.AWS_ERROR_INVALID_ARGUMENT)
UNKNOWN = (-1, harness.AWS_ERROR_COMPRESSION_UNKNOWN_SYMBOL)
SHORT = (-1, harness.AWS_ERROR_SHORT_BUFFER)
EOS = (0x00, 0xFF, 0x20)  # paddings: of the test coder's codes none is all zeros or all ones, 0x20 starts with a five-bit one
DECODE_PLAN_KINDS = ["host", "strided", "device", "packed-input", "packed-input-lengths", "threads", "from-encode"]
DECODE_ROADS = ["long-way", "lean-sync", "tails-apart", "all-kernels"]
OTHER_CODERS = ["from_lengths 4..12", "hpack_lengths", "len8", "len9"]


class Batch:
    """(encoded bytes, first bit) streams in device memory and the oracle's word on them.  The items' own out_offset /
    out_capacity are whatever `own` says (default: no room at all -- a packed launch must not look at them)."""

    def __init__(self, sc, streams, rng, own=None, eng=None, ocoder=None, min_bits=None, align=1):
        self.eng, self.streams = eng or sc.eng, streams
        n = len(streams)
        self.host_in, self.in_offs = lay_out(streams, rng, first=1 if rng is not None else 0, align=align)
        self.d_in = self.eng.alloc(self.host_in.size)
        self.eng.upload(self.d_in, self.host_in)
        own = own or [(0, 0)] * n
        self.items = [dict(in_offset=self.in_offs[i], in_len=int(streams[i][0].size), first_bit=streams[i][1],
                           out_offset=own[i][0], out_capacity=own[i][1]) for i in range(n)]
        self.expect = Expect(sc.oracle, ocoder or sc.w.ocoder, streams, min_bits or sc.min_bits)

    def close(self):
        self.eng.free(self.d_in)


def with_first_bits(rng, streams, every=3):
    """Every third stream entered inside its first byte (the bits in front of it are the call before's)."""
    return [(enc, int(rng.integers(1, 8)) if i % every == 1 and enc.size else 0) for i, enc in enumerate(streams)]


def mixed_streams(sc, rng, with_large=True):
    """Encoded lengths 0, 1, a few bytes, around 512 and 768 (a thread's and a wave's), around one chunk, several chunks,
    more than HUFD_SCAN_SMALL_MAX chunks; paddings 0x00, 0xFF and 0x20 (which spells a symbol of the test coder) in turn."""
    targets = [0, 1, 5, 40, 500, 512, 520, 760, 768, 775, 3000, CHUNK - 9, CHUNK, CHUNK + 5, 0, 3 * CHUNK + 77, 5 * CHUNK + 4]
    if with_large:
        targets.append((LARGE + 1) * CHUNK + 300)
    encs = [sc.encoded(t, EOS[i % 3], rng, pc.KINDS[i % 4]) if t else np.zeros(0, np.uint8) for i, t in enumerate(targets)]
    return with_first_bits(rng, encs)


def mixed_batch(sc):
    """Empty items up to one above HUFD_SCAN_SMALL_MAX chunks in one plan, every third entered inside its first byte, at
    three alignments."""
    rng = np.random.default_rng(501)
    streams = mixed_streams(sc, rng)
    b = Batch(sc, streams, rng)
    plan = sc.eng.decode_plan(b.items)
    try:
        stats = sc.eng.decode_stats(plan)
        assert stats["by_thread"] and stats["by_wave"] and stats["by_pieces"] and stats["empty"], stats
        # padding spells symbols for some items and none for others: sym_i is not the length of the text
        for align in (1, 4, 16):
            _, _, _, res = check_launch(sc.eng, plan, b.d_in, b.expect, align, label="mixed")
            assert all(r[:2] == (0, 0) for r, (_, fb) in zip(res, streams) if fb == 0), res  # (whole streams from bit 0)
    finally:
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        b.close()


def every_way_a_plan_is_made(sc, kind):
    """Host items, strided, device items, a packed input without and with lengths, items that are all a thread's work, and a
    plan chained to a packed encode launch: two packed decode launches each at two alignments against the oracle."""
    rng = np.random.default_rng(511)
    eng = sc.eng
    d_extra, enc_plan = [], None
    if kind == "strided":
        # equal items a stride apart: the shorter streams run on into the ones (no code) behind them
        encs = [sc.encoded(int(rng.integers(20000, 20400)), EOS[i % 3], rng) for i in range(12)]
        longest = max(e.size for e in encs)
        streams = [(np.concatenate([e, np.full(longest - e.size, 0xFF, np.uint8)]), 0) for e in encs]
        b = Batch(sc, streams, None)
        plan = eng.plan_strided(False, count=12, in_offset=b.in_offs[0], in_stride=longest, in_len=longest, out_offset=0,
                                out_stride=0, out_capacity=0, first_bit=0, eos_padding=0)
    elif kind == "threads":
        encs = [pc.oracle_encode(sc.w, pc.inputs(rng, int(rng.integers(1, 90)), pc.KINDS[i % 4]), eos=EOS[i % 3])
                for i in range(4300)]
        b = Batch(sc, with_first_bits(rng, encs, every=7), rng)
        plan = eng.decode_plan(b.items)
        assert eng.decode_stats(plan)["by_thread"] == len(encs)
    elif kind == "from-encode":
        blobs = [pc.inputs(rng, n, pc.KINDS[i % 4]) for i, n in enumerate([70000, 300, 20000, 16384, 1, 140000, 900, 0])]
        host_in, in_offs = pa.lay_out(blobs, rng, first=1)
        d_plain = eng.alloc(host_in.size)
        eng.upload(d_plain, host_in)
        d_extra.append(d_plain)
        enc_plan = eng.encode_plan([dict(in_offset=in_offs[i], in_len=int(blobs[i].size), out_offset=0, out_capacity=0,
                                         eos_padding=EOS[i % 3]) for i in range(len(blobs))])
        d_enc_off = eng.alloc(8 * (len(blobs) + 1))
        d_extra.append(d_enc_off)
        assert pa.launch_packed(eng, enc_plan, d_plain, None, 0, d_enc_off, 4) == (0, 0)
        total = pa.packed_size(eng, enc_plan)[2]
        d_enc = eng.alloc(total + 64)
        assert pa.launch_packed(eng, enc_plan, d_plain, d_enc, total, d_enc_off, 4) == (0, 0)
        offs = pa.download_u64(eng, d_enc_off, len(blobs) + 1)
        produced = [r[3] for r in eng.encode_results(enc_plan, len(blobs))]
        host_enc = eng.download(d_enc, total + 64)
        streams = [(host_enc[int(o):int(o) + int(p)].copy(), 0) for o, p in zip(offs[:-1], produced)]
        b = Batch.__new__(Batch)
        b.eng, b.streams, b.d_in = eng, streams, d_enc
        b.expect = Expect(sc.oracle, sc.w.ocoder, streams, sc.min_bits)
        plan = eng.empty_decode_plan()
        assert eng.decode_plan_from_encode(plan, enc_plan)
    elif kind.startswith("packed-input"):
        streams = mixed_streams(sc, rng, with_large=False)
        streams = [(enc, 0) for enc, _ in streams]  # (such a plan enters every item at bit 0)
        with_lengths = kind.endswith("lengths")
        b = Batch(sc, streams, None, align=8 if with_lengths else 1)
        if with_lengths:
            d_offs, d_lens = upload_u64(eng, b.in_offs), upload_u64(eng, [e.size for e, _ in streams])
            d_extra += [d_offs, d_lens]
        else:
            assert all(b.in_offs[i] + streams[i][0].size == b.in_offs[i + 1] for i in range(len(streams) - 1))
            d_offs, d_lens = upload_u64(eng, b.in_offs + [b.in_offs[-1] + streams[-1][0].size]), None
            d_extra.append(d_offs)
        plan = eng.empty_decode_plan()
        assert reset_packed_input(eng, plan, d_offs, d_lens, len(streams)) == (0, 0)
        stats = eng.decode_stats(plan)
        assert stats["items"] == len(streams) and stats["by_pieces"] and stats["by_thread"], stats
    else:
        streams = mixed_streams(sc, rng, with_large=False)
        b = Batch(sc, streams, rng)
        if kind == "host":
            plan = eng.decode_plan(b.items)
        else:
            plan, d_items = eng.decode_plan_from_device_items(b.items)
            d_extra.append(d_items)
    try:
        for align in (1, 8):
            check_launch(eng, plan, b.d_in, b.expect, align, label=kind, launches=2)
        if kind.startswith("packed-input"):
            # the items' own room is none: a plain launch of such a plan reports SHORT_BUFFER for every item with a symbol
            eng.decode_launch(plan, b.d_in, None)
            for r, sym in zip(eng.decode_results(plan, len(b.streams)), b.expect.syms()):
                assert (r[:3] == SHORT + (0,)) == (sym > 0), (r, sym)
    finally:
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        if enc_plan:
            sc.lib.aws_huffman_amd_encode_plan_destroy(enc_plan)
        for d in d_extra:
            eng.free(d)
        b.close()


def decode_road_switches(sc, road):
    """The mixed batch and seventy short end-of-stream chunks under one of the decode-road switches, and once more behind it."""
    rng = np.random.default_rng(521)
    streams = mixed_streams(sc, rng, with_large=False)
    # many short end-of-stream chunks as well: the kernels that share a workgroup between them, or do not
    streams += with_first_bits(rng, [sc.encoded(int(rng.integers(900, 2500)), EOS[i % 3], rng) for i in range(70)])
    b = Batch(sc, streams, rng)
    plan = sc.eng.decode_plan(b.items)
    try:
        with harness.decode_road(sc.lib, road):
            for align in (1, 16):
                check_launch(sc.eng, plan, b.d_in, b.expect, align, label=road, launches=2)
        check_launch(sc.eng, plan, b.d_in, b.expect, 1, label="after " + road)
    finally:
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        b.close()


def scan_boundaries(sc, tile, counts):
    """The offset scan in tiles of a few items: item counts of exactly a tile (or a whole number of them), one more, one
    less, a number that is no multiple, more tiles than a workgroup has threads; against numpy's cumulative sum of the
    oracle's symbol counts."""
    rng = np.random.default_rng(523 + tile)
    most = max(counts)
    encs = [pc.oracle_encode(sc.w, pc.inputs(rng, int(rng.integers(0, 40)), pc.KINDS[i % 4]), eos=EOS[i % 3])
            for i in range(most)]
    b = Batch(sc, [(e, 0) for e in encs], None)
    all_syms = b.expect.syms()
    try:
        with pa.pack_tile_items(sc.lib, tile):
            for n in counts:
                plan = sc.eng.decode_plan(b.items[:n])
                for align in (1, 16):
                    offsets, total, _, _ = check_launch(sc.eng, plan, b.d_in, b.expect.first(n), align,
                                                        label="tile %d, %d items" % (tile, n))
                    rounded = (all_syms[:n] + align - 1) // align * align
                    assert np.array_equal(offsets[1:], np.cumsum(rounded)) and total == int(rounded.sum())
                sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
    finally:
        b.close()


def early_stops(sc, rng):
    """Streams that stop before their end: damaged (a window without a code, 32 bits or more in front of the end), cut
    inside a code, arbitrary bytes; of a thread's, a wave's, a chunk's and several chunks' length."""
    streams = []
    for i, target in enumerate([60, 300, 700, 2000, 9000, CHUNK + 900, 2 * CHUNK + 50, 4 * CHUNK + 7000]):
        enc = sc.encoded(target, EOS[i % 3], rng)
        damaged = enc.copy()
        at = int(rng.integers(0, max(enc.size - 12, 1)))
        damaged[at:at + 4] = 0xFF  # ten one bits: no code of the test coder
        streams += [damaged, enc[:int(rng.integers(enc.size // 2, enc.size))], rng.integers(0, 256, target, dtype=np.uint8)]
        late = enc.copy()
        late[-2:] = 0xFF  # ... and one fewer than 32 bits in front of the end: no error, the walk just ends there
        streams.append(late)
    return with_first_bits(rng, streams, every=5)


def streams_that_stop_early(sc):
    """early_stops() in one plan: UNKNOWN_SYMBOL items shorten the layout, and the launch says by how much."""
    rng = np.random.default_rng(541)
    b = Batch(sc, early_stops(sc, rng), rng)
    plan = sc.eng.decode_plan(b.items)
    try:
        for align in (1, 4):
            _, _, _, res = check_launch(sc.eng, plan, b.d_in, b.expect, align, label="early stops", launches=2)
            kinds = {r[:2] for r in res}
            assert UNKNOWN in kinds and (0, 0) in kinds, kinds
            # a stream cut inside a code: success, and fewer bits consumed than it has
            assert any(r[:2] == (0, 0) and r[3] < 8 * s[0].size - s[1] for r, s in zip(res, b.streams))
            assert all(r[2] == sym for r, sym in zip(res, b.expect.syms()))
    finally:
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        b.close()


def capacity_clipping(sc, road, aligns=(1, 16)):
    """Capacities of nothing, at, just behind, inside and at the end of every other item's place, and around the total: an
    item gets all of its room or none."""
    rng = np.random.default_rng(547)
    targets = [40, 0, 700, 6000, 300, CHUNK + 1, 2 * CHUNK + 500, 17, 3 * CHUNK, 90, 1]
    encs = [sc.encoded(t, EOS[i % 3], rng) if t else np.zeros(0, np.uint8) for i, t in enumerate(targets)]
    damaged = encs[6].copy()
    damaged[CHUNK + 40:CHUNK + 44] = 0xFF
    encs[6] = damaged
    b = Batch(sc, with_first_bits(rng, encs, every=4), rng)
    plan = sc.eng.decode_plan(b.items)
    syms = b.expect.syms()
    try:
        with harness.decode_road(sc.lib, road):
            for align in aligns:
                offsets, _ = expected_offsets(syms, align)
                total = int(offsets[-1])
                caps = [0, total - 1, total + 5]
                for k in (0, 2, 3, 5, 6, 8, 10):
                    caps += [int(offsets[k]), int(offsets[k]) + 1, int(offsets[k] + syms[k] // 2), int(offsets[k] + syms[k]) - 1,
                             int(offsets[k] + syms[k])]
                for cap in sorted(set(c for c in caps if c >= 0)):
                    _, _, _, res = check_launch(sc.eng, plan, b.d_in, b.expect, align, capacity=cap, label="clip/%s" % road)
                    for i, r in enumerate(res):
                        fits = offsets[i] + syms[i] <= cap
                        if not fits and syms[i]:  # (no partial room: nothing produced, nothing consumed)
                            assert r == SHORT + (0, 0), (cap, i, r)
                        elif not fits:  # (an item without symbols: the reference's answer for no room, never SHORT_BUFFER)
                            assert r[:2] in ((0, 0), UNKNOWN) and r[2] == 0, (cap, i, r)
                        else:
                            assert r[2] == syms[i] and r[:2] in ((0, 0), UNKNOWN), (cap, i, r)
    finally:
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        b.close()


def shaped_coders(sc, name):
    """(oracle coder, product coder, code lengths)."""
    if name == "from_lengths 4..12":
        lengths = cs.shape(*cs.LEN4TO12)
        patterns, lens = pc.canonical_code(lengths)
        oc = sc.oracle.lib.oracle_table_coder_new((C.c_uint32 * 256)(*patterns), (C.c_uint8 * 256)(*lens))
        pcoder = sc.lib.aws_huffman_amd_table_coder_from_lengths((C.c_uint8 * 256)(*lengths))
        assert oc and pcoder
        return oc, pcoder, lengths
    return pc.profile_coders(sc.w, name)


def other_coders(sc, name):
    """A coder built from lengths of 4 to 12 bits (the chunk kernels, tables of 12 bits), one with HPACK's lengths of 5 to
    30 bits (linked tables: items a thread, a workgroup, or blocks across the chip each; plans from device sources are
    made through the host) and coders with codes of one length (no walk at all; len9: half the windows without a code)."""
    rng = np.random.default_rng(557)
    oc, pcoder, lengths = shaped_coders(sc, name)
    coded = np.flatnonzero(np.asarray(lengths))
    min_bits = int(min(l for l in lengths if l))
    eng = harness.Engine(sc.lib, pcoder)
    encs = []
    for i, n in enumerate([0, 1, 30, 200, 700, 1500, 9000, 40_000, 100_000, 300_000]):
        plain = coded[rng.integers(0, coded.size, n)].astype(np.uint8)
        enc = sc.oracle.encode_all(oc, plain, eos_padding=EOS[i % 3], slack=64 + 4 * n)
        encs.append(enc)
        if n >= 700:
            cut = enc[:int(rng.integers(enc.size // 2, enc.size))]
            noisy = enc.copy()
            at = int(rng.integers(0, enc.size - 8))
            noisy[at:at + 6] = rng.integers(0, 256, 6, dtype=np.uint8)
            encs += [cut, noisy]
    streams = with_first_bits(rng, encs, every=4)
    b = Batch(sc, streams, rng, eng=eng, ocoder=oc, min_bits=min_bits)
    plan = eng.decode_plan(b.items)
    d_extra = []
    try:
        with harness.decode_road(sc.lib, None):
            sc.lib.aws_huffman_amd_testing_set_wide_min_bytes(60_000)  # (the long items of HPACK's lengths across the chip)
            for align in (1, 8):
                check_launch(eng, plan, b.d_in, b.expect, align, label=name, launches=2)
            total = int(expected_offsets(b.expect.syms(), 8)[0][-1])
            check_launch(eng, plan, b.d_in, b.expect, 8, capacity=total // 2, label=name + " clipped")
            # ... and the same streams as a packed input
            flat = [(enc, 0) for enc, _ in streams]
            fb = Batch(sc, flat, None, eng=eng, ocoder=oc, min_bits=min_bits)
            d_offs = upload_u64(eng, fb.in_offs + [fb.in_offs[-1] + flat[-1][0].size])
            d_extra += [d_offs, fb.d_in]
            assert reset_packed_input(eng, plan, d_offs, None, len(flat)) == (0, 0)
            check_launch(eng, plan, fb.d_in, fb.expect, 4, label=name + " packed input")
    finally:
        sc.lib.aws_huffman_amd_testing_set_wide_min_bytes(0)
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        for d in d_extra:
            eng.free(d)
        b.close()
        eng.close()
        sc.lib.aws_huffman_amd_table_coder_destroy(pcoder)


def the_plans_own_layout_survives(sc):
    """A plain launch, a packed launch, a plain launch of one plan whose items have room of their own (roomy, too short and
    exact in turn): the third is the first again."""
    rng = np.random.default_rng(563)
    streams = mixed_streams(sc, rng, with_large=False) + early_stops(sc, rng)[:8]
    expect = Expect(sc.oracle, sc.w.ocoder, streams, sc.min_bits)
    own, pos = [], 5
    for i, sym in enumerate(expect.syms()):
        cap = [int(sym) + 8, int(sym) // 3, int(sym)][i % 3]  # roomy, too short, exact
        own.append((pos, cap))
        pos += cap + 3
    b = Batch(sc, streams, rng, own=own)
    eng = sc.eng
    plan = eng.decode_plan(b.items)
    d_out = eng.alloc(pos + 64)

    def plain():
        eng.fill(d_out, MARKER, pos + 64)
        eng.decode_launch(plan, b.d_in, d_out)
        return eng.download(d_out, pos + 64), eng.decode_results(plan, len(streams))

    try:
        first_bytes, first_res = plain()
        for i, (enc, fb) in enumerate(streams):  # (the plain launch itself, against the oracle)
            rec, data = oracle_item(sc.oracle, sc.w.ocoder, enc, fb, own[i][1])
            assert first_res[i] == rec and np.array_equal(first_bytes[own[i][0]:own[i][0] + own[i][1]], data), i
        assert SHORT in {r[:2] for r in first_res}
        check_launch(eng, plan, b.d_in, b.expect, 4, label="between")
        third_bytes, third_res = plain()
        assert third_res == first_res and np.array_equal(third_bytes, first_bytes)
    finally:
        eng.free(d_out)
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        b.close()
