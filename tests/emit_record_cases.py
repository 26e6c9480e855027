"""What the scan stage hands the emit stage per chunk (struct hufd_emit_rec, csrc/hip/device_types.h): the record
dec_scan_small / dec_scan_apply write for the state a chunk is truly entered in, dec_sync_true rewrites for its chunks and
dec_emit_fast / dec_emit_big decide from.  Used by tests/test_gpu_emit_record.py (MI355X) and
tests/test_emulated_emit_record.py (emulator build), at the same sizes.

Every scenario is one or more plans through parity_cases.decode_items_like_the_oracle: each item's rc / error / produced /
bits consumed as the oracle's decoder has them for the item's own bytes, first bit and room, every output byte, and the
bytes between and around the outputs untouched -- call by call, two launches a road.

Streams are two chunks of 32 KiB and a tail (about 70 000 encoded bytes): chunk 1 lies inside its stream, the one kind of
chunk whose record dec_emit_fast<TAIL = false> reads; its entry state, its symbol count and the symbols in front of it are
the scan's to find.
"""
import ctypes as C

import numpy as np

import harness
import parity_cases as pc

CHUNK = 32768                # HUFD_DEC_CHUNK_BYTES
STAGE = 34304                # HUFD_DEC_STAGE_BYTES: the symbols dec_emit_fast's stage holds
ENC_BYTES = 2 * CHUNK + 4500  # two chunks and a tail
ROADS = (None, "all-kernels", "long-way")


def code_lengths(w):
    return np.array([w.table[1][i] for i in range(256)], dtype=np.int64)


def cut_to(w, lens, data, enc_bytes=ENC_BYTES):
    """The first symbols of `data` that encode to enc_bytes or a few bits less, and the oracle's bytes for them."""
    n = int(np.searchsorted(np.cumsum(lens[data]), enc_bytes * 8, side="right"))
    assert n < data.size, "not enough symbols for %d bytes" % enc_bytes
    data = data[:n].copy()
    enc = pc.oracle_encode(w, data)
    assert enc_bytes - 2 <= enc.size <= enc_bytes, enc.size
    return data, enc


def starts(lens, data):
    """Bit at which every symbol's code starts, and the bit behind the last."""
    return np.concatenate([[0], np.cumsum(lens[data])])


def entry_state_of_chunk(lens, data, chunk):
    """Bits of the code that straddles the chunk's first byte which lie inside the chunk: the state the chunk is entered in."""
    at = starts(lens, data)
    return int(at[np.searchsorted(at, chunk * CHUNK * 8, side="left")]) - chunk * CHUNK * 8


def symbols_before_chunk(lens, data, chunk):
    """Symbols whose code starts in front of the chunk: chunk_base of the chunk."""
    return int(np.searchsorted(starts(lens, data)[:-1], chunk * CHUNK * 8, side="left"))


def room_for(w, lens, enc):
    """Room for whatever a stream of these bytes decodes to, entered at any bit."""
    return enc.size * 8 // int(lens[lens > 0].min()) + 8


# ----------------------------------------------------------------------------- every entry state of a chunk inside a stream
def every_entry_state(w, eng, seed=401):
    """Uniform bytes, two chunks and a tail.  For every state s = 0 .. n_states - 1 of the coder (n_states = its longest
    code, at least 8): (a) a stream whose chunk 1 is entered in state s -- found by dropping symbols from the front until the
    code lengths say so, asserted here from numpy's running sum --, entered at bit 0; (b) one stream entered k = s bits into
    its first byte (bytes k // 8, bit k % 8: an item's first bit is below 8), as first_bit_offsets and streams_out_of_step
    enter theirs.  The record's s0, its merged bit and the count of sub-chunk 0 that follows from it are different in each."""
    rng = np.random.default_rng(seed)
    lens = code_lengths(w)
    n_states = max(int(lens.max()), 8)
    base = pc.inputs(rng, ENC_BYTES * 8 // int(lens[lens > 0].min()) + 300, "uniform")
    by_state = {}
    for drop in range(256):
        s = entry_state_of_chunk(lens, base[drop:], 1)
        by_state.setdefault(s, drop)
        if len(by_state) == int(lens.max()):
            break
    # (a code of the longest length can lie across the chunk's first byte with all but one of its bits inside the chunk)
    assert sorted(by_state) == list(range(int(lens.max()))), sorted(by_state)
    streams = []
    for s in range(int(lens.max())):
        data, enc = cut_to(w, lens, base[by_state[s]:])
        assert entry_state_of_chunk(lens, data, 1) == s
        streams.append((enc, 0, data.size))
    data, enc = cut_to(w, lens, base)
    for k in range(n_states):
        part = enc[k // 8:]
        streams.append((part, k % 8, room_for(w, lens, part)))
    pc.decode_items_like_the_oracle(w, eng, w.ocoder, streams, rng, "every entry state", kinds=1)


# ----------------------------------------------------------------------------- the lists
def listed_streams(w, seed=409):
    """{name: (encoded bytes, first bit, room)}: the four streams whose chunk 1 leaves dec_emit_fast's common path."""
    rng = np.random.default_rng(seed)
    lens = code_lengths(w)
    shortest = int(lens[lens > 0].min())
    short = np.flatnonzero(lens == shortest)
    out = {}
    # one symbol short of room inside chunk 1: the chunk's symbols do not all fit (the slow list), by exactly one
    data, enc = cut_to(w, lens, pc.inputs(rng, ENC_BYTES * 8 // shortest + 300, "uniform"))
    before_2 = symbols_before_chunk(lens, data, 2)
    assert symbols_before_chunk(lens, data, 1) < before_2 - 1
    out["one symbol short in chunk 1"] = (enc, 0, before_2 - 1)
    out["room to the end of chunk 1"] = (enc, 0, before_2)  # (the same chunk with the one symbol more: it fits)
    # the shortest codes only: more symbols in a chunk than the stage holds (the dense list, dec_emit_big)
    data, enc = cut_to(w, lens, short[rng.integers(0, short.size, ENC_BYTES * 8 // shortest + 300)].astype(np.uint8))
    assert symbols_before_chunk(lens, data, 2) - symbols_before_chunk(lens, data, 1) + 16 > STAGE
    out["shortest codes"] = (enc, 0, data.size)
    # one symbol over and over: walks that never fall into step (dec_sync_few lists the chunk, dec_sync_true writes its records)
    data, enc = cut_to(w, lens, np.full(ENC_BYTES * 8 // shortest + 300, short[0], np.uint8))
    out["one symbol"] = (enc, 0, data.size)
    # damage in chunk 1: four bytes of ones, which no code of the table is
    data, enc = cut_to(w, lens, pc.inputs(rng, ENC_BYTES * 8 // shortest + 300, "printable"))
    enc = enc.copy()
    enc[CHUNK + 9000:CHUNK + 9004] = 0xFF
    out["damaged in chunk 1"] = (enc, 0, data.size)
    return out


def the_lists(w, eng, name, seed=419):
    """One of listed_streams, as it comes and under the two road switches that take listed chunks other ways."""
    stream = listed_streams(w)[name]
    pc.decode_items_like_the_oracle(w, eng, w.ocoder, [stream], np.random.default_rng(seed), name, modes=ROADS, kinds=1)


LISTED = ["one symbol short in chunk 1", "room to the end of chunk 1", "shortest codes", "one symbol", "damaged in chunk 1"]


# ----------------------------------------------------------------------------- a stream scanned in runs
def stream_scanned_in_runs(w, eng, seed=431):
    """One stream of 67 chunks (above HUFD_SCAN_SMALL_MAX: dec_scan_runs / dec_scan_apply write the records, a thread a chunk
    behind the sixteen chains), entered inside its first byte, with a stretch of one symbol in its middle (chunks whose
    records dec_sync_true rewrites behind the scan), and the same bytes with damage behind that (chunks the stream does not
    reach)."""
    rng = np.random.default_rng(seed)
    lens = code_lengths(w)
    shortest = int(lens[lens > 0].min())
    short = np.flatnonzero(lens == shortest)
    data = np.concatenate([pc.inputs(rng, 30 * CHUNK * 8 // 7, "uniform"), np.full(4 * CHUNK * 8 // shortest, short[0], np.uint8),
                           pc.inputs(rng, 40 * CHUNK * 8 // shortest, "uniform")])
    _, enc = cut_to(w, lens, data, 66 * CHUNK + 5000)
    part = enc[2:]
    damaged = part.copy()
    damaged[60 * CHUNK + 77:60 * CHUNK + 81] = 0xFF
    room = room_for(w, lens, part)
    streams = [(part, 5, room), (damaged, 5, room)]
    pc.decode_items_like_the_oracle(w, eng, w.ocoder, streams, rng, "scanned in runs", modes=(None, "all-kernels"), kinds=1)


# ----------------------------------------------------------------------------- stale records
def three_streams_and_a_refill(w, eng, seed=421):
    """One plan object: three streams at odd offsets, each entered inside its first byte (first chunks with an entry bit);
    launched, refilled with a different plan (one stream of the shortest codes and one of one symbol: other chunk counts,
    other entry states, other bases in the same records), launched, refilled with the three streams, launched again.  Every
    launch's records and bytes are the oracle's."""
    rng = np.random.default_rng(seed)
    lens = code_lengths(w)
    shortest = int(lens[lens > 0].min())
    lib = eng.lib
    three = []
    for kind, first_bit, skip in (("uniform", 3, 1), ("printable", 5, 2), ("uniform", 7, 3)):
        _, enc = cut_to(w, lens, pc.inputs(rng, ENC_BYTES * 8 // shortest + 300, kind))
        part = enc[skip:]
        three.append((part, first_bit, room_for(w, lens, part)))
    listed = listed_streams(w)
    other = [listed["shortest codes"], listed["one symbol"]]

    def lay_out(streams, first):
        items, in_pos, out_pos = [], first, 5
        for enc, fb, cap in streams:
            items.append(dict(in_offset=in_pos, in_len=int(enc.size), first_bit=fb, out_offset=out_pos, out_capacity=cap))
            in_pos += enc.size + 3   # (odd offsets: 1, then whatever the odd lengths make)
            out_pos += cap + 7
        host = np.zeros(in_pos + 64, np.uint8)
        for it, (enc, _, _) in zip(items, streams):
            host[it["in_offset"]:it["in_offset"] + enc.size] = enc
        want, recs = np.full(out_pos + 64, pc.SENTINEL, np.uint8), []
        for it, (enc, fb, cap) in zip(items, streams):
            d = w.oracle.new_decoder(w.ocoder)
            start = 0
            if fb:  # (parity_cases.decode_items_like_the_oracle: the rest of the first byte is what a call before left)
                d.working_bits = (int(enc[0]) & (0xFF >> fb)) << (56 + fb)
                d.num_bits = 8 - fb
                start = 1
            dst = np.full(cap + 1, pc.SENTINEL, np.uint8)
            r = w.oracle.decode_call(d, enc, start, enc.size, dst, 0, cap)
            recs.append((r.rc, r.err, r.produced, (8 - fb if fb else 0) + r.consumed * 8 - r.state[0]))
            want[it["out_offset"]:it["out_offset"] + cap] = dst[:cap]
        d_in = eng.alloc(host.size)
        eng.upload(d_in, host)
        return items, d_in, want, recs

    sides = {"three": lay_out(three, 1), "other": lay_out(other, 3)}
    plan = eng.empty_decode_plan()
    lib.aws_huffman_amd_decode_plan_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    try:
        for step, side in enumerate(("three", "other", "three")):
            items, d_in, want, recs = sides[side]
            assert lib.aws_huffman_amd_decode_plan_reset(plan, eng._decode_item_array(items), len(items)) == 0, (step, side)
            d_out = eng.alloc(want.size)
            try:
                eng.fill(d_out, pc.SENTINEL, want.size)
                eng.decode_launch(plan, d_in, d_out)
                assert eng.decode_results(plan, len(items)) == recs, (step, side)
                bad = np.flatnonzero(eng.download(d_out, want.size) != want)
                assert bad.size == 0, (step, side, "first wrong byte at %d of %d" % (int(bad[0]), want.size))
            finally:
                eng.free(d_out)
    finally:
        lib.aws_huffman_amd_decode_plan_destroy(plan)
        for _, d_in, _, _ in sides.values():
            eng.free(d_in)
