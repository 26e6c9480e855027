"""What the sync stage hands the emit stage per sub-chunk (struct hufd_lane_rec, csrc/hip/device_types.h): one 16-byte record
a lane -- three quarter checkpoints, the merged-state / exit word, the symbol count -- that every sync kernel stores once and
every emit kernel loads whole.  The scenarios here are the smallest shapes at which a record can be misplaced, one for every
writer and reader of the array.  Used by tests/test_gpu_lane_record.py (MI355X) and tests/test_emulated_lane_record.py
(emulator build), at the same sizes.

Every scenario is one or more plans through parity_cases.decode_items_like_the_oracle (or the range / locate checks of
tests/ranges_api.py): each item's rc / error / produced / bits consumed as the oracle's decoder has them for the item's own
bytes, first bit and room, every output byte, and the bytes between and around the outputs untouched -- call by call, two
launches a road.  `sc` is a packed_api.Scene of the build under test, bound by ranges_api.bind."""
import numpy as np

import emit_record_cases as er
import index_api as ia
import parity_cases as pc
import ranges_api as ra

CHUNK = er.CHUNK
SUB = 128                        # HUFD_DEC_SUB_BYTES
TAILS = (7, 8, 135, 136, 137)    # bytes behind the last whole chunk: none, one or two sub-chunks for the careful walk
FOLD_CHUNKS = 16                 # whole chunks in front of an end that goes INTO the big kernels' grids (at most one end in eight chunks)


def exact_stream(w, rng, enc_bytes, kind="uniform"):
    """Symbols that encode to exactly enc_bytes bytes (the last code ends in the last byte), and the oracle's bytes."""
    lens = er.code_lengths(w)
    base = pc.inputs(rng, enc_bytes * 8 // int(lens[lens > 0].min()) + 600, kind)
    for drop in range(256):
        data = base[drop:]
        ends = np.cumsum(lens[data])
        n = int(np.searchsorted(ends, enc_bytes * 8, side="right"))
        assert n < data.size
        if n and int(ends[n - 1]) > (enc_bytes - 1) * 8:
            enc = pc.oracle_encode(w, data[:n])
            assert enc.size == enc_bytes, (enc.size, enc_bytes)
            return data[:n].copy(), enc
    raise AssertionError("no stream of this coder ends in byte %d" % enc_bytes)


def whole_lanes(valid):
    """Sub-chunks of a chunk of `valid` bytes that lie inside the stream with 8 bytes behind them (n_full of the kernels)."""
    return min((valid - 8) // SUB, 256) if valid >= 8 else 0


def launch(sc, streams, label, modes=(None,), seed=1, ends=None):
    """ends: (folded, packed, single) -- how the plan says the chunks its streams end in are taken, where the scenario is
    about that."""
    def with_plan(plan, items):
        st = sc.eng.decode_stats(plan)
        got = (st["end_pieces_folded"], st["end_pieces_packed"], st["end_pieces_single"])
        assert ends is None or got == ends, (label, st)

    pc.decode_items_like_the_oracle(sc.w, sc.eng, sc.w.ocoder, streams, np.random.default_rng(seed), label, modes=modes, kinds=1,
                                    with_plan=with_plan)


# ----------------------------------------------------------------------------- a chunk inside a stream, barely
def one_chunk_plus_8(sc, seed=701):
    """32 KiB + 8 bytes: chunk 0 is the shortest chunk that lies INSIDE its stream (all 256 lanes whole, dec_sync_one<false>
    and dec_emit_fast<false> with every record written and read), chunk 1 is eight bytes, one thread's work."""
    data, enc = exact_stream(sc.w, np.random.default_rng(seed), CHUNK + 8)
    assert whole_lanes(enc.size) == 256 and whole_lanes(enc.size - 1) == 255
    launch(sc, [(enc, 0, data.size)], "one chunk + 8", modes=(None, "all-kernels"))


# ----------------------------------------------------------------------------- the one or two lanes a stream ends in
def two_chunks_and_a_tail(sc, tail, seed=709):
    """Two chunks and `tail` bytes.  7: chunk 1 is one its stream ends in with 255 whole lanes, the careful walk is lane 255's
    alone; 8: chunk 1 lies inside the stream, the end is chunk 2's eight bytes; 135: 0 whole lanes behind chunk 1 (a thread's
    work); 136 and 137: one whole lane, the careful walk writes the records of lanes 1 and 2.  The same end behind sixteen whole
    chunks: an end among eight chunks or more goes into the big kernels' grids, where the workgroup's first thread follows the stream
    to its end and writes those records itself -- and, "tails-apart", through kernels of their own."""
    rng = np.random.default_rng(seed + tail)
    last = whole_lanes(tail)
    assert last == {7: 0, 8: 0, 135: 0, 136: 1, 137: 1}[tail]
    data, enc = exact_stream(sc.w, rng, 2 * CHUNK + tail)
    n_ends = 2 if tail < 8 else 1  # (7 bytes: the last whole chunk has fewer than 8 bytes behind it -- an end as well)
    launch(sc, [(enc, 0, data.size)], "two chunks + %d" % tail, modes=(None, "lean-sync"), ends=(0, 0, n_ends))
    data, enc = exact_stream(sc.w, rng, FOLD_CHUNKS * CHUNK + tail)
    launch(sc, [(enc, 0, data.size)], "sixteen chunks + %d" % tail, modes=(None, "tails-apart"), ends=(n_ends, 0, 0))


def entered_inside_a_byte(sc, seed=719):
    """Two chunks and 136 bytes entered 3 and 5 bits into a byte of the stream: lane 0's record holds the entry states that
    reach its walk, and its count runs from the meeting bit on."""
    lens = er.code_lengths(sc.w)
    _, enc = exact_stream(sc.w, np.random.default_rng(seed), 2 * CHUNK + 136 + 5)
    streams = []
    for skip, fb in ((2, 3), (5, 5)):
        part = enc[skip:]
        streams.append((part, fb, er.room_for(sc.w, lens, part)))
    launch(sc, streams, "entry bit")


# ----------------------------------------------------------------------------- several chunks a workgroup
def seventy_items_and_a_long_one(sc, seed=727):
    """70 items of about 2 KiB of encoded bytes (dec_sync_pack and dec_emit_pack: a slot a chunk, records of the whole lanes
    and of the two behind them only), one entered inside a byte, one cut, and a stream of three chunks and as short an end among them;
    "lean-sync": a workgroup a chunk."""
    rng = np.random.default_rng(seed)
    lens = er.code_lengths(sc.w)
    streams = []
    for i in range(70):
        data, enc = er.cut_to(sc.w, lens, pc.inputs(rng, 4000, "uniform"), int(rng.integers(1900, 2200)))
        if i == 11:
            part = enc[1:]
            streams.append((part, 6, er.room_for(sc.w, lens, part)))
        elif i == 23:
            streams.append((enc[:1500], 0, data.size))
        else:
            streams.append((enc, 0, data.size))
        if i == 40:
            data, enc = er.cut_to(sc.w, lens, pc.inputs(rng, 3 * CHUNK * 8 // 5 + 2000, "uniform"), 3 * CHUNK + 2100)
            streams.append((enc, 0, data.size))
    launch(sc, streams, "70 items and a long one", modes=(None, "lean-sync"), ends=(0, 71, 0))


# ----------------------------------------------------------------------------- records written twice
def one_repeated_symbol(sc, seed=733):
    """64 KiB of one symbol of the shortest code: walks that never fall into step.  dec_sync_few writes chunk 0's records
    without checkpoints or counts, dec_sync_true writes them anew behind the scan; as it comes, with every kernel queued, and
    the long way."""
    lens = er.code_lengths(sc.w)
    shortest = int(lens[lens > 0].min())
    sym = int(np.flatnonzero(lens == shortest)[0])
    data, enc = er.cut_to(sc.w, lens, np.full(2 * CHUNK * 8 // shortest + 300, sym, np.uint8), 2 * CHUNK)
    launch(sc, [(enc, 0, data.size)], "one symbol", modes=er.ROADS)


def damaged_and_cut(sc, seed=739):
    """A stream with four bytes of ones in chunk 1 and one cut in the middle of chunk 1: the long way's records (dec_sync,
    dec_emit) for the chunks the stream stops in."""
    rng = np.random.default_rng(seed)
    data, enc = exact_stream(sc.w, rng, 2 * CHUNK + 137)
    damaged = enc.copy()
    damaged[CHUNK + 9000:CHUNK + 9004] = 0xFF
    cut = enc[:CHUNK + 9001]
    launch(sc, [(damaged, 0, data.size), (cut, 0, data.size)], "damaged and cut", modes=(None, "all-kernels"))


# ----------------------------------------------------------------------------- ranges of an indexed stream
def ranges_and_locate(sc, seed=743):
    """100 003 symbols in blocks of 512 (two chunks and an end): positions located across the stream, and symbol ranges inside
    a block, across a chunk boundary and over the whole stream decoded through a plan."""
    n, B = 100_003, 512
    data = ia.data_of(sc, "uniform", n, seed=seed)
    bits = ra.symbol_bits(sc.lens, data)
    st = ia.Stream(sc, sc.eng, sc.lens, sc.w.ocoder, data, B)
    rg = ra.Ranges(st)
    rg.bits = bits
    plan = sc.eng.empty_decode_plan()
    try:
        assert st.enc.size > 2 * CHUNK + 136
        over = int(np.searchsorted(bits, CHUNK * 8))  # the first symbol that starts in chunk 1
        ra.check_locate(sc.eng, st, bits, [0, 1, B - 1, B, over - 1, over, n - 1, n], label="lane records")
        spans = [(over - 3000, 45_000), (0, n), (7 * B + 100, 60), (n - 1, 1), (3 * B - 30, 9000)]
        ranges, at = [], 3
        for s0, count in spans:
            ranges.append((s0, count, at))
            at += count + 3
        assert rg.reset(plan, ranges) == (0, 0)
        rg.check_launch(plan, ranges, at + 64, label="lane records, symbol ranges")
    finally:
        sc.lib.aws_huffman_amd_decode_plan_destroy(plan)
        st.close()
