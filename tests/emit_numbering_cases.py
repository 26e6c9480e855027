"""The chunks dec_emit_fast / dec_emit_big take, by every arm that the numbering of the workgroup's threads touches (quarter
first: thread t walks quarter t % 4 of the sub-chunks 2 (t / 4) and 2 (t / 4) + 1, inside a stream as in the chunk a stream
ends in): the loads of the stream's words, the count scan and the lane bases, thread 0's walk through sub-chunk 0's later
quarters, the copy-out.  Used by tests/test_gpu_emit_numbering.py (MI355X) and tests/test_emulated_emit_numbering.py
(emulator build), at the same sizes.

Every scenario is plans of items laid out here (source and output offsets are the scenario's, not drawn): each item's rc /
error / produced / bits consumed as the oracle's decoder has them for the item's own bytes, first bit and room, every output
byte, and the bytes between and around the outputs untouched; two launches a plan.  Where a scenario says so the plan is
QUIET after its results are fetched: no chunk was listed for another kernel, the regular ones took them all.

Streams are three chunks of 32 KiB and an end (about 100 KiB encoded, 85 000 symbols of the test coder): chunks 0 .. 2 lie
inside their stream -- dec_emit_fast<TAIL = false>'s --, the fourth is the one the stream ends in -- <TAIL = true>'s."""
import numpy as np

import emit_record_cases as er
import harness
import parity_cases as pc

CHUNK = er.CHUNK
SUB_BITS = 1024                 # HUFD_DEC_SUB_BYTES * 8
ROW_BITS = 32
QUARTER_ROWS = 8                # rows between two checkpoints of a sub-chunk
ENC_BYTES = 3 * CHUNK + 2100    # three chunks and an end of sixteen whole lanes


def uniform_stream(w, rng, enc_bytes=ENC_BYTES):
    lens = er.code_lengths(w)
    return er.cut_to(w, lens, pc.inputs(rng, enc_bytes * 8 // int(lens[lens > 0].min()) + 300, "uniform"), enc_bytes)


def launch_placed(w, eng, placed, label, quiet=False, modes=(None,)):
    """placed: (encoded bytes, first bit, room, source offset mod 16, output offset mod 16) each; one plan of them all."""
    items, in_pos, out_pos = [], 0, 0
    for enc, fb, cap, in_mod, out_mod in placed:
        items.append(dict(in_offset=in_pos + in_mod, in_len=int(enc.size), first_bit=fb, out_offset=out_pos + out_mod, out_capacity=cap))
        in_pos = (in_pos + in_mod + enc.size + 255) & ~255
        out_pos = (out_pos + out_mod + cap + 16 + 15) & ~15
    host = np.zeros(in_pos + 64, np.uint8)
    want, recs = np.full(out_pos + 64, pc.SENTINEL, np.uint8), []
    for it, (enc, fb, cap, _, _) in zip(items, placed):
        host[it["in_offset"]:it["in_offset"] + enc.size] = enc
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
    d_in, d_out = eng.alloc(host.size), eng.alloc(want.size)
    assert d_in % 16 == 0 and d_out % 16 == 0, "the offsets' low bits are to be the addresses'"
    eng.upload(d_in, host)
    plan = eng.decode_plan(items)
    try:
        for mode in modes:
            with harness.decode_road(eng.lib, mode):
                for launch in range(2):
                    eng.fill(d_out, pc.SENTINEL, want.size)
                    eng.decode_launch(plan, d_in, d_out)
                    got = eng.decode_results(plan, len(items))
                    assert got == recs, (label, mode, launch, got, recs)
                    bad = np.flatnonzero(eng.download(d_out, want.size) != want)
                    assert bad.size == 0, (label, mode, launch, "first wrong byte at %d of %d" % (int(bad[0]), want.size))
                    if quiet:
                        assert eng.decode_plan_is_quiet(plan), (label, mode, launch, "a chunk left the regular kernels")
    finally:
        eng.lib.aws_huffman_amd_decode_plan_destroy(plan)
        eng.free(d_in)
        eng.free(d_out)


# ----------------------------------------------------------------------------- offsets
def source_and_output_offsets(w, eng, seed=601):
    """One stream at source addresses 0, 1 and 15 past a multiple of 16 (the 16-byte loads of a quarter straddle their lines
    or do not), each with its output at a multiple of 16 (chunk 0's rows go out whole: mis = 0) and 5 past one."""
    data, enc = uniform_stream(w, np.random.default_rng(seed))
    placed = [(enc, 0, data.size, in_mod, out_mod) for in_mod in (0, 1, 15) for out_mod in (0, 5)]
    launch_placed(w, eng, placed, "offsets", quiet=True)


def entered_inside_a_byte(w, eng, seed=607):
    """The same stream entered 3 and 7 bits into a byte of it: chunk 0's sub-chunk 0 starts in a state other than 0, which is
    thread 0's to walk from."""
    rng = np.random.default_rng(seed)
    lens = er.code_lengths(w)
    _, enc = uniform_stream(w, rng)
    placed = []
    for skip, fb, in_mod, out_mod in ((2, 3, 1, 5), (5, 7, 0, 0)):
        part = enc[skip:]
        placed.append((part, fb, er.room_for(w, lens, part), in_mod, out_mod))
    launch_placed(w, eng, placed, "entry bit")


# ----------------------------------------------------------------------------- sub-chunk 0 without its first checkpoint
def code_starts(w, bits, at, end):
    """Where the codes of a walk over `bits` from bit `at` start, up to `end`; None: the walk comes to a window that is no code."""
    patterns, lens = w.table
    codes = {(int(lens[s]), int(patterns[s])): s for s in range(256) if int(lens[s])}
    shortest, longest = min(n for n, _ in codes), max(n for n, _ in codes)
    out = []
    while at < end:
        out.append(at)
        window = 0
        for n in range(1, longest + 1):
            window = (window << 1) | int(bits[at + n - 1])
            if n >= shortest and (n, window) in codes:
                at += n
                break
        else:
            return None
    return out


def stream_whose_chunk_1_meets_late(w, seed=613):
    """A uniform stream whose chunk 1 opens with 45 times one symbol of the longest code that, rotated, is a code again: the
    walk dec_sync_one starts at the chunk's bit 0 on a guess and the walk from the chunk's true entry do not stand at the
    same bit at any of the row boundaries 0 .. 8 of sub-chunk 0 (asserted here, from the table), so the sync kernel has no
    first checkpoint for that sub-chunk and dec_emit_fast's thread 0 walks on through its second quarter."""
    rng = np.random.default_rng(seed)
    lens = er.code_lengths(w)
    longest = np.flatnonzero(lens == lens.max())
    base = pc.inputs(rng, ENC_BYTES * 8 // int(lens[lens > 0].min()) + 400, "uniform")
    for drop in range(64):
        data = base[drop:].copy()
        k1 = er.symbols_before_chunk(lens, data, 1)
        state = er.entry_state_of_chunk(lens, data, 1)
        if state == 0:
            continue
        for sym in longest:
            data[k1:k1 + 45] = sym
            cut, enc = er.cut_to(w, lens, data, ENC_BYTES)
            assert er.symbols_before_chunk(lens, cut, 1) == k1 and er.entry_state_of_chunk(lens, cut, 1) == state
            bits = np.unpackbits(enc[CHUNK:CHUNK + SUB_BITS // 8 + 8])
            guess, true = code_starts(w, bits, 0, SUB_BITS), code_starts(w, bits, state, SUB_BITS)
            if guess is None or true is None:
                continue
            guess, true = np.array(guess), np.array(true)
            rows = np.arange(0, 2 * QUARTER_ROWS + 1) * ROW_BITS
            apart = guess[np.searchsorted(guess, rows)] != true[np.searchsorted(true, rows)]
            if apart[:QUARTER_ROWS + 1].all() and not apart[-1]:
                return cut, enc
    raise AssertionError("no stream of this coder keeps chunk 1's guessed walk apart for a quarter")


def missing_first_checkpoint(w, eng):
    """That stream, whole and entered inside a byte: every chunk is the regular kernels' all the same (the plan is quiet)."""
    lens = er.code_lengths(w)
    data, enc = stream_whose_chunk_1_meets_late(w)
    launch_placed(w, eng, [(enc, 0, data.size, 0, 0), (enc, 0, data.size, 15, 5)], "late meeting", quiet=True)
    part = enc[1:]
    launch_placed(w, eng, [(part, 4, er.room_for(w, lens, part), 1, 0)], "late meeting, entry bit")


def lanes_that_never_meet(w, eng):
    """parity_cases.walks_that_never_meet's streams (a stretch of one long code in a long stream, in a wide end and in a narrow
    one), one run length."""
    pc.walks_that_never_meet(w, engine=eng, runs=(260,))


# ----------------------------------------------------------------------------- the stage twice as long
def short_codes_over_the_stage(w):
    """parity_cases.dense_symbols with one chunk inside the stream: 52 429 symbols of five bits, more than dec_emit_fast's
    stage holds and fewer than dec_emit_big's."""
    n = 60_000
    lens = er.code_lengths(w)
    assert CHUNK * 8 // int(lens[lens > 0].min()) + 16 > er.STAGE and CHUNK + 8 <= n * int(lens[lens > 0].min()) // 8 < 2 * CHUNK
    pc.dense_symbols(w, n=n)


# ----------------------------------------------------------------------------- both instantiations in one launch
def long_item_among_short_ones(w, eng, seed=617):
    """One plan: a stream of three chunks and an end, one of the shortest codes (its chunk 1 is dec_emit_big's), and items of a
    few KiB whose only chunk is the one they end in -- narrow ones and a nearly whole one."""
    rng = np.random.default_rng(seed)
    lens = er.code_lengths(w)
    data, enc = uniform_stream(w, rng)
    placed = [(enc, 0, data.size, 1, 5)]
    for k, size in enumerate((300, 4100, CHUNK - 130, 9000, CHUNK + 7)):
        d, e = uniform_stream(w, rng, size)
        placed.append((e, 0, d.size, (0, 15, 1)[k % 3], (5, 0)[k % 2]))
    dense = er.listed_streams(w)["shortest codes"]
    placed.append((dense[0], dense[1], dense[2], 15, 0))
    d, e = uniform_stream(w, rng, 2 * CHUNK + 140)
    placed.append((e, 0, d.size, 0, 5))
    launch_placed(w, eng, placed, "long among short", modes=(None, "all-kernels"))
