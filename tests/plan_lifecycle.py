"""One plan through every fill, launch and road in turn (include/aws/compression/huffman_amd*.h: "a plan is built to be
kept") and what its tests share.  Used by tests/test_emulated_plan_lifecycle.py (emulator build) and
tests/test_gpu_plan_lifecycle.py (MI355X): every run_* scenario below takes a packed_api.Scene and is called by both, at the
same sizes.

A decode plan can be filled seven ways (FILL_KINDS), an encode plan three (ENC_FILL_KINDS); between two fills a plan keeps
its arena (entries of earlier, larger fills stay behind the current counts), its list counters and summary, `quiet`,
`chained`, `packed` / `packed_sized`, the located bits of a range fill and the widths of its stream ends; an encode plan
keeps the block its one-pass kernels want clear, laid out by the CURRENT fill's segment and item counts.  The scenarios
here keep ONE plan and walk it through fills of every kind and shape, launches of every kind and the roads back.

Expected values never come from the library under test: records and bytes are the oracle's (packed_api.oracle_item,
packed_decode_api.oracle_item) for the item's own bytes and room, offsets numpy's cumulative sums, a range's output the
data's own slice.  Every step fills the output with MARKER and compares the whole buffer (guard bytes and the gaps between
items included), compares every item's record, and compares *_plan_stats with a plan freshly made (*_plan_new) from the same
items on the host.  One exception, said where it is made: a decode plan chained to an encode launch whose items are all a
thread's work never learns the items' lengths, so its statistics count an empty item as a thread's and give the bound it
was made under as `thread_limit`.

Shapes are the smallest that reach each class of csrc/hip/device_types.h, and every shape asserts its class through the
statistics (Shape.check_class): one that lands in another class fails the test.

  decode (encoded bytes)                                          encode (symbols)
  T  300 items of 0 .. 120 B, some empty: a thread each           S0t  50 items of 100: a thread each, no segment
  W  60 items of 129 .. 768 B: a wave each                        S0s  5 items of 3 000: a wave each where the engine encodes in
  C  40 items of 1 .. 3 chunks of 32 KiB: ends single                  one pass (no segment), a segment each elsewhere
  P  70 items of a chunk and a narrow end (at most 83 whole       S2   20 000: two segments       S3   40 000: three
     lanes of 128 B): 70 ends packed                              S67  66 * 16 384 + 5: 67 segments (above HUFD_SCAN_SMALL_MAX)
  L  one item of 66 chunks (above HUFD_SCAN_SMALL_MAX): runs      MIX  all of these and an empty item
  L+ one of 150 chunks: growth over everything before it (P has 140)
  X  T + W + C + L in shuffled order
"""
import ctypes as C

import numpy as np

import harness
import index_api as ia
import packed_api as pa
import packed_decode_api as pda
import parity_cases as pc
import ranges_api as ra

MARKER = pa.MARKER
CHUNK, SUB, SEG = pda.CHUNK, 128, pa.SEG
SCAN_SMALL_MAX = pa.LARGE            # HUFD_SCAN_SMALL_MAX
THREAD_BYTES = 128                   # HUFD_TINY_FEW_BYTES: the class that always goes to a thread
WAVE_BYTES = 768                     # HUFD_DEC_COOP_BYTES
PACK_LANES, PACK_MIN = 83, 64        # HUFD_DEC_PACK_LANES, HUFD_DEC_PACK_MIN_CHUNKS
NARROW_END = 8 + PACK_LANES * SUB    # the most bytes of a last chunk with at most PACK_LANES whole lanes (and 127 more)
INVALID = pda.INVALID

FILL_KINDS = ["reset", "strided", "device_items", "from_encode", "packed_input", "block_ranges", "symbol_ranges"]
ANY_SHAPE = ("reset", "device_items")  # fills that take items of any lengths, offsets and first bits
BIG_KINDS = ANY_SHAPE + ("strided",)   # ... and the ones L and L+ go through
STREAM_SYMBOLS = 300_000


def blob_for(sc, rng, target, kind):
    """Symbols of `kind` that encode to `target` bytes or at most two fewer (numpy's running sum of the code lengths)."""
    if target == 0:
        return np.zeros(0, np.uint8)
    plain = pc.inputs(rng, target * 8 // sc.min_bits + 8, kind)
    n = int(np.searchsorted(np.cumsum(sc.lens[plain]), target * 8, side="right"))
    return plain[:n].copy()


class Shape:
    """Symbols and what the oracle encodes them to (padding 0xFF, nothing carried: of the test coder's codes none is all
    ones, so a stream entered at bit 0 decodes to exactly its symbols)."""

    def __init__(self, sc, name, blobs, encs=None):
        self.name, self.blobs = name, blobs
        self.encs = encs or [pc.oracle_encode(sc.w, b, eos=0xFF) if b.size else np.zeros(0, np.uint8) for b in blobs]

    def check_class(self, stats, n_empty=None, label=""):
        """The class the shape is there for, from a plan's statistics."""
        n, kind = stats["items"], self.name.rstrip("=")
        empty = sum(1 for e in self.encs if e.size == 0) if n_empty is None else n_empty
        assert stats["empty"] == empty, (label, stats)
        if kind == "T":
            assert stats["by_thread"] == n - empty and stats["pieces"] == 0 and stats["thread_limit"] == THREAD_BYTES, (label, stats)
            assert n_empty is not None or self.name == "T=" or empty >= 3, (label, empty)
        elif kind == "W":
            assert stats["by_wave"] == n and stats["pieces"] == 0, (label, stats)
        elif kind == "C":
            assert stats["by_pieces"] == n and n <= stats["pieces"] <= 3 * n, (label, stats)
            assert stats["end_pieces_packed"] == 0 and stats["end_pieces_folded"] == 0 and stats["end_pieces_single"] >= n, (label, stats)
        elif kind == "P":
            assert stats["by_pieces"] == n and stats["pieces"] == 2 * n and stats["end_pieces_packed"] == n >= PACK_MIN, (label, stats)
        elif kind in ("L", "L+"):
            assert stats["by_pieces"] == 1 and stats["pieces"] == {"L": 66, "L+": 150}[kind] > SCAN_SMALL_MAX, (label, stats)
        elif kind == "X":
            assert stats["by_thread"] and stats["by_wave"] and stats["by_pieces"] > 40 and stats["pieces"] > 66 + 40, (label, stats)


def make_shapes(sc):
    rng = np.random.default_rng(1201)
    kinds = pc.KINDS[:4]
    out = {}
    targets = [int(t) for t in rng.integers(1, 121, 300)]
    for i in (0, 17, 101, 250, 299):
        targets[i] = 0
    targets[5], targets[6] = 120, 1
    out["T"] = Shape(sc, "T", [blob_for(sc, rng, t, kinds[i % 4]) for i, t in enumerate(targets)])
    targets = [131, 768, 132, 767] + [int(t) for t in rng.integers(131, 769, 56)]
    out["W"] = Shape(sc, "W", [blob_for(sc, rng, t, kinds[i % 4]) for i, t in enumerate(targets)])
    targets = [CHUNK + 5, 2 * CHUNK + 5, 3 * CHUNK, CHUNK - 9, CHUNK, 2 * CHUNK - 300, 800, 2 * CHUNK + 9000]
    targets += [int(t) for t in rng.integers(800, 70_000, 32)]
    out["C"] = Shape(sc, "C", [blob_for(sc, rng, t, kinds[i % 4]) for i, t in enumerate(targets)])
    targets = [CHUNK + 200, CHUNK + NARROW_END - 2] + [CHUNK + int(t) for t in rng.integers(200, NARROW_END - 2, 68)]
    out["P"] = Shape(sc, "P", [blob_for(sc, rng, t, kinds[i % 2]) for i, t in enumerate(targets)])
    out["L"] = Shape(sc, "L", [blob_for(sc, rng, 65 * CHUNK + 5000, "uniform")])
    out["L+"] = Shape(sc, "L+", [blob_for(sc, rng, 149 * CHUNK + 300, "uniform")])
    order = rng.permutation(300 + 60 + 40 + 1)
    blobs = out["T"].blobs + out["W"].blobs + out["C"].blobs + out["L"].blobs
    encs = out["T"].encs + out["W"].encs + out["C"].encs + out["L"].encs
    out["X"] = Shape(sc, "X", [blobs[i] for i in order], [encs[i] for i in order])
    # what a quiet plan is made of (parity_cases.quiet_plans at n = 150 000): ordinary streams list nothing
    out["Q"] = Shape(sc, "Q", [pc.inputs(rng, m, "uniform") for m in (150_000, 50_000, 40_000)])
    for name in ("T", "W", "C", "P"):  # equal items a stride apart: the shorter streams run on into ones (no code)
        longest = max(e.size for e in out[name].encs)
        out[name + "="] = Shape(sc, name + "=", out[name].blobs,
                                [np.concatenate([e, np.full(longest - e.size, 0xFF, np.uint8)]) for e in out[name].encs])
    for name, sh in out.items():
        sizes = np.asarray([e.size for e in sh.encs])
        lo, hi = {"T": (0, 120), "W": (129, WAVE_BYTES), "C": (WAVE_BYTES + 1, 3 * CHUNK), "P": (CHUNK + 8, CHUNK + NARROW_END),
                  "L": (65 * CHUNK + 1, 66 * CHUNK), "L+": (149 * CHUNK + 1, 150 * CHUNK)}.get(name, (0, 1 << 40))
        assert sizes.min() >= lo and sizes.max() <= hi, (name, int(sizes.min()), int(sizes.max()))
    return out


class Filled:
    """What a fill of one kind with one shape comes to, in the terms every check needs: the device input a launch reads,
    the items as a host plan would be given them, each item's own bytes and first bit, and how to fill a plan so."""

    def __init__(self, kind, shape, d_in, items, streams, out_size, apply, align=None):
        self.kind, self.shape, self.d_in, self.items, self.streams = kind, shape, d_in, items, streams
        self.out_size, self.apply, self.align = out_size, apply, align
        self.stats = self.want = self.recs = self.expect = None
        self.label = "%s/%s" % (kind, shape.name)


class Life:
    """One decode plan on the scene's engine, the shapes, and every (fill kind, shape) made once and kept: device inputs,
    the oracle's records and bytes, the statistics of a fresh plan of the same items."""

    def __init__(self, sc):
        self.sc, self.eng, self.lib = sc, sc.eng, sc.lib
        self.shapes = make_shapes(sc)
        self.plan = self.eng.empty_decode_plan()
        self.fills, self.owned, self.enc_plans, self.streams = {}, [], [], {}
        self.data = ia.data_of(sc, "uniform", STREAM_SYMBOLS, seed=1203)
        self.bits = ra.symbol_bits(sc.lens, self.data)

    def close(self):
        self.lib.aws_huffman_amd_decode_plan_destroy(self.plan)
        for p in self.enc_plans:
            self.lib.aws_huffman_amd_encode_plan_destroy(p)
        for d in self.owned:
            self.eng.free(d)
        for st in self.streams.values():
            st.close()

    def device(self, arr):
        arr = np.ascontiguousarray(arr).view(np.uint8).ravel()
        d = self.eng.alloc(max(arr.size, 8))
        if arr.size:
            self.eng.upload(d, arr)
        self.owned.append(d)
        return d

    def stream(self, block_symbols):
        if block_symbols not in self.streams:
            self.streams[block_symbols] = ia.Stream(self.sc, self.eng, self.sc.lens, self.sc.w.ocoder, self.data, block_symbols)
        return self.streams[block_symbols]

    # ------------------------------------------------------------------ the seven ways
    def fill(self, kind, name):
        key = (kind, name)
        if key not in self.fills:
            if kind == "device_items":
                host = self.fill("reset", name)
                d_items = self.device(np.frombuffer(self.eng._decode_item_array(host.items), dtype=np.uint8))
                f = Filled(kind, host.shape, host.d_in, host.items, host.streams, host.out_size,
                           lambda plan, n=len(host.items): self.lib.aws_huffman_amd_decode_plan_reset_device_items(plan, d_items, n, None))
            else:
                f = getattr(self, "_fill_" + kind)(name)
            self.finish(f)
            self.fills[key] = f
        return self.fills[key]

    def finish(self, f):
        """The oracle's word on the items, and the statistics of a fresh plan of them."""
        sc = self.sc
        f.want = np.full(f.out_size, MARKER, np.uint8)
        f.recs = []
        for it, (enc, fb) in zip(f.items, f.streams):
            rec, data = pda.oracle_item(sc.oracle, sc.w.ocoder, enc, fb, it["out_capacity"])
            f.recs.append(rec)
            f.want[it["out_offset"]:it["out_offset"] + it["out_capacity"]] = data
        fresh = self.eng.decode_plan(f.items)
        f.stats = self.eng.decode_stats(fresh)
        self.lib.aws_huffman_amd_decode_plan_destroy(fresh)
        if f.shape.name != "Q":
            f.shape.check_class(f.stats, n_empty=None if f.kind in ANY_SHAPE + ("from_encode", "packed_input") else
                                sum(1 for it in f.items if it["in_len"] == 0), label=f.label)

    def _fill_reset(self, name):
        sc, sh = self.sc, self.shapes[name]
        rng = np.random.default_rng(1210 + len(name) + ord(name[0]))
        streams = pda.with_first_bits(rng, sh.encs) if len(sh.encs) > 3 else [(e, 0) for e in sh.encs]
        host_in, in_offs = pda.lay_out(streams, rng, first=1)
        items, pos = [], 5
        for i, ((enc, fb), blob) in enumerate(zip(streams, sh.blobs)):
            # (a stream entered inside its first byte decodes to whatever the oracle says: room for the most that can be)
            sym = int(blob.size) if fb == 0 else enc.size * 8 // sc.min_bits + 8
            cap = sym + 8 if len(streams) <= 3 else [sym + 8, sym, sym + 8, sym // 3, sym + 1][i % 5]  # roomy, exact, too short
            if name == "Q":  # (room for the densest stream of that many bytes: what run_listed_then_clean loads)
                cap = enc.size * 8 // sc.min_bits + 9
            items.append(dict(in_offset=in_offs[i], in_len=int(enc.size), first_bit=fb, out_offset=pos, out_capacity=cap))
            pos += cap + 3
        arr = self.eng._decode_item_array(items)
        return Filled("reset", sh, self.device(host_in), items, streams, pos + 64,
                      lambda plan: self.lib.aws_huffman_amd_decode_plan_reset(plan, arr, len(items)))

    def _fill_strided(self, name):
        sh = self.shapes[name if name in ("L", "L+") else name + "="]
        n, length = len(sh.encs), int(sh.encs[0].size)
        assert all(e.size == length for e in sh.encs)
        cap = max(int(b.size) for b in sh.blobs) + 8
        streams = [(e, 0) for e in sh.encs]
        host_in = np.concatenate([np.zeros(16, np.uint8)] + sh.encs + [np.zeros(64, np.uint8)])
        items = [dict(in_offset=16 + i * length, in_len=length, first_bit=0, out_offset=3 + i * (cap + 3), out_capacity=cap)
                 for i in range(n)]
        desc = harness.StridedItems(count=n, in_offset=16, in_stride=length, in_len=length, out_offset=3, out_stride=cap + 3,
                                    out_capacity=cap, first_bit=0, eos_padding=0)
        return Filled("strided", sh, self.device(host_in), items, streams, 3 + n * (cap + 3) + 64,
                      lambda plan: self.lib.aws_huffman_amd_decode_plan_reset_strided(plan, C.byref(desc), None))

    def _encode_side(self, sh, own):
        """The shape's symbols in device memory and an encode plan of them on the scene's engine (padding 0xFF, nothing
        carried; out_offset / out_capacity as `own` says)."""
        rng = np.random.default_rng(1220)
        host_in, in_offs = pa.lay_out(sh.blobs, rng, first=1)
        items = [dict(in_offset=in_offs[i], in_len=int(b.size), out_offset=own[i][0], out_capacity=own[i][1], eos_padding=0xFF)
                 for i, b in enumerate(sh.blobs)]
        plan = self.eng.encode_plan(items)
        self.enc_plans.append(plan)
        return host_in, in_offs, self.device(host_in), plan

    def _fill_from_encode(self, name):
        """Chained to a plain encode launch of the shape's symbols: the decode plan reads what that launch wrote, where it
        wrote it, and writes the symbols back where they came from.  T: every item's room is its encoded length, at most
        128 bytes, so the chained plan is one of threads (made without a look at the lengths)."""
        sh = self.shapes[name]
        own, pos = [], 2
        for e in sh.encs:
            cap = int(e.size) + (0 if name == "T" else 5)
            own.append((pos, cap))
            pos += cap + 2
        host_in, in_offs, d_plain, enc_plan = self._encode_side(sh, own)
        d_enc = self.eng.alloc(pos + 64)
        self.owned.append(d_enc)
        items = [dict(in_offset=own[i][0], in_len=int(e.size), first_bit=0, out_offset=in_offs[i], out_capacity=int(sh.blobs[i].size))
                 for i, e in enumerate(sh.encs)]

        def apply(plan):
            self.eng.encode_launch(enc_plan, d_plain, d_enc)
            return 0 if self.eng.decode_plan_from_encode(plan, enc_plan) else -1

        return Filled("from_encode", sh, d_enc, items, [(e, 0) for e in sh.encs], host_in.size, apply)

    def _fill_packed_input(self, name):
        """The offsets a packed encode launch wrote (checked against numpy's running sum of the oracle's lengths, as the
        bytes are against the oracle's) are the decode plan's input; T: rounded to 8, with the lengths beside them."""
        sc, sh, eng = self.sc, self.shapes[name], self.eng
        n, with_lengths = len(sh.encs), name == "T"
        align = 8 if with_lengths else 1
        lens = np.asarray([e.size for e in sh.encs], dtype=np.int64)
        offsets, _ = pa.expected_offsets(lens, align)
        total = int(offsets[-1])
        host_in, in_offs, d_plain, enc_plan = self._encode_side(sh, [(0, 0)] * n)
        d_enc, d_off = eng.alloc(total + 64), eng.alloc(8 * (n + 1))
        self.owned += [d_enc, d_off]
        eng.fill(d_enc, 0, total + 64)
        assert pa.launch_packed(eng, enc_plan, d_plain, d_enc, total, d_off, align) == (0, 0)
        assert np.array_equal(pa.download_u64(eng, d_off, n + 1), offsets), name
        want = np.zeros(total + 64, np.uint8)
        for o, e in zip(offsets, sh.encs):
            want[int(o):int(o) + e.size] = e
        assert np.array_equal(eng.download(d_enc, total + 64), want), name
        d_lens = self.device(lens.astype(np.uint64)) if with_lengths else None
        items = [dict(in_offset=int(offsets[i]), in_len=int(lens[i]), first_bit=0, out_offset=0, out_capacity=0) for i in range(n)]
        f = Filled("packed_input", sh, d_enc, items, [(e, 0) for e in sh.encs], 64,
                   lambda plan: self.lib.aws_huffman_amd_decode_plan_reset_packed_input(plan, d_off, d_lens, n, None), align=4)
        return f

    def _ranges(self, name, by_blocks):
        """(stream, ranges): T and W from blocks of 64, C and P from blocks of 16 384."""
        rng = np.random.default_rng(1230 + ord(name[0]) + by_blocks)
        n, bits = STREAM_SYMBOLS, self.bits
        st = self.stream(64 if name in ("T", "W") else 16_384)
        if by_blocks:
            nb = st.nb
            spans = {"T": [(int(b), 1) for b in rng.integers(0, nb, 296)] + [(5, 0), (nb, 0), (nb - 1, 1), (0, 1)],
                     "W": [(int(b), int(c)) for b, c in zip(rng.integers(0, nb - 9, 60), rng.integers(4, 9, 60))],
                     "C": [(int(b), int(c)) for b, c in zip(rng.integers(0, nb - 4, 38), rng.integers(1, 5, 38))] + [(nb - 1, 1), (nb - 3, 3)],
                     "P": [(i % (nb - 2), 2) for i in range(70)]}[name]
        else:
            def chunk_and_end(s0, end):  # as many symbols from s0 on as make one chunk and `end` bytes (or a few bits less)
                return int(np.searchsorted(bits, int(bits[s0]) - int(bits[s0]) % 8 + 8 * (CHUNK + end), side="right")) - 1 - s0
            spans = {"T": [(int(s), int(c)) for s, c in zip(rng.integers(0, n - 90, 296), rng.integers(1, 91, 296))] + [(n, 0), (7, 0), (n - 1, 1), (0, 1)],
                     "W": [(int(s), int(c)) for s, c in zip(rng.integers(0, n - 610, 60), rng.integers(210, 611, 60))],
                     "C": [(int(s), int(c)) for s, c in zip(rng.integers(0, n - 58_000, 39), rng.integers(1_300, 58_001, 39))] + [(n - 30_000, 30_000)],
                     "P": [(int(s), chunk_and_end(int(s), int(e))) for s, e in zip(rng.integers(0, n - 40_000, 70), rng.integers(200, NARROW_END - 8, 70))]}[name]
        ranges, at = [], 3
        for first, count in spans:
            ranges.append((first, count, at))
            at += (st.item(first, count)[2] if by_blocks else count) + 3
        return st, ranges, at + 64

    def _fill_ranges(self, name, by_blocks):
        st, ranges, out_size = self._ranges(name, by_blocks)
        rg = ra.Ranges(st)
        rg.bits = self.bits
        items, streams = [], []
        for first, count, out_off in ranges:
            enc, fb, cap, syms = st.item(first, count) if by_blocks else rg.item(first, count)
            start = int(st.index[first] if by_blocks else self.bits[first]) // 8
            items.append(dict(in_offset=st.enc_offset + start if count else 0, in_len=int(enc.size), first_bit=fb,
                              out_offset=out_off, out_capacity=cap))
            streams.append((enc, fb))
        if by_blocks:
            d_ranges = st.upload_ranges(ranges)
            apply = lambda plan: ia.reset_block_ranges(self.eng, plan, st.d_index, st.n, st.B, st.enc_offset, st.enc.size, d_ranges, len(ranges))[0]
        else:
            d_ranges = rg.upload(ranges)
            apply = lambda plan: ra.reset_symbol_ranges(self.eng, plan, st.d_enc, st.d_index, st.n, st.B, st.enc_offset, st.enc.size, d_ranges, len(ranges))[0]
        f = Filled("block_ranges" if by_blocks else "symbol_ranges", self.shapes[name], st.d_enc, items, streams, out_size, apply)
        f.block_symbols = st.B
        # (a range's output is the data's own slice: the oracle's bytes for the range's encoded bytes must be that)
        f.slices = [(out_off, self.data[first * st.B:min((first + count) * st.B, st.n)] if by_blocks else self.data[first:first + count])
                    for first, count, out_off in ranges]
        return f

    def _fill_block_ranges(self, name):
        return self._fill_ranges(name, True)

    def _fill_symbol_ranges(self, name):
        return self._fill_ranges(name, False)

    # ------------------------------------------------------------------ the checks of a step
    def refill(self, f, plan=None):
        """Fills the plan; its statistics are those of a fresh plan of the same items."""
        plan = plan or self.plan
        assert f.apply(plan) == 0, (f.label, self.lib.aws_last_error())
        got = self.eng.decode_stats(plan)
        if f.kind == "from_encode" and f.shape.name == "T":
            # made without a look at the lengths: every item a thread's (an empty one as well), under the bound it was made by
            assert got["items"] == got["by_thread"] == f.stats["items"] and got["pieces"] == got["by_wave"] == got["empty"] == 0, (f.label, got)
            assert max(it["in_len"] for it in f.items) <= got["thread_limit"] <= THREAD_BYTES, (f.label, got)
        else:
            assert got == f.stats, (f.label, got, f.stats)
        assert not self.eng.decode_plan_is_quiet(plan), f.label
        assert pda.packed_size(self.eng, plan)[:2] == INVALID, f.label  # (no packed launch of these items yet)
        return f

    def compare(self, f, got, res, label):
        for i, rec in enumerate(f.recs):
            assert res[i] == rec, (label, i, f.items[i], res[i], rec)
        bad = np.flatnonzero(got != f.want)
        assert bad.size == 0, (label, "first wrong byte at %d of %d" % (int(bad[0]), got.size))
        for out_off, syms in getattr(f, "slices", ()):
            assert np.array_equal(got[out_off:out_off + syms.size], syms), (label, out_off)

    def plain(self, f, label="", launches=1, plan=None):
        """Plain launches (no fetch between them), one fetch: the whole output and every record the oracle's, for the
        items' own room."""
        eng, plan = self.eng, plan or self.plan
        d_out = eng.alloc(f.out_size)
        try:
            eng.fill(d_out, MARKER, f.out_size)
            for _ in range(launches):
                eng.decode_launch(plan, f.d_in, d_out)
            got = eng.download(d_out, f.out_size)
            res = eng.decode_results(plan, len(f.items))
        finally:
            eng.free(d_out)
        self.compare(f, got, res, "%s %s" % (f.label, label))

    def packed(self, f, align=4, label="", capacity=None):
        """A packed launch into dense output: offsets, sizes, every byte and record (packed_decode_api.check_launch)."""
        if f.expect is None:
            f.expect = pda.Expect(self.sc.oracle, self.sc.w.ocoder, f.streams, self.sc.min_bits)
        return pda.check_launch(self.eng, self.plan, f.d_in, f.expect, align, capacity=capacity, label="%s %s" % (f.label, label))

    def step(self, kind, name, label=""):
        f = self.refill(self.fill(kind, name))
        self.plain(f, label)
        if kind == "packed_input":  # (such a plan's items have no room of their own: the launch that is of use is the packed one)
            self.packed(f, f.align, label)
        return f


# ----------------------------------------------------------------------------- 1: every ordered pair of fill kinds
def euler_tour(nodes, rng):
    """A walk over the complete digraph with loops on `nodes` that takes every edge once (Hierholzer): len(nodes)^2 + 1 stops."""
    out_edges = {a: [nodes[i] for i in rng.permutation(len(nodes))] for a in nodes}
    stack, walk = [nodes[int(rng.integers(0, len(nodes)))]], []
    while stack:
        if out_edges[stack[-1]]:
            stack.append(out_edges[stack[-1]].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def decode_tour(seed=1249):
    """[(fill kind, shape)] x 50: every ordered pair of fill kinds once; L first and again behind two small shapes, L+ (more
    chunks than anything before it) in front of the first X, X and P at least three times, the sizes going up and down."""
    rng = np.random.default_rng(seed)
    while True:
        kinds = euler_tour(FILL_KINDS, rng)
        big = [i for i, k in enumerate(kinds) if i > 5 and k in BIG_KINDS]
        any_shape = [i for i, k in enumerate(kinds) if i > 5 and k in ANY_SHAPE]
        if kinds[0] in BIG_KINDS and kinds[3] in BIG_KINDS and big and len([i for i in any_shape if i > big[0]]) >= 3:
            break
    shapes = {0: "L", 1: "T", 2: "W", 3: "L", big[0]: "L+"}
    later = [i for i in any_shape if i > big[0]]
    for i in (later[0], later[len(later) // 2], later[-1]):
        shapes[i] = "X"
    small = 0
    for i in range(len(kinds)):
        if i not in shapes:
            shapes[i] = ("P", "T", "C", "W", "T", "W", "C")[small % 7]
            small += 1
    return [(k, shapes[i]) for i, k in enumerate(kinds)]


def check_tour(tour):
    """What the issue asks of the tour, computed from the tour itself."""
    pairs = {(a[0], b[0]) for a, b in zip(tour, tour[1:])}
    assert len(tour) >= 50 and pairs == {(a, b) for a in FILL_KINDS for b in FILL_KINDS}, sorted(pairs)
    names = [s for _, s in tour]
    assert names[0] == "L" and names[1] in ("T", "W") and names[2] in ("T", "W") and names[3] == "L"
    assert names.count("P") >= 3 and names.count("X") >= 3 and names.count("L+") == 1
    assert names.index("L+") < names.index("X")


def run_decode_tour(life, start=0, stop=None):
    """Fill, launch, fetch, compare, fifty times on one plan (steps start .. stop - 1 of the tour: the emulator side takes it
    in two halves, one behind the other on the same plan; a second half whose first half was not run to its end on this
    plan takes the whole tour)."""
    tour = decode_tour()
    check_tour(tour)
    if start and getattr(life, "tour", {"next": -1})["next"] != start:
        start = 0  # (the steps in front were not taken on this plan, or not to their end: the tour from its first step)
    if start == 0:
        life.tour = {"most": 0, "blocks": {"block_ranges": set(), "symbol_ranges": set()}, "next": 0}
    stop = len(tour) if stop is None else stop
    for i, (kind, name) in enumerate(tour[start:stop], start):
        f = life.step(kind, name, "step %d" % i)
        if name == "L+":
            assert f.stats["pieces"] > life.tour["most"], "L+ is no growth over what came before it"
        life.tour["most"] = max(life.tour["most"], f.stats["pieces"])
        if kind in life.tour["blocks"]:
            life.tour["blocks"][kind].add(f.block_symbols)
        life.tour["next"] = i + 1
    if stop == len(tour):
        assert life.tour["blocks"] == {"block_ranges": {64, 16_384}, "symbol_ranges": {64, 16_384}}, life.tour["blocks"]


# ----------------------------------------------------------------------------- 2: launch kinds and roads between fills
def run_launch_kinds(life):
    """Plain, packed into dense output, plain again; a packed size query, the sizes, the packed launch; two plain launches
    and one fetch -- each broken by a refill of another kind and shape.  After a refill aws_huffman_amd_decode_plan_packed_size
    is refused until a packed launch has been made (Life.refill asserts it); after a packed launch, a refill and a plain
    launch the results are reported against the items' own capacities (Life.plain compares them with the oracle's for that
    room)."""
    eng, plan = life.eng, life.plan
    f = life.refill(life.fill("reset", "C"))
    life.plain(f, "plain")
    life.packed(f, 4, "packed")
    life.plain(f, "plain again")
    life.step("symbol_ranges", "W", "behind a packed launch")
    # the size query: NULL output, no capacity -- offsets and sizes, every item with a symbol short of room
    f = life.refill(life.fill("device_items", "P"))
    if f.expect is None:
        f.expect = pda.Expect(life.sc.oracle, life.sc.w.ocoder, f.streams, life.sc.min_bits)
    syms = f.expect.syms()
    offsets, reserved = pda.expected_offsets(syms, 16)
    d_off = eng.alloc(8 * (len(syms) + 1))
    try:
        assert pda.launch_packed(eng, plan, f.d_in, None, 0, d_off, 16) == (0, 0)
        assert pda.packed_size(eng, plan) == (0, 0, int(offsets[-1]), int(reserved.max()))
        assert np.array_equal(pa.download_u64(eng, d_off, len(syms) + 1), offsets)
        res = eng.decode_results(plan, len(syms))
        for i, s in enumerate(syms):  # (the oracle's record for no room at all)
            assert res[i] == f.expect.item(i, 0)[0], (f.label, i, int(s), res[i], f.expect.item(i, 0)[0])
    finally:
        eng.free(d_off)
    life.packed(f, 16, "behind the size query")
    life.step("strided", "T", "behind a packed launch")
    life.step("from_encode", "C", "behind a strided fill")
    f = life.refill(life.fill("strided", "C"))
    life.plain(f, "two launches, one fetch", launches=2)
    life.step("block_ranges", "P", "behind two launches")
    f = life.refill(life.fill("packed_input", "W"))
    life.packed(f, 1, "packed only")
    life.step("reset", "T", "behind a packed launch of a packed input")


def run_roads(life, road):
    """A launch under one of the decode-road switches, and a plain one behind it, of X and of P, a refill of another kind
    and shape between them."""
    for kind, name, other in (("device_items", "X", ("block_ranges", "T")), ("reset", "P", ("from_encode", "W"))):
        f = life.refill(life.fill(kind, name))
        with harness.decode_road(life.lib, road):
            life.plain(f, road)
        life.plain(f, "behind " + road)
        life.step(other[0], other[1], "behind " + road)


QUIET_VARIANTS = ["one symbol", "short codes", "damage", "bytes"]


def quiet_variant(life, kind):
    """parity_cases.quiet_plans' streams that list chunks, of the lengths of Q's: one symbol over and over (walks that never
    fall into step), the shortest codes only (more symbols in a chunk than the emit stage holds), damage, arbitrary bytes."""
    sc, q = life.sc, life.shapes["Q"]
    rng = np.random.default_rng(1260 + QUIET_VARIANTS.index(kind))
    short = np.flatnonzero(sc.lens == sc.lens[sc.lens > 0].min())
    out = [e.copy() for e in q.encs]

    def of_length(data, size):
        enc = pc.oracle_encode(sc.w, data, eos=0xFF)
        assert enc.size >= size
        return enc[:size].copy()

    if kind == "one symbol":
        out[0] = of_length(np.full(out[0].size * 8 // 5 + 8, short[0], np.uint8), out[0].size)
    elif kind == "short codes":
        out[1] = of_length(short[rng.integers(0, short.size, out[1].size * 8 // 5 + 8)].astype(np.uint8), out[1].size)
    elif kind == "damage":
        out[0][out[0].size // 2:out[0].size // 2 + 4] = 0xFF
    else:
        out[2] = rng.integers(0, 256, out[2].size, dtype=np.uint8)
    return out


def run_listed_then_clean(life, kind):
    """The plan over Q, quiet; the same lengths with other bytes that list chunks (they go the long way, the fetch says so,
    the kernels are back); clean bytes again (quiet again); a refill of another kind and shape and back: not quiet until a
    fetched launch of the clean bytes."""
    eng, plan, sc = life.eng, life.plan, life.sc
    life.step("device_items", "X", "arrays larger than anything below")
    f = life.refill(life.fill("reset", "Q"))
    assert f.stats["by_pieces"] == 3, f.stats
    host_in = eng.download(f.d_in, f.items[-1]["in_offset"] + f.items[-1]["in_len"])
    clean = Filled("reset", f.shape, f.d_in, f.items, f.streams, f.out_size, f.apply)
    clean.want, clean.recs, clean.stats, clean.label = f.want, f.recs, f.stats, f.label

    def load(streams):
        g = Filled("reset", f.shape, f.d_in, f.items, [(e, 0) for e in streams], f.out_size, f.apply)
        g.label = "reset/Q " + kind
        host = host_in.copy()
        g.want, g.recs = np.full(f.out_size, MARKER, np.uint8), []
        for it, e in zip(f.items, streams):
            host[it["in_offset"]:it["in_offset"] + e.size] = e
            rec, data = pda.oracle_item(sc.oracle, sc.w.ocoder, e, 0, it["out_capacity"])
            g.recs.append(rec)
            g.want[it["out_offset"]:it["out_offset"] + it["out_capacity"]] = data
        eng.upload(f.d_in, host)
        return g

    try:
        life.plain(clean, "first launch")
        assert eng.decode_plan_is_quiet(plan)
        life.plain(clean, "quiet")
        listed = load(quiet_variant(life, kind))
        life.plain(listed, "by a quiet plan")  # (what is listed goes the long way)
        assert not eng.decode_plan_is_quiet(plan), kind
        life.plain(listed, "with the kernels back")
        assert not eng.decode_plan_is_quiet(plan), kind
        eng.upload(f.d_in, host_in)
        life.plain(clean, "clean again")
        assert eng.decode_plan_is_quiet(plan), kind
        listed = load(quiet_variant(life, kind))
        life.packed(listed, 8, "listed, packed, by a quiet plan")
        assert not eng.decode_plan_is_quiet(plan), kind
        eng.upload(f.d_in, host_in)
        life.step("symbol_ranges", "C", "between")  # (refill asserts: not quiet)
        life.refill(clean)
        life.plain(clean, "back")
        assert eng.decode_plan_is_quiet(plan), kind
    finally:
        eng.upload(f.d_in, host_in)


# ----------------------------------------------------------------------------- 3: what is_quiet may say
def refused_fill(life, kind):
    """A reset of `kind` that is refused with AWS_ERROR_INVALID_ARGUMENT; returns (rc, error)."""
    eng, lib, plan = life.eng, life.lib, life.plan
    c = life.fill("reset", "C")
    lib.aws_reset_error()
    if kind in ("reset", "device_items"):
        items = [dict(it) for it in c.items[:4]]
        items[2]["first_bit"] = 9
        arr = eng._decode_item_array(items)
        if kind == "reset":
            rc = lib.aws_huffman_amd_decode_plan_reset(plan, arr, len(items))
        else:
            rc = lib.aws_huffman_amd_decode_plan_reset_device_items(plan, life.device(np.frombuffer(arr, dtype=np.uint8)), len(items), None)
    elif kind == "strided":
        desc = harness.StridedItems(count=1 << 32, in_offset=0, in_stride=64, in_len=64, out_offset=0, out_stride=64, out_capacity=64)
        rc = lib.aws_huffman_amd_decode_plan_reset_strided(plan, C.byref(desc), None)
    elif kind == "from_encode":
        never = eng.encode_plan([dict(in_offset=0, in_len=40_000, out_offset=0, out_capacity=60_000)])
        life.enc_plans.append(never)
        rc = lib.aws_huffman_amd_decode_plan_from_encode(plan, never, None)  # (never launched: no records to read lengths from)
    elif kind == "packed_input":
        rc = lib.aws_huffman_amd_decode_plan_reset_packed_input(plan, life.device(np.asarray([0, 70_000, 40_000, 90_000], np.uint64)), None, 3, None)
    else:
        st = life.stream(16_384)
        if kind == "block_ranges":
            rc = ia.reset_block_ranges(eng, plan, st.d_index, st.n, st.B, st.enc_offset, st.enc.size, st.upload_ranges([(0, 2, 0), (st.nb, 1, 40_000)]), 2)[0]
        else:
            rg = ra.Ranges(st)
            rc = ra.reset_symbol_ranges(eng, plan, st.d_enc, st.d_index, st.n, st.B, st.enc_offset, st.enc.size,
                                        rg.upload([(0, 30_000, 0), (st.n - 5, 6, 40_000)]), 2)[0]
    return rc, lib.aws_last_error() if rc else 0


def make_quiet(life):
    """The plan over Q, launched and fetched: quiet, its arrays as large as X needs (a refill below allocates nothing)."""
    f = life.refill(life.fill("reset", "Q"))
    life.plain(f, "towards a quiet plan")
    assert life.eng.decode_plan_is_quiet(life.plan)
    return f


def run_is_quiet(life, kind):
    """aws_huffman_amd_decode_plan_is_quiet is true only behind a fetched launch of the CURRENT items that listed nothing.
    From a quiet plan whose arrays are larger than what follows: a reset of `kind`, successful or refused, a fetch with no
    launch since the reset, a fetch behind a launch that was refused -- false every time.

    The refused launch here is one refused for its arguments, before anything is queued.  The other half of the fix -- a
    launch is counted only when hufk_decode_launch returned 0 -- is held by no test: that function's one early return (a plan
    with chunks for a decode table of more than 12 bits) cannot be reached through the C ABI, since no fill makes chunks
    for such a coder."""
    eng, plan = life.eng, life.plan
    life.step("reset", "X", "arrays larger than anything below")
    results = lambda n: eng.decode_results(plan, n)
    # a successful reset (items with chunks, within the arrays), then a fetch with no launch
    make_quiet(life)
    f = life.refill(life.fill(kind, "C"))
    assert f.stats["pieces"] > 0
    assert not eng.decode_plan_is_quiet(plan), kind
    results(len(f.items))
    assert not eng.decode_plan_is_quiet(plan), "%s: a fetch with no launch since the reset made the plan quiet" % kind
    results(len(f.items))
    assert not eng.decode_plan_is_quiet(plan), kind
    # ... a fetch behind a launch that was refused
    d_off = eng.alloc(64)
    try:
        assert pda.launch_packed(eng, plan, f.d_in, None, 0, d_off, 3) == INVALID
        results(len(f.items))
        assert not eng.decode_plan_is_quiet(plan), "%s: a fetch behind a refused launch made the plan quiet" % kind
    finally:
        eng.free(d_off)
    life.plain(f, "behind the fetches")
    # a refused reset, then a fetch
    make_quiet(life)
    assert refused_fill(life, kind) == INVALID, kind
    assert not eng.decode_plan_is_quiet(plan), "%s: quiet behind a refused reset" % kind
    results(eng.decode_stats(plan)["items"])
    assert not eng.decode_plan_is_quiet(plan), "%s: a fetch behind a refused reset made the plan quiet" % kind
    life.step(kind, "C", "behind the refusal")


# ----------------------------------------------------------------------------- 4: encode plans
ENC_FILL_KINDS = ["reset", "strided", "device_items"]
ENC_ENGINES = [None, "three-kernel", "one-pass-fails", "holes"]
ENC_SIZES = {"S67": [66 * SEG + 5], "S3": [40_000], "S2": [20_000], "S0t": [100] * 50, "S0s": [3_000] * 5,
             "MIX": [100, 0, 3_000, 20_000, 40_000, 66 * SEG + 5, 128, 129, 4_096, 16_385]}
# (fill kind, shape): every ordered pair of the three kinds; segments 67, 0, 3, 67, 2, 0, 67, then the mix, 0 and 2
ENC_LIFE = [("reset", "S67"), ("reset", "S0t"), ("strided", "S3"), ("strided", "S67"), ("device_items", "S2"),
            ("device_items", "S0s"), ("reset", "S67"), ("device_items", "MIX"), ("strided", "S0t"), ("reset", "S2")]
# the launch kinds between fills take turns in this order, an engine starting where its number says: with it every engine's
# third, sixth .. launch is a plain one AND a packed one at least once (a cycle of the four kinds alone never puts a
# packed launch there for two of the engines: its six launches a turn keep the packed one at 4 or 1 modulo 6)
ENC_LAUNCHES = ["plain", "length_only then plain", "packed size then plain", "packed", "packed"]
assert {(a[0], b[0]) for a, b in zip(ENC_LIFE, ENC_LIFE[1:])} == {(a, b) for a in ENC_FILL_KINDS for b in ENC_FILL_KINDS}


def enc_want_pieces(sizes, one_pass):
    """Segments of a plan of items of these sizes: none for an item of at most 128 symbols (a thread's) or, where the
    engine encodes in one pass, of at most 4 096 (a wave's)."""
    solo = pa.TILE if one_pass else 0
    return sum((n + SEG - 1) // SEG for n in sizes if n > max(THREAD_BYTES, solo))


class EncFilled:
    def __init__(self, kind, name, blobs, items, d_in, host_in, in_offs, out_size, apply):
        self.kind, self.name, self.blobs, self.items, self.d_in = kind, name, blobs, items, d_in
        self.host_in, self.in_offs, self.out_size, self.apply = host_in, in_offs, out_size, apply
        self.label = "%s/%s" % (kind, name)


class EncLife:
    """One encode plan on an engine of its own, and the decode plan of a Life to chain behind its launches."""

    def __init__(self, life, engine):
        sc = self.sc = life.sc
        self.life, self.name = life, engine
        self.holes = engine == "holes"
        self.eng, self.coder = sc.engine(holes=True) if self.holes else sc.engine(engine)
        self.one_pass = engine in (None, "one-pass-fails")
        self.ocoder = sc.w.ocoder_holes if self.holes else sc.w.ocoder
        self.lens = sc.lens_holes if self.holes else sc.lens
        self.plan = self.eng.empty_encode_plan()
        self.fills, self.owned, self.launches = {}, [], 0
        self.chain_due, self.chains, self.chains_behind_packed = False, 0, 0

    def close(self):
        self.sc.lib.aws_huffman_amd_encode_plan_destroy(self.plan)
        for d in self.owned:
            self.eng.free(d)
        self.sc.done(self.eng, self.coder)

    def device(self, arr):
        d = self.eng.alloc(max(arr.size, 8))
        self.eng.upload(d, arr)
        self.owned.append(d)
        return d

    def fill(self, kind, name):
        if (kind, name) in self.fills:
            return self.fills[(kind, name)]
        sc, eng, lib = self.sc, self.eng, self.sc.lib
        rng = np.random.default_rng(1270 + len(name) + ord(name[1]))
        sizes = ENC_SIZES[name]
        blobs = [pc.inputs(rng, n, pc.KINDS[i % 4] if len(sizes) > 1 else "uniform") for i, n in enumerate(sizes)]
        if self.holes:  # symbols 7 and 200 have no code: kept in a few items (they stop there, as in the oracle), out of the others
            for i, b in enumerate(blobs):
                if not (name in ("S0t", "MIX") and i % 3 == 2):
                    b[b == 7], b[b == 200] = 8, 201
        lens = pa.encoded_lengths(sc.lens, blobs, [0] * len(blobs))
        if kind == "strided":
            host_in, in_offs = pa.lay_out(blobs, None, first=16)
            cap = int(lens.max()) + 4
            own = [(5 + i * (cap + 3), cap) for i in range(len(blobs))]
        else:
            host_in, in_offs = pa.lay_out(blobs, rng, first=1)
            own, pos = [], 5
            for i, n in enumerate(lens):
                cap = int(n) // 2 if name in ("S0t", "MIX") and i % 4 == 2 else int(n) + 4  # (too short: SHORT_BUFFER)
                own.append((pos, cap))
                pos += cap + 3
        items = [dict(in_offset=in_offs[i], in_len=int(b.size), out_offset=own[i][0], out_capacity=own[i][1], eos_padding=0xFF)
                 for i, b in enumerate(blobs)]
        out_size = own[-1][0] + own[-1][1] + 64
        arr = eng._encode_item_array(items)
        if kind == "reset":
            apply = lambda: lib.aws_huffman_amd_encode_plan_reset(self.plan, arr, len(items))
        elif kind == "device_items":
            d_items = self.device(np.frombuffer(arr, dtype=np.uint8))
            apply = lambda: lib.aws_huffman_amd_encode_plan_reset_device_items(self.plan, d_items, len(items), None)
        else:
            desc = harness.StridedItems(count=len(items), in_offset=16, in_stride=int(blobs[0].size), in_len=int(blobs[0].size),
                                        out_offset=5, out_stride=own[0][1] + 3, out_capacity=own[0][1], first_bit=0, eos_padding=0xFF)
            apply = lambda: lib.aws_huffman_amd_encode_plan_reset_strided(self.plan, C.byref(desc), None)
        f = EncFilled(kind, name, blobs, items, self.device(host_in), host_in, in_offs, out_size, apply)
        f.want, f.recs = np.full(out_size, MARKER, np.uint8), []
        for it, b in zip(items, blobs):
            rec, data = pa.oracle_item(sc.oracle, self.ocoder, b, (0, 0), 0xFF, it["out_capacity"])
            f.recs.append(rec)
            f.want[it["out_offset"]:it["out_offset"] + it["out_capacity"]] = data
        f.lens = pa.encoded_lengths(self.lens, blobs, [0] * len(blobs))  # (the length query: a symbol without a code 0 bits)
        fresh = eng.encode_plan(items)
        f.stats = eng.encode_stats(fresh)
        lib.aws_huffman_amd_encode_plan_destroy(fresh)
        assert f.stats["pieces"] == enc_want_pieces(sizes, self.one_pass), (self.name, f.label, f.stats)
        assert f.stats["by_thread"] == sum(1 for n in sizes if 0 < n <= THREAD_BYTES), (self.name, f.label, f.stats)
        if self.one_pass:
            assert f.stats["by_wave"] == sum(1 for n in sizes if THREAD_BYTES < n <= pa.TILE), (self.name, f.label, f.stats)
        self.fills[(kind, name)] = f
        return f

    def want_road(self, f):
        """What the engine's road implies: three kernels where it keeps to them (or the coder has symbols without a code) and
        for a plan of threads only; one pass otherwise -- given up where a tile of a SEGMENT is made to fail (a plan
        without segments has no such tile)."""
        if not self.one_pass or f.stats["by_wave"] + f.stats["by_pieces"] == 0:
            return pc.ROAD_TWO_PASS
        return pc.ROAD_GAVE_UP if self.name == "one-pass-fails" and f.stats["pieces"] else pc.ROAD_ONE_PASS

    def refill(self, f):
        assert f.apply() == 0, (self.name, f.label, self.sc.lib.aws_last_error())
        got = self.eng.encode_stats(self.plan)
        assert got == f.stats, (self.name, f.label, got, f.stats)
        assert pa.packed_size(self.eng, self.plan)[:2] == INVALID, (self.name, f.label)
        return f

    def count(self):
        """One more launch of the encode plan, of whatever kind; every third one wants the decode plan chained behind it."""
        self.launches += 1
        if self.launches % 3 == 0:
            assert not self.chain_due, "two thirds without a launch that writes output between them"
            self.chain_due = True

    def chain(self, f, d_enc, in_offsets, produced, label, packed=False):
        """Behind every third launch -- or, where that one wrote no output (a length or size query), behind the next that
        does: the Life's decode plan chained to it (produced: the oracle's bytes of every item, as many as the launch had
        room for, lying at in_offsets of d_enc), launched, and the data back where it was."""
        if not self.chain_due:
            return
        self.chain_due = False
        self.chains += 1
        self.chains_behind_packed += packed
        life, sc = self.life, self.sc
        streams = [(np.ascontiguousarray(e), 0) for e in produced]
        items = [dict(in_offset=int(o), in_len=int(e.size), first_bit=0, out_offset=f.in_offs[i], out_capacity=int(f.blobs[i].size))
                 for i, (o, (e, _)) in enumerate(zip(in_offsets, streams))]
        g = Filled("from_encode", life.shapes["Q"], d_enc, items, streams, f.host_in.size,
                   lambda plan: 0 if life.eng.decode_plan_from_encode(plan, self.plan) else -1)
        g.label = "chained to %s %s (%s)" % (f.label, label, self.name)
        g.want, g.recs = np.full(g.out_size, MARKER, np.uint8), []
        for it, (enc, _), blob in zip(items, streams, f.blobs):
            rec, data = pda.oracle_item(sc.oracle, sc.w.ocoder, enc, 0, it["out_capacity"])
            g.recs.append(rec)
            g.want[it["out_offset"]:it["out_offset"] + it["out_capacity"]] = data
            if not self.holes and enc.size == (int(sc.lens[blob].sum()) + 7) // 8:  # (whole: the data comes back)
                assert rec[:3] == (0, 0, blob.size) and np.array_equal(data, blob), g.label
        assert g.apply(life.plan) == 0, g.label
        got = life.eng.decode_stats(life.plan)
        assert got["items"] == len(items) and not life.eng.decode_plan_is_quiet(life.plan), (g.label, got)
        if max(it["in_len"] for it in items) > THREAD_BYTES:  # (a chained plan of threads is made without a look at the lengths)
            fresh = life.eng.decode_plan(items)
            want = life.eng.decode_stats(fresh)
            sc.lib.aws_huffman_amd_decode_plan_destroy(fresh)
            assert got == want, (g.label, got, want)
        life.plain(g, "")

    def plain(self, f, label, length_only_first=False):
        eng = self.eng
        d_out = eng.alloc(f.out_size)
        try:
            eng.fill(d_out, MARKER, f.out_size)
            if length_only_first:
                eng.encode_launch(self.plan, f.d_in, d_out, length_only=True)
                assert eng.encoded_lengths(self.plan, len(f.items)) == [int(n) for n in f.lens], (self.name, f.label, label)
                assert eng.encode_road(self.plan) == pc.ROAD_TWO_PASS
                assert np.all(eng.download(d_out, f.out_size) == MARKER), (self.name, f.label, "a length query wrote output")
                self.count()
            eng.encode_launch(self.plan, f.d_in, d_out)
            self.count()
            got = eng.download(d_out, f.out_size)
            res = eng.encode_results(self.plan, len(f.items))
            for i, rec in enumerate(f.recs):
                assert res[i] == rec, (self.name, f.label, label, i, res[i], rec)
            bad = np.flatnonzero(got != f.want)
            assert bad.size == 0, (self.name, f.label, label, "first wrong byte at %d" % int(bad[0]))
            assert eng.encode_road(self.plan) == self.want_road(f), (self.name, f.label, label, eng.encode_road(self.plan))
            produced = [f.want[it["out_offset"]:it["out_offset"] + min(rec[3], it["out_capacity"])] for it, rec in zip(f.items, f.recs)]
            self.chain(f, d_out, [it["out_offset"] for it in f.items], produced, label)
        finally:
            eng.free(d_out)

    def packed(self, f, label, align=4):
        """One packed launch into exactly its total, the output kept for a decode plan to be chained to it: the offsets
        numpy's running sum of the rounded lengths, every item the oracle's encode into the room the layout reserves for it,
        MARKER in the gaps and behind the total, the sizes, the road."""
        sc, eng, n = self.sc, self.eng, len(f.items)
        offsets, reserved = pa.expected_offsets(f.lens, align)
        total = int(offsets[-1])
        want, recs = np.full(total + 64, MARKER, np.uint8), []
        for i, blob in enumerate(f.blobs):
            rec, data = pa.oracle_item(sc.oracle, self.ocoder, blob, (0, 0), 0xFF, int(reserved[i]))
            recs.append(rec)
            want[int(offsets[i]):int(offsets[i]) + int(reserved[i])] = data
        d_out, d_off = eng.alloc(total + 64), eng.alloc(8 * (n + 1))
        try:
            eng.fill(d_out, MARKER, total + 64)
            eng.fill(d_off, 0xEE, 8 * (n + 1))
            assert pa.launch_packed(eng, self.plan, f.d_in, d_out, total, d_off, align) == (0, 0), (self.name, f.label, label)
            self.count()
            got = eng.download(d_out, total + 64)
            res = eng.encode_results(self.plan, n)
            assert np.array_equal(pa.download_u64(eng, d_off, n + 1), offsets), (self.name, f.label, label)
            assert pa.packed_size(eng, self.plan) == (0, 0, total, int(reserved.max())), (self.name, f.label, label)
            for i, rec in enumerate(recs):
                assert res[i] == rec, (self.name, f.label, label, i, res[i], rec)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (self.name, f.label, label, "first wrong byte at %d" % int(bad[0]))
            assert eng.encode_road(self.plan) == self.want_road(f), (self.name, f.label, label, eng.encode_road(self.plan))
            produced = [want[int(o):int(o) + min(r[3], int(room))] for o, r, room in zip(offsets, recs, reserved)]
            self.chain(f, d_out, offsets[:-1], produced, label, packed=True)
        finally:
            eng.free(d_out)
            eng.free(d_off)

    def size_query(self, f):
        eng, n = self.eng, len(f.items)
        offsets, reserved = pa.expected_offsets(f.lens, 8)
        d_off = eng.alloc(8 * (n + 1))
        try:
            assert pa.launch_packed(eng, self.plan, f.d_in, None, 0, d_off, 8) == (0, 0)
            assert pa.packed_size(eng, self.plan) == (0, 0, int(offsets[-1]), int(reserved.max()))
            assert np.array_equal(pa.download_u64(eng, d_off, n + 1), offsets), (self.name, f.label)
            self.count()
        finally:
            eng.free(d_off)


def run_encode_life(life, engine, steps=None):
    """One encode plan through ENC_LIFE on an engine made under `engine`, the launch kinds taking turns; behind every third
    launch (EncLife.count, EncLife.chain) the Life's decode plan is chained to it, launched, and the data checked."""
    el = EncLife(life, engine)
    try:
        for i, (kind, name) in enumerate(ENC_LIFE[:steps]):
            f = el.refill(el.fill(kind, name))
            how = ENC_LAUNCHES[(i + ENC_ENGINES.index(engine)) % len(ENC_LAUNCHES)]
            label = "step %d, %s" % (i, how)
            if how == "plain":
                el.plain(f, label)
            elif how == "length_only then plain":
                el.plain(f, label, length_only_first=True)
            elif how == "packed":
                el.packed(f, label)
            else:
                el.size_query(f)
                el.plain(f, label)
        if steps is None:  # (every third launch was chained behind, a packed one among them)
            assert el.launches >= 12 and not el.chain_due and el.chains == el.launches // 3, (engine, el.launches, el.chains)
            assert el.chains_behind_packed >= 1 and el.chains > el.chains_behind_packed, (engine, el.chains, el.chains_behind_packed)
    finally:
        el.close()


# ----------------------------------------------------------------------------- 5: no host wait where the contract needs none
def run_decode_tour_without_waits(life, steps=20):
    """The tour's first steps with nothing between a launch and the next reset: no synchronise, no download, no fetch (a
    reset is ordered behind the launch on the engine's stream, huffman_amd.h).  Every step's output goes to a buffer of its
    own, made and filled before the first step, and is read only when the following reset has returned."""
    eng, plan = life.eng, life.plan
    tour = decode_tour()[:steps]
    fills = [life.fill(kind, name) for kind, name in tour]  # (inputs, expectations: all made before the first step)
    outs = [eng.alloc(f.out_size) for f in fills]
    try:
        for f, d in zip(fills, outs):
            eng.fill(d, MARKER, f.out_size)
        eng.sync()
        for i, f in enumerate(fills):
            assert f.apply(plan) == 0, (f.label, i)
            if i:
                g = fills[i - 1]
                bad = np.flatnonzero(eng.download(outs[i - 1], g.out_size) != g.want)
                assert bad.size == 0, ("step %d, %s" % (i - 1, g.label), "first wrong byte at %d" % int(bad[0]))
            eng.decode_launch(plan, f.d_in, outs[i])
        res = eng.decode_results(plan, len(fills[-1].items))
        life.compare(fills[-1], eng.download(outs[-1], fills[-1].out_size), res, "last step")
    finally:
        for d in outs:
            eng.free(d)


def run_encode_life_without_waits(life, steps=20):
    """ENC_LIFE twice over on the default engine, plain launches, in the same manner."""
    el = EncLife(life, None)
    outs = []
    try:
        eng = el.eng
        fills = [el.fill(kind, name) for kind, name in (ENC_LIFE * 2)[:steps]]
        outs = [eng.alloc(f.out_size) for f in fills]
        for f, d in zip(fills, outs):
            eng.fill(d, MARKER, f.out_size)
        eng.sync()
        for i, f in enumerate(fills):
            assert f.apply() == 0, (f.label, i)
            if i:
                g = fills[i - 1]
                bad = np.flatnonzero(eng.download(outs[i - 1], g.out_size) != g.want)
                assert bad.size == 0, ("step %d, %s" % (i - 1, g.label), "first wrong byte at %d" % int(bad[0]))
            eng.encode_launch(el.plan, f.d_in, outs[i])
        g = fills[-1]
        assert np.array_equal(eng.download(outs[-1], g.out_size), g.want), "last step"
        assert eng.encode_results(el.plan, len(g.items)) == g.recs
    finally:
        for d in outs:
            el.eng.free(d)
        el.close()
