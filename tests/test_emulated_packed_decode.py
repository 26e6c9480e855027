"""CPU logic tests of the packed batch decode (huffman_amd_packed.h: the offset kernels of pack_kernels.hip between the scan
and the emit stage of a decode launch) through the fiber emulator (tests/emu, UBSan).  Every expectation is the oracle's:
sym_i from its decode of the item with room for everything -- symbols the padding bits spell included --, records and
bytes from its decode into the room the layout gives the item.  The claim at size is tests/test_gpu_packed_decode.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import build_api as ba
import coder_shapes as cs
import harness
import packed_api as pa
import packed_decode_api as pd
import parity_cases as pc

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libaws-c-compression-emu.so")

CHUNK = 32768  # HUFD_DEC_CHUNK_BYTES
LARGE = 64     # HUFD_SCAN_SMALL_MAX chunks: above it the workgroup scan
INVALID = (-1, harness.AWS_ERROR_INVALID_ARGUMENT)
UNKNOWN = (-1, harness.AWS_ERROR_COMPRESSION_UNKNOWN_SYMBOL)
SHORT = (-1, harness.AWS_ERROR_SHORT_BUFFER)
EOS = (0x00, 0xFF, 0x20)  # paddings: of the test coder's codes none is all zeros or all ones, 0x20 starts with a five-bit one


class Emu:
    def __init__(self, oracle):
        self.oracle = oracle
        self.lib = ba.bind(pd.bind(harness.load_product(EMU_SO)))
        self.w = pc.World(oracle, harness.Codec(self.lib, "aws_"))
        self.min_bits = min(int(l) for l in self.w.table[1] if l)
        self.eng = harness.Engine(self.lib, self.w.pcoder)
        # symbols for a stream of about 3 MB: what the long items are cut from
        self.long_plain = pc.inputs(np.random.default_rng(401), 3_400_000, "uniform")

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


@pytest.fixture(scope="module")
def emu(oracle):
    subprocess.check_call(["make", "-s", "-C", EMU_DIR], stdout=subprocess.DEVNULL)
    e = Emu(oracle)
    yield e
    e.lib.aws_huffman_amd_testing_set_pack_tile_items(0)
    e.lib.aws_huffman_amd_testing_set_decode_road(0)
    e.eng.close()


class Batch:
    """(encoded bytes, first bit) streams in device memory and the oracle's word on them.  The items' own out_offset /
    out_capacity are whatever `own` says (default: no room at all -- a packed launch must not look at them)."""

    def __init__(self, emu, streams, rng, own=None, eng=None, ocoder=None, min_bits=None, align=1):
        self.eng, self.streams = eng or emu.eng, streams
        n = len(streams)
        self.host_in, self.in_offs = pd.lay_out(streams, rng, first=1 if rng is not None else 0, align=align)
        self.d_in = self.eng.alloc(self.host_in.size)
        self.eng.upload(self.d_in, self.host_in)
        own = own or [(0, 0)] * n
        self.items = [dict(in_offset=self.in_offs[i], in_len=int(streams[i][0].size), first_bit=streams[i][1],
                           out_offset=own[i][0], out_capacity=own[i][1]) for i in range(n)]
        self.expect = pd.Expect(emu.oracle, ocoder or emu.w.ocoder, streams, min_bits or emu.min_bits)

    def close(self):
        self.eng.free(self.d_in)


def with_first_bits(rng, streams, every=3):
    """Every third stream entered inside its first byte (the bits in front of it are the call before's)."""
    return [(enc, int(rng.integers(1, 8)) if i % every == 1 and enc.size else 0) for i, enc in enumerate(streams)]


def mixed_streams(emu, rng, with_large=True):
    """Encoded lengths 0, 1, a few bytes, around 512 and 768 (a thread's and a wave's), around one chunk, several chunks,
    more than HUFD_SCAN_SMALL_MAX chunks; paddings 0x00, 0xFF and 0x20 (which spells a symbol of the test coder) in turn."""
    targets = [0, 1, 5, 40, 500, 512, 520, 760, 768, 775, 3000, CHUNK - 9, CHUNK, CHUNK + 5, 0, 3 * CHUNK + 77, 5 * CHUNK + 4]
    if with_large:
        targets.append((LARGE + 1) * CHUNK + 300)
    encs = [emu.encoded(t, EOS[i % 3], rng, pc.KINDS[i % 4]) if t else np.zeros(0, np.uint8) for i, t in enumerate(targets)]
    return with_first_bits(rng, encs)


def test_mixed_batch(emu):
    rng = np.random.default_rng(501)
    streams = mixed_streams(emu, rng)
    b = Batch(emu, streams, rng)
    plan = emu.eng.decode_plan(b.items)
    try:
        stats = emu.eng.decode_stats(plan)
        assert stats["by_thread"] and stats["by_wave"] and stats["by_pieces"] and stats["empty"], stats
        # padding spells symbols for some items and none for others: sym_i is not the length of the text
        for align in (1, 4, 16):
            _, _, _, res = pd.check_launch(emu.eng, plan, b.d_in, b.expect, align, label="mixed")
            assert all(r[:2] == (0, 0) for r, (_, fb) in zip(res, streams) if fb == 0), res  # (whole streams from bit 0)
    finally:
        emu.lib.aws_huffman_amd_decode_plan_destroy(plan)
        b.close()


def test_padding_adds_symbols_or_not(emu):
    """The premise of the layout: sym_i is not the length of the text.  The test coder has no code of all ones or all
    zeros, so paddings 0xFF and 0x00 spell nothing; 0x20 starts with its five-bit code 00100 and spells a symbol more
    wherever five bits or more are padding.  The canonical coder of 4 .. 12 bits has the code 0000: there 0x00 does."""
    rng = np.random.default_rng(503)
    oc, pcoder, lengths = shaped_coders(emu, "from_lengths 4..12")
    coded = np.flatnonzero(np.asarray(lengths))
    more = {}
    for i in range(60):
        plain = pc.inputs(rng, int(rng.integers(1, 300)), "uniform")
        other = coded[rng.integers(0, coded.size, plain.size)].astype(np.uint8)
        for name, coder, data, eos in (("test 0x00", emu.w.ocoder, plain, 0x00), ("test 0xFF", emu.w.ocoder, plain, 0xFF),
                                       ("test 0x20", emu.w.ocoder, plain, 0x20), ("4..12 0x00", oc, other, 0x00),
                                       ("4..12 0xFF", oc, other, 0xFF)):
            enc = emu.oracle.encode_all(coder, data, eos_padding=eos)
            rec, _ = pd.oracle_item(emu.oracle, coder, enc, 0, data.size + 16)
            assert rec[:2] == (0, 0) and rec[2] >= data.size
            more[name] = more.get(name, 0) + (rec[2] > data.size)
    emu.lib.aws_huffman_amd_table_coder_destroy(pcoder)
    assert more["test 0x00"] == 0 and more["test 0xFF"] == 0 and more["4..12 0xFF"] == 0, more
    assert 5 < more["test 0x20"] < 55 and 5 < more["4..12 0x00"] < 55, more


@pytest.mark.parametrize("kind", ["host", "strided", "device", "packed-input", "packed-input-lengths", "threads", "from-encode"])
def test_every_way_a_plan_is_made(emu, kind):
    rng = np.random.default_rng(511)
    eng = emu.eng
    d_extra, enc_plan = [], None
    if kind == "strided":
        # equal items a stride apart: the shorter streams run on into the ones (no code) behind them
        encs = [emu.encoded(int(rng.integers(20000, 20400)), EOS[i % 3], rng) for i in range(12)]
        longest = max(e.size for e in encs)
        streams = [(np.concatenate([e, np.full(longest - e.size, 0xFF, np.uint8)]), 0) for e in encs]
        b = Batch(emu, streams, None)
        plan = eng.plan_strided(False, count=12, in_offset=b.in_offs[0], in_stride=longest, in_len=longest, out_offset=0,
                                out_stride=0, out_capacity=0, first_bit=0, eos_padding=0)
    elif kind == "threads":
        encs = [pc.oracle_encode(emu.w, pc.inputs(rng, int(rng.integers(1, 90)), pc.KINDS[i % 4]), eos=EOS[i % 3])
                for i in range(4300)]
        b = Batch(emu, with_first_bits(rng, encs, every=7), rng)
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
        b.expect = pd.Expect(emu.oracle, emu.w.ocoder, streams, emu.min_bits)
        plan = eng.empty_decode_plan()
        assert eng.decode_plan_from_encode(plan, enc_plan)
    elif kind.startswith("packed-input"):
        streams = mixed_streams(emu, rng, with_large=False)
        streams = [(enc, 0) for enc, _ in streams]  # (such a plan enters every item at bit 0)
        with_lengths = kind.endswith("lengths")
        b = Batch(emu, streams, None, align=8 if with_lengths else 1)
        if with_lengths:
            d_offs, d_lens = pd.upload_u64(eng, b.in_offs), pd.upload_u64(eng, [e.size for e, _ in streams])
            d_extra += [d_offs, d_lens]
        else:
            assert all(b.in_offs[i] + streams[i][0].size == b.in_offs[i + 1] for i in range(len(streams) - 1))
            d_offs, d_lens = pd.upload_u64(eng, b.in_offs + [b.in_offs[-1] + streams[-1][0].size]), None
            d_extra.append(d_offs)
        plan = eng.empty_decode_plan()
        assert pd.reset_packed_input(eng, plan, d_offs, d_lens, len(streams)) == (0, 0)
        stats = eng.decode_stats(plan)
        assert stats["items"] == len(streams) and stats["by_pieces"] and stats["by_thread"], stats
    else:
        streams = mixed_streams(emu, rng, with_large=False)
        b = Batch(emu, streams, rng)
        if kind == "host":
            plan = eng.decode_plan(b.items)
        else:
            plan, d_items = eng.decode_plan_from_device_items(b.items)
            d_extra.append(d_items)
    try:
        for align in (1, 8):
            pd.check_launch(eng, plan, b.d_in, b.expect, align, label=kind, launches=2)
        if kind.startswith("packed-input"):
            # the items' own room is none: a plain launch of such a plan reports SHORT_BUFFER for every item with a symbol
            eng.decode_launch(plan, b.d_in, None)
            for r, sym in zip(eng.decode_results(plan, len(b.streams)), b.expect.syms()):
                assert (r[:3] == SHORT + (0,)) == (sym > 0), (r, sym)
    finally:
        emu.lib.aws_huffman_amd_decode_plan_destroy(plan)
        if enc_plan:
            emu.lib.aws_huffman_amd_encode_plan_destroy(enc_plan)
        for d in d_extra:
            eng.free(d)
        b.close()


@pytest.mark.parametrize("road", ["long-way", "lean-sync", "tails-apart", "all-kernels"])
def test_decode_road_switches(emu, road):
    rng = np.random.default_rng(521)
    streams = mixed_streams(emu, rng, with_large=False)
    # many short end-of-stream chunks as well: the kernels that share a workgroup between them, or do not
    streams += with_first_bits(rng, [emu.encoded(int(rng.integers(900, 2500)), EOS[i % 3], rng) for i in range(70)])
    b = Batch(emu, streams, rng)
    plan = emu.eng.decode_plan(b.items)
    try:
        with harness.decode_road(emu.lib, road):
            for align in (1, 16):
                pd.check_launch(emu.eng, plan, b.d_in, b.expect, align, label=road, launches=2)
        pd.check_launch(emu.eng, plan, b.d_in, b.expect, 1, label="after " + road)
    finally:
        emu.lib.aws_huffman_amd_decode_plan_destroy(plan)
        b.close()


@pytest.mark.parametrize("tile,counts", [(4096, (4095, 4096, 4097)), (300, (29999, 30000, 30001)), (64, (23457,)), (1, (301,))])
def test_scan_boundaries(emu, tile, counts):
    """The offset scan in tiles of a few items: item counts of exactly a tile (or a whole number of them), one more, one
    less, a number that is no multiple, more tiles than a workgroup has threads; against numpy's cumulative sum of the
    oracle's symbol counts."""
    rng = np.random.default_rng(523 + tile)
    most = max(counts)
    encs = [pc.oracle_encode(emu.w, pc.inputs(rng, int(rng.integers(0, 40)), pc.KINDS[i % 4]), eos=EOS[i % 3])
            for i in range(most)]
    b = Batch(emu, [(e, 0) for e in encs], None)
    all_syms = b.expect.syms()
    try:
        with pa.pack_tile_items(emu.lib, tile):
            for n in counts:
                plan = emu.eng.decode_plan(b.items[:n])
                for align in (1, 16):
                    offsets, total, _, _ = pd.check_launch(emu.eng, plan, b.d_in, b.expect.first(n), align,
                                                           label="tile %d, %d items" % (tile, n))
                    rounded = (all_syms[:n] + align - 1) // align * align
                    assert np.array_equal(offsets[1:], np.cumsum(rounded)) and total == int(rounded.sum())
                emu.lib.aws_huffman_amd_decode_plan_destroy(plan)
    finally:
        b.close()


def early_stops(emu, rng):
    """Streams that stop before their end: damaged (a window without a code, 32 bits or more in front of the end), cut
    inside a code, arbitrary bytes; of a thread's, a wave's, a chunk's and several chunks' length."""
    streams = []
    for i, target in enumerate([60, 300, 700, 2000, 9000, CHUNK + 900, 2 * CHUNK + 50, 4 * CHUNK + 7000]):
        enc = emu.encoded(target, EOS[i % 3], rng)
        damaged = enc.copy()
        at = int(rng.integers(0, max(enc.size - 12, 1)))
        damaged[at:at + 4] = 0xFF  # ten one bits: no code of the test coder
        streams += [damaged, enc[:int(rng.integers(enc.size // 2, enc.size))], rng.integers(0, 256, target, dtype=np.uint8)]
        late = enc.copy()
        late[-2:] = 0xFF  # ... and one fewer than 32 bits in front of the end: no error, the walk just ends there
        streams.append(late)
    return with_first_bits(rng, streams, every=5)


def test_streams_that_stop_early(emu):
    rng = np.random.default_rng(541)
    b = Batch(emu, early_stops(emu, rng), rng)
    plan = emu.eng.decode_plan(b.items)
    try:
        for align in (1, 4):
            _, _, _, res = pd.check_launch(emu.eng, plan, b.d_in, b.expect, align, label="early stops", launches=2)
            kinds = {r[:2] for r in res}
            assert UNKNOWN in kinds and (0, 0) in kinds, kinds
            # a stream cut inside a code: success, and fewer bits consumed than it has
            assert any(r[:2] == (0, 0) and r[3] < 8 * s[0].size - s[1] for r, s in zip(res, b.streams))
            assert all(r[2] == sym for r, sym in zip(res, b.expect.syms()))
    finally:
        emu.lib.aws_huffman_amd_decode_plan_destroy(plan)
        b.close()


@pytest.mark.parametrize("road", [None, "long-way"])
def test_capacity_clipping(emu, road):
    rng = np.random.default_rng(547)
    targets = [40, 0, 700, 6000, 300, CHUNK + 1, 2 * CHUNK + 500, 17, 3 * CHUNK, 90, 1]
    encs = [emu.encoded(t, EOS[i % 3], rng) if t else np.zeros(0, np.uint8) for i, t in enumerate(targets)]
    damaged = encs[6].copy()
    damaged[CHUNK + 40:CHUNK + 44] = 0xFF
    encs[6] = damaged
    b = Batch(emu, with_first_bits(rng, encs, every=4), rng)
    plan = emu.eng.decode_plan(b.items)
    syms = b.expect.syms()
    try:
        with harness.decode_road(emu.lib, road):
            for align in (1, 16):
                offsets, _ = pd.expected_offsets(syms, align)
                total = int(offsets[-1])
                caps = [0, total - 1, total + 5]
                for k in (0, 2, 3, 5, 6, 8, 10):
                    caps += [int(offsets[k]), int(offsets[k]) + 1, int(offsets[k] + syms[k] // 2), int(offsets[k] + syms[k]) - 1,
                             int(offsets[k] + syms[k])]
                for cap in sorted(set(c for c in caps if c >= 0)):
                    _, _, _, res = pd.check_launch(emu.eng, plan, b.d_in, b.expect, align, capacity=cap, label="clip/%s" % road)
                    for i, r in enumerate(res):
                        fits = offsets[i] + syms[i] <= cap
                        if not fits and syms[i]:  # (no partial room: nothing produced, nothing consumed)
                            assert r == SHORT + (0, 0), (cap, i, r)
                        elif not fits:  # (an item without symbols: the reference's answer for no room, never SHORT_BUFFER)
                            assert r[:2] in ((0, 0), UNKNOWN) and r[2] == 0, (cap, i, r)
                        else:
                            assert r[2] == syms[i] and r[:2] in ((0, 0), UNKNOWN), (cap, i, r)
    finally:
        emu.lib.aws_huffman_amd_decode_plan_destroy(plan)
        b.close()


def shaped_coders(emu, name):
    """(oracle coder, product coder, code lengths)."""
    if name == "from_lengths 4..12":
        lengths = cs.shape(*cs.LEN4TO12)
        patterns, lens = pc.canonical_code(lengths)
        oc = emu.oracle.lib.oracle_table_coder_new((C.c_uint32 * 256)(*patterns), (C.c_uint8 * 256)(*lens))
        pcoder = emu.lib.aws_huffman_amd_table_coder_from_lengths((C.c_uint8 * 256)(*lengths))
        assert oc and pcoder
        return oc, pcoder, lengths
    return pc.profile_coders(emu.w, name)


@pytest.mark.parametrize("name", ["from_lengths 4..12", "hpack_lengths", "len8", "len9"])
def test_other_coders(emu, name):
    """A coder built from lengths of 4 to 12 bits (the chunk kernels, tables of 12 bits), one with HPACK's lengths of 5 to
    30 bits (linked tables: items a thread, a workgroup, or blocks across the chip each; plans from device sources are
    made through the host) and coders with codes of one length (no walk at all; len9: half the windows without a code)."""
    rng = np.random.default_rng(557)
    oc, pcoder, lengths = shaped_coders(emu, name)
    coded = np.flatnonzero(np.asarray(lengths))
    min_bits = int(min(l for l in lengths if l))
    eng = harness.Engine(emu.lib, pcoder)
    encs = []
    for i, n in enumerate([0, 1, 30, 200, 700, 1500, 9000, 40_000, 100_000, 300_000]):
        plain = coded[rng.integers(0, coded.size, n)].astype(np.uint8)
        enc = emu.oracle.encode_all(oc, plain, eos_padding=EOS[i % 3], slack=64 + 4 * n)
        encs.append(enc)
        if n >= 700:
            cut = enc[:int(rng.integers(enc.size // 2, enc.size))]
            noisy = enc.copy()
            at = int(rng.integers(0, enc.size - 8))
            noisy[at:at + 6] = rng.integers(0, 256, 6, dtype=np.uint8)
            encs += [cut, noisy]
    streams = with_first_bits(rng, encs, every=4)
    b = Batch(emu, streams, rng, eng=eng, ocoder=oc, min_bits=min_bits)
    plan = eng.decode_plan(b.items)
    d_extra = []
    try:
        with harness.decode_road(emu.lib, None):
            emu.lib.aws_huffman_amd_testing_set_wide_min_bytes(60_000)  # (the long items of HPACK's lengths across the chip)
            for align in (1, 8):
                pd.check_launch(eng, plan, b.d_in, b.expect, align, label=name, launches=2)
            total = int(pd.expected_offsets(b.expect.syms(), 8)[0][-1])
            pd.check_launch(eng, plan, b.d_in, b.expect, 8, capacity=total // 2, label=name + " clipped")
            # ... and the same streams as a packed input
            flat = [(enc, 0) for enc, _ in streams]
            fb = Batch(emu, flat, None, eng=eng, ocoder=oc, min_bits=min_bits)
            d_offs = pd.upload_u64(eng, fb.in_offs + [fb.in_offs[-1] + flat[-1][0].size])
            d_extra += [d_offs, fb.d_in]
            assert pd.reset_packed_input(eng, plan, d_offs, None, len(flat)) == (0, 0)
            pd.check_launch(eng, plan, fb.d_in, fb.expect, 4, label=name + " packed input")
    finally:
        emu.lib.aws_huffman_amd_testing_set_wide_min_bytes(0)
        emu.lib.aws_huffman_amd_decode_plan_destroy(plan)
        for d in d_extra:
            eng.free(d)
        b.close()
        eng.close()
        emu.lib.aws_huffman_amd_table_coder_destroy(pcoder)


def test_the_plans_own_layout_survives(emu):
    rng = np.random.default_rng(563)
    streams = mixed_streams(emu, rng, with_large=False) + early_stops(emu, rng)[:8]
    expect = pd.Expect(emu.oracle, emu.w.ocoder, streams, emu.min_bits)
    own, pos = [], 5
    for i, sym in enumerate(expect.syms()):
        cap = [int(sym) + 8, int(sym) // 3, int(sym)][i % 3]  # roomy, too short, exact
        own.append((pos, cap))
        pos += cap + 3
    b = Batch(emu, streams, rng, own=own)
    eng = emu.eng
    plan = eng.decode_plan(b.items)
    d_out = eng.alloc(pos + 64)

    def plain():
        eng.fill(d_out, pd.MARKER, pos + 64)
        eng.decode_launch(plan, b.d_in, d_out)
        return eng.download(d_out, pos + 64), eng.decode_results(plan, len(streams))

    try:
        first_bytes, first_res = plain()
        for i, (enc, fb) in enumerate(streams):  # (the plain launch itself, against the oracle)
            rec, data = pd.oracle_item(emu.oracle, emu.w.ocoder, enc, fb, own[i][1])
            assert first_res[i] == rec and np.array_equal(first_bytes[own[i][0]:own[i][0] + own[i][1]], data), i
        assert SHORT in {r[:2] for r in first_res}
        pd.check_launch(eng, plan, b.d_in, b.expect, 4, label="between")
        third_bytes, third_res = plain()
        assert third_res == first_res and np.array_equal(third_bytes, first_bytes)
    finally:
        eng.free(d_out)
        emu.lib.aws_huffman_amd_decode_plan_destroy(plan)
        b.close()


def test_arguments(emu):
    rng = np.random.default_rng(569)
    eng = emu.eng
    streams = [(emu.encoded(t, 0x00, rng), 0) for t in (50, 5000, 40_000)]
    b = Batch(emu, streams, None)
    plan = eng.decode_plan(b.items)
    n = len(streams)
    d_out, d_off = eng.alloc(200_000), eng.alloc(8 * (n + 1))
    d_extra = []
    try:
        assert pd.packed_size(eng, plan)[:2] == INVALID  # (no packed launch yet)
        assert pd.launch_packed(eng, plan, b.d_in, d_out, 8192, None, 1) == INVALID
        for align in (0, 3, 8192):
            assert pd.launch_packed(eng, plan, b.d_in, d_out, 8192, d_off, align) == INVALID
        assert pd.launch_packed(eng, plan, b.d_in, None, 8192, d_off, 1) == INVALID
        assert pd.packed_size(eng, plan)[:2] == INVALID  # (none of those was one)
        # NULL output with no capacity: the offsets and the sizes, nothing written
        assert pd.launch_packed(eng, plan, b.d_in, None, 0, d_off, 4096) == (0, 0)
        syms = b.expect.syms()
        offsets, reserved = pd.expected_offsets(syms, 4096)
        assert np.array_equal(pa.download_u64(eng, d_off, n + 1), offsets)
        assert pd.packed_size(eng, plan) == (0, 0, int(offsets[-1]), int(reserved.max()))
        assert eng.decode_results(plan, n) == [SHORT + (0, 0)] * n
        total, longest = C.c_uint64(), C.c_uint64()
        assert emu.lib.aws_huffman_amd_decode_plan_packed_size(plan, None, C.byref(longest), None) == 0 and longest.value == reserved.max()
        assert emu.lib.aws_huffman_amd_decode_plan_packed_size(plan, C.byref(total), None, None) == 0 and total.value == offsets[-1]
        # a reset: the sizes of the items before say nothing about these
        arr = eng._decode_item_array(b.items[:1])
        assert emu.lib.aws_huffman_amd_decode_plan_reset(plan, arr, 1) == 0
        assert pd.packed_size(eng, plan)[:2] == INVALID
        # a packed input whose offsets decrease, with and without lengths: refused, a plan without items
        good = b.in_offs + [b.in_offs[-1] + streams[-1][0].size]
        d_good, d_bad = pd.upload_u64(eng, good), pd.upload_u64(eng, [good[0], good[2], good[1], good[3]])
        d_lens = pd.upload_u64(eng, [s[0].size for s in streams])
        d_extra += [d_good, d_bad, d_lens]
        for lens in (None, d_lens):
            assert pd.reset_packed_input(eng, plan, d_good, lens, n) == (0, 0)
            assert eng.decode_stats(plan)["items"] == n
            assert pd.reset_packed_input(eng, plan, d_bad, lens, n) == INVALID
            assert eng.decode_stats(plan)["items"] == 0
            assert pd.packed_size(eng, plan)[:2] == INVALID
        assert pd.reset_packed_input(eng, plan, None, None, n) == INVALID
        # ... an item of 4 GiB: refused as well
        d_huge = pd.upload_u64(eng, [0, 1 << 32])
        d_extra.append(d_huge)
        assert pd.reset_packed_input(eng, plan, d_huge, None, 1) == INVALID
        # a plan without items: success, offsets[0] = 0 written, sizes 0
        for make_empty in ("new", "packed-input"):
            empty = eng.empty_decode_plan()
            if make_empty == "packed-input":
                assert pd.reset_packed_input(eng, empty, d_good, None, 0) == (0, 0)
            eng.fill(d_off, 0xEE, 8 * (n + 1))
            assert pd.launch_packed(eng, empty, None, None, 0, d_off, 1) == (0, 0)
            eng.sync()
            got = eng.download(d_off, 16).view(np.uint64)
            assert got[0] == 0 and got[1] == 0xEEEEEEEEEEEEEEEE
            assert pd.packed_size(eng, empty) == (0, 0, 0, 0)
            emu.lib.aws_huffman_amd_decode_plan_destroy(empty)
    finally:
        eng.free(d_out)
        eng.free(d_off)
        for d in d_extra:
            eng.free(d)
        emu.lib.aws_huffman_amd_decode_plan_destroy(plan)
        b.close()
