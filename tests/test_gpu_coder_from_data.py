"""Coders built from data on an MI355X (`pytest -m gpu`): exact symbol counts at size (1 GiB, 4.5 GiB of one byte value,
any alignment, two streams into one array), and count -> lengths -> coder -> engine end to end, checked against the
CPU oracle with the same rows."""
import ctypes as C
import math

import numpy as np
import pytest

import build_api as ba
import coder_shapes as cs
import harness

pytestmark = pytest.mark.gpu

MiB, GiB = 1 << 20, 1 << 30


@pytest.fixture(scope="module")
def lib():
    lib = ba.bind(harness.load_product())
    assert lib.aws_huffman_amd_device_count() >= 1, "no HIP device visible: the product has no CPU path"
    return lib


@pytest.fixture(scope="module")
def eng(lib):
    patterns, lens = harness.load_table()
    coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    e = harness.Engine(lib, coder)
    yield e
    e.close()
    lib.aws_huffman_amd_table_coder_destroy(coder)


def count_on_device(lib, eng, d_in, length, d_counts=None):
    """On the engine's stream, behind the zeroing of the counts and in front of their copy back."""
    own = d_counts is None
    if own:
        d_counts = eng.alloc(256 * 8)
    eng.fill(d_counts, 0, 256 * 8)
    before = lib.aws_huffman_amd_current_device()
    assert lib.aws_huffman_amd_symbol_counts(-1, d_in, length, d_counts, eng.stream) == 0
    assert lib.aws_huffman_amd_current_device() == before
    got = eng.download(d_counts, 256 * 8).view(np.uint64).copy()
    if own:
        eng.free(d_counts)
    return got


def test_counts_1gib_splitmix(lib, eng):
    d_in = eng.alloc(GiB)
    try:
        eng.fill_splitmix64(d_in, GiB, 77)
        got = count_on_device(lib, eng, d_in, GiB)
    finally:
        eng.free(d_in)
    assert np.array_equal(got, ba.bincount(harness.splitmix64_bytes(77, GiB)))


def test_counts_printable_and_odd_ranges(lib, eng):
    data = harness.printable_map(harness.splitmix64_bytes(4, 256 * MiB))
    d_in = eng.alloc(data.size + 64)
    try:
        eng.upload(d_in, data)
        assert np.array_equal(count_on_device(lib, eng, d_in, data.size), ba.bincount(data))
        rng = np.random.default_rng(5)
        for _ in range(12):
            off = int(rng.integers(0, 64))
            length = int(rng.integers(0, 40 * MiB)) | 1
            length = min(length, data.size - off)
            got = count_on_device(lib, eng, d_in + off, length)
            assert np.array_equal(got, ba.bincount(data[off:off + length])), (off, length)
        for off, length in [(1, 0), (3, 1), (7, 15), (15, 17), (0, 16), (9, 4097), (5, 65 * MiB + 3)]:
            got = count_on_device(lib, eng, d_in + off, length)
            assert np.array_equal(got, ba.bincount(data[off:off + length])), (off, length)
    finally:
        eng.free(d_in)


def test_counts_past_4gib_of_one_byte(lib, eng):
    """count == length > 2^32: the u64 adds, and (flushes every MiB) the flushes inside a launch on the chip."""
    n = 4 * GiB + GiB // 2
    d_in = eng.alloc(n + 16)
    try:
        eng.fill(d_in, 0x5A, n + 16)
        for flush in (0, MiB):
            lib.aws_huffman_amd_testing_set_count_flush_bytes(flush)
            got = count_on_device(lib, eng, d_in + 3, n)
            want = np.zeros(256, np.uint64)
            want[0x5A] = n
            assert np.array_equal(got, want), flush
    finally:
        lib.aws_huffman_amd_testing_set_count_flush_bytes(0)
        eng.free(d_in)


def test_two_streams_into_one_array(lib, eng):
    patterns, lens = harness.load_table()
    coder2 = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    eng2 = harness.Engine(lib, coder2)
    a = harness.splitmix64_bytes(11, 96 * MiB + 5)
    b = harness.printable_map(harness.splitmix64_bytes(12, 80 * MiB + 9))
    d_a, d_b, d_counts = eng.alloc(a.size), eng.alloc(b.size), eng.alloc(256 * 8)
    try:
        eng.upload(d_a, a)
        eng.upload(d_b, b)
        eng.fill(d_counts, 0, 256 * 8)
        for _ in range(3):
            assert lib.aws_huffman_amd_symbol_counts(-1, d_a, a.size, d_counts, eng.stream) == 0
            assert lib.aws_huffman_amd_symbol_counts(-1, d_b + 1, b.size - 1, d_counts, eng2.stream) == 0
        eng.sync()
        eng2.sync()
        got = eng.download(d_counts, 256 * 8).view(np.uint64)
        assert np.array_equal(got, 3 * (ba.bincount(a) + ba.bincount(b[1:])))
    finally:
        for p in (d_a, d_b, d_counts):
            eng.free(p)
        eng2.close()
        lib.aws_huffman_amd_table_coder_destroy(coder2)


def geometric_bytes(n, seed, p=0.25):
    rng = np.random.default_rng(seed)
    return np.minimum(rng.geometric(p, n) - 1, 255).astype(np.uint8)


def fitted_round_trip(lib, eng, oracle, data, lo, hi, flags, one_pass):
    n = data.size
    d_in = eng.alloc(n)
    eng.upload(d_in, data)
    counts = count_on_device(lib, eng, d_in, n)
    assert np.array_equal(counts, ba.bincount(data))
    rc, err, lengths = ba.lengths_from_counts(lib, counts, lo, hi, flags)
    assert rc == 0, err
    coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*lengths))
    assert coder
    rows = ba.coder_rows(coder)
    fitted = harness.Engine(lib, coder)
    try:
        assert bool(lib.aws_huffman_amd_engine_encodes_in_one_pass(fitted.h)) == one_pass
        assert lib.aws_huffman_amd_engine_max_code_bits(fitted.h) <= hi
        bits = sum(int(c) * l for c, l in zip(counts, lengths))
        cap = bits // 8 + 64
        d_in2, d_out, d_back = fitted.alloc(n), fitted.alloc(cap), fitted.alloc(n)
        fitted.upload(d_in2, data)
        plan = fitted.encode_plan([{"in_offset": 0, "in_len": n, "out_offset": 0, "out_capacity": cap}])
        fitted.encode_launch(plan, d_in2, d_out)
        (rc, err, consumed, produced, _, _), = fitted.encode_results(plan, 1)
        assert rc == 0 and consumed == n and produced == math.ceil(bits / 8)
        assert fitted.encode_road(plan) == (1 if one_pass else 0)
        got = fitted.download(d_out, produced)
        ocoder = oracle.lib.oracle_table_coder_new((C.c_uint32 * 256)(*[p for p, _ in rows]),
                                                   (C.c_uint8 * 256)(*[l for _, l in rows]))
        assert np.array_equal(got, oracle.encode_all(ocoder, data))
        dplan = fitted.decode_plan([{"in_offset": 0, "in_len": produced, "out_offset": 0, "out_capacity": n}])
        fitted.decode_launch(dplan, d_out, d_back)
        (rc, err, dproduced, _), = fitted.decode_results(dplan, 1)
        assert rc == 0 and dproduced == n
        stats = fitted.decode_stats(dplan)
        if ba.decode_rule(lengths) == "fixed":
            assert stats["by_blocks"] > 0, stats  # codes of one length (uniform bytes: the flat 8-bit code): dec_fixed
        elif ba.decode_rule(lengths) == "linked":
            # a code past 12 bits: the item is a workgroup's, or (long enough) decoded in blocks across the chip; no chunks
            assert stats["by_workgroup"] + stats["by_wave"] + stats["by_blocks"] > 0 and stats["by_pieces"] == 0, stats
        else:
            assert stats["by_pieces"] > 0, stats
        assert np.array_equal(fitted.download(d_back, n), data)
        lib.aws_huffman_amd_encode_plan_destroy(plan)
        lib.aws_huffman_amd_decode_plan_destroy(dplan)
        for p in (d_in2, d_out, d_back):
            fitted.free(p)
    finally:
        fitted.close()
        eng.free(d_in)
        lib.aws_huffman_amd_table_coder_destroy(coder)
    return lengths


@pytest.mark.parametrize("shape", ["printable", "geometric", "uniform"])
def test_fitted_coder_end_to_end(lib, eng, oracle, shape):
    n = 64 * MiB
    data = {"printable": lambda: harness.printable_map(harness.splitmix64_bytes(21, n)),
            "geometric": lambda: geometric_bytes(n, 22),
            "uniform": lambda: harness.splitmix64_bytes(23, n)}[shape]()
    lengths = fitted_round_trip(lib, eng, oracle, data, 4, 12, ba.CODE_EVERY_SYMBOL, True)
    assert ba.one_pass_rule(lengths) and ba.chunked_decode_rule(lengths)


def test_heavy_bytes_and_a_flat_tail(lib, eng, oracle):
    """A few heavy bytes, a flat tail and three rare bytes at (1, 16), only the bytes that occur coded: most of the codes
    have 11-12 bits and a few more, under more ten-bit prefixes than 8-bit linked tables had room for.  The engine of
    the library's own coder must decode what it encodes."""
    counts = cs.heavy_flat_rare_counts(np.random.default_rng(45))
    once = np.repeat(np.arange(256, dtype=np.uint8), counts.astype(np.int64))
    data = np.tile(once, max(1, 32 * MiB // once.size))
    np.random.default_rng(42).shuffle(data)
    lengths = fitted_round_trip(lib, eng, oracle, data, 1, 16, 0, False)
    assert ba.decode_rule(lengths) == "linked" and not ba.one_pass_rule(lengths), sorted(set(lengths))
    prefixes = {p >> (l - 10) for p, l in ba.canonical_rows(lengths) if l > 10}
    assert len(prefixes) > 60, len(prefixes)  # (more linked tables than fitted before they were narrowed)


def test_no_lower_bound(lib, eng, oracle):
    """90 % zero bytes, min_bits 1: a 1-bit code, which the one-pass encoder does not take (the two-pass road)."""
    n = 32 * MiB + 7
    raw = harness.splitmix64_bytes(31, n)
    data = np.where(raw % 10 != 0, 0, harness.splitmix64_bytes(32, n)).astype(np.uint8)
    lengths = fitted_round_trip(lib, eng, oracle, data, 1, 12, 0, False)
    assert lengths[0] == 1


def test_small_strings_through_the_reference_abi(lib, oracle):
    counts = ba.bincount(np.frombuffer(b"the quick brown fox jumps over the lazy dog " * 50, np.uint8))
    _, _, lengths = ba.lengths_from_counts(lib, counts, 4, 12, ba.CODE_EVERY_SYMBOL)
    coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*lengths))
    rows = ba.coder_rows(coder)
    ocoder = oracle.lib.oracle_table_coder_new((C.c_uint32 * 256)(*[p for p, _ in rows]),
                                               (C.c_uint8 * 256)(*[l for _, l in rows]))
    product = harness.Codec(lib, "aws_")
    try:
        for text in (b"a", b"hello, world", b"the lazy dog", bytes(range(256)), b"\x00\xff" * 999):
            data = np.frombuffer(text, np.uint8)
            got = product.encode_all(coder, data)
            assert np.array_equal(got, oracle.encode_all(ocoder, data)), text
            r, back = product.decode_all(coder, got, data.size)
            assert r.rc == 0 and np.array_equal(back, data), text
    finally:
        lib.aws_huffman_amd_table_coder_destroy(coder)
