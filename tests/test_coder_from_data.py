"""CPU checks of huffman_amd_build.h's host half on the product library (no device needed): optimal length-limited code
lengths from counts, the canonical coder of those lengths, its table as .def text, and that text through the reference's
own generator."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import build_api as ba
import coder_shapes as cs
import harness


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(harness.PRODUCT_SO):
        import __graft_entry__

        __graft_entry__.build()
    return ba.bind(harness.load_product())


def check_lengths(counts, lengths, lo, hi, every):
    coded = [s for s in range(256) if counts[s] > 0 or every]
    assert all((lengths[s] != 0) == (s in set(coded)) for s in range(256))
    assert all(lo <= lengths[s] <= hi for s in coded)
    assert ba.kraft_ok(lengths)
    for a in coded:  # a higher count never gets a longer code; equal counts: lengths non-decreasing in symbol value
        for b in coded:
            if counts[a] > counts[b]:
                assert lengths[a] <= lengths[b], (a, b)
            if counts[a] == counts[b] and a < b:
                assert lengths[a] <= lengths[b], (a, b)


@pytest.mark.parametrize("lo,hi", [(1, 6), (2, 8), (4, 12), (1, 32)])
@pytest.mark.parametrize("every", [False, True])
def test_optimal_on_small_alphabets(lib, lo, hi, every):
    rng = random.Random(lo * 100 + hi + every)
    for trial in range(6):
        n = rng.randint(1, 48 if hi > 6 else 40)
        symbols = rng.sample(range(256), n)
        counts = [0] * 256
        for s in symbols:
            counts[s] = rng.choice([1, rng.randint(1, 20), rng.randint(1, 10 ** 6), rng.randint(1, 10 ** 12)])
        if trial == 0:
            for s in symbols:
                counts[s] = 7  # all equal
        flags = ba.CODE_EVERY_SYMBOL if every else 0
        n_coded = 256 if every else n
        rc, err, lengths = ba.lengths_from_counts(lib, counts, lo, hi, flags)
        if n_coded > (1 << hi):
            assert rc == -1 and err == harness.AWS_ERROR_INVALID_ARGUMENT
            continue
        assert rc == 0, err
        check_lengths(counts, lengths, lo, hi, every)
        want = ba.exact_optimum([counts[s] for s in symbols], n_coded - n, lo, hi)
        assert ba.cost(counts, lengths) == want, (lo, hi, every, trial)


def test_matches_huffman_where_it_fits(lib):
    rng = random.Random(7)
    for trial in range(20):
        counts = [rng.randint(1, 1000) for _ in range(256)]
        huff = ba.huffman_lengths(counts)
        lo, hi = min(huff.values()), max(huff.values())
        rc, _, lengths = ba.lengths_from_counts(lib, counts, lo, hi)
        assert rc == 0
        assert ba.cost(counts, lengths) == sum(counts[s] * l for s, l in huff.items())
        rc, _, lengths = ba.lengths_from_counts(lib, counts, 1, 32)
        assert rc == 0 and ba.cost(counts, lengths) == sum(counts[s] * l for s, l in huff.items())


def test_limited_below_huffman(lib):
    counts = ba.skewed_geometric_counts()
    assert max(ba.huffman_lengths(counts).values()) > 12
    for hi in (9, 10, 12, 15):
        rc, _, lengths = ba.lengths_from_counts(lib, counts, 1, hi)
        assert rc == 0 and max(lengths) <= hi
        check_lengths(counts, lengths, 1, hi, False)
        assert ba.cost(counts, lengths) == ba.package_merge_cost(counts, hi), hi


def test_fast_path_rules_by_construction(lib):
    rng = random.Random(11)
    shapes = [ba.skewed_geometric_counts(), [1] * 256, [0] * 255 + [5], [10 ** 9 if s < 3 else 0 for s in range(256)],
              [rng.randint(0, 10 ** rng.randint(0, 15)) for _ in range(256)]]
    for counts in shapes:
        rc, _, lengths = ba.lengths_from_counts(lib, counts, 4, 12, ba.CODE_EVERY_SYMBOL)
        assert rc == 0
        assert ba.one_pass_rule(lengths) and ba.chunked_decode_rule(lengths)
        check_lengths(counts, lengths, 4, 12, True)


def test_edge_cases(lib):
    bad = harness.AWS_ERROR_INVALID_ARGUMENT
    one = [0] * 256
    one[65] = 1000
    rc, _, lengths = ba.lengths_from_counts(lib, one, 3, 9)
    assert rc == 0 and lengths[65] == 3 and sum(lengths) == 3  # one coded symbol: min_bits
    rc, _, lengths = ba.lengths_from_counts(lib, one, 1, 1)
    assert rc == 0 and lengths[65] == 1
    zero = [0] * 256
    assert ba.lengths_from_counts(lib, zero, 1, 12)[:2] == (-1, bad)
    rc, _, lengths = ba.lengths_from_counts(lib, zero, 1, 12, ba.CODE_EVERY_SYMBOL)
    assert rc == 0 and lengths == [8] * 256  # no counts: the flat code
    ones = [1] * 256
    rc, _, lengths = ba.lengths_from_counts(lib, ones, 1, 8)
    assert rc == 0 and lengths == [8] * 256
    assert ba.lengths_from_counts(lib, ones, 1, 7)[:2] == (-1, bad)
    assert ba.lengths_from_counts(lib, ones, 9, 8)[:2] == (-1, bad)  # min > max
    assert ba.lengths_from_counts(lib, ones, 1, 33)[:2] == (-1, bad)
    assert ba.lengths_from_counts(lib, ones, 0, 12)[:2] == (-1, bad)
    assert ba.lengths_from_counts(lib, ones, 1, 12, 2)[:2] == (-1, bad)  # unknown flag
    rc, _, lengths = ba.lengths_from_counts(lib, [1 << 50] * 255 + [0], 1, 12)  # 2^58 - 2^50 in all
    assert rc == 0 and lengths == [7] + [8] * 254 + [0]
    assert ba.lengths_from_counts(lib, [1 << 50] * 256, 1, 12)[:2] == (-1, bad)  # 2^58 in all
    big = [0] * 256
    big[0], big[1] = (1 << 57), (1 << 57)  # total 2^58
    assert ba.lengths_from_counts(lib, big, 1, 12)[:2] == (-1, bad)
    big[1] = (1 << 57) - 1
    assert ba.lengths_from_counts(lib, big, 1, 12)[0] == 0
    assert ba.lengths_from_counts(lib, [(1 << 64) - 1] + [0] * 255, 1, 12)[:2] == (-1, bad)
    # all 256 coded with a lower bound of 8 and room for more: the flat code, whatever the counts
    rc, _, lengths = ba.lengths_from_counts(lib, ba.skewed_geometric_counts(), 8, 12)
    assert rc == 0 and lengths == [8] * 256
    rc, _, lengths = ba.lengths_from_counts(lib, ba.skewed_geometric_counts(), 32, 32)
    assert rc == 0 and lengths == [32] * 256


def decode_all(coder, rows):
    dec = harness.DECODE_FN(coder.contents.decode)
    sym = C.c_uint8()
    for s, (pattern, n) in enumerate(rows):
        if not n:
            continue
        left = (pattern << (32 - n)) & 0xFFFFFFFF
        for fill in (0, (1 << (32 - n)) - 1):
            assert dec(left | fill, C.byref(sym), coder.contents.userdata) == n and sym.value == s, (s, n, fill)


def test_canonical_coder(lib):
    for counts, lo, hi, flags in [(ba.skewed_geometric_counts(), 4, 12, ba.CODE_EVERY_SYMBOL),
                                  (ba.skewed_geometric_counts(), 1, 32, 0),
                                  ([5 if s % 3 == 0 else 0 for s in range(256)], 1, 15, 0),
                                  ([1] * 256, 1, 8, 0)]:
        rc, _, lengths = ba.lengths_from_counts(lib, counts, lo, hi, flags)
        assert rc == 0
        coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*lengths))
        assert coder
        rows = ba.coder_rows(coder)
        assert rows == ba.canonical_rows(lengths)
        decode_all(coder, rows)
        lib.aws_huffman_amd_table_coder_destroy(coder)
    # Kraft > 1, a length > 32
    for lengths in ([1, 1, 1] + [0] * 253, [8] * 255 + [7], [33] + [0] * 255):
        lib.aws_reset_error()
        assert not lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*lengths))
        assert lib.aws_last_error() == harness.AWS_ERROR_INVALID_ARGUMENT
    # a complete code with a 32-bit code in it
    lengths = [0] * 256
    for s in range(32):
        lengths[s] = s + 1
    lengths[32] = 32
    coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*lengths))
    assert coder and ba.coder_rows(coder) == ba.canonical_rows(lengths)
    decode_all(coder, ba.coder_rows(coder))
    lib.aws_huffman_amd_table_coder_destroy(coder)


def test_def_round_trip(lib):
    holes = [0] * 256
    for s in range(0, 256, 5):
        holes[s] = 1 + s
    cases = [(ba.skewed_geometric_counts(), 4, 12, ba.CODE_EVERY_SYMBOL), (holes, 1, 16, 0)]
    for counts, lo, hi, flags in cases:
        _, _, lengths = ba.lengths_from_counts(lib, counts, lo, hi, flags)
        coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*lengths))
        text = ba.to_def(lib, coder)
        assert text.count(b"HUFFMAN_CODE(") == sum(1 for l in lengths if l)
        back = lib.aws_huffman_amd_table_coder_from_def(text, len(text))
        assert back
        assert ba.coder_rows(back) == ba.coder_rows(coder)
        # a buffer one byte short: SHORT_BUFFER, the length needed
        need = C.c_size_t()
        small = C.create_string_buffer(len(text))
        lib.aws_reset_error()
        assert lib.aws_huffman_amd_table_coder_to_def(coder, small, len(text) - 1, C.byref(need)) == -1
        assert lib.aws_last_error() == harness.AWS_ERROR_SHORT_BUFFER and need.value == len(text)
        lib.aws_huffman_amd_table_coder_destroy(back)
        lib.aws_huffman_amd_table_coder_destroy(coder)
    # any coder: the reference's test table
    patterns, lens = harness.load_table()
    coder = lib.aws_huffman_amd_table_coder_new(patterns, lens)
    text = ba.to_def(lib, coder)
    back = lib.aws_huffman_amd_table_coder_from_def(text, len(text))
    assert ba.coder_rows(back) == ba.coder_rows(coder)


@pytest.mark.parametrize("max_bits", [13, 15, 16, 20, 32])
def test_swept_coders_def_round_trip(lib, max_bits):
    """Every coder the build path makes of the random count families of tests/coder_shapes.py (half of them a few heavy
    bytes, a flat tail and three rare bytes) at (1, max_bits): its .def text gives the same coder back."""
    for name, lengths in cs.product_shapes(lib, 300 + max_bits, 40, max_bits=max_bits):
        coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*lengths))
        assert coder, name
        rows = ba.coder_rows(coder)
        assert rows == ba.canonical_rows(lengths), name
        text = ba.to_def(lib, coder)
        back = lib.aws_huffman_amd_table_coder_from_def(text, len(text))
        assert back and ba.coder_rows(back) == rows, name
        decode_all(back, rows)
        lib.aws_huffman_amd_table_coder_destroy(back)
        lib.aws_huffman_amd_table_coder_destroy(coder)


@pytest.mark.parametrize("max_bits", [13, 15, 16, 20, 32])
def test_swept_coders_can_be_decoded(lib, max_bits):
    """... and an engine of it decodes (the emulator library: an engine needs a device): whatever
    aws_huffman_amd_table_coder_from_lengths returns, the linked decode tables hold."""
    emu_dir = os.path.join(harness.REPO, "tests", "emu")
    subprocess.check_call(["make", "-s", "-C", emu_dir], stdout=subprocess.DEVNULL)
    emu = ba.bind(harness.load_product(os.path.join(emu_dir, "libaws-c-compression-emu.so")))
    past_12 = 0
    for name, lengths in cs.product_shapes(lib, 300 + max_bits, 40, max_bits=max_bits):
        coder = emu.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*lengths))
        assert coder, name
        eng = harness.Engine(emu, coder)
        assert emu.aws_huffman_amd_engine_can_decode(eng.h), (name, sorted(set(lengths)))
        assert emu.aws_huffman_amd_engine_max_code_bits(eng.h) == max(lengths), name
        past_12 += max(lengths) > 12
        eng.close()
        emu.aws_huffman_amd_table_coder_destroy(coder)
    assert past_12 >= 10, past_12  # (the linked tables are what this is about)


GENERATOR = os.path.join(harness.REPO, "oracle", "_ref", "huffman_generator")


@pytest.mark.skipif(not os.path.exists(GENERATOR), reason="oracle/_ref/huffman_generator not built (make -C oracle ref)")
@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_def_through_the_reference_generator(lib, tmp_path):
    holes = [0] * 256
    for s in range(0, 256, 3):
        holes[s] = (s * 7919) % 1000 + 1
    cases = [("fitted", ba.skewed_geometric_counts(), 4, 12, ba.CODE_EVERY_SYMBOL), ("holes", holes, 1, 16, 0),
             ("flat", [1] * 256, 1, 8, 0)]
    include = os.path.join(harness.REPO, "include")
    for name, counts, lo, hi, flags in cases:
        _, _, lengths = ba.lengths_from_counts(lib, counts, lo, hi, flags)
        coder = lib.aws_huffman_amd_table_coder_from_lengths(ba.U8x256(*lengths))
        def_path, c_path, so_path = tmp_path / (name + ".def"), tmp_path / (name + ".c"), tmp_path / (name + ".so")
        def_path.write_bytes(ba.to_def(lib, coder))
        subprocess.check_call([GENERATOR, str(def_path), str(c_path), name])
        subprocess.check_call(["gcc", "-O1", "-std=c99", "-shared", "-fPIC", "-I" + include,
                               "-I" + os.path.join(include, "compat"), str(c_path), "-o", str(so_path)])
        gen = C.CDLL(str(so_path))
        getter = getattr(gen, name + "_get_coder")
        getter.restype = C.POINTER(harness.SymbolCoder)
        theirs = getter()
        assert ba.coder_rows(theirs) == ba.coder_rows(coder)
        dec_t = harness.DECODE_FN(theirs.contents.decode)
        dec_o = harness.DECODE_FN(coder.contents.decode)
        st, so = C.c_uint8(), C.c_uint8()
        for prefix in range(1 << 16):
            bits = prefix << 16
            nt = dec_t(bits, C.byref(st), theirs.contents.userdata)
            no = dec_o(bits, C.byref(so), coder.contents.userdata)
            assert nt == no and (nt == 0 or st.value == so.value), (name, prefix)
        lib.aws_huffman_amd_table_coder_destroy(coder)
