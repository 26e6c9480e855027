"""ctypes face of include/aws/compression/huffman_amd_build.h (coders built from data) and the pure-Python yardsticks
the tests measure it against: an exact search for optimal bounded code lengths, heapq Huffman, plain package-merge."""
import ctypes as C
import heapq
import os
import sys

import numpy as np

import harness

CODE_EVERY_SYMBOL = 1
U64x256 = C.c_uint64 * 256
U8x256 = C.c_uint8 * 256


def bind(lib):
    """Declares the five entry points of huffman_amd_build.h on a loaded product (or emulator) library."""
    P, V = C.POINTER, C.c_void_p
    lib.aws_huffman_amd_symbol_counts.restype = C.c_int
    lib.aws_huffman_amd_symbol_counts.argtypes = [C.c_int, V, C.c_uint64, V, V]
    lib.aws_huffman_amd_code_lengths_from_counts.restype = C.c_int
    lib.aws_huffman_amd_code_lengths_from_counts.argtypes = [P(C.c_uint64), C.c_uint32, C.c_uint32, C.c_uint32, P(C.c_uint8)]
    lib.aws_huffman_amd_table_coder_from_lengths.restype = P(harness.SymbolCoder)
    lib.aws_huffman_amd_table_coder_from_lengths.argtypes = [P(C.c_uint8)]
    lib.aws_huffman_amd_table_coder_to_def.restype = C.c_int
    lib.aws_huffman_amd_table_coder_to_def.argtypes = [P(harness.SymbolCoder), C.c_char_p, C.c_size_t, P(C.c_size_t)]
    lib.aws_huffman_amd_testing_set_count_flush_bytes.restype = None
    lib.aws_huffman_amd_testing_set_count_flush_bytes.argtypes = [C.c_uint64]
    return lib


def lengths_from_counts(lib, counts, lo, hi, flags=0):
    """(rc, error, list of 256 lengths)."""
    lib.aws_reset_error()
    out = U8x256()
    rc = lib.aws_huffman_amd_code_lengths_from_counts(U64x256(*[int(c) for c in counts]), lo, hi, flags, out)
    return rc, lib.aws_last_error() if rc else 0, list(out)


def coder_rows(coder):
    """[(pattern, num_bits)] * 256 through the coder's encode callback."""
    enc = harness.ENCODE_FN(coder.contents.encode)
    rows = []
    for s in range(256):
        c = enc(s, coder.contents.userdata)
        rows.append((c.pattern, c.num_bits))
    return rows


def to_def(lib, coder):
    need = C.c_size_t()
    lib.aws_reset_error()
    assert lib.aws_huffman_amd_table_coder_to_def(coder, None, 0, C.byref(need)) == -1
    assert lib.aws_last_error() == harness.AWS_ERROR_SHORT_BUFFER
    buf = C.create_string_buffer(need.value)
    got = C.c_size_t()
    assert lib.aws_huffman_amd_table_coder_to_def(coder, buf, need.value, C.byref(got)) == 0
    assert got.value == need.value
    return buf.raw[: got.value]


def cost(counts, lengths):
    return sum(int(c) * int(l) for c, l in zip(counts, lengths))


def kraft_ok(lengths):
    return sum(1 << (32 - l) for l in lengths if l) <= 1 << 32


def exact_optimum(weights, n_zero, lo, hi):
    """The least sum(w * length) over prefix codes with lengths in [lo, hi] for the symbols of these (positive) weights
    plus n_zero symbols of weight 0, by a search over levels: sorted heaviest first, the symbols take lengths in order
    (an optimal code never gives a heavier symbol a longer code); at level l with `a` free nodes the next symbol takes
    one, or every free node splits in two for level l + 1.  Zero-weight symbols go to level hi, where they cost nothing
    but the room they need.  None: no such code."""
    w = sorted(weights, reverse=True)
    n = len(w)
    sys.setrecursionlimit(10000)
    memo = {}

    def best(level, i, free):
        if i == n:
            return 0 if free * (1 << (hi - level)) >= n_zero else None
        key = (level, i, free)
        if key in memo:
            return memo[key]
        options = []
        if free > 0:
            rest = best(level, i + 1, free - 1)
            if rest is not None:
                options.append(w[i] * level + rest)
        if level < hi and free > 0:
            need_zero = -(-n_zero // (1 << (hi - level - 1)))
            cap = (n - i) + need_zero  # more free nodes than this serve nobody
            rest = best(level + 1, i, min(2 * free, cap))
            if rest is not None:
                options.append(rest)
        memo[key] = min(options) if options else None
        return memo[key]

    start = min(1 << lo, n + -(-n_zero // (1 << (hi - lo))))
    return best(lo, 0, start)


def huffman_lengths(counts):
    """Plain Huffman (heapq) over the symbols with a count > 0: {symbol: length}."""
    heap = [(c, s, (s,)) for s, c in enumerate(counts) if c > 0]
    if len(heap) == 1:
        return {heap[0][1]: 1}
    depth = {s: 0 for _, s, _ in heap}
    heapq.heapify(heap)
    tie = 256
    while len(heap) > 1:
        c1, _, a = heapq.heappop(heap)
        c2, _, b = heapq.heappop(heap)
        for s in a + b:
            depth[s] += 1
        heapq.heappush(heap, (c1 + c2, tie, a + b))
        tie += 1
    return depth


def package_merge_cost(weights, limit):
    """Least sum(w * length) with lengths in [1, limit] (Kraft <= 1), by plain package-merge on the coin lists."""
    items = sorted((w, (i,)) for i, w in enumerate(weights))
    n = len(weights)
    merged = list(items)
    for _ in range(limit - 1):
        packages = [(merged[k][0] + merged[k + 1][0], merged[k][1] + merged[k + 1][1]) for k in range(0, len(merged) - 1, 2)]
        merged = sorted(items + packages, key=lambda x: x[0])
    lengths = [0] * n
    for _, members in merged[: 2 * n - 2]:
        for i in members:
            lengths[i] += 1
    return sum(w * l for w, l in zip(weights, lengths))


def one_pass_rule(lengths):
    """hufk_encode_one_pass_applies: every symbol coded, codes of 4 .. 15 bits."""
    return all(4 <= l <= 15 for l in lengths)


def chunked_decode_rule(lengths):
    """HUFD_DEC_MAX_LUT_BITS: codes of at most 12 bits decode through the 12-bit table -- by the chunk kernels, or, when
    all codes have one length, by dec_fixed (decode_rule tells the two apart)."""
    return max(lengths) <= 12


def decode_rule(lengths):
    """Which decoder a coder of these lengths (0 = no code) gets: "linked" (a code of more than HUFD_DEC_MAX_LUT_BITS bits:
    linked tables, an item a thread / a workgroup / blocks of dec_wide), "fixed" (all codes of one length: dec_fixed,
    symbol k at bit k * length) or "chunked" (sync + scan + emit over chunks of 32 KiB)."""
    coded = [l for l in lengths if l]
    if max(coded) > 12:
        return "linked"
    return "fixed" if min(coded) == max(coded) else "chunked"


def skewed_geometric_counts(n_symbols=256, ratio=0.7, scale=1 << 40):
    """Counts falling by `ratio` from symbol to symbol: Huffman gives this a code far longer than 12 bits."""
    return [max(1, int(scale * ratio ** s)) for s in range(n_symbols)]


def canonical_rows(lengths):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import parity_cases

    patterns, lens = parity_cases.canonical_code(lengths)
    return list(zip(patterns, lens))


def bincount(arr):
    return np.bincount(np.asarray(arr, dtype=np.uint8), minlength=256).astype(np.uint64)
