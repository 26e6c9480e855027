"""Coder shapes for the sweep of parity_cases.coder_shape_sweep: 256-entry lists of code lengths (0 = no code), whose
canonical code (parity_cases.canonical_code) both libraries are built from.

Everything the engine derives from a coder -- the 12-bit look-up table, the linked tables of longer codes, n_states, the
min_bits / max_bits bounds on outputs and images, fixed_bits, the one-pass rule -- follows from such a list, and the
roads an item takes turn at lengths of 3|4 (one-pass encode), 12|13 (chunked | linked decode), 15|16 (one-pass encode),
at "all 256 symbols coded" and at "all codes of one length".  BOUNDARY names the shapes either side of each of those;
product_shapes / independent_shapes draw more of them from a seed.  expected_roads says, from the lengths alone, which
roads the engine must report: the sweep asserts that, so that a coder which falls from a fast road to a slow one fails.

A plain helper module: no fixtures, no pytest hooks.
"""
import numpy as np

import build_api as ba


def shape(*runs, holes=None):
    """256 lengths from (how many symbols, code length) runs in symbol order, the rest uncoded; holes(s) -> True takes
    symbol s's code away again."""
    lengths = [l for count, l in runs for _ in range(count)]
    assert len(lengths) <= 256
    lengths += [0] * (256 - len(lengths))
    if holes:
        lengths = [0 if holes(s) else l for s, l in enumerate(lengths)]
    assert ba.kraft_ok(lengths) and any(lengths)
    return lengths


LEN4TO12 = [(8, 4), (16, 6), (32, 8), (64, 10), (136, 12)]  # parity_cases.CODER_PROFILES["len4to12"]
# what aws_huffman_amd_code_lengths_from_counts made of a few heavy bytes, a flat tail and three rare bytes at (1, 16): a
# complete code with a handful of codes past 12 bits and codes of 11 .. 15 bits under some 120 ten-bit prefixes
FITTED_EXAMPLE = [(2, 2), (3, 3), (1, 4), (9, 11), (237, 12), (1, 13), (1, 14), (2, 15)]

BOUNDARY = {
    # decode table of 1 bit, both windows a code: fixed_bits 1, fixed_complete; 8192 symbols a sub-chunk
    "2x1": shape((2, 1)),
    # one code in all: min_bits == max_bits == 1, half the windows without a code; every stream is one symbol repeated
    "1x1": shape((1, 1)),
    # three symbols, complete: lut_bits 2, n_states at its floor of 8
    "1,2,2": shape((1, 1), (2, 2)),
    # all 256 coded and min_bits 1 beside max_bits 12: the widest spread the chunk kernels take (1024 symbols a lane)
    "1,2,3,4+252x12": shape((1, 1), (1, 2), (1, 3), (1, 4), (252, 12)),
    # all 256 coded, a 1-bit code, max 12: not one-pass for the 1-bit code alone; lut_bits 12, incomplete
    "1,3,5,5,4x7,8x9+240x12": shape((1, 1), (1, 3), (2, 5), (4, 7), (8, 9), (240, 12)),
    # four symbols of one length: fixed_bits 2, complete, 252 symbols uncoded
    "4x2": shape((4, 2)),
    # all coded but min_bits 3: one bit below the one-pass rule's 4
    "4x3,8x5,16x7,32x9,196x12": shape((4, 3), (8, 5), (16, 7), (32, 9), (196, 12)),
    # fixed_bits 11: dec_fixed with a symbol every 11 bits, 1/8 of the windows a code; one-pass encode
    "256x11": shape((256, 11)),
    # fixed_bits at HUFD_DEC_MAX_LUT_BITS, the last length dec_fixed takes; one-pass encode
    "256x12": shape((256, 12)),
    # one length, but past 12 bits: linked tables, not dec_fixed; n_states 13
    "256x13": shape((256, 13)),
    # the last length of the one-pass encoder (5-word octs); linked tables under 8 ten-bit prefixes, 32 codes each
    "256x15": shape((256, 15)),
    # one bit past the one-pass rule: count / scan / pack; n_states 16 = HUFD_DEC_MAX_STATES
    "256x16": shape((256, 16)),
    # len4to12 with its last symbol one bit longer: max_bits 13, the first length of the linked tables; still one-pass
    "len4to12,last13": shape(*LEN4TO12[:-1], (135, 12), (1, 13)),
    # ... at 15: the last one-pass length, reached by one symbol only
    "len4to12,last15": shape(*LEN4TO12[:-1], (135, 12), (1, 15)),
    # ... at 16: one symbol takes the coder off the one-pass road
    "len4to12,last16": shape(*LEN4TO12[:-1], (135, 12), (1, 16)),
    # max_bits 32 with min_bits 32: the widest images and stages (4 bytes a symbol), three levels of linked tables
    "200x32": shape((200, 32)),
    # min_bits 1 beside max_bits 32: output bounds of 8 symbols a byte next to images of 4 bytes a symbol
    "1x1+255x32": shape((1, 1), (255, 32)),
    # holes: every third symbol without a code (encode stops there), the decode table with windows of no code
    "len4to12,holes": shape(*LEN4TO12, holes=lambda s: s % 3 == 2),
    # 128 ten-bit prefixes with 11-bit codes below them and one 13-bit code: 128 linked tables, 127 of them narrowed to
    # one bit; at full width (256 entries each) they would be twice what the kernels keep in LDS
    "255x11+1x13": shape((255, 11), (1, 13)),
    # 9-bit codes answered by the root, then 64 prefixes of 11-bit codes and the 13-bit one
    "128x9,127x11,1x13": shape((128, 9), (127, 11), (1, 13)),
    # 63 linked tables, 62 of them narrowed: one more than 16 384 entries hold at full width beside the root (60)
    "124x11+1x13": shape((124, 11), (1, 13)),
    # the fitted example: what the library's own build path hands out
    "fitted(1,16)": shape(*FITTED_EXAMPLE),
}

BOUNDS = [(1, 8), (1, 12), (1, 13), (3, 12), (4, 12), (4, 13), (4, 15), (4, 16), (1, 32), (6, 32)]


def heavy_flat_rare_counts(rng):
    """A few heavy bytes, a flat tail and three rare bytes: optimal lengths put the tail at 11-12 bits and the rare
    bytes a few bits past it."""
    n_heavy = int(rng.integers(2, 9))
    order = rng.permutation(256)
    counts = np.zeros(256, np.uint64)
    tail = int(rng.integers(200, 5000))
    counts[order] = rng.integers(tail, tail + max(tail // 8, 2), 256)
    counts[order[:n_heavy]] = rng.integers(40, 400, n_heavy) * tail
    counts[order[-3:]] = rng.integers(1, 4, 3)
    return counts


def random_counts(rng):
    family = int(rng.integers(0, 5))
    if family == 0:
        return heavy_flat_rare_counts(rng)
    if family == 1:  # geometric: a long code, whatever the bound lets through
        ratio = float(rng.uniform(0.5, 0.97))
        return np.maximum(1, (float(1 << 40) * ratio ** rng.permutation(256))).astype(np.uint64)
    if family == 2:  # a few symbols only
        counts = np.zeros(256, np.uint64)
        n = int(rng.integers(1, 20))
        counts[rng.choice(256, n, replace=False)] = rng.integers(1, 1000, n)
        return counts
    if family == 3:  # flat
        return rng.integers(900, 1100, 256).astype(np.uint64)
    counts = rng.integers(0, 1 << int(rng.integers(1, 30)), 256).astype(np.uint64)  # anything, zeros included
    counts[int(rng.integers(0, 256))] += 1
    return counts


def product_shapes(lib, seed, n, max_bits=None):
    """n shapes through the product's own build path: random counts into aws_huffman_amd_code_lengths_from_counts (lib: a
    library with build_api.bind on it), bounds from BOUNDS (or (1, max_bits)), with and without CODE_EVERY_SYMBOL."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        counts = random_counts(rng) if k % 2 else heavy_flat_rare_counts(rng)
        lo, hi = BOUNDS[int(rng.integers(0, len(BOUNDS)))] if max_bits is None else (1, max_bits)
        flags = ba.CODE_EVERY_SYMBOL if rng.integers(0, 2) else 0
        rc, err, lengths = ba.lengths_from_counts(lib, counts, lo, hi, flags)
        assert rc == 0, (err, lo, hi, flags, list(counts))
        assert ba.kraft_ok(lengths) and all(l == 0 or lo <= l <= hi for l in lengths), (lo, hi, flags, lengths)
        assert (0 in lengths) == (not flags and bool((counts == 0).any())), (lo, hi, flags)
        out.append(("fitted(%d,%d)%s seed %d #%d" % (lo, hi, "+every" if flags else "", seed, k), lengths))
    return out


def independent_shapes(seed, n):
    """n shapes that owe nothing to the product: a code tree grown by splitting random leaves down to a random depth
    limit, then leaves dropped or pushed down (incomplete codes, Kraft < 1), on random symbols (holes)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        limit = int(rng.choice([2, 3, 4, 8, 11, 12, 13, 15, 16, 20, 32]))
        n_syms = int(rng.choice([1, 2, 3, int(rng.integers(4, 256)), 256]))
        n_syms = min(n_syms, 1 << limit)
        leaves = [int(rng.integers(1, limit + 1))] if n_syms == 1 else [1, 1]
        deepen = float(rng.uniform(0.0, 0.9))  # how often the leaf that was just made is split again: skew
        at = 0
        while len(leaves) < n_syms:
            splittable = [i for i, d in enumerate(leaves) if d < limit]
            if not (rng.random() < deepen and leaves[at] < limit):
                at = splittable[int(rng.integers(0, len(splittable)))]
            leaves[at] += 1
            leaves.append(leaves[at])
            at = len(leaves) - 1
        kind = int(rng.integers(0, 3))
        if kind == 1 and len(leaves) > 1:  # incomplete: some leaves are nobody's
            leaves = [d for d in leaves if rng.random() < 0.8] or leaves[:1]
        elif kind == 2:  # incomplete: some codes longer than they need to be
            leaves = [min(limit, d + int(rng.integers(0, 3))) if rng.random() < 0.3 else d for d in leaves]
        lengths = [0] * 256
        for s, d in zip(rng.permutation(256), leaves):
            lengths[int(s)] = int(d)
        assert ba.kraft_ok(lengths) and any(lengths)
        out.append(("grown(limit %d, %d symbols) seed %d #%d" % (limit, len(leaves), seed, k), lengths))
    return out


def random_shapes(lib, seed, n):
    """Half through the product's build path, half through the independent generator."""
    return product_shapes(lib, seed, n - n // 2) + independent_shapes(seed, n // 2)


def expected_roads(lengths):
    """From the lengths alone, never from the engine: {"one_pass": encode plans run as the one-pass kernel,
    "decode": "fixed" (dec_fixed_*), "linked" (linked tables, an item a thread / workgroup / blocks of dec_wide_*) or
    "chunked" (sync + scan + emit)}."""
    return {"one_pass": ba.one_pass_rule(lengths), "decode": ba.decode_rule(lengths)}


ROAD_CLASSES = ("one-pass encode", "other encode", "chunked decode", "fixed decode", "linked decode")


def road_classes(lengths):
    roads = expected_roads(lengths)
    return ("one-pass encode" if roads["one_pass"] else "other encode", roads["decode"] + " decode")
