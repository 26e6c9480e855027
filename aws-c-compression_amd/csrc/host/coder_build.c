/*
 * Coders from data (huffman_amd_build.h): code lengths for 256 symbol counts, the canonical coder of those lengths, and
 * a coder's table as .def text.  The counts themselves come from the device (aws_huffman_amd_symbol_counts, engine.c,
 * count_kernels.hip); everything here is a few microseconds of host work on 256 numbers.
 *
 * Lengths: package-merge (Larmore and Hirschberg 1990) with the lower bound folded in.  With l = min_bits + d and
 * 0 <= d <= D = max_bits - min_bits, Kraft's sum(2^-l) <= 1 reads sum(2^-d) <= 2^min_bits, and since
 * 2^-d = 1 - (2^-1 + ... + 2^-d) that is: the coins 2^-1 .. 2^-d of every coded symbol (each coin costing the symbol's
 * count) add up to at least X = n - 2^min_bits.  The cheapest such choice of coins is the coin collector's problem,
 * which package-merge solves exactly: lists for the denominations 2^-D .. 2^-1, each the symbols' coins merged with the
 * pairs ("packages") of the list below it, and the 2 X cheapest items of the 2^-1 list taken.  A symbol's d is the
 * number of its coins taken.  X <= 0: every coded symbol gets min_bits.
 */
#include <aws/compression/huffman_amd_build.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define COUNTS_LIMIT (1ull << 58) /* a package holds at most 31 coins of each symbol: its weight stays below 2^63 */

struct pm_item {
    uint64_t weight;
    int32_t symbol; /* -1: a package of two items of the list below */
};

struct by_count {
    uint64_t count;
    int symbol;
};

/* the cheapest first; among equal counts the higher symbol first (it is taken first and ends up no shorter) */
static int leaf_order(const void *a, const void *b) {
    const struct by_count *x = a, *y = b;
    if (x->count != y->count) {
        return x->count < y->count ? -1 : 1;
    }
    return y->symbol - x->symbol;
}

/* the highest count first; among equal counts the lower symbol first */
static int length_order(const void *a, const void *b) {
    const struct by_count *x = a, *y = b;
    if (x->count != y->count) {
        return x->count > y->count ? -1 : 1;
    }
    return x->symbol - y->symbol;
}

int aws_huffman_amd_code_lengths_from_counts(
    const uint64_t counts[256],
    uint32_t min_bits,
    uint32_t max_bits,
    uint32_t flags,
    uint8_t num_bits[256]) {

    if (!counts || !num_bits || (flags & ~AWS_HUFFMAN_AMD_CODE_EVERY_SYMBOL) || min_bits < 1 || max_bits > 32 ||
        min_bits > max_bits) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    struct by_count leaves[256];
    int n = 0;
    uint64_t total = 0;
    for (int s = 0; s < 256; ++s) {
        if (counts[s] >= COUNTS_LIMIT - total) {
            return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
        }
        total += counts[s];
        if (counts[s] || (flags & AWS_HUFFMAN_AMD_CODE_EVERY_SYMBOL)) {
            leaves[n].count = counts[s];
            leaves[n].symbol = s;
            ++n;
        }
    }
    if (n == 0 || (uint64_t)n > (1ull << max_bits)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    qsort(leaves, (size_t)n, sizeof(leaves[0]), leaf_order);

    uint32_t extra[256] = {0}; /* d of leaves[i] */
    const int64_t x = min_bits >= 9 ? -1 : (int64_t)n - (int64_t)(1u << min_bits);
    if (x > 0) {
        const uint32_t depth = max_bits - min_bits; /* >= 1: n <= 2^max_bits and n > 2^min_bits */
        struct pm_item *lists = malloc(sizeof(struct pm_item) * 512u * depth);
        uint32_t *sizes = malloc(sizeof(uint32_t) * depth);
        if (!lists || !sizes) {
            free(lists);
            free(sizes);
            return aws_raise_error(AWS_ERROR_OOM);
        }
        /* list k (k = 0 .. depth - 1) is the list of denomination 2^-(k + 1); built from the deepest up */
        for (int k = (int)depth - 1; k >= 0; --k) {
            struct pm_item *out = lists + 512u * (uint32_t)k;
            const struct pm_item *below = k + 1 < (int)depth ? lists + 512u * (uint32_t)(k + 1) : NULL;
            const uint32_t packages = below ? sizes[k + 1] / 2 : 0;
            uint32_t li = 0, pi = 0, m = 0;
            while (li < (uint32_t)n || pi < packages) {
                const uint64_t pw = pi < packages ? below[2 * pi].weight + below[2 * pi + 1].weight : 0;
                if (li < (uint32_t)n && (pi >= packages || leaves[li].count <= pw)) {
                    out[m].weight = leaves[li].count;
                    out[m].symbol = (int32_t)li;
                    ++li;
                } else {
                    out[m].weight = pw;
                    out[m].symbol = -1;
                    ++pi;
                }
                ++m;
            }
            sizes[k] = m;
        }
        uint64_t take = 2u * (uint64_t)x;
        const bool feasible = take <= sizes[0];
        for (uint32_t k = 0; feasible && k < depth && take; ++k) {
            uint64_t packages = 0;
            for (uint64_t i = 0; i < take; ++i) {
                const struct pm_item *it = &lists[512u * k + i];
                if (it->symbol >= 0) {
                    ++extra[it->symbol];
                } else {
                    ++packages;
                }
            }
            take = 2 * packages;
        }
        free(lists);
        free(sizes);
        if (!feasible) {
            return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
        }
    }

    /* The same multiset of lengths, the shortest to the highest count (ties: the lower symbol): Kraft's sum does not
     * change, the cost cannot grow, and the promises on order hold whatever order the lists took ties in. */
    uint8_t lengths[256];
    for (int i = 0; i < n; ++i) {
        lengths[i] = (uint8_t)(min_bits + extra[i]);
    }
    for (int i = 1; i < n; ++i) { /* ascending */
        const uint8_t v = lengths[i];
        int j = i - 1;
        while (j >= 0 && lengths[j] > v) {
            lengths[j + 1] = lengths[j];
            --j;
        }
        lengths[j + 1] = v;
    }
    qsort(leaves, (size_t)n, sizeof(leaves[0]), length_order);
    memset(num_bits, 0, 256);
    for (int i = 0; i < n; ++i) {
        num_bits[leaves[i].symbol] = lengths[i];
    }
    return AWS_OP_SUCCESS;
}

struct aws_huffman_symbol_coder *aws_huffman_amd_table_coder_from_lengths(const uint8_t num_bits[256]) {
    if (!num_bits) {
        aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
        return NULL;
    }
    uint64_t kraft = 0; /* in units of 2^-32 */
    for (int s = 0; s < 256; ++s) {
        if (num_bits[s] > 32) {
            aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
            return NULL;
        }
        kraft += num_bits[s] ? 1ull << (32 - num_bits[s]) : 0;
    }
    if (kraft > (1ull << 32)) {
        aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
        return NULL;
    }
    uint32_t patterns[256] = {0};
    uint64_t code = 0;
    uint32_t previous = 0;
    for (uint32_t len = 1; len <= 32; ++len) {
        for (int s = 0; s < 256; ++s) {
            if (num_bits[s] == len) {
                code <<= previous ? len - previous : 0;
                previous = len;
                patterns[s] = (uint32_t)code;
                ++code;
            }
        }
    }
    return aws_huffman_amd_table_coder_new(patterns, num_bits);
}

int aws_huffman_amd_table_coder_to_def(
    struct aws_huffman_symbol_coder *coder,
    char *text,
    size_t capacity,
    size_t *length) {

    if (!coder || !coder->encode || !length || (!text && capacity)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    /* the guard of the reference's own tables (its generator and aws_huffman_amd_table_coder_from_def skip it) */
    static const char header[] = "#ifndef HUFFMAN_CODE\n"
                                 "#error \"Macro HUFFMAN_CODE must be defined before including this header file!\"\n"
                                 "#endif\n\n";
    size_t at = sizeof(header) - 1;
    if (at <= capacity) {
        memcpy(text, header, at);
    }
    for (int s = 0; s < 256; ++s) {
        const struct aws_huffman_code c = coder->encode((uint8_t)s, coder->userdata);
        if (c.num_bits == 0) {
            continue;
        }
        if (c.num_bits > 32) {
            return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
        }
        const uint32_t pattern = c.num_bits < 32 ? c.pattern & ((1u << c.num_bits) - 1u) : c.pattern;
        char bits[33];
        for (uint32_t b = 0; b < c.num_bits; ++b) {
            bits[b] = (pattern >> (c.num_bits - 1 - b)) & 1u ? '1' : '0';
        }
        bits[c.num_bits] = '\0';
        char row[96];
        const int n = snprintf(row, sizeof(row), "HUFFMAN_CODE(%3d, \"%s\", 0x%x, %u)\n", s, bits, pattern, c.num_bits);
        if (at + (size_t)n <= capacity) {
            memcpy(text + at, row, (size_t)n);
        }
        at += (size_t)n;
    }
    *length = at;
    return at <= capacity ? AWS_OP_SUCCESS : aws_raise_error(AWS_ERROR_SHORT_BUFFER);
}
