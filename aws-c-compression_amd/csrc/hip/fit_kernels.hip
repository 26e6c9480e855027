/*
 * A coder fitted on the device (huffman_amd_fit.h): 256 symbol counts -> length-limited code lengths -> the canonical code
 * -> an engine's encode table and decode table, in ONE launch of one workgroup, with no host round trip.  The lengths are
 * the ones aws_huffman_amd_code_lengths_from_counts(counts, min_bits, max_bits, EVERY_SYMBOL) makes and the code the one
 * of aws_huffman_amd_table_coder_from_lengths (csrc/host/coder_build.c): what the host would have built, entry for entry.
 *
 * fit_kernel, 256 threads, a symbol a thread, every list in LDS:
 *   1. sort: the (count, symbol) pairs by coder_build.c's leaf_order (count ascending, among equal counts the higher
 *      symbol first), by rank: a thread counts the pairs in front of its own (256 broadcast reads).
 *   2. the D = max_bits - min_bits package-merge lists, the deepest first.  A list is the 256 leaves merged with the pairs
 *      ("packages") of the list below.  Both are sorted, so the merge is by rank: a leaf goes to its index plus the number
 *      of packages STRICTLY lighter, a package to its index plus the number of leaves NOT heavier -- the host loop's
 *      `leaves[li].count <= pw` (a leaf wins a tie), on which the multiset of lengths depends.  Two binary searches a
 *      thread and list.  Weights are u64 (the counts sum to less than 2^58: a package stays below 2^63).  Of a list the
 *      next one needs the weights (`list`, rewritten in place) and the selection needs where its leaves went (`pos`).
 *   3. the selection, backwards: take = 2 (256 - 2^min_bits) items of list 0; of the first `take` items of list k,
 *      leaves_k are leaves (a binary search in pos[k]: the positions rise with the rank) and the rest packages, each two
 *      items of list k + 1.  The leaf of rank i gets min_bits + #{k : i < leaves_k}.
 *   4. the lengths to the symbols.  The host sorts the multiset of lengths and hands it out in length_order (count
 *      descending, the lower symbol first).  That order is leaf_order backwards, and the lengths of step 3 do not rise
 *      with the rank, so the hand-out is the identity here: the symbol of rank i keeps the length of rank i.
 *   5. the canonical code: symbols per length (LDS atomics), the first code of every length, a symbol's rank among the
 *      lower symbols of its length.
 *   6. the tables: encode table entry s = length << 32 | code; decode table entry w = symbol << 8 | length of the code
 *      that is a prefix of the max_bits-bit window w, 0 where there is none.  The codes in canonical order tile the
 *      windows from 0 up, so a window finds its length among at most nine limits and its symbol by index: eight windows
 *      a thread and turn, one 16-byte store.
 * from_lengths: the receiver's half enters at step 5 with 256 lengths from device memory, validated first.
 * A status other than 0 (one word, uniform in the workgroup) leaves both tables as they were.
 */
#include "kernels_common.hpp"
#include "launch_common.hpp"

namespace {

constexpr u32 kFitThreads = 256;
constexpr u32 kFitMaxDepth = 8; /* max_bits - min_bits of 4 .. 12 */

/* the carves of dyn_lds, 16-byte aligned */
constexpr u32 kFitLeafW = 0;                              /* u64[256]  the counts in leaf_order */
constexpr u32 kFitList = kFitLeafW + 256 * 8;             /* u64[512]  the list below (first: the counts by symbol) */
constexpr u32 kFitPw = kFitList + 512 * 8;                /* u64[256]  the weights of its pairs */
constexpr u32 kFitPos = kFitPw + 256 * 8;                 /* u16[8][256]  where the leaf of rank i went in list k */
constexpr u32 kFitLeafSym = kFitPos + kFitMaxDepth * 512; /* u32[256]  the symbol of rank i */
constexpr u32 kFitLens = kFitLeafSym + 256 * 4;           /* u32[256]  the length of symbol s */
constexpr u32 kFitCanon = kFitLens + 256 * 4;             /* u32[256]  the symbol of canonical index c */
constexpr u32 kFitPerLen = kFitCanon + 256 * 4;           /* u32[4][16]  per length: symbols, first code, first index, window limit */
constexpr u32 kFitSlots = kFitPerLen + 4 * 16 * 4;        /* u64[8]  the reductions' words */
constexpr u32 kFitLdsBytes = kFitSlots + 8 * 8;

/* two sums over the workgroup at once */
__device__ __forceinline__ void fit_block_sums(u64 &a, u64 &b, u64 *slots) {
#pragma unroll
    for (u32 d = kWave / 2; d > 0; d >>= 1) {
        a += __shfl_xor(a, d);
        b += __shfl_xor(b, d);
    }
    const u32 wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        slots[wave] = a;
        slots[4 + wave] = b;
    }
    __syncthreads();
    a = slots[0] + slots[1] + slots[2] + slots[3];
    b = slots[4] + slots[5] + slots[6] + slots[7];
    __syncthreads();
}

/* how many of the n rising values at v are below x (or_equal: not above x) */
__device__ __forceinline__ u32 fit_count_below(const u64 *v, u32 n, u64 x, bool or_equal) {
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = (lo + hi) / 2;
        const u64 m = v[mid];
        if (or_equal ? m <= x : m < x) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo;
}

__global__ __launch_bounds__(kFitThreads) void fit_kernel(
    u32 from_lengths, const u64 *counts, const u8 *lengths_in, u32 min_bits, u32 max_bits, u64 *enc_table, u16 *dec_lut,
    u8 *num_bits_out, u32 *status_out) {
    u64 *leaf_w = reinterpret_cast<u64 *>(dyn_lds + kFitLeafW);
    u64 *list = reinterpret_cast<u64 *>(dyn_lds + kFitList);
    u64 *pw = reinterpret_cast<u64 *>(dyn_lds + kFitPw);
    u16 *pos = reinterpret_cast<u16 *>(dyn_lds + kFitPos);
    u32 *leaf_sym = reinterpret_cast<u32 *>(dyn_lds + kFitLeafSym);
    u32 *lens = reinterpret_cast<u32 *>(dyn_lds + kFitLens);
    u32 *canon = reinterpret_cast<u32 *>(dyn_lds + kFitCanon);
    u32 *per_len = reinterpret_cast<u32 *>(dyn_lds + kFitPerLen);
    u64 *slots = reinterpret_cast<u64 *>(dyn_lds + kFitSlots);
    u32 *n_of = per_len, *first_of = per_len + 16, *index_of = per_len + 32, *limit_of = per_len + 48;
    const u32 t = threadIdx.x;
    u32 status = 0;
    u32 len; /* of symbol t */

    if (t < 64) {
        per_len[t] = 0;
    }
    if (!from_lengths) {
        const u64 c = counts[t];
        list[t] = c;
        /* the host's limit: counts that sum to 2^58 or more (no 64-bit sum of 256 counts can say so: two sums of parts) */
        u64 high = c >> 10, low = c & 1023u;
        fit_block_sums(high, low, slots); /* (its barriers are also the ones behind the stores above) */
        if (high + (low >> 10) >= (1ull << 48)) {
            status = HUFK_FIT_COUNTS_TOO_LARGE;
        }
        if (status) {
            if (t == 0 && status_out) {
                *status_out = status;
            }
            return;
        }
        /* 1. the rank of (c, t) in leaf_order */
        u32 rank = 0;
#pragma unroll 8
        for (u32 j = 0; j < 256; ++j) {
            const u64 o = list[j];
            rank += (o < c || (o == c && j > t)) ? 1u : 0u;
        }
        leaf_w[rank] = c;
        leaf_sym[rank] = t;
        __syncthreads();
        /* 2. the lists; from here on thread t is the leaf of rank t */
        const u64 w = leaf_w[t];
        const u32 depth = max_bits - min_bits;
        u32 extra = 0;
        if (min_bits < 8) { /* (8: 256 codes of 8 bits, nothing to lengthen) */
            u32 m = 256;
            list[t] = w;
            pos[(depth - 1) * 256 + t] = (u16)t;
            __syncthreads();
            for (u32 k = depth - 1; k-- > 0;) {
                const u32 packages = m / 2;
                u64 mine = 0;
                if (t < packages) {
                    mine = list[2 * t] + list[2 * t + 1];
                    pw[t] = mine;
                }
                __syncthreads();
                const u32 leaf_at = t + fit_count_below(pw, packages, w, false);
                list[leaf_at] = w;
                pos[k * 256 + t] = (u16)leaf_at;
                if (t < packages) {
                    list[t + fit_count_below(leaf_w, 256, mine, true)] = mine;
                }
                m = 256 + packages;
                __syncthreads();
            }
            /* 3. the selection (every thread walks the same few words) */
            u32 take = 2u * (256u - (1u << min_bits));
            for (u32 k = 0; k < depth; ++k) {
                u32 lo = 0, hi = 256;
                while (lo < hi) {
                    const u32 mid = (lo + hi) / 2;
                    if (pos[k * 256 + mid] < take) {
                        lo = mid + 1;
                    } else {
                        hi = mid;
                    }
                }
                extra += t < lo ? 1u : 0u;
                take = 2u * (take - lo);
            }
        }
        /* 4. to the symbols */
        lens[leaf_sym[t]] = min_bits + extra;
        __syncthreads();
        len = lens[t];
        if (num_bits_out) {
            num_bits_out[t] = (u8)len;
        }
    } else {
        len = lengths_in[t];
        const bool none = len == 0, outside = len != 0 && (len < min_bits || len > max_bits);
        u64 flags = (none ? 1u : 0u) | (outside ? 1u << 16 : 0u);
        u64 kraft = none || outside ? 0u : 1u << (max_bits - len);
        fit_block_sums(flags, kraft, slots);
        if (flags & 0xFFFFu) {
            status = HUFK_FIT_LENGTH_ZERO;
        } else if (flags) {
            status = HUFK_FIT_LENGTH_OUT_OF_BOUNDS;
        } else if (kraft > (1ull << max_bits)) {
            status = HUFK_FIT_KRAFT_ABOVE_ONE;
        }
        if (status) {
            if (t == 0 && status_out) {
                *status_out = status;
            }
            return;
        }
        lens[t] = len;
        __syncthreads();
    }
    if (t == 0 && status_out) {
        *status_out = 0;
    }

    /* 5. the canonical code */
    atomicAdd(&n_of[len], 1u);
    u32 rank = 0;
#pragma unroll 8
    for (u32 j = 0; j < 256; ++j) {
        rank += (lens[j] == len && j < t) ? 1u : 0u;
    }
    __syncthreads();
    u32 code = 0, index = 0;
    for (u32 l = min_bits; l < len; ++l) {
        code = (code + n_of[l]) << 1;
        index += n_of[l];
    }
    if (rank == 0) { /* the first symbol of its length says where the length starts and ends */
        first_of[len] = code;
        index_of[len] = index;
        limit_of[len] = (code + n_of[len]) << (max_bits - len);
    }
    canon[index + rank] = t;
    enc_table[t] = ((u64)len << 32) | (code + rank);
    /* (a length nobody has ends where the one before it ended) */
    if (t >= min_bits && t <= max_bits && n_of[t] == 0) {
        u32 c = 0;
        for (u32 l = min_bits; l < t; ++l) {
            c = (c + n_of[l]) << 1;
        }
        limit_of[t] = c << (max_bits - t);
    }
    __syncthreads();

    /* 6. the decode table, eight windows a thread and turn */
    for (u32 base = t * 8; base < (1u << max_bits); base += kFitThreads * 8) {
        u32 e[8];
        u32 l = min_bits;
#pragma unroll
        for (u32 i = 0; i < 8; ++i) {
            const u32 win = base + i;
            while (l <= max_bits && win >= limit_of[l]) { /* (the limits rise with the length, the windows with i) */
                ++l;
            }
            e[i] = l <= max_bits ? (canon[index_of[l] + ((win >> (max_bits - l)) - first_of[l])] << 8) | l : 0u;
        }
        uint4 v;
        v.x = e[0] | (e[1] << 16);
        v.y = e[2] | (e[3] << 16);
        v.z = e[4] | (e[5] << 16);
        v.w = e[6] | (e[7] << 16);
        *reinterpret_cast<uint4 *>(dec_lut + base) = v;
    }
}

} /* namespace */

extern "C" {

int hufk_fit_tables(
    uint32_t from_lengths, const uint64_t *counts, const uint8_t *lengths, uint32_t min_bits, uint32_t max_bits, uint64_t *enc_table,
    uint16_t *dec_lut, uint8_t *num_bits_out, uint32_t *status, void *stream) {
    hipLaunchKernelGGL(
        fit_kernel, dim3(1), dim3(kFitThreads), kFitLdsBytes, (hipStream_t)stream, from_lengths, counts, lengths, min_bits, max_bits,
        enc_table, dec_lut, num_bits_out, status);
    return (int)hipGetLastError();
}

} /* extern "C" */
