/*
 * Byte planes of arrays of 1-, 2-, 4- and 8-byte elements (huffman_amd_planes.h): the split, with the 256 counts of every
 * plane taken in the same read, and the merge.  With E the element's bytes, n the elements and S the plane stride,
 *   split   planes[p * S + j] = input[j * E + p]        merge   output[j * E + p] = planes[p * S + j]        p < E, j < n.
 *
 * Both are BODIES of kernels that exist, chosen by a launch argument, as every pass since the fit has been: the library links
 * 90 kernels and is held to that many (tests/test_library_boundary.py).
 *   planes_split   the fifth body of count_kernel (count_kernels.hip): 512 threads, persistent workgroups, the same kind of
 *                  histogram in dynamic LDS, flushed the same way.  Its arguments travel in index_job's words.
 *   planes_merge   a body of unpack_records_kernel (pack_kernels.hip), beside the copy of stored items: 256 threads, no LDS.
 *
 * A lane takes a GROUP of 16 consecutive elements (8 where E is 8, so that loads and results stay inside 64 registers): E (at
 * most four) 16-byte loads at any address, a transposition in registers with byte permutes, and one store of 16 (8) bytes to
 * each plane at any address.  The 512 (256) lanes' groups are consecutive, so a wave's store to a plane is one KiB in a row.
 * A step is what a workgroup's lanes take at 64 bytes each -- 32 KiB of elements in the split, 16 KiB in the merge -- and the
 * workgroups take the steps in grid-stride order.  The last n % 16 (8) elements go byte by byte through workgroup 0, a thread
 * a byte.  Nothing outside the E ranges of n bytes is written, and nothing outside the n * E bytes is read.
 *
 * The counts: E histograms of 32 interleaved copies, as the first body keeps one, would be 256 KiB at E = 8.  The budget is
 * 64 KiB a workgroup (two workgroups a CU): 32 copies for E <= 2, 16 for E = 4, 8 for E = 8 -- bin b of copy c of plane p is
 * word (p * 256 + b) * copies + c, and lane l adds to copy l % copies.  With fewer than 32 copies the lanes of a half wave
 * that share a copy meet on one word where a plane is dominated by one value (a sign-and-exponent plane is): two lanes a
 * word at 16 copies, four at 8 (profiles/planes_mi355x.json has what that costs).
 *
 * DELTA IN RUNS (huffman_amd_planes_delta.h): the same two bodies with the difference to the previous element in front of
 * the split and its sum behind the merge, restarted every R elements -- R a power of two from 16 to 2048, so a run starts on
 * a group boundary and never crosses a step (the merge's is 2048 elements at E = 8).  They are template arms: the plain
 * calls run the code they ran.
 *   split   the subtraction on the group's words in element order, before the transposition; the predecessor of a group's
 *           first element is one more load of E bytes, taken only where the group does not start a run.  The counts are
 *           of the difference planes: they are taken from the words that are stored.
 *   merge   behind planes_to_elements a lane sums its 16 (8) elements in registers; the lanes' totals are scanned over the
 *           R / 16 (R / 8) consecutive lanes of a run with wave shuffles, and where a run is two or four waves (R = 2048,
 *           and R = 1024 at E = 8) the waves' totals go through 128 bytes of LDS between two barriers a step.  Nothing
 *           passes between workgroups.  The tail's base is made by workgroup 0 from the PLANES (the differences of its run
 *           in front of the tail, fewer than R): the output in front of the tail is another workgroup's to write.
 */
#ifndef HUFFMAN_AMD_PLANES_HPP
#define HUFFMAN_AMD_PLANES_HPP
#include "kernels_common.hpp"

namespace {

constexpr u32 kPlanesLaneBytes = 64;       /* what a lane takes of the elements a step */
constexpr u32 kPlanesSplitThreads = 512;   /* count_kernel's */
constexpr u32 kPlanesMergeThreads = 256;   /* unpack_records_kernel's */
constexpr u32 kPlanesSplitStepBytes = kPlanesSplitThreads * kPlanesLaneBytes; /* 32 KiB */
constexpr u32 kPlanesMergeStepBytes = kPlanesMergeThreads * kPlanesLaneBytes; /* 16 KiB */

/* the geometry of an element size */
template <u32 E>
struct planes_shape {
    static_assert(E == 1 || E == 2 || E == 4 || E == 8, "element sizes");
    static constexpr u32 kGroupElems = E == 8 ? 8u : 16u;
    static constexpr u32 kGroupBytes = kGroupElems * E;                /* 16, 32, 64, 64 */
    static constexpr u32 kGroupWords = kGroupBytes / 4u;
    static constexpr u32 kLaneGroups = kPlanesLaneBytes / kGroupBytes; /* groups a lane takes a step: 4, 2, 1, 1 */
    static constexpr u32 kPlaneWords = kGroupElems / 4u;               /* words a group gives a plane: 4, 4, 4, 2 */
    static constexpr u32 kCopies = E <= 2 ? 32u : 64u / E;             /* of a plane's histogram: 32, 32, 16, 8 */
    static constexpr u32 kHistWords = E * 256u * kCopies;              /* 32 KiB for E = 1, 64 KiB for the others */
};

constexpr u32 planes_hist_bytes(u32 element_bytes) {
    return element_bytes == 1 ? planes_shape<1>::kHistWords * 4u : planes_shape<2>::kHistWords * 4u;
}
static_assert(planes_shape<4>::kHistWords == planes_shape<2>::kHistWords && planes_shape<8>::kHistWords == planes_shape<2>::kHistWords, "one budget");

/* what the merge is given (the split's arguments are index_job's words, index_block_bits.hpp) */
struct planes_job {
    const u8 *planes;
    u8 *out;
    u64 n, stride;
    u32 element_bytes;
    u32 run_elements; /* not 0: the merge sums differences in runs of that many elements (a power of two, 16 .. 2048) */
};
constexpr u32 kPlanesMergeSlotBytes = 4u * 4u * 8u; /* dynamic LDS of a merge of differences: a 64-bit total a wave and group of a lane */

/* a 4 x 4 byte matrix transposed: word i of the result holds byte i of a, b, c and d in turn (its own inverse) */
__device__ __forceinline__ void planes_transpose4(u32 a, u32 b, u32 c, u32 d, u32 &p0, u32 &p1, u32 &p2, u32 &p3) {
    const u32 x0 = byte_perm(b, a, 0x05010400u), x1 = byte_perm(b, a, 0x07030602u); /* a0 b0 a1 b1, a2 b2 a3 b3 */
    const u32 y0 = byte_perm(d, c, 0x05010400u), y1 = byte_perm(d, c, 0x07030602u);
    p0 = byte_perm(y0, x0, 0x05040100u);
    p1 = byte_perm(y0, x0, 0x07060302u);
    p2 = byte_perm(y1, x1, 0x05040100u);
    p3 = byte_perm(y1, x1, 0x07060302u);
}

/* a group's words w[] (its elements in order) to out[p * kPlaneWords + k]: word k of what the group gives plane p */
template <u32 E>
__device__ __forceinline__ void planes_to_planes(const u32 (&w)[planes_shape<E>::kGroupWords], u32 (&out)[planes_shape<E>::kGroupWords]) {
    if constexpr (E == 1) {
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            out[k] = w[k];
        }
    } else if constexpr (E == 2) {
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            out[k] = byte_perm(w[2 * k + 1], w[2 * k], 0x06040200u);
            out[4 + k] = byte_perm(w[2 * k + 1], w[2 * k], 0x07050301u);
        }
    } else if constexpr (E == 4) {
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            planes_transpose4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3], out[k], out[4 + k], out[8 + k], out[12 + k]);
        }
    } else { /* element e is words 2 e and 2 e + 1: half h of elements 4 q .. 4 q + 3 gives planes 4 h .. 4 h + 3 their word q */
#pragma unroll
        for (u32 h = 0; h < 2; ++h) {
#pragma unroll
            for (u32 q = 0; q < 2; ++q) {
                planes_transpose4(
                    w[8 * q + h], w[8 * q + 2 + h], w[8 * q + 4 + h], w[8 * q + 6 + h], out[(4 * h + 0) * 2 + q],
                    out[(4 * h + 1) * 2 + q], out[(4 * h + 2) * 2 + q], out[(4 * h + 3) * 2 + q]);
            }
        }
    }
}

/* ... and back: in[p * kPlaneWords + k] to the group's words */
template <u32 E>
__device__ __forceinline__ void planes_to_elements(const u32 (&in)[planes_shape<E>::kGroupWords], u32 (&w)[planes_shape<E>::kGroupWords]) {
    if constexpr (E == 1) {
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            w[k] = in[k];
        }
    } else if constexpr (E == 2) {
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            w[2 * k] = byte_perm(in[4 + k], in[k], 0x05010400u);
            w[2 * k + 1] = byte_perm(in[4 + k], in[k], 0x07030602u);
        }
    } else if constexpr (E == 4) {
#pragma unroll
        for (u32 k = 0; k < 4; ++k) {
            planes_transpose4(in[k], in[4 + k], in[8 + k], in[12 + k], w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
        }
    } else {
#pragma unroll
        for (u32 h = 0; h < 2; ++h) {
#pragma unroll
            for (u32 q = 0; q < 2; ++q) {
                planes_transpose4(
                    in[(4 * h + 0) * 2 + q], in[(4 * h + 1) * 2 + q], in[(4 * h + 2) * 2 + q], in[(4 * h + 3) * 2 + q], w[8 * q + h],
                    w[8 * q + 2 + h], w[8 * q + 4 + h], w[8 * q + 6 + h]);
            }
        }
    }
}

/* 16 * N bytes at any address into 4 * N words, and back */
template <u32 N>
__device__ __forceinline__ void planes_load16(const u8 *src, u32 *w) {
#pragma unroll
    for (u32 i = 0; i < N; ++i) {
        const unaligned_uint4 v = *reinterpret_cast<const unaligned_uint4 *>(src + 16u * i);
        w[4 * i + 0] = v.x;
        w[4 * i + 1] = v.y;
        w[4 * i + 2] = v.z;
        w[4 * i + 3] = v.w;
    }
}

template <u32 N>
__device__ __forceinline__ void planes_store16(u8 *dst, const u32 *w) {
#pragma unroll
    for (u32 i = 0; i < N; ++i) {
        *reinterpret_cast<unaligned_uint4 *>(dst + 16u * i) = unaligned_uint4{w[4 * i + 0], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
    }
}

/* what a group gives one plane (16 bytes, 8 where E is 8) from / to any address */
template <u32 E>
__device__ __forceinline__ void planes_store_plane(u8 *dst, const u32 *w) {
    if constexpr (planes_shape<E>::kPlaneWords == 4) {
        *reinterpret_cast<unaligned_uint4 *>(dst) = unaligned_uint4{w[0], w[1], w[2], w[3]};
    } else {
        *reinterpret_cast<unaligned_uint2 *>(dst) = unaligned_uint2{w[0], w[1]};
    }
}

template <u32 E>
__device__ __forceinline__ void planes_load_plane(const u8 *src, u32 *w) {
    if constexpr (planes_shape<E>::kPlaneWords == 4) {
        const unaligned_uint4 v = *reinterpret_cast<const unaligned_uint4 *>(src);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    } else {
        const unaligned_uint2 v = *reinterpret_cast<const unaligned_uint2 *>(src);
        w[0] = v.x;
        w[1] = v.y;
    }
}

/* ---- differences in runs: arithmetic on the words of a group in element order */
struct __attribute__((packed, aligned(1))) unaligned_u16 {
    u16 x;
};

/* what a sum over elements of E bytes is kept in (taken modulo 2^(8 E) where it is used) */
template <u32 E>
struct planes_sum {
    typedef typename std::conditional<E == 8, u64, u32>::type type;
};

/* a word of four 8-bit (E = 1) or two 16-bit (E = 2) fields: a - b and a + b field by field, no carry between fields */
template <u32 E>
__device__ __forceinline__ u32 planes_field_sub(u32 a, u32 b) {
    constexpr u32 kTop = E == 1 ? 0x80808080u : 0x80008000u;
    return ((a | kTop) - (b & ~kTop)) ^ ((a ^ ~b) & kTop);
}

template <u32 E>
__device__ __forceinline__ u32 planes_field_add(u32 a, u32 b) {
    constexpr u32 kTop = E == 1 ? 0x80808080u : 0x80008000u;
    return ((a & ~kTop) + (b & ~kTop)) ^ ((a ^ b) & kTop);
}

/* an element's low E bytes in every field of a word */
template <u32 E>
__device__ __forceinline__ u32 planes_field_all(u32 x) {
    return E == 1 ? (x & 0xFFu) * 0x01010101u : (x & 0xFFFFu) * 0x00010001u;
}

/* the element of E bytes at any address */
template <u32 E>
__device__ __forceinline__ typename planes_sum<E>::type planes_load_element(const u8 *src) {
    if constexpr (E == 1) {
        return *src;
    } else if constexpr (E == 2) {
        return reinterpret_cast<const unaligned_u16 *>(src)->x;
    } else if constexpr (E == 4) {
        return reinterpret_cast<const unaligned_u32 *>(src)->x;
    } else {
        const unaligned_uint2 v = *reinterpret_cast<const unaligned_uint2 *>(src);
        return ((u64)v.y << 32) | v.x;
    }
}

/* element j of planes, byte by byte */
template <u32 E>
__device__ __forceinline__ typename planes_sum<E>::type planes_plane_element(const u8 *planes, u64 stride, u64 j) {
    typename planes_sum<E>::type v = 0;
    const u8 *src = planes + j;
#pragma unroll
    for (u32 p = 0; p < E; ++p, src += stride) {
        v |= (typename planes_sum<E>::type)(*src) << (8u * p);
    }
    return v;
}

/* a group's elements to their differences, prev in front of the first (0 where the group starts a run) */
template <u32 E>
__device__ __forceinline__ void planes_delta_words(u32 (&w)[planes_shape<E>::kGroupWords], typename planes_sum<E>::type prev) {
    constexpr u32 kWords = planes_shape<E>::kGroupWords;
    if constexpr (E == 8) {
#pragma unroll
        for (u32 e = kWords / 2u; e-- > 0;) {
            const u64 x = ((u64)w[2 * e + 1] << 32) | w[2 * e];
            const u64 y = e ? ((u64)w[2 * e - 1] << 32) | w[2 * e - 2] : prev;
            const u64 d = x - y;
            w[2 * e] = (u32)d;
            w[2 * e + 1] = (u32)(d >> 32);
        }
    } else if constexpr (E == 4) {
#pragma unroll
        for (u32 k = kWords; k-- > 0;) {
            w[k] -= k ? w[k - 1] : prev;
        }
    } else { /* the word of the predecessors: the fields moved up by one, the field below them on top of the word in front */
        constexpr u32 kField = 8u * E;
#pragma unroll
        for (u32 k = kWords; k-- > 0;) {
            const u32 below = k ? w[k - 1] : prev << (32u - kField);
            w[k] = planes_field_sub<E>(w[k], (w[k] << kField) | (below >> (32u - kField)));
        }
    }
}

/* a group's differences to their inclusive sums within the group; returns the last */
template <u32 E>
__device__ __forceinline__ typename planes_sum<E>::type planes_sum_words(u32 (&w)[planes_shape<E>::kGroupWords]) {
    constexpr u32 kWords = planes_shape<E>::kGroupWords;
    if constexpr (E == 8) {
        u64 acc = 0;
#pragma unroll
        for (u32 e = 0; e < kWords / 2u; ++e) {
            acc += ((u64)w[2 * e + 1] << 32) | w[2 * e];
            w[2 * e] = (u32)acc;
            w[2 * e + 1] = (u32)(acc >> 32);
        }
        return acc;
    } else if constexpr (E == 4) {
#pragma unroll
        for (u32 k = 1; k < kWords; ++k) {
            w[k] += w[k - 1];
        }
        return w[kWords - 1];
    } else {
        constexpr u32 kField = 8u * E;
#pragma unroll
        for (u32 k = 0; k < kWords; ++k) {
            u32 x = planes_field_add<E>(w[k], w[k] << kField);
            if constexpr (E == 1) {
                x = planes_field_add<E>(x, x << 16);
            }
            w[k] = k ? planes_field_add<E>(x, planes_field_all<E>(w[k - 1] >> (32u - kField))) : x;
        }
        return w[kWords - 1] >> (32u - kField);
    }
}

/* base added to every element of a group */
template <u32 E>
__device__ __forceinline__ void planes_add_base(u32 (&w)[planes_shape<E>::kGroupWords], typename planes_sum<E>::type base) {
    constexpr u32 kWords = planes_shape<E>::kGroupWords;
    if constexpr (E == 8) {
#pragma unroll
        for (u32 e = 0; e < kWords / 2u; ++e) {
            const u64 x = (((u64)w[2 * e + 1] << 32) | w[2 * e]) + base;
            w[2 * e] = (u32)x;
            w[2 * e + 1] = (u32)(x >> 32);
        }
    } else if constexpr (E == 4) {
#pragma unroll
        for (u32 k = 0; k < kWords; ++k) {
            w[k] += base;
        }
    } else {
        const u32 all = planes_field_all<E>(base);
#pragma unroll
        for (u32 k = 0; k < kWords; ++k) {
            w[k] = planes_field_add<E>(w[k], all);
        }
    }
}

/* the inclusive sum of v over the lanes of a run that lie in this wave: run_lanes consecutive lanes (a power of two; 64 and
 * more: the whole wave).  Every lane of the wave takes part. */
template <typename T>
__device__ __forceinline__ T planes_run_scan(T v, u32 lane, u32 run_lanes) {
    const u32 r = lane & (run_lanes - 1u);
    for (u32 d = 1; d < kWave && d < run_lanes; d <<= 1) {
        T up;
        if constexpr (sizeof(T) == 8) {
            up = (T)__shfl_up((unsigned long long)v, d);
        } else {
            up = __shfl_up(v, d);
        }
        if (r >= d) {
            v += up;
        }
    }
    return v;
}

template <typename T>
__device__ __forceinline__ T planes_wave_sum(T v) {
#pragma unroll
    for (u32 d = kWave / 2; d > 0; d >>= 1) {
        if constexpr (sizeof(T) == 8) {
            v += (T)__shfl_xor((unsigned long long)v, d);
        } else {
            v += __shfl_xor(v, d);
        }
    }
    return v;
}

/* rows r = p * 256 + b of the histograms: a row's sum over its copies added to the caller's count r, and the row cleared
 * (rotated by r, as count_flush: the lanes of a read touch different banks) */
template <u32 E>
__device__ __forceinline__ void planes_flush(u32 *tab, u64 *counts) {
    constexpr u32 kCopies = planes_shape<E>::kCopies;
    for (u32 r = threadIdx.x; r < E * 256u; r += kPlanesSplitThreads) {
        u32 *row = tab + r * kCopies;
        u64 sum = 0;
#pragma unroll 8
        for (u32 c = 0; c < kCopies; ++c) {
            const u32 k = (c + r) & (kCopies - 1);
            sum += row[k];
            row[k] = 0;
        }
        if (sum) {
            __hip_atomic_fetch_add(&counts[r], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

/* the four bytes of a word of plane p counted by this lane (copy: the lane's copy of bin 0 of plane 0) */
template <u32 E>
__device__ __forceinline__ void planes_count_word(u32 *copy, u32 p, u32 w) {
    constexpr u32 kCopies = planes_shape<E>::kCopies;
    u32 *plane = copy + p * 256u * kCopies;
    atomicAdd(&plane[((w >> 0) & 0xFFu) * kCopies], 1u);
    atomicAdd(&plane[((w >> 8) & 0xFFu) * kCopies], 1u);
    atomicAdd(&plane[((w >> 16) & 0xFFu) * kCopies], 1u);
    atomicAdd(&plane[(w >> 24) * kCopies], 1u);
}

/*
 * The split of n elements of E bytes, COUNT: with the counts.  per_flush: the steps a workgroup takes between two flushes of
 * its 32-bit counters (>= 1): a counter sees at most the bytes its workgroup reads in between, and workgroup 0's tail, below
 * 128 bytes, on top.  (Steps and barriers are the same in every thread of a workgroup.)
 * DELTA: the planes are of the differences in runs of `run` elements (and so are the counts); without it `run` is not read.
 */
template <u32 E, bool COUNT, bool DELTA>
__device__ __forceinline__ void planes_split_run(const u8 *in, u8 *planes, u64 n, u64 stride, u64 *counts, u32 per_flush, u32 run) {
    typedef planes_shape<E> shape;
    typedef typename planes_sum<E>::type sum_t;
    constexpr u32 kStepGroups = kPlanesSplitThreads * shape::kLaneGroups;
    const u32 t = threadIdx.x;
    u32 *tab = reinterpret_cast<u32 *>(dyn_lds);
    u32 *copy = tab + (t & (shape::kCopies - 1));
    if constexpr (COUNT) {
        uint4 *rows = reinterpret_cast<uint4 *>(tab);
        for (u32 i = t; i < shape::kHistWords / 4u; i += kPlanesSplitThreads) {
            rows[i] = uint4{0u, 0u, 0u, 0u};
        }
        __syncthreads();
    }
    const u64 n_groups = n / shape::kGroupElems;
    if (blockIdx.x == 0) { /* the last n % kGroupElems elements, a thread a byte */
        const u64 first = n_groups * shape::kGroupElems;
        const u32 tail_bytes = (u32)(n - first) * E;
        if (t < tail_bytes) {
            const u64 j = first + t / E;
            const u32 p = t % E;
            u8 b = in[j * E + p];
            if constexpr (DELTA) { /* the element and, inside a run, the one in front of it: both lie in the input */
                sum_t d = 0;
                const u8 *src = in + j * E;
#pragma unroll
                for (u32 q = 0; q < E; ++q) {
                    d |= (sum_t)src[q] << (8u * q);
                }
                if (j & (run - 1u)) {
                    sum_t y = 0;
#pragma unroll
                    for (u32 q = 0; q < E; ++q) {
                        y |= (sum_t)(src - E)[q] << (8u * q);
                    }
                    d -= y;
                }
                b = (u8)(d >> (8u * p));
            }
            planes[p * stride + j] = b;
            if constexpr (COUNT) {
                atomicAdd(&copy[(p * 256u + b) * shape::kCopies], 1u);
            }
        }
    }
    const u64 n_steps = (n_groups + kStepGroups - 1) / kStepGroups;
    u32 steps = 0;
    for (u64 step = blockIdx.x; step < n_steps; step += gridDim.x) {
        if constexpr (COUNT) {
            if (steps == per_flush) {
                __syncthreads();
                planes_flush<E>(tab, counts);
                __syncthreads();
                steps = 0;
            }
            ++steps;
        }
        /* the step's bases are the same in every lane (scalars); a lane's own offsets are 32-bit */
        const u64 first_group = step * kStepGroups;
        const u64 groups_left = n_groups - first_group;
        const u32 step_groups = groups_left < kStepGroups ? (u32)groups_left : kStepGroups;
        const u8 *step_in = in + first_group * shape::kGroupBytes;
        u8 *step_planes = planes + first_group * shape::kGroupElems;
        u32 w[shape::kLaneGroups][shape::kGroupWords];
        sum_t prev[shape::kLaneGroups];
        (void)prev;
        bool ok[shape::kLaneGroups];
#pragma unroll
        for (u32 u = 0; u < shape::kLaneGroups; ++u) {
            const u32 g = u * kPlanesSplitThreads + t;
            ok[u] = g < step_groups;
            if constexpr (shape::kLaneGroups > 1) { /* (several groups in flight: every word has a value) */
#pragma unroll
                for (u32 k = 0; k < shape::kGroupWords; ++k) {
                    w[u][k] = 0;
                }
            }
            if (ok[u]) {
                planes_load16<shape::kGroupBytes / 16u>(step_in + g * shape::kGroupBytes, w[u]);
            }
            if constexpr (DELTA) { /* a step is whole runs: where the group starts one is in the lane's own number */
                prev[u] = 0;
                if (ok[u] && ((g * shape::kGroupElems) & (run - 1u))) {
                    prev[u] = planes_load_element<E>(step_in + g * shape::kGroupBytes - E);
                }
            }
        }
#pragma unroll
        for (u32 u = 0; u < shape::kLaneGroups; ++u) {
            if (ok[u]) {
                const u32 g = u * kPlanesSplitThreads + t;
                u32 out[shape::kGroupWords];
                if constexpr (DELTA) {
                    planes_delta_words<E>(w[u], prev[u]);
                }
                planes_to_planes<E>(w[u], out);
                u8 *dst = step_planes;
#pragma unroll
                for (u32 p = 0; p < E; ++p, dst += stride) {
                    planes_store_plane<E>(dst + g * shape::kGroupElems, out + p * shape::kPlaneWords);
                }
                if constexpr (COUNT) {
#pragma unroll
                    for (u32 p = 0; p < E; ++p) {
#pragma unroll
                        for (u32 k = 0; k < shape::kPlaneWords; ++k) {
                            planes_count_word<E>(copy, p, out[p * shape::kPlaneWords + k]);
                        }
                    }
                }
            }
        }
    }
    if constexpr (COUNT) {
        __syncthreads();
        planes_flush<E>(tab, counts);
    }
}

/* the word of index_job that chooses the split: the element's bytes, and above them the run of a split of differences */
constexpr u32 kPlanesRunShift = 8;

template <bool DELTA>
__device__ __forceinline__ void planes_split_sized(
    const u8 *in, u8 *planes, u64 n, u64 stride, u32 element_bytes, u64 *counts, u32 per_flush, u32 run) {
    if (counts) {
        if (element_bytes == 1) {
            planes_split_run<1, true, DELTA>(in, planes, n, stride, counts, per_flush, run);
        } else if (element_bytes == 2) {
            planes_split_run<2, true, DELTA>(in, planes, n, stride, counts, per_flush, run);
        } else if (element_bytes == 4) {
            planes_split_run<4, true, DELTA>(in, planes, n, stride, counts, per_flush, run);
        } else {
            planes_split_run<8, true, DELTA>(in, planes, n, stride, counts, per_flush, run);
        }
    } else if (element_bytes == 1) {
        planes_split_run<1, false, DELTA>(in, planes, n, stride, counts, per_flush, run);
    } else if (element_bytes == 2) {
        planes_split_run<2, false, DELTA>(in, planes, n, stride, counts, per_flush, run);
    } else if (element_bytes == 4) {
        planes_split_run<4, false, DELTA>(in, planes, n, stride, counts, per_flush, run);
    } else {
        planes_split_run<8, false, DELTA>(in, planes, n, stride, counts, per_flush, run);
    }
}

/* the body count_kernel hosts: plane_bytes (index_job's word) and `counts` are the same in every thread of the launch */
__device__ __forceinline__ void planes_split(
    const u8 *in, u8 *planes, u64 n, u64 stride, u32 plane_bytes, u64 *counts, u32 per_flush) {
    const u32 element_bytes = plane_bytes & ((1u << kPlanesRunShift) - 1u), run = plane_bytes >> kPlanesRunShift;
    if (run) {
        planes_split_sized<true>(in, planes, n, stride, element_bytes, counts, per_flush, run);
    } else {
        planes_split_sized<false>(in, planes, n, stride, element_bytes, counts, per_flush, 0u);
    }
}

/* the merge of n elements of E bytes: the split's groups and steps the other way round */
/* DELTA: the planes hold differences in runs of `run` elements and the output is their sums (kPlanesMergeSlotBytes of
 * dynamic LDS; the barriers are taken by every thread of a workgroup: the steps, `run` and the tail are the same in all) */
template <u32 E, bool DELTA>
__device__ __forceinline__ void planes_merge_run(const u8 *planes, u8 *out, u64 n, u64 stride, u32 run) {
    typedef planes_shape<E> shape;
    typedef typename planes_sum<E>::type sum_t;
    constexpr u32 kStepGroups = kPlanesMergeThreads * shape::kLaneGroups;
    constexpr u32 kWaves = kPlanesMergeThreads / kWave;
    static_assert(shape::kLaneGroups * kWaves * sizeof(u64) <= kPlanesMergeSlotBytes, "a slot a wave and group of a lane");
    const u32 t = threadIdx.x;
    const u32 lane = t & (kWave - 1u), wave = t / kWave;
    u64 *slots = reinterpret_cast<u64 *>(dyn_lds);
    const u64 n_groups = n / shape::kGroupElems;
    if (blockIdx.x == 0) {
        const u64 first = n_groups * shape::kGroupElems;
        const u32 tail_bytes = (u32)(n - first) * E;
        if constexpr (DELTA) {
            /* a run's start is a group's start: the tail lies in one run, and its base is the sum of that run's differences
             * in front of it, taken from the planes -- the sums in front of the tail are another workgroup's to write */
            if (tail_bytes) {
                sum_t base = 0;
                for (u64 i = (first & ~(u64)(run - 1u)) + t; i < first; i += kPlanesMergeThreads) {
                    base += planes_plane_element<E>(planes, stride, i);
                }
                base = planes_wave_sum(base);
                if (lane == 0) {
                    slots[wave] = base;
                }
                __syncthreads();
                base = 0;
#pragma unroll
                for (u32 x = 0; x < kWaves; ++x) {
                    base += (sum_t)slots[x];
                }
                __syncthreads();
                if (t < tail_bytes) {
                    const u64 j = first + t / E;
                    const u32 p = t % E;
                    for (u64 i = first; i <= j; ++i) {
                        base += planes_plane_element<E>(planes, stride, i);
                    }
                    out[j * E + p] = (u8)(base >> (8u * p));
                }
            }
        } else if (t < tail_bytes) {
            const u64 j = first + t / E;
            const u32 p = t % E;
            out[j * E + p] = planes[p * stride + j];
        }
    }
    const u32 run_lanes = DELTA ? run / shape::kGroupElems : 0u; /* the consecutive lanes of a run: 1 .. 256 */
    (void)slots, (void)lane, (void)wave, (void)run_lanes;
    const u64 n_steps = (n_groups + kStepGroups - 1) / kStepGroups;
    for (u64 step = blockIdx.x; step < n_steps; step += gridDim.x) {
        const u64 first_group = step * kStepGroups;
        const u64 groups_left = n_groups - first_group;
        const u32 step_groups = groups_left < kStepGroups ? (u32)groups_left : kStepGroups;
        const u8 *step_planes = planes + first_group * shape::kGroupElems;
        u8 *step_out = out + first_group * shape::kGroupBytes;
        u32 in[shape::kLaneGroups][shape::kGroupWords];
        bool ok[shape::kLaneGroups];
#pragma unroll
        for (u32 u = 0; u < shape::kLaneGroups; ++u) {
            const u32 g = u * kPlanesMergeThreads + t;
            ok[u] = g < step_groups;
            if constexpr (shape::kLaneGroups > 1 || DELTA) { /* (a lane without a group sums zeros) */
#pragma unroll
                for (u32 k = 0; k < shape::kGroupWords; ++k) {
                    in[u][k] = 0;
                }
            }
            if (ok[u]) {
                const u8 *src = step_planes;
#pragma unroll
                for (u32 p = 0; p < E; ++p, src += stride) {
                    planes_load_plane<E>(src + g * shape::kGroupElems, in[u] + p * shape::kPlaneWords);
                }
            }
        }
        if constexpr (DELTA) {
            /* a step is whole runs and so is what the lanes take at one u (4096 elements, 2048 at E = 8): a run's groups
             * are run_lanes consecutive lanes' at one u.  Every lane takes every shuffle and barrier; ok[] guards stores */
            u32 w[shape::kLaneGroups][shape::kGroupWords];
            sum_t upto[shape::kLaneGroups], own[shape::kLaneGroups];
#pragma unroll
            for (u32 u = 0; u < shape::kLaneGroups; ++u) {
                planes_to_elements<E>(in[u], w[u]);
                own[u] = planes_sum_words<E>(w[u]);
                upto[u] = planes_run_scan(own[u], lane, run_lanes);
            }
            if (run_lanes > kWave) { /* a run of two or four waves: each adds the totals of the run's waves in front of it */
#pragma unroll
                for (u32 u = 0; u < shape::kLaneGroups; ++u) {
                    if (lane == kWave - 1u) {
                        slots[u * kWaves + wave] = upto[u];
                    }
                }
                __syncthreads();
                const u32 run_first_wave = wave & ~(run_lanes / kWave - 1u);
#pragma unroll
                for (u32 u = 0; u < shape::kLaneGroups; ++u) {
#pragma unroll
                    for (u32 x = 0; x + 1u < kWaves; ++x) {
                        const sum_t before = (sum_t)slots[u * kWaves + x];
                        upto[u] += x >= run_first_wave && x < wave ? before : (sum_t)0;
                    }
                }
                __syncthreads();
            }
#pragma unroll
            for (u32 u = 0; u < shape::kLaneGroups; ++u) {
                if (ok[u]) {
                    const u32 g = u * kPlanesMergeThreads + t;
                    planes_add_base<E>(w[u], upto[u] - own[u]);
                    planes_store16<shape::kGroupBytes / 16u>(step_out + g * shape::kGroupBytes, w[u]);
                }
            }
        } else {
#pragma unroll
            for (u32 u = 0; u < shape::kLaneGroups; ++u) {
                if (ok[u]) {
                    const u32 g = u * kPlanesMergeThreads + t;
                    u32 w[shape::kGroupWords];
                    planes_to_elements<E>(in[u], w);
                    planes_store16<shape::kGroupBytes / 16u>(step_out + g * shape::kGroupBytes, w);
                }
            }
        }
    }
}

/* the body unpack_records_kernel hosts */
template <bool DELTA>
__device__ __forceinline__ void planes_merge_sized(const planes_job &job) {
    if (job.element_bytes == 1) { /* (the same in every thread of the launch) */
        planes_merge_run<1, DELTA>(job.planes, job.out, job.n, job.stride, job.run_elements);
    } else if (job.element_bytes == 2) {
        planes_merge_run<2, DELTA>(job.planes, job.out, job.n, job.stride, job.run_elements);
    } else if (job.element_bytes == 4) {
        planes_merge_run<4, DELTA>(job.planes, job.out, job.n, job.stride, job.run_elements);
    } else {
        planes_merge_run<8, DELTA>(job.planes, job.out, job.n, job.stride, job.run_elements);
    }
}

__device__ __forceinline__ void planes_merge(const planes_job &job) {
    if (job.run_elements) {
        planes_merge_sized<true>(job);
    } else {
        planes_merge_sized<false>(job);
    }
}

} /* namespace */

#endif /* HUFFMAN_AMD_PLANES_HPP */
