/*
 * Symbol counts of a byte range on the device (aws_huffman_amd_symbol_counts, huffman_amd_build.h): the step in front of
 * a coder fitted to the data (csrc/host/coder_build.c makes the code lengths and the coder from the 256 counts).
 *
 * count_kernel, a persistent grid: every workgroup keeps one histogram in LDS and reads its share of the 16-byte aligned
 * body in grid-stride order, four 16-byte loads a lane in flight; workgroup 0 also counts the head (the bytes in front
 * of the first aligned address) and the tail (behind the last whole 16 bytes).  At the end -- and after every
 * `flush_bytes` it has read, so that no 32-bit LDS counter can overflow -- a workgroup adds its 256 sums to the
 * caller's u64 counts with agent-scope atomic adds (one per bin that is not zero) and clears its histogram.
 *
 * The histogram is 32 copies of the 256 bins, interleaved: bin b of copy c is word 32 b + c, and lane l adds to copy
 * l mod 32.  A ds_add_u32 of a wave is served in two groups of 32 lanes, and a group's 32 addresses then lie in 32
 * different banks ((a / 4) mod 32) whatever the bytes are: uniform bytes and one repeated byte cost the same LDS cycles
 * (with one copy a wave, 32 lanes on one bin take turns; profiles/tools/micro/probe_counts.hip measures both layouts).
 *
 * The same kernel has a second body, chosen by a launch argument: the hot pass of the block index (index_block_bits.hpp,
 * hufk_block_bits below), which reads the same bytes the same way and looks code lengths up where this one counts -- and a
 * third, the same pass over the items of a batch (index_batch_bits, hufk_batch_block_bits).  The fourth counts again: the
 * symbols of the items of an encode plan, into the same histogram (count_plan_items, hufk_plan_symbol_counts).  The fifth
 * splits elements of 2, 4 or 8 bytes into byte planes and counts every plane in that read (planes.hpp, hufk_planes_split).
 */
#include "kernels_common.hpp"
#include "index_block_bits.hpp"
#include "launch_common.hpp"
#include "planes.hpp"

namespace {

constexpr u32 kCountThreads = 512;
constexpr u32 kCountCopies = 32;
constexpr u32 kCountUnroll = 4;                               /* 16-byte loads a lane has in flight */
constexpr u32 kCountLdsBytes = 256u * kCountCopies * 4u;      /* 32 KiB: four workgroups (32 waves) a CU */
constexpr u64 kCountStepBytes = (u64)kCountThreads * 16u * kCountUnroll; /* what a workgroup reads a step: 32 KiB */

__device__ __forceinline__ void count_word(u32 *copy, u32 w) {
    atomicAdd(&copy[((w >> 0) & 0xFFu) * kCountCopies], 1u);
    atomicAdd(&copy[((w >> 8) & 0xFFu) * kCountCopies], 1u);
    atomicAdd(&copy[((w >> 16) & 0xFFu) * kCountCopies], 1u);
    atomicAdd(&copy[(w >> 24) * kCountCopies], 1u);
}

/* thread t < 256: bin t's sum over the copies to the caller's count, and the bin cleared (rotated by t: the 256 lanes
 * of a read touch 32 banks, not one) */
__device__ __forceinline__ void count_flush(u32 *tab, u64 *counts) {
    const u32 t = threadIdx.x;
    if (t < 256) {
        u32 *row = tab + t * kCountCopies;
        u64 sum = 0;
#pragma unroll 8
        for (u32 c = 0; c < kCountCopies; ++c) {
            const u32 k = (c + t) & (kCountCopies - 1);
            sum += row[k];
            row[k] = 0;
        }
        if (sum) {
            __hip_atomic_fetch_add(&counts[t], sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

/* the histogram cleared, behind a barrier */
__device__ __forceinline__ void count_clear(u32 *tab) {
    const u32 t = threadIdx.x;
    if (t < 256) {
        uint4 *row = reinterpret_cast<uint4 *>(tab + t * kCountCopies);
#pragma unroll
        for (u32 i = 0; i < kCountCopies / 4; ++i) {
            row[i] = uint4{0u, 0u, 0u, 0u};
        }
    }
    __syncthreads();
}

constexpr u32 kCountWaves = kCountThreads / kWave;
constexpr u32 kCountWaveStepBytes = kWave * 16u * kCountUnroll;            /* what a wave reads of its span a step: 4 KiB */
constexpr u32 kCountSpanSteps = HUFD_ENC_SEG_BYTES / kCountWaveStepBytes;  /* ... so the longest span takes four */
constexpr u32 kCountLaneStepBytes = 16u * kCountUnroll;                    /* what a lane reads of its item a step: 64 bytes */
static_assert(HUFD_ENC_SOLO_MANY_BYTES <= HUFD_ENC_SEG_BYTES, "a wave's item is no longer than a segment");

/*
 * The fourth body: the symbols of the current items of an encode plan (aws_huffman_amd_encode_plan_symbol_counts), into the
 * same histogram, flushed the same way.  The plan's own lists cover every item exactly once, so they are the work: a
 * UNIT is one segment, one item a wave encodes (both: a span of at most 16 KiB, read by one wave, lane l the 16 bytes at
 * 16 l of every KiB) or 64 items a thread encodes (a lane an item).  The grid's waves take the units in turns; a turn is
 * round_steps steps, the same number in every wave of the launch -- what the plan's longest unit takes, known to the
 * host -- so that the flush's barriers are met by all.  In a step a lane issues four 16-byte loads at any alignment, a
 * workgroup reads at most kCountStepBytes as in the first body, and steps_per_flush means the same.  Only whole groups of
 * 16 bytes inside a span are loaded; its last len % 16 bytes go one by one, and nothing behind it is read.
 */
__device__ __forceinline__ void count_plan_items(const index_job &job, u64 *counts, u64 steps_per_flush) {
    u32 *tab = reinterpret_cast<u32 *>(dyn_lds);
    count_clear(tab);
    const u32 t = threadIdx.x;
    const u32 lane = t & (kWave - 1);
    u32 *copy = tab + (t & (kCountCopies - 1));
    /* (units, and the steps between two flushes, are numbered in 32 bits: the host sees to it -- fewer scalar registers) */
    const u32 n_spans = job.n_segs + job.n_solo;
    const u32 n_units = n_spans + (job.n_tiny + kWave - 1) / kWave;
    const u32 round_steps = job.round_steps, per_flush = (u32)steps_per_flush;
    const u32 rounds = (n_units + gridDim.x * kCountWaves - 1) / (gridDim.x * kCountWaves);
    u32 steps = 0;
    /* (the two loops' trips are the same in every thread of a workgroup: the barriers below are uniform) */
    for (u32 r = 0; r < rounds; ++r) {
        const u32 unit = (r * gridDim.x + blockIdx.x) * kCountWaves + wave_uniform(t / kWave);
        const u8 *src = job.in;
        u32 len = 0, at = 0;                                                     /* the span, and where this lane starts in it */
        u32 load_stride = kWave * 16u, step_stride = kCountWaveStepBytes;        /* a wave's span */
        if (unit < job.n_segs) {
            const hufd_enc_seg *seg = job.segs + unit;
            src += wave_uniform64(seg->in_off);
            len = wave_uniform(seg->len);
            at = lane * 16u;
        } else if (unit < n_spans) {
            const hufd_enc_item *item = job.items + wave_uniform(job.solo[unit - job.n_segs]);
            src += wave_uniform64(item->in_off);
            len = wave_uniform((u32)item->in_len);
            at = lane * 16u;
        } else if (unit < n_units) {
            const u32 k = (unit - n_spans) * kWave + lane;
            load_stride = 16u;
            step_stride = kCountLaneStepBytes;
            if (k < job.n_tiny) {
                const hufd_enc_item *item = job.items + job.tiny[k];
                src += item->in_off;
                len = (u32)item->in_len;
            }
        }
        /* the span's last len % 16 symbols, one by one, by the lane whose group they are (of a wave's span: the one that
         * starts there in its KiB; of a lane's item: its own) -- in front of the turn's steps, fifteen symbols at the most:
         * a counter sees them on top of what steps_per_flush lets it see, and has the room */
        const u32 whole = len & ~15u;
        if (whole != len && (whole & (load_stride - 1u)) == at) {
            for (u32 a = whole; a < len; ++a) {
                atomicAdd(&copy[(u32)src[a] * kCountCopies], 1u);
            }
        }
        for (u32 s = 0; s < round_steps; ++s, at += step_stride) {
            if (steps == per_flush) {
                __syncthreads();
                count_flush(tab, counts);
                __syncthreads();
                steps = 0;
            }
            ++steps;
            uint4 v[kCountUnroll];
            bool ok[kCountUnroll];
#pragma unroll
            for (u32 u = 0; u < kCountUnroll; ++u) {
                const u32 a = at + u * load_stride;
                ok[u] = a < whole;
                v[u] = uint4{0u, 0u, 0u, 0u};
                if (ok[u]) {
                    const unaligned_uint4 w = *reinterpret_cast<const unaligned_uint4 *>(src + a);
                    v[u] = uint4{w.x, w.y, w.z, w.w};
                }
            }
#pragma unroll
            for (u32 u = 0; u < kCountUnroll; ++u) {
                if (ok[u]) {
                    count_word(copy, v[u].x);
                    count_word(copy, v[u].y);
                    count_word(copy, v[u].z);
                    count_word(copy, v[u].w);
                }
            }
        }
    }
    __syncthreads();
    count_flush(tab, counts);
}

/* body: n_vec 16-byte vectors at a 16-byte aligned address; head / tail: the bytes around it (workgroup 0's);
 * steps_per_flush: steps of kCountStepBytes a workgroup reads between two flushes (>= 1) */
__global__ __launch_bounds__(kCountThreads) void count_kernel(
    const u8 *head, u32 head_len, const uint4 *body, u64 n_vec, const u8 *tail, u32 tail_len, u64 *counts,
    u64 steps_per_flush, index_job index) {
    if (index.plane_bytes) { /* (the same in every thread of the launch) */
        planes_split(index.in, index.planes, index.length, index.block_symbols, index.plane_bytes, counts, (u32)steps_per_flush);
        return;
    }
    if (index.index) {
        if (index.items) {
            index_batch_bits(index);
        } else {
            index_block_bits(index);
        }
        return;
    }
    if (index.items) {
        count_plan_items(index, counts, steps_per_flush);
        return;
    }
    u32 *tab = reinterpret_cast<u32 *>(dyn_lds);
    const u32 t = threadIdx.x;
    count_clear(tab);
    u32 *copy = tab + (t & (kCountCopies - 1));
    if (blockIdx.x == 0) {
        if (t < head_len) {
            atomicAdd(&copy[(u32)head[t] * kCountCopies], 1u);
        }
        if (t < tail_len) {
            atomicAdd(&copy[(u32)tail[t] * kCountCopies], 1u);
        }
    }
    const u64 stride = (u64)gridDim.x * kCountThreads * kCountUnroll;
    u64 base = (u64)blockIdx.x * kCountThreads * kCountUnroll; /* the same in every lane: the barriers below are uniform */
    u64 steps = 0;
    while (base < n_vec) {
        if (steps == steps_per_flush) {
            __syncthreads();
            count_flush(tab, counts);
            __syncthreads();
            steps = 0;
        }
        uint4 v[kCountUnroll];
        bool ok[kCountUnroll];
#pragma unroll
        for (u32 u = 0; u < kCountUnroll; ++u) {
            const u64 i = base + u * kCountThreads + t;
            ok[u] = i < n_vec;
            v[u] = ok[u] ? body[i] : uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (u32 u = 0; u < kCountUnroll; ++u) {
            if (ok[u]) {
                count_word(copy, v[u].x);
                count_word(copy, v[u].y);
                count_word(copy, v[u].z);
                count_word(copy, v[u].w);
            }
        }
        base += stride;
        ++steps;
    }
    __syncthreads();
    count_flush(tab, counts);
}

} /* namespace */

extern "C" {

int hufk_symbol_counts(const void *input, uint64_t length, uint64_t *counts, uint64_t flush_bytes, void *stream) {
    if (length == 0) {
        return 0;
    }
    const u8 *in = (const u8 *)input;
    const u64 misalign = (u64)((uintptr_t)in & 15u);
    const u64 head_len = misalign ? (16u - misalign < length ? 16u - misalign : length) : 0u;
    const u64 n_vec = (length - head_len) / 16u;
    const u64 tail_len = length - head_len - n_vec * 16u;
    const u64 steps = (n_vec + (u64)kCountThreads * kCountUnroll - 1) / ((u64)kCountThreads * kCountUnroll);
    const uint32_t grid = hufk_host::persistent_grid(
        count_kernel, kCountThreads, kCountLdsBytes, (uint32_t)(steps < 0xFFFFFFFFull ? (steps ? steps : 1) : 0xFFFFFFFFull));
    /* a counter of a copy sees at most the bytes its workgroup reads between two flushes: below 2^32 */
    u64 per_flush = flush_bytes / kCountStepBytes;
    per_flush = per_flush ? per_flush : 1;
    hipLaunchKernelGGL(
        count_kernel, dim3(grid), dim3(kCountThreads), kCountLdsBytes, (hipStream_t)stream, in, (u32)head_len,
        reinterpret_cast<const uint4 *>(in + head_len), n_vec, in + head_len + n_vec * 16u, (u32)tail_len, counts, per_flush,
        index_job{});
    return (int)hipGetLastError();
}

int hufk_planes_split(
    const void *input, uint64_t element_count, uint32_t element_bytes, uint32_t run_elements, void *planes, uint64_t plane_stride,
    uint64_t *counts, uint64_t flush_bytes, uint32_t grid_cap, void *stream) {
    static_assert(kPlanesSplitThreads == kCountThreads && kPlanesSplitStepBytes == kCountStepBytes, "hosted by count_kernel");
    if (element_count == 0) {
        return 0;
    }
    index_job job{};
    job.in = (const u8 *)input;
    job.planes = (u8 *)planes;
    job.length = element_count;
    job.block_symbols = plane_stride;
    job.plane_bytes = element_bytes | run_elements << kPlanesRunShift; /* (a run: at most 2048) */
    /* (a step is 32 KiB of elements whatever their size; fewer elements than a group's still need workgroup 0) */
    const u64 step_elements = kPlanesSplitStepBytes / element_bytes;
    const u64 steps = (element_count + step_elements - 1) / step_elements;
    /* the grid is what is resident with the LDS this launch really uses: none without the counts */
    const u32 lds_bytes = counts ? planes_hist_bytes(element_bytes) : 0u;
    uint32_t grid = hufk_host::persistent_grid(
        count_kernel, kCountThreads, lds_bytes, (uint32_t)(steps < 0xFFFFFFFFull ? steps : 0xFFFFFFFFull));
    grid = grid_cap && grid_cap < grid ? grid_cap : grid;
    u64 per_flush = flush_bytes / kCountStepBytes;
    per_flush = per_flush ? (per_flush < 0xFFFFFFFFull ? per_flush : 0xFFFFFFFFull) : 1;
    hipLaunchKernelGGL(
        count_kernel, dim3(grid), dim3(kCountThreads), lds_bytes, (hipStream_t)stream, (const u8 *)nullptr, 0u, (const uint4 *)nullptr,
        (u64)0, (const u8 *)nullptr, 0u, counts, per_flush, job);
    return (int)hipGetLastError();
}

int hufk_plan_symbol_counts(
    const struct hufd_enc_item *items, const struct hufd_enc_seg *segs, uint32_t n_segs, const uint32_t *solo, uint32_t n_solo,
    const uint32_t *tiny, uint32_t n_tiny, uint64_t thread_limit, const void *input, uint64_t *counts, uint64_t flush_bytes,
    void *stream) {
    const u64 n_units = (u64)n_segs + n_solo + ((u64)n_tiny + kWave - 1) / kWave;
    if (n_units == 0) {
        return 0;
    }
    if ((n_units + 0xFFFFu) >> 32) { /* (64 TiB of segments: the kernel numbers the units of every turn in 32 bits) */
        return (int)hipErrorInvalidValue;
    }
    index_job job{};
    job.in = (const u8 *)input;
    job.items = items;
    job.segs = segs;
    job.solo = solo;
    job.tiny = tiny;
    job.n_segs = n_segs;
    job.n_solo = n_solo;
    job.n_tiny = n_tiny;
    /* a turn: the steps of a whole segment where a wave has a span, of the longest item a thread may have where a lane has one */
    const u64 lane_steps = n_tiny ? (thread_limit + kCountLaneStepBytes - 1) / kCountLaneStepBytes : 0;
    const u64 span_steps = n_segs || n_solo ? kCountSpanSteps : 0;
    job.round_steps = (u32)(lane_steps > span_steps ? lane_steps : span_steps);
    const u64 want = (n_units + kCountWaves - 1) / kCountWaves;
    const uint32_t grid = hufk_host::persistent_grid(
        count_kernel, kCountThreads, kCountLdsBytes, (uint32_t)(want < 0xFFFFFFFFull ? want : 0xFFFFFFFFull));
    u64 per_flush = flush_bytes / kCountStepBytes; /* (a workgroup reads at most kCountStepBytes a step here too) */
    per_flush = per_flush ? (per_flush < 0xFFFFFFFFull ? per_flush : 0xFFFFFFFFull) : 1;
    hipLaunchKernelGGL(
        count_kernel, dim3(grid), dim3(kCountThreads), kCountLdsBytes, (hipStream_t)stream, (const u8 *)nullptr, 0u,
        (const uint4 *)nullptr, (u64)0, (const u8 *)nullptr, 0u, counts, per_flush, job);
    return (int)hipGetLastError();
}

int hufk_block_bits(
    const uint64_t *enc_table, const void *input, uint64_t length, uint64_t block_symbols, uint64_t *index, void *stream) {
    static_assert(kIndexThreads == kCountThreads, "one kernel, one workgroup size");
    const u64 n_blocks = (length + block_symbols - 1) / block_symbols;
    if (n_blocks == 0) {
        return 0;
    }
    index_job job{};
    job.enc_table = enc_table;
    job.in = (const u8 *)input;
    job.length = length;
    job.block_symbols = block_symbols;
    job.groups_per_block = (u32)(block_symbols / 16);
    job.tile_blocks = (u32)(block_symbols < kIndexStepBytes ? kIndexStepBytes / block_symbols : 1u);
    job.inverse = job.tile_blocks > 1 ? (u32)(((1ull << 32) + job.groups_per_block - 1) / job.groups_per_block) : 0u;
    job.n_tiles = (n_blocks + job.tile_blocks - 1) / job.tile_blocks;
    job.n_blocks = n_blocks;
    job.index = index;
    const uint32_t grid = hufk_host::persistent_grid(
        count_kernel, kCountThreads, kIndexLdsBytes, (uint32_t)(job.n_tiles < 0xFFFFFFFFull ? job.n_tiles : 0xFFFFFFFFull));
    hipLaunchKernelGGL(
        count_kernel, dim3(grid), dim3(kCountThreads), kIndexLdsBytes, (hipStream_t)stream, (const u8 *)nullptr, 0u,
        (const uint4 *)nullptr, (u64)0, (const u8 *)nullptr, 0u, (u64 *)nullptr, (u64)1, job);
    return (int)hipGetLastError();
}

uint32_t hufk_batch_tile_blocks(uint64_t block_symbols) {
    return (uint32_t)(block_symbols < kIndexStepBytes ? kIndexStepBytes / block_symbols : 1u);
}

int hufk_batch_block_bits(const struct hufk_batch_index *batch, uint64_t most_blocks, void *stream) {
    index_job job{};
    job.enc_table = batch->enc_table;
    job.in = (const u8 *)batch->input;
    job.block_symbols = batch->block_symbols;
    job.groups_per_block = (u32)(batch->block_symbols / 16);
    job.tile_blocks = hufk_batch_tile_blocks(batch->block_symbols);
    job.inverse = job.tile_blocks > 1 ? (u32)(((1ull << 32) + job.groups_per_block - 1) / job.groups_per_block) : 0u;
    job.wave_inverse = job.groups_per_block <= 1024u ? (u32)(((1ull << 32) + job.groups_per_block - 1) / job.groups_per_block) : 0u;
    job.index = batch->index;
    job.items = batch->items;
    job.directory = batch->directory;
    job.tile_first = batch->tile_first;
    job.wave_bytes = batch->wave_bytes;
    job.capacity = batch->capacity;
    job.n_items = batch->n_items;
    /* the tiles are counted on the device: at most one a tile's blocks of what the index has room for, and a ragged one an
     * item; the waves want a workgroup for every eight items */
    const u64 tiles = most_blocks / job.tile_blocks + batch->n_items;
    const u64 by_waves = ((u64)batch->n_items + kCountThreads / kWave - 1) / (kCountThreads / kWave);
    const u64 want = tiles > by_waves ? tiles : by_waves;
    const uint32_t grid = hufk_host::persistent_grid(
        count_kernel, kCountThreads, kIndexLdsBytes, (uint32_t)(want < 0xFFFFFFFFull ? want : 0xFFFFFFFFull));
    hipLaunchKernelGGL(
        count_kernel, dim3(grid), dim3(kCountThreads), kIndexLdsBytes, (hipStream_t)stream, (const u8 *)nullptr, 0u,
        (const uint4 *)nullptr, (u64)0, (const u8 *)nullptr, 0u, (u64 *)nullptr, (u64)1, job);
    return (int)hipGetLastError();
}

} /* extern "C" */
