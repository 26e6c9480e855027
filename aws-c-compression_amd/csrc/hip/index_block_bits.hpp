/*
 * The hot pass of the block index (aws_huffman_amd_block_index, huffman_amd_index.h; the rest is in index_kernels.hip): one
 * read of a stream's symbols, index[k] = the code bits of block k alone -- bit 63 of a tile's first entry: the tile holds a
 * symbol without a code, counted as 0 bits -- which the scan then sums in place.
 *
 * It is the second body of count_kernel (count_kernels.hip), chosen by a launch argument, not a kernel of its own: the two
 * read the same bytes the same way (persistent workgroups of 512 threads, four 16-byte loads a lane in flight), differ in
 * what they do with a byte in LDS, and the library's kernel census is held at 90.
 *
 * The 256 code lengths are kept once per LDS bank, as enc_count keeps them ("Encode"): lane l reads entry b at
 * word 32 b + l % 32 and shares a bank with no lane of its half wave; entry = length | (length == 0) << 20.  A workgroup takes
 * a TILE of whole blocks at a time -- as many as fit into the 32 KiB its threads read in one step, one block where a block is
 * longer (it then takes several steps) -- so that every block's sum is made by one workgroup and nobody has to add to
 * memory.  Block edges are multiples of 64 symbols from the base, so the 16 symbols at base + 16 g lie in one block
 * whatever the base's alignment: a lane reads them with one load at that address (the memory system takes any alignment,
 * as load_be32_run's loads), and the only bytes read one by one are the stream's last length % 16.
 * A wave's 64 lanes hold 64 consecutive groups of 16 symbols.  Their sums are scanned across the wave (DPP, no LDS traffic);
 * the last lane of every block -- and the last lane of the wave, for a block that goes on -- takes the scan's value at the
 * lane in front of its block's first (one ds_bpermute) and adds the difference to its block's word in LDS: one add a
 * wave for blocks of 1 024 symbols and more, sixteen a wave (to sixteen words) for blocks of 64.  The words are kept twice
 * and cleared by the thread that has just written one out, so a tile costs one workgroup barrier.
 */
#ifndef HUFFMAN_AMD_INDEX_BLOCK_BITS_HPP
#define HUFFMAN_AMD_INDEX_BLOCK_BITS_HPP
#include "kernels_common.hpp"

namespace {

constexpr u32 kIndexThreads = 512;                             /* count_kernel's */
constexpr u32 kIndexUnroll = 4;                                /* 16-byte loads a lane has in flight */
constexpr u32 kIndexStepGroups = kIndexThreads * kIndexUnroll; /* groups of 16 symbols a workgroup reads a step */
constexpr u32 kIndexStepBytes = kIndexStepGroups * 16u;        /* 32 KiB */
constexpr u32 kIndexMaxTileBlocks = kIndexStepBytes / 64u;     /* blocks of 64 symbols: 512 a tile */
/* the table, two sets of block sums, two flag words (16 bytes) */
constexpr u32 kIndexLdsBytes = 256u * 32u * 4u + 2u * kIndexMaxTileBlocks * 4u + 16u;
constexpr u64 kIndexHole = 1ull << 63; /* on a tile's first entry, between this pass and the scan */

/*
 * What a launch of the pass is given (index == nullptr: the launch counts symbols).
 * tile_blocks: whole blocks a tile (1 where no two fit into a step); n_tiles tiles cover the stream's n_blocks.
 * groups_per_block = block_symbols / 16.  inverse = ceil(2^32 / groups_per_block) for tiles of several blocks: the high
 * word of g * inverse is g / groups_per_block for every group of such a tile (g < 2^12, groups_per_block <= 2^10: the
 * error, below g / 2^32, stays below 1 / groups_per_block); 0 for tiles of one block, whose groups are all block 0's.
 */
struct index_job {
    const u64 *enc_table;
    const u8 *in;
    u64 length, block_symbols;
    u32 groups_per_block, inverse, tile_blocks, pad;
    u64 n_tiles, n_blocks;
    u64 *index;
};

/* length | hole << 20 of the 16 symbols of a group, through the lane's own copy of the table */
__device__ __forceinline__ u32 group_bits(const u8 *mine, const u32 (&w)[4]) {
    u32 sum = 0;
#pragma unroll
    for (u32 j = 0; j < 16; ++j) {
        sum += *reinterpret_cast<const u32 *>(mine + ((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) * 128u);
    }
    return sum;
}

__device__ __forceinline__ void index_block_bits(const index_job &job) {
    const u64 *enc_table = job.enc_table;
    const u8 *in = job.in;
    const u64 length = job.length, block_symbols = job.block_symbols, n_tiles = job.n_tiles, n_blocks = job.n_blocks;
    const u32 groups_per_block = job.groups_per_block, inverse = job.inverse, tile_blocks = job.tile_blocks;
    u64 *index = job.index;
    u32 *tab = reinterpret_cast<u32 *>(dyn_lds);   /* [256][32] */
    u32 *sums = tab + 256 * 32;                    /* [2][kIndexMaxTileBlocks] */
    u32 *holes = sums + 2 * kIndexMaxTileBlocks;   /* [2] */
    const u32 tid = threadIdx.x;
    const u32 lane = tid & (kWave - 1);
    if (tid < 256) {
        const u32 len = (u32)(enc_table[tid] >> 32);
        const u32 e = len | (len == 0 ? 1u << 20 : 0u);
#pragma unroll
        for (u32 k = 0; k < 32; ++k) {
            tab[tid * 32 + ((k + tid) & 31u)] = e; /* rotated so that the 32 stores of a group hit 32 banks */
        }
    }
    for (u32 k = tid; k < 2 * kIndexMaxTileBlocks + 2; k += kIndexThreads) {
        sums[k] = 0; /* (the flag words lie behind the sums) */
    }
    __syncthreads();
    const u8 *mine = reinterpret_cast<const u8 *>(tab) + (lane & 31u) * 4u;
    u32 set = 0;
    for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x, set ^= 1u) { /* (the same trips in every thread) */
        u32 *acc = sums + set * kIndexMaxTileBlocks;
        const u64 first_block = t * tile_blocks;
        const u64 blocks_left = n_blocks - first_block;
        const u32 blocks = blocks_left < tile_blocks ? (u32)blocks_left : tile_blocks;
        const u64 lo = first_block * block_symbols;
        const u64 whole = (u64)blocks * block_symbols;
        const u64 bytes = length - lo < whole ? length - lo : whole; /* (at most 2^24: one block, or one step) */
        const u32 n_groups = (u32)((bytes + 15) / 16);
        const u8 *src = in + lo;
        for (u32 g0 = 0; g0 < n_groups; g0 += kIndexStepGroups) {
            u32 w[kIndexUnroll][4], valid[kIndexUnroll];
#pragma unroll
            for (u32 u = 0; u < kIndexUnroll; ++u) {
                const u32 g = g0 + u * kIndexThreads + tid;
                const u64 at = (u64)g * 16;
                valid[u] = at < bytes ? (bytes - at < 16 ? (u32)(bytes - at) : 16u) : 0u;
                w[u][0] = w[u][1] = w[u][2] = w[u][3] = 0;
                if (valid[u] == 16) {
                    const unaligned_uint4 v = *reinterpret_cast<const unaligned_uint4 *>(src + at);
                    w[u][0] = v.x;
                    w[u][1] = v.y;
                    w[u][2] = v.z;
                    w[u][3] = v.w;
                }
            }
#pragma unroll
            for (u32 u = 0; u < kIndexUnroll; ++u) {
                const u32 g = g0 + u * kIndexThreads + tid;
                u32 sum = 0;
                if (valid[u] == 16) {
                    sum = group_bits(mine, w[u]);
                } else {
                    for (u32 j = 0; j < valid[u]; ++j) { /* the stream's last length % 16 symbols, one by one */
                        sum += *reinterpret_cast<const u32 *>(mine + (u32)src[(u64)g * 16 + j] * 128u);
                    }
                }
                const u32 incl = wave_inclusive_sum_dpp(sum, lane);
                const u32 block = (u32)(((u64)g * inverse) >> 32);
                const u32 in_block = g - block * groups_per_block; /* groups of the block in front of this one */
                const u32 first_lane = in_block < lane ? lane - in_block : 0u;
                const u32 before = __shfl(incl, (first_lane - 1u) & (kWave - 1));
                if (valid[u] && (in_block + 1 == groups_per_block || lane == kWave - 1 || g + 1 == n_groups)) {
                    const u32 part = incl - (first_lane ? before : 0u);
                    atomicAdd(&acc[block], part & 0xFFFFFu);
                    if (part >> 20) {
                        atomicOr(&holes[set], 1u);
                    }
                }
            }
        }
        __syncthreads();
        for (u32 k = tid; k < blocks; k += kIndexThreads) {
            index[first_block + k] = (u64)acc[k] | (k == 0 && holes[set] ? kIndexHole : 0ull);
            acc[k] = 0; /* (for the tile after the next: behind the next tile's barrier) */
        }
        if (tid == 0) {
            holes[set] = 0; /* (read above by this thread alone) */
        }
    }
}


} /* namespace */

#endif /* HUFFMAN_AMD_INDEX_BLOCK_BITS_HPP */
