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
 *
 * index_batch_bits is the pass over the items of a batch: the same tiles, each of ONE item, and a wave an item for the short
 * ones (index_wave_item).
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
 *
 * index == nullptr and items != nullptr: the launch counts the symbols of a plan's items (count_plan_items,
 * count_kernels.hip).  What only that body needs shares the words of what only the index needs, as in hufd_locate: the
 * kernel holds every word of this argument in a scalar register, and more of them would cost the other bodies.  Its four
 * small numbers lie on length and block_symbols, which the kernel loads at its entry for every body: on the four words
 * behind them, which only the index loads, the build had 81 scalar registers -- one band of residency lost -- and has 78 so.
 *
 * plane_bytes != 0: the launch splits elements into byte planes (planes_split, planes.hpp) -- `in` the elements, `planes`
 * where the planes go, length the elements, block_symbols the plane stride; the counts and the steps between two flushes
 * are the kernel's own arguments.  The word was padding: no body got a word to hold.
 */
struct index_job {
    union {
        const u64 *enc_table;
        const u32 *tiny; /* (count) the plan's items a thread encodes: n_tiny numbers of items[] */
        u8 *planes;      /* (planes) where the planes go */
    };
    const u8 *in;
    union {
        u64 length;
        struct {
            u32 n_segs, n_solo; /* (count) */
        };
    };
    union {
        u64 block_symbols;
        struct {
            u32 n_tiny, round_steps; /* (count) steps of a turn: what the plan's longest unit takes, see count_plan_items */
        };
    };
    u32 groups_per_block, inverse, tile_blocks;
    u32 plane_bytes; /* not 0: the launch splits elements of that many bytes (its low 8 bits) into planes, and above them the
                      * run of a split of differences, 0 for the plain split (planes.hpp) */
    u64 n_tiles, n_blocks;
    u64 *index;
    /* the index of a batch (index_batch_bits below; items == nullptr: one stream): `in` is the input base of the plan's
     * items, and length, n_tiles and n_blocks are not the host's to know -- the directory and tile_first say them */
    const hufd_enc_item *items;
    union {
        const u64 *directory;     /* [n_items + 1][2]: the blocks in front of an item, its symbols */
        const hufd_enc_seg *segs; /* (count) the plan's segments: n_segs */
    };
    union {
        const u64 *tile_first; /* [n_items + 1]: the tiles in front of an item */
        const u32 *solo;       /* (count) the plan's items a wave encodes: n_solo numbers of items[] */
    };
    u64 wave_bytes, capacity;
    u32 n_items, wave_inverse; /* ceil(2^32 / groups_per_block) where that is at most 2^10, else 0 */
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

/* the table and the clear sums, behind a barrier */
__device__ __forceinline__ void index_fill_lds(const u64 *enc_table, u32 *tab, u32 *sums) {
    const u32 tid = threadIdx.x;
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
}

/* the `bytes` symbols of one tile at src, n_groups groups of 16: every block's bits added to acc[block of the tile] */
__device__ __forceinline__ void index_tile_groups(
    const u8 *src, u64 bytes, u32 n_groups, u32 groups_per_block, u32 inverse, const u8 *mine, u32 *acc, u32 *hole) {
    const u32 tid = threadIdx.x;
    const u32 lane = tid & (kWave - 1);
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
                    atomicOr(hole, 1u);
                }
            }
        }
    }
}

/* behind a tile's barrier: its blocks' sums to index[0 .. blocks), and the set cleared for the tile after the next */
__device__ __forceinline__ void index_tile_out(u64 *index, u32 blocks, u32 *acc, u32 *hole) {
    const u32 tid = threadIdx.x;
    for (u32 k = tid; k < blocks; k += kIndexThreads) {
        index[k] = (u64)acc[k] | (k == 0 && *hole ? kIndexHole : 0ull);
        acc[k] = 0; /* (for the tile after the next: behind the next tile's barrier) */
    }
    if (tid == 0) {
        *hole = 0; /* (read above by this thread alone) */
    }
}

__device__ __forceinline__ void index_block_bits(const index_job &job) {
    const u8 *in = job.in;
    const u64 length = job.length, block_symbols = job.block_symbols, n_tiles = job.n_tiles, n_blocks = job.n_blocks;
    const u32 groups_per_block = job.groups_per_block, inverse = job.inverse, tile_blocks = job.tile_blocks;
    u64 *index = job.index;
    u32 *tab = reinterpret_cast<u32 *>(dyn_lds);   /* [256][32] */
    u32 *sums = tab + 256 * 32;                    /* [2][kIndexMaxTileBlocks] */
    u32 *holes = sums + 2 * kIndexMaxTileBlocks;   /* [2] */
    index_fill_lds(job.enc_table, tab, sums);
    const u8 *mine = reinterpret_cast<const u8 *>(tab) + (threadIdx.x & 31u) * 4u;
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
        index_tile_groups(in + lo, bytes, n_groups, groups_per_block, inverse, mine, acc, holes + set);
        __syncthreads();
        index_tile_out(index + first_block, blocks, acc, holes + set);
    }
}

/* a word that is the same in every lane of the wave, as scalars */
__device__ __forceinline__ u64 wave_uniform64(u64 x) {
    return ((u64)wave_uniform((u32)(x >> 32)) << 32) | wave_uniform((u32)x);
}

/*
 * One short item, a wave's: lanes take its groups of 16 symbols in turns of 64, the same scan, and the last lane of every
 * block writes the block's entry itself -- out[block of the item] -- with bit 63 where the block holds a symbol without a
 * code (the scan takes it from any entry).  A block that goes on over several turns is carried in `carry_bits` and
 * `carry_hole`, the same in every lane.  No LDS but the table, no barrier.  len < HUFK_BATCH_WAVE_MAX_BYTES: a group's
 * number is below 2^12, what `inverse` divides exactly (0: blocks of more than 2^10 groups, divided as they are).
 * Only the item's own bytes are read: whole groups with one load, the last len % 16 symbols one by one.
 */
__device__ __forceinline__ void index_wave_item(
    const u8 *src, u32 len, u32 groups_per_block, u32 inverse, const u8 *mine, u64 *out, u32 lane) {
    const u32 n_groups = (len + 15) / 16;
    u32 carry_bits = 0, carry_hole = 0;
    for (u32 g0 = 0; g0 < n_groups; g0 += kWave) { /* (the same trips in every lane) */
        const u32 g = g0 + lane;
        const u32 at = g * 16;
        const u32 valid = at < len ? (len - at < 16 ? len - at : 16u) : 0u;
        u32 sum = 0;
        if (valid == 16) {
            const unaligned_uint4 v = *reinterpret_cast<const unaligned_uint4 *>(src + at);
            const u32 w[4] = {v.x, v.y, v.z, v.w};
            sum = group_bits(mine, w);
        } else {
            for (u32 j = 0; j < valid; ++j) {
                sum += *reinterpret_cast<const u32 *>(mine + (u32)src[at + j] * 128u);
            }
        }
        const u32 incl = wave_inclusive_sum_dpp(sum, lane);
        const u32 block = inverse ? (u32)(((u64)g * inverse) >> 32) : g / groups_per_block;
        const u32 in_block = g - block * groups_per_block;
        const u32 first_lane = in_block < lane ? lane - in_block : 0u;
        const u32 before = __shfl(incl, (first_lane - 1u) & (kWave - 1));
        const u32 part = incl - (first_lane ? before : 0u);
        const u32 bits = (part & 0xFFFFFu) + (first_lane ? 0u : carry_bits);
        const u32 hole = (part >> 20) | (first_lane ? 0u : carry_hole);
        const bool ends = valid && (in_block + 1 == groups_per_block || g + 1 == n_groups);
        if (ends) {
            out[block] = (u64)bits | (hole ? kIndexHole : 0ull);
        }
        carry_bits = __shfl(ends ? 0u : bits, kWave - 1);
        carry_hole = __shfl(ends ? 0u : hole, kWave - 1);
    }
}

/*
 * The hot pass over the items of a batch (aws_huffman_amd_encode_plan_block_index): the third body of count_kernel.  Which
 * road an item takes is decided by its length alone, so every block is written by one road:
 *   shorter than wave_bytes   a wave an item (index_wave_item), the grid's waves in turns over the items
 *   any other                 the tiles of index_block_bits, each a tile of whole blocks of ONE item: the base is the item's
 *                             own, so 16 symbols at base + 16 g lie in one block at any alignment of the item.  The
 *                             workgroups take the batch's tiles in turns; tile_first[] (the tiles in front of each item,
 *                             scanned with the directory) says whose a tile is.  The search is the same in every thread --
 *                             loads of one address, which the memory system serves as one -- and starts at the
 *                             workgroup's last item: no LDS word and no barrier to hand the answer round.
 * The counts are the device's: the directory's last record says how many blocks there are, and where they do not fit into
 * the caller's index nothing is written.
 */
__device__ __forceinline__ void index_batch_bits(const index_job &job) {
    const u64 n_items = job.n_items;
    const u64 total = job.directory[2 * n_items];
    if (total == 0 || total >= job.capacity || total >> 32) { /* (the same in every thread of the launch) */
        return;
    }
    const u8 *in = job.in;
    const u64 block_symbols = job.block_symbols;
    const u32 groups_per_block = job.groups_per_block, tile_blocks = job.tile_blocks;
    u64 *index = job.index;
    u32 *tab = reinterpret_cast<u32 *>(dyn_lds);   /* [256][32] */
    u32 *sums = tab + 256 * 32;                    /* [2][kIndexMaxTileBlocks] */
    u32 *holes = sums + 2 * kIndexMaxTileBlocks;   /* [2] */
    index_fill_lds(job.enc_table, tab, sums);
    const u32 tid = threadIdx.x;
    const u32 lane = tid & (kWave - 1);
    const u8 *mine = reinterpret_cast<const u8 *>(tab) + (lane & 31u) * 4u;

    constexpr u32 kWaves = kIndexThreads / kWave;
    const u64 wave_stride = (u64)gridDim.x * kWaves;
    for (u64 i = (u64)blockIdx.x * kWaves + wave_uniform(tid / kWave); i < n_items; i += wave_stride) {
        const u64 len = wave_uniform64(job.directory[2 * i + 1]);
        if (len == 0 || len >= job.wave_bytes) {
            continue;
        }
        const u64 first = wave_uniform64(job.directory[2 * i]);
        const u64 in_off = wave_uniform64(job.items[i].in_off);
        index_wave_item(in + in_off, (u32)len, groups_per_block, job.wave_inverse, mine, index + first, lane);
    }

    /* (fewer than 2^32 blocks, so tiles and items are numbered in 32 bits) */
    const u32 n_tiles = (u32)job.tile_first[n_items];
    u32 item = 0, item_tiles_end = 0; /* the item of the last tile, and the first tile behind it */
    u32 set = 0;
    for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x, set ^= 1u) { /* (the same trips in every thread) */
        if ((u32)t >= item_tiles_end) { /* the largest i with tile_first[i] <= t: tile_first[lo] <= t < tile_first[hi] throughout */
            u32 lo = item, hi = job.n_items;
            while (hi - lo > 1) {
                const u32 mid = lo + (hi - lo) / 2;
                if ((u32)job.tile_first[mid] <= (u32)t) {
                    lo = mid;
                } else {
                    hi = mid;
                }
            }
            item = lo;
            item_tiles_end = (u32)job.tile_first[(u64)item + 1];
        }
        /* (the item's few words again for every tile: loads that do not wait for each other, and fewer registers held) */
        const u64 *record = job.directory + 2 * (u64)item;
        const u64 first = record[0], length = record[1];
        const u32 n_blocks = (u32)(record[2] - first);
        const u32 first_block = ((u32)t - (u32)job.tile_first[item]) * tile_blocks;
        u64 *item_index = index + first;
        const u8 *src = in + job.items[item].in_off;
        u32 *acc = sums + set * kIndexMaxTileBlocks;
        const u32 blocks_left = n_blocks - first_block;
        const u32 blocks = blocks_left < tile_blocks ? blocks_left : tile_blocks;
        const u64 lo = (u64)first_block * block_symbols;
        const u64 whole = (u64)blocks * block_symbols;
        const u64 bytes = length - lo < whole ? length - lo : whole; /* (at most 2^24: one block, or one step) */
        const u32 n_groups = (u32)((bytes + 15) / 16);
        index_tile_groups(src + lo, bytes, n_groups, groups_per_block, job.inverse, mine, acc, holes + set);
        __syncthreads();
        index_tile_out(item_index + first_block, blocks, acc, holes + set);
    }
}


} /* namespace */

#endif /* HUFFMAN_AMD_INDEX_BLOCK_BITS_HPP */
