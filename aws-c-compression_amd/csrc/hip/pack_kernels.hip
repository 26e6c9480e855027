/*
 * Packed batch encode (aws_huffman_amd_encode_plan_launch_packed, huffman_amd_packed.h): what runs between the length
 * pass and the encode pass of such a launch.  From the length pass's result records,
 *
 *   len_i        = (total_bits_i + 7) / 8                       (aws_huffman_get_encoded_length, reference
 *                                                                source/huffman.c:121-128)
 *   reserved_i   = round_up(len_i, align)
 *   offsets[i]   = the sum of reserved_k for k < i,  offsets[n] = the total
 *
 * and, for the encode pass, a second array of the plan's item records with out_off = offsets[i] and out_cap = what of
 * reserved_i lies in front of the caller's output capacity.  The plan's own records are read, never written.
 *
 * Reduce, then scan -- two kernels, no workgroup waits for another, nothing to clear between launches (so a launch can be
 * captured in a graph and replayed):
 *   pack_tile_sums   a workgroup a tile of `tile_items` items: the tile's sum and its largest reserved length
 *   pack_offsets     a workgroup a tile again: the sums of the tiles in front of it (read from memory, a few thousand
 *                    words at most: the launch wrapper grows the tile with the batch), then the tile's items in rounds of
 *                    one a thread, a workgroup scan a round; the last workgroup also writes the total and the maximum
 * A batch of one tile goes without the first kernel.
 *
 * Packed batch decode (aws_huffman_amd_decode_plan_launch_packed) is the mirror: the same two kernels over the symbol counts
 * the decode scan left (hufd_dec_result.total_symbols), between the scan and the emit stage of such a launch,
 *
 *   sym_i        = what the reference's aws_huffman_decode writes for item i when it never runs out of room
 *   offsets[i+1] = round_up(offsets[i] + sym_i, align)
 *
 * with out_cap = sym_i for an item whose symbols all lie in front of the caller's capacity and 0 for any other, and
 *   unpack_records   a thread a chunk: the plan's per-chunk records with their item's new place, for the emit kernels; or
 *                    a thread an item: the second record array with no room at all, for the walk that only counts (the
 *                    kernels that walk and write an item in one go run twice in a packed launch)
 */
#include "kernels_common.hpp"
#include "launch_common.hpp"
#include "planes.hpp"

namespace {

constexpr u32 kPackThreads = 256;
constexpr u32 kPackWaves = kPackThreads / kWave;
constexpr u32 kPackTileItems = 1024; /* a workgroup's items: four rounds (65 536 items: 64 workgroups, a million: 1024) */
constexpr u32 kPackMaxTiles = 8192;  /* what a workgroup of pack_offsets reads of the sums in front of it at most: 128 KiB */
constexpr u32 kPackLdsBytes = 3 * kPackWaves * sizeof(u64);

/* The two kinds of batch the two kernels take (`decode`: a launch argument, the same in every thread -- not a second
 * build of each kernel): the length of an item in its first pass's record, and the item's record for the second pass */
struct pack_encode {
    typedef hufd_enc_item item;
    typedef hufd_enc_result measured;
    static __device__ __forceinline__ u64 length(const measured *lengths, u64 i) {
        return (lengths[i].total_bits + 7) / 8;
    }
    /* (field by field: the record copied as a whole went through scratch memory) */
    static __device__ __forceinline__ void place(const item *from, item *to, u64 off, u64 len, u64 reserved, u64 capacity) {
        (void)len;
        const u64 room = capacity > off ? capacity - off : 0;
        to->in_off = from->in_off;
        to->in_len = from->in_len;
        to->out_off = off;
        to->out_cap = reserved < room ? reserved : room;
        to->ovf_pattern = from->ovf_pattern;
        to->ovf_bits = from->ovf_bits;
        to->eos_padding = from->eos_padding;
        to->first_seg = from->first_seg;
        to->n_segs = from->n_segs;
        to->tiny = from->tiny;
    }
};
struct pack_decode {
    typedef hufd_dec_item item;
    typedef hufd_dec_result measured;
    static __device__ __forceinline__ u64 length(const measured *counts, u64 i) {
        return counts[i].total_symbols;
    }
    /* all of the item's symbols or none: there is no partial room (the caller allocates the total and launches again) */
    static __device__ __forceinline__ void place(const item *from, item *to, u64 off, u64 len, u64 reserved, u64 capacity) {
        (void)reserved;
        const bool fits = off <= capacity && len <= capacity - off;
        to->in_off = from->in_off;
        to->in_len = from->in_len;
        to->out_off = off;
        to->out_cap = fits ? len : 0;
        to->first_bit = from->first_bit;
        to->first_chunk = from->first_chunk;
        to->n_chunks = from->n_chunks;
        to->tiny = from->tiny;
    }
};

/* A third kind of batch (`decode` == kPackIndex), the block index of a stream (index_kernels.hip, huffman_amd_index.h): "item"
 * i is block i, its length the code bits index_block_bits left in index[i], scanned in place -- a thread reads index[i] in
 * front of the scan's barriers and writes the same word behind them; nothing to place.  Bit 63 of an entry says that a
 * symbol without a code was met: it travels where the other kinds' largest length travels, and ends in a status word */
constexpr u32 kPackIndex = 2;
constexpr u64 kPackIndexHole = 1ull << 63;

/* Two more kinds, the directory of a batch's block index (aws_huffman_amd_encode_plan_block_index, huffman_amd_batch_index.h):
 * the "lengths" are an encode plan's item records.  kPackBlocks: an item's length is its blocks, ceil(in_len / block_symbols),
 * and what is written is the directory -- record i = {the blocks in front of item i, in_len}, record n_items = {all blocks, 0}
 * -- with the verdict on the caller's capacity.  kPackTiles: an item's length is the tiles the hot pass cuts it into (none
 * for an item a wave takes), and what is written is tile_first[0 .. n_items].
 * The scan of such an index (kPackIndex) reads its entries' count from device memory -- the host knows the capacity only and
 * sizes the grid from that: workgroups without work leave, as all do where the entries do not fit.
 *
 * pack_offsets_kernel sits at 80 scalar registers, the most that admits eight of its workgroups a CU, and with these kinds
 * compiled into it (106) the scans of ALL kinds lost two of them: the single stream's index at 64 symbols a block measured
 * 3.6 % slower (profiles/batch_index_mi355x.json, scan_kinds_inside_pack_offsets_kernel).  So the scan's bodies are
 * templates: the two pack kernels are the builds without these kinds, as they were, and the builds with them are further
 * bodies of unpack_records_kernel (a thread a record, nowhere near a limit), chosen by a launch argument.  What these kinds
 * need beyond the scan's own arguments travels in a pack_batch, a member of that launch argument. */
constexpr u32 kPackBlocks = 3;
constexpr u32 kPackTiles = 4;
/* A sixth kind, the offsets of a packed launch that has made the batch's block index in place of its length pass
 * (aws_huffman_amd_encode_plan_launch_packed_indexed, huffman_amd_packed_index.h): the "lengths" are the plan's item records
 * again, and an item's length is what the scanned index says of it, with f_i = directory[i].first_block
 *   len_i = ceil((index[f_{i+1}] - index[f_i] + ovf_bits_i) / 8)
 * -- the carried bits count towards the length, not towards the index -- rounded and placed as kind 0 does (pack_encode::place).
 * Where the index does not fit the device has no lengths: every length is 0, so every offset, every room and both summary
 * words are.  It lives here, not in pack_offsets_kernel, for the reason above, and as builds of the bodies of its own
 * (INDEXED, the kind a constant in them): compiled into the builds of the other batch kinds the kernel parked sixteen scalar
 * registers in vector lanes, with builds of its own four (no scratch memory either way). */
constexpr u32 kPackIndexed = 5;
constexpr u64 kPackMaxBlocks = 1ull << 32; /* what an item counts at most: no sum of 2^32 items overflows */
/* Two kinds with items stored raw (huffman_amd_stored.h), builds of the bodies of their own (STORED, the kind a constant in
 * them) for the reason above.  kPackStored, the offsets of aws_huffman_amd_encode_plan_launch_packed_stored: kind 0 with
 *   len_i = stored_i ? in_len_i : ceil(total_bits_i / 8),   stored_i = in_len_i > 0 && ovf_bits_i == 0 && ceil(..) >= in_len_i
 * -- the plan's item records travel beside the length pass's records --; the offsets pass also writes the caller's flag, gives
 * a stored item no room in the second record array (the encode pass writes nothing for it: stored_copy.hpp copies it
 * behind that pass) and clears the two words the copy counts the stored items in.  kPackUnstored, the offsets of a packed
 * decode launch of a plan with stored items: kind 1 with sym_i = the packed length of a stored item, as the plan's stored
 * records {source offset, length or kPackNotStored} say.  A ninth, kPackStoredTiles, a build of the batch kinds: the tiles
 * the copy cuts the long stored items of such a plan into, from the same records, scanned into tile_first[0 .. n_items]. */
constexpr u32 kPackStored = 6;
constexpr u32 kPackUnstored = 7;
constexpr u32 kPackStoredTiles = 8;
/* A tenth, the offsets of aws_huffman_amd_encode_plan_launch_packed_stored_indexed (huffman_amd_stored_index.h): kPackStored
 * with the coded length kPackIndexed reads out of the scanned index in place of the length pass's record -- builds of the
 * bodies with both constants, INDEXED and STORED == kPackStored.  `lengths` and batch.second are both the plan's item records.
 * Where the index does not fit every coded length is 0, so no item is stored and every flag is 0. */
constexpr u32 kPackStoredIndexed = 9;
/* An eleventh, the offsets of aws_huffman_amd_encode_plan_launch_packed_constant (huffman_amd_constant.h): kPackStored with one
 * rule in front,
 *   constant_i = ovf_bits_i == 0 && in_len_i > 9 && ceil(total_bits_i / 8) > 9 && !differs[i],   len_i = 9 for such an item
 * -- differs[]: what the detection (stored_copy.hpp) left in front of the scan --; the flag it writes is the item's kind, 0, 1
 * or 2, a constant item gets no room in the second record array either, and four words are cleared for the copy's counts.
 * Builds of the bodies of its own again (STORED == kPackConstant). */
constexpr u32 kPackConstant = 10;
constexpr u64 kPackConstantBytes = 9; /* AWS_HUFFMAN_AMD_CONSTANT_BYTES */
constexpr u64 kPackNotStored = HUFK_NOT_STORED;

struct pack_batch {
    u64 block_symbols, tile_blocks, wave_bytes; /* kPackBlocks, kPackTiles */
    u64 capacity;     /* kPackBlocks, and kPackIndex with a device count: the entries of the caller's index */
    u64 *index;       /* kPackBlocks: the caller's index (index[0] = 0 is written where the batch has no block) */
    u32 *status;      /* kPackBlocks: the caller's status word, or NULL */
    const u64 *count; /* kPackIndex: the batch's blocks, counted on the device (NULL: n_items holds); kPackIndexed: the same word */
    const u64 *directory; /* kPackIndexed: [n_items + 1][2], and `index` scanned, `capacity` its entries;
                           * kPackUnstored, kPackStoredTiles: the plan's stored records, [n_items][2] */
    const void *second;   /* kPackStored, kPackUnstored: the plan's item records (what `lengths` is not) */
    u8 *stored;           /* kPackStored: the caller's flags; kPackConstant: the caller's kinds */
    const u8 *differs;    /* kPackConstant: the detection's marks */
};

/* the rule of huffman_amd_stored.h: a tie is stored, carried bits and empty items never */
__device__ __forceinline__ bool pack_item_stored(const hufd_enc_item *item, u64 coded_len) {
    return item->in_len > 0 && item->ovf_bits == 0 && coded_len >= item->in_len;
}

/* the rule of huffman_amd_constant.h in front of it: 2 constant, 1 stored, 0 coded */
__device__ __forceinline__ u32 pack_item_kind(const hufd_enc_item *item, u64 coded_len, u32 differs) {
    if (item->ovf_bits == 0 && item->in_len > kPackConstantBytes && coded_len > kPackConstantBytes && !differs) {
        return 2u;
    }
    return pack_item_stored(item, coded_len) ? 1u : 0u;
}

/* whether a batch of `blocks` blocks has an index in `capacity` entries (blocks + 1 of them, blocks below 2^32) */
__device__ __forceinline__ bool pack_batch_fits(u64 blocks, u64 capacity) {
    return blocks < capacity && blocks < kPackMaxBlocks;
}

/* what the scanned index says of item i's code, with its carried bits, in bytes (0 where the index does not fit) */
__device__ __forceinline__ u64 pack_indexed_length(const hufd_enc_item *item, u64 i, const pack_batch &batch) {
    if (!pack_batch_fits(*batch.count, batch.capacity)) { /* (the same in every thread of the launch) */
        return 0;
    }
    const u64 from = batch.index[batch.directory[2 * i]], to = batch.index[batch.directory[2 * i + 2]];
    return (to - from + item->ovf_bits + 7) / 8;
}

/* the coded length of item i of a sender's batch: the length pass's record, or (INDEXED) the scanned index */
template <bool INDEXED>
__device__ __forceinline__ u64 pack_coded_length(const void *lengths, const hufd_enc_item *item, u64 i, const pack_batch &batch) {
    return INDEXED ? pack_indexed_length(item, i, batch)
                   : pack_encode::length(reinterpret_cast<const pack_encode::measured *>(lengths), i);
}

template <bool BATCH, bool INDEXED = false, u32 STORED = 0>
__device__ __forceinline__ u64 pack_length(const void *lengths, u32 decode, u64 i, const pack_batch &batch) {
    if (STORED == kPackStored) {
        const hufd_enc_item *item = reinterpret_cast<const hufd_enc_item *>(batch.second) + i;
        const u64 coded = pack_coded_length<INDEXED>(lengths, item, i, batch);
        return pack_item_stored(item, coded) ? item->in_len : coded;
    }
    if (STORED == kPackConstant) {
        const hufd_enc_item *item = reinterpret_cast<const hufd_enc_item *>(batch.second) + i;
        const u64 coded = pack_coded_length<INDEXED>(lengths, item, i, batch);
        const u32 kind = pack_item_kind(item, coded, batch.differs[i]);
        return kind == 2u ? kPackConstantBytes : (kind ? item->in_len : coded);
    }
    if (STORED == kPackUnstored) {
        const u64 raw = batch.directory[2 * i + 1];
        return raw != kPackNotStored ? raw : pack_decode::length(reinterpret_cast<const pack_decode::measured *>(lengths), i);
    }
    if (decode == kPackIndex) {
        return reinterpret_cast<const u64 *>(lengths)[i] & ~kPackIndexHole;
    }
    if (BATCH && decode == kPackStoredTiles) { /* (`lengths`: the stored records; tile_blocks: a tile's bytes) */
        const u64 len = reinterpret_cast<const u64 *>(lengths)[2 * i + 1];
        return len == kPackNotStored || len < batch.wave_bytes ? 0 : (len + batch.tile_blocks - 1) / batch.tile_blocks;
    }
    if (INDEXED) {
        return pack_indexed_length(reinterpret_cast<const hufd_enc_item *>(lengths) + i, i, batch);
    }
    if (BATCH && decode >= kPackBlocks) {
        const u64 block_symbols = batch.block_symbols, tile_blocks = batch.tile_blocks, wave_bytes = batch.wave_bytes;
        const u64 len = reinterpret_cast<const hufd_enc_item *>(lengths)[i].in_len;
        u64 blocks = len / block_symbols + (len % block_symbols ? 1u : 0u);
        blocks = blocks < kPackMaxBlocks ? blocks : kPackMaxBlocks;
        if (decode == kPackBlocks) {
            return blocks;
        }
        return len < wave_bytes ? 0 : (blocks + tile_blocks - 1) / tile_blocks;
    }
    return decode ? pack_decode::length(reinterpret_cast<const pack_decode::measured *>(lengths), i)
                  : pack_encode::length(reinterpret_cast<const pack_encode::measured *>(lengths), i);
}

/* what an item adds to the maximum: its reserved length, or the index entry as it stands (bit 63 and all) */
__device__ __forceinline__ u64 pack_most(const void *lengths, u32 decode, u64 i, u64 reserved) {
    return decode == kPackIndex ? reinterpret_cast<const u64 *>(lengths)[i] : reserved;
}

template <bool BATCH, bool INDEXED = false, u32 STORED = 0>
__device__ __forceinline__ u64 pack_reserved(const void *lengths, u32 decode, u64 i, u64 align_mask, const pack_batch &batch) {
    const u64 len = pack_length<BATCH, INDEXED, STORED>(lengths, decode, i, batch);
    return BATCH && !INDEXED && !STORED && decode >= kPackBlocks ? len : (len + align_mask) & ~align_mask;
}

/* the entries a scan has: for the index of a batch (`count` != NULL) what the device says, 0 where there is nothing to scan
 * (no block, or an index that does not fit) */
template <bool BATCH>
__device__ __forceinline__ u32 pack_counted(u32 n_items, u32 decode, const pack_batch &batch) {
    if (!BATCH || decode != kPackIndex || batch.count == nullptr) {
        return n_items;
    }
    const u64 blocks = *batch.count;
    return pack_batch_fits(blocks, batch.capacity) ? (u32)blocks : 0u;
}

/* the workgroup's sum and maximum, in every thread; `slots`: 2 * kPackWaves words of LDS */
__device__ __forceinline__ void pack_block_sum_max(u64 &sum, u64 &most, u64 *slots) {
#pragma unroll
    for (u32 d = kWave / 2; d > 0; d >>= 1) {
        sum += __shfl_xor(sum, d);
        const u64 o = __shfl_xor(most, d);
        most = o > most ? o : most;
    }
    const u32 wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        slots[wave] = sum;
        slots[kPackWaves + wave] = most;
    }
    __syncthreads();
    sum = 0;
    most = 0;
#pragma unroll
    for (u32 w = 0; w < kPackWaves; ++w) {
        sum += slots[w];
        most = slots[kPackWaves + w] > most ? slots[kPackWaves + w] : most;
    }
    __syncthreads();
}

/* block_exclusive_sum (kernels_common.hpp) over 64-bit values; `slots`: kPackWaves words of LDS */
__device__ __forceinline__ u64 pack_block_exclusive_sum(u64 v, u64 *slots, u64 &total) {
    const u32 lane = threadIdx.x & (kWave - 1);
    const u32 wave = threadIdx.x / kWave;
    u64 incl = v;
#pragma unroll
    for (u32 d = 1; d < kWave; d <<= 1) {
        const u64 up = __shfl_up(incl, d);
        if (lane >= d) {
            incl += up;
        }
    }
    if (lane == kWave - 1) {
        slots[wave] = incl;
    }
    __syncthreads();
    u64 before = 0, all = 0;
#pragma unroll
    for (u32 w = 0; w < kPackWaves; ++w) {
        const u64 t = slots[w];
        before += w < wave ? t : 0;
        all += t;
    }
    __syncthreads();
    total = all;
    return before + incl - v;
}

/* tile_sums[2 b] = the sum of reserved_i over tile b, tile_sums[2 b + 1] = the largest of them */
template <bool BATCH, bool INDEXED = false, u32 STORED = 0>
__device__ __forceinline__ void pack_tile_sums_body(
    const void *lengths, u32 decode, u32 n_items, u32 tile_items, u64 align_mask, u64 *tile_sums, const pack_batch &batch) {
    u64 *slots = reinterpret_cast<u64 *>(dyn_lds);
    n_items = pack_counted<BATCH>(n_items, decode, batch);
    const u64 lo = (u64)blockIdx.x * tile_items;
    if (BATCH && lo >= n_items) { /* (the same in every thread; never so where the host knows the count) */
        return;
    }
    const u64 hi = lo + tile_items < n_items ? lo + tile_items : n_items;
    u64 sum = 0, most = 0;
    for (u64 i = lo + threadIdx.x; i < hi; i += kPackThreads) {
        const u64 r = pack_reserved<BATCH, INDEXED, STORED>(lengths, decode, i, align_mask, batch);
        const u64 m = pack_most(lengths, decode, i, r);
        sum += r;
        most = m > most ? m : most;
    }
    pack_block_sum_max(sum, most, slots);
    if (threadIdx.x == 0) {
        tile_sums[2 * (u64)blockIdx.x] = sum;
        tile_sums[2 * (u64)blockIdx.x + 1] = most;
    }
}

/* offsets[0 .. n_items], packed[0 .. n_items), summary[0] = the total, summary[1] = the largest reserved length */
template <bool BATCH, bool INDEXED = false, u32 STORED = 0>
__device__ __forceinline__ void pack_offsets_body(
    const void *items, const void *lengths, u32 decode, u32 n_items, u32 tile_items, u64 align_mask, u64 capacity,
    const u64 *tile_sums, u64 *offsets, void *packed, u64 *summary, const pack_batch &batch) {
    u64 *slots = reinterpret_cast<u64 *>(dyn_lds);
    n_items = pack_counted<BATCH>(n_items, decode, batch);
    if (BATCH && decode == kPackIndex && (u64)blockIdx.x * tile_items >= n_items) { /* (the same in every thread; only with a device count) */
        return;
    }
    /* where the tile starts: the sums of the tiles in front (and, for the last workgroup's sake, their maximum) */
    u64 at = 0, most = 0;
    for (u32 k = threadIdx.x; k < blockIdx.x; k += kPackThreads) {
        at += tile_sums[2 * (u64)k];
        const u64 m = tile_sums[2 * (u64)k + 1];
        most = m > most ? m : most;
    }
    pack_block_sum_max(at, most, slots + kPackWaves);
    const u64 lo = (u64)blockIdx.x * tile_items;
    const u64 hi = lo + tile_items < n_items ? lo + tile_items : n_items;
    u64 mine = 0; /* the largest reserved length this thread met */
    for (u64 round = lo; round < hi; round += kPackThreads) { /* (the same trips in every thread: the scan has barriers) */
        const u64 i = round + threadIdx.x;
        const u64 reserved = i < hi ? pack_reserved<BATCH, INDEXED, STORED>(lengths, decode, i, align_mask, batch) : 0;
        const u64 marked = i < hi ? pack_most(lengths, decode, i, reserved) : 0;
        u64 total = 0;
        const u64 off = at + pack_block_exclusive_sum(reserved, slots, total);
        if (i < hi) {
            if (STORED == kPackStored) {
                const pack_encode::item *from = reinterpret_cast<const pack_encode::item *>(batch.second) + i;
                pack_encode::item *to = reinterpret_cast<pack_encode::item *>(packed) + i;
                const bool stored = pack_item_stored(from, pack_coded_length<INDEXED>(lengths, from, i, batch));
                pack_encode::place(from, to, off, 0, reserved, capacity);
                if (stored) {
                    to->out_cap = 0;
                }
                batch.stored[i] = stored ? 1u : 0u;
            } else if (STORED == kPackConstant) {
                const pack_encode::item *from = reinterpret_cast<const pack_encode::item *>(batch.second) + i;
                pack_encode::item *to = reinterpret_cast<pack_encode::item *>(packed) + i;
                const u32 kind = pack_item_kind(from, pack_coded_length<INDEXED>(lengths, from, i, batch), batch.differs[i]);
                pack_encode::place(from, to, off, 0, reserved, capacity);
                if (kind) {
                    to->out_cap = 0;
                }
                batch.stored[i] = (u8)kind;
            } else if (STORED == kPackUnstored) {
                pack_decode::place(
                    reinterpret_cast<const pack_decode::item *>(batch.second) + i, reinterpret_cast<pack_decode::item *>(packed) + i, off,
                    pack_length<BATCH, INDEXED, STORED>(lengths, decode, i, batch), reserved, capacity);
            } else if (decode == 1) {
                pack_decode::place(
                    reinterpret_cast<const pack_decode::item *>(items) + i, reinterpret_cast<pack_decode::item *>(packed) + i, off,
                    pack_length<BATCH>(lengths, decode, i, batch), reserved, capacity);
            } else if (decode == 0 || INDEXED) {
                pack_encode::place(
                    reinterpret_cast<const pack_encode::item *>(items) + i, reinterpret_cast<pack_encode::item *>(packed) + i, off, 0,
                    reserved, capacity);
            }
            if (BATCH && decode == kPackBlocks) {
                offsets[2 * i] = off;
                offsets[2 * i + 1] = reinterpret_cast<const hufd_enc_item *>(lengths)[i].in_len;
            } else {
                offsets[i] = off; /* (never clipped: what the caller would have needed) */
            }
            mine = marked > mine ? marked : mine;
        }
        at += total;
    }
    /* the last workgroup -- of those that have work, where the count came from the device */
    if (BATCH ? hi == n_items : blockIdx.x == gridDim.x - 1) {
        u64 unused = 0;
        pack_block_sum_max(unused, mine, slots + kPackWaves);
        if (threadIdx.x == 0) {
            if (BATCH && decode == kPackBlocks) {
                offsets[2 * (u64)n_items] = at;
                offsets[2 * (u64)n_items + 1] = 0;
                summary[0] = at;
                /* a batch with blocks that fit: the scan of the index writes the status behind the hot pass */
                const bool fits = pack_batch_fits(at, batch.capacity);
                if (fits && at == 0) {
                    batch.index[0] = 0;
                }
                if (batch.status && (!fits || at == 0)) {
                    *batch.status = fits ? HUFK_INDEX_OK : HUFK_INDEX_TOO_SMALL;
                }
                return;
            }
            offsets[n_items] = at;
            if (BATCH && (decode == kPackTiles || decode == kPackStoredTiles)) {
                return;
            }
            if (decode == kPackIndex) {
                if (summary) { /* (the caller's status word: four bytes) */
                    *reinterpret_cast<u32 *>(summary) =
                        ((mine | most) & kPackIndexHole) ? HUFK_INDEX_SYMBOL_WITHOUT_CODE : HUFK_INDEX_OK;
                }
            } else {
                summary[0] = at;
                summary[1] = mine > most ? mine : most;
                if (STORED == kPackStored) { /* (the stored items and their bytes: the copy behind the encode pass adds them) */
                    summary[2] = 0;
                    summary[3] = 0;
                }
                if (STORED == kPackConstant) { /* (... and the constant items and theirs) */
                    summary[2] = 0;
                    summary[3] = 0;
                    summary[4] = 0;
                    summary[5] = 0;
                }
            }
        }
    }
}

__global__ __launch_bounds__(kPackThreads) void pack_tile_sums_kernel(
    const void *lengths, u32 decode, u32 n_items, u32 tile_items, u64 align_mask, u64 *tile_sums) {
    pack_tile_sums_body<false>(lengths, decode, n_items, tile_items, align_mask, tile_sums, pack_batch{});
}

__global__ __launch_bounds__(kPackThreads) void pack_offsets_kernel(
    const void *items, const void *lengths, u32 decode, u32 n_items, u32 tile_items, u64 align_mask, u64 capacity,
    const u64 *tile_sums, u64 *offsets, void *packed, u64 *summary) {
    pack_offsets_body<false>(
        items, lengths, decode, n_items, tile_items, align_mask, capacity, tile_sums, offsets, packed, summary, pack_batch{});
}

#include "stored_copy.hpp"
static_assert(kPlanesMergeThreads == kPackThreads, "planes_merge is hosted by unpack_records_kernel");

/* what unpack_records_kernel is given where it runs a pass of the scan with the batch kinds (pass 0: it does not) */
struct pack_scan {
    u32 pass; /* 1: the tile sums, 2: the offsets, 3: the copy of items stored raw (stored_copy.hpp), 4: byte planes merged, or their differences summed in runs (planes.hpp) */
    u32 unused;
    union { /* (a launch is a pass of the scan or the copy, never both: the copy's job shares the scan's words) */
        struct {
            u32 decode, n_items, tile_items;
            const void *lengths;
            u64 *tile_sums, *offsets, *summary;
            pack_batch batch;
            /* kPackIndexed, kPackStored, kPackUnstored (0 and NULL for every other kind): what kinds 0 and 1 are given as
             * arguments of pack_offsets_kernel -- the items are `lengths` (kPackIndexed) or batch.second */
            u64 align_mask, out_capacity;
            void *packed;
        };
        stored_job stored; /* pass 3 */
        planes_job planes; /* pass 4 */
    };
};

/* The records of a packed decode launch that are not the scan's to write, a thread each (ONE kernel for both uses):
 *   chunk_rec == nullptr   packed[i] = items[i] with no room at all, i < n: what the kernels that walk and write in one go
 *                          count against
 *   otherwise              packed_rec[c] = chunk_rec[c] with out_off / out_cap of its item's packed record, c < n
 * and, chosen by a launch argument that is the same in every thread, the scan's two passes with the batch kinds (above) */
__global__ __launch_bounds__(kPackThreads) void unpack_records_kernel(
    const hufd_dec_item *items, hufd_dec_item *packed, const hufd_chunk_rec *chunk_rec, hufd_chunk_rec *packed_rec, u32 n,
    pack_scan scan) {
    if (scan.pass == 3) {
        stored_copy_body(scan.stored);
        return;
    }
    if (scan.pass == 4) {
        planes_merge(scan.planes);
        return;
    }
    if (scan.pass == 1) {
        if (scan.decode == kPackIndexed) {
            pack_tile_sums_body<true, true>(
                scan.lengths, kPackIndexed, scan.n_items, scan.tile_items, scan.align_mask, scan.tile_sums, scan.batch);
        } else if (scan.decode == kPackStored) {
            pack_tile_sums_body<true, false, kPackStored>(
                scan.lengths, kPackStored, scan.n_items, scan.tile_items, scan.align_mask, scan.tile_sums, scan.batch);
        } else if (scan.decode == kPackConstant) {
            pack_tile_sums_body<true, false, kPackConstant>(
                scan.lengths, kPackConstant, scan.n_items, scan.tile_items, scan.align_mask, scan.tile_sums, scan.batch);
        } else if (scan.decode == kPackStoredIndexed) {
            pack_tile_sums_body<true, true, kPackStored>(
                scan.lengths, kPackStoredIndexed, scan.n_items, scan.tile_items, scan.align_mask, scan.tile_sums, scan.batch);
        } else if (scan.decode == kPackUnstored) {
            pack_tile_sums_body<true, false, kPackUnstored>(
                scan.lengths, kPackUnstored, scan.n_items, scan.tile_items, scan.align_mask, scan.tile_sums, scan.batch);
        } else {
            pack_tile_sums_body<true>(scan.lengths, scan.decode, scan.n_items, scan.tile_items, 0, scan.tile_sums, scan.batch);
        }
        return;
    }
    if (scan.pass == 2) {
        if (scan.decode == kPackIndexed) {
            pack_offsets_body<true, true>(
                scan.lengths, scan.lengths, kPackIndexed, scan.n_items, scan.tile_items, scan.align_mask, scan.out_capacity,
                scan.tile_sums, scan.offsets, scan.packed, scan.summary, scan.batch);
        } else if (scan.decode == kPackStored) {
            pack_offsets_body<true, false, kPackStored>(
                scan.batch.second, scan.lengths, kPackStored, scan.n_items, scan.tile_items, scan.align_mask, scan.out_capacity,
                scan.tile_sums, scan.offsets, scan.packed, scan.summary, scan.batch);
        } else if (scan.decode == kPackConstant) {
            pack_offsets_body<true, false, kPackConstant>(
                scan.batch.second, scan.lengths, kPackConstant, scan.n_items, scan.tile_items, scan.align_mask, scan.out_capacity,
                scan.tile_sums, scan.offsets, scan.packed, scan.summary, scan.batch);
        } else if (scan.decode == kPackStoredIndexed) {
            pack_offsets_body<true, true, kPackStored>(
                scan.batch.second, scan.lengths, kPackStoredIndexed, scan.n_items, scan.tile_items, scan.align_mask, scan.out_capacity,
                scan.tile_sums, scan.offsets, scan.packed, scan.summary, scan.batch);
        } else if (scan.decode == kPackUnstored) {
            pack_offsets_body<true, false, kPackUnstored>(
                scan.batch.second, scan.lengths, kPackUnstored, scan.n_items, scan.tile_items, scan.align_mask, scan.out_capacity,
                scan.tile_sums, scan.offsets, scan.packed, scan.summary, scan.batch);
        } else {
            pack_offsets_body<true>(
                nullptr, scan.lengths, scan.decode, scan.n_items, scan.tile_items, 0, 0, scan.tile_sums, scan.offsets, nullptr,
                scan.summary, scan.batch);
        }
        return;
    }
    const u32 k = blockIdx.x * kPackThreads + threadIdx.x;
    if (k >= n) {
        return;
    }
    if (chunk_rec == nullptr) {
        pack_decode::place(items + k, packed + k, 0, 1, 0, 0);
        return;
    }
    const hufd_chunk_rec *from = chunk_rec + k;
    hufd_chunk_rec *to = packed_rec + k;
    const u32 item = from->item;
    to->src_off = from->src_off;
    to->out_off = packed[item].out_off;
    to->out_cap = packed[item].out_cap;
    to->valid = from->valid;
    to->item = item;
    to->entry_bit = from->entry_bit;
    to->reserved = 0;
}

int pack_offsets_launch(
    const void *items, const void *lengths, uint32_t decode, uint32_t n_items, uint32_t tile_items, uint64_t align,
    uint64_t capacity, uint64_t *tile_sums, uint64_t *offsets, void *packed, uint64_t *summary, hipStream_t st) {
    if (n_items == 0 || tile_items == 0) {
        return 0;
    }
    const uint32_t tiles = hufk_pack_tiles(n_items, tile_items);
    const u64 align_mask = align - 1;
    if (tiles > 1) {
        hipLaunchKernelGGL(
            pack_tile_sums_kernel, dim3(tiles - 1), dim3(kPackThreads), kPackLdsBytes, st, lengths, decode, n_items, tile_items,
            align_mask, tile_sums); /* (nobody reads the last tile's sums) */
    }
    hipLaunchKernelGGL(
        pack_offsets_kernel, dim3(tiles), dim3(kPackThreads), kPackLdsBytes, st, items, lengths, decode, n_items, tile_items,
        align_mask, capacity, (const u64 *)tile_sums, offsets, packed, summary);
    return (int)hipGetLastError();
}

/* the same two passes with the batch kinds: the bodies unpack_records_kernel hosts (align, out_capacity, packed: kPackIndexed's) */
int pack_batch_launch(
    const void *lengths, uint32_t decode, uint32_t n_items, uint32_t tile_items, uint64_t *tile_sums, uint64_t *offsets,
    uint64_t *summary, const pack_batch &batch, hipStream_t st, uint64_t align = 1, uint64_t out_capacity = 0,
    void *packed = nullptr) {
    /* (a directory of no items is still a record, a total and a status: one workgroup) */
    const uint32_t tiles = n_items ? hufk_pack_tiles(n_items, tile_items) : 1u;
    pack_scan scan{};
    scan.decode = decode;
    scan.n_items = n_items;
    scan.tile_items = tile_items;
    scan.lengths = lengths;
    scan.tile_sums = tile_sums;
    scan.offsets = offsets;
    scan.summary = summary;
    scan.batch = batch;
    scan.align_mask = align - 1;
    scan.out_capacity = out_capacity;
    scan.packed = packed;
    for (scan.pass = tiles > 1 ? 1 : 2; scan.pass <= 2; ++scan.pass) { /* (nobody reads the last tile's sums) */
        hipLaunchKernelGGL(
            unpack_records_kernel, dim3(scan.pass == 1 ? tiles - 1 : tiles), dim3(kPackThreads), kPackLdsBytes, st,
            (const hufd_dec_item *)nullptr, (hufd_dec_item *)nullptr, (const hufd_chunk_rec *)nullptr, (hufd_chunk_rec *)nullptr, 0u, scan);
    }
    return (int)hipGetLastError();
}

/* a launch of the bodies of stored_copy.hpp */
void stored_launch(const stored_job &job, uint32_t blocks, hipStream_t st) {
    pack_scan scan{};
    scan.pass = 3;
    scan.stored = job;
    hipLaunchKernelGGL(
        unpack_records_kernel, dim3(blocks), dim3(kPackThreads), kPackLdsBytes, st, (const hufd_dec_item *)nullptr, (hufd_dec_item *)nullptr,
        (const hufd_chunk_rec *)nullptr, (hufd_chunk_rec *)nullptr, 0u, scan);
}

} /* namespace */

extern "C" {

uint32_t hufk_pack_tile_items(uint32_t n_items, uint32_t asked) {
    if (asked) {
        return asked;
    }
    /* at most kPackMaxTiles tiles, of whole rounds */
    const uint64_t per = ((uint64_t)n_items + kPackMaxTiles - 1) / kPackMaxTiles;
    const uint64_t rounded = (per + kPackThreads - 1) / kPackThreads * kPackThreads;
    return (uint32_t)(rounded > kPackTileItems ? rounded : kPackTileItems);
}

uint32_t hufk_pack_tiles(uint32_t n_items, uint32_t tile_items) {
    return (uint32_t)(((uint64_t)n_items + tile_items - 1) / tile_items);
}

int hufk_pack_offsets(
    const struct hufd_enc_item *items, const struct hufd_enc_result *lengths, uint32_t n_items, uint32_t tile_items, uint64_t align,
    uint64_t capacity, uint64_t *tile_sums, uint64_t *offsets, struct hufd_enc_item *packed, uint64_t *summary, void *stream) {
    return pack_offsets_launch(
        items, lengths, 0u, n_items, tile_items, align, capacity, tile_sums, offsets, packed, summary, (hipStream_t)stream);
}

int hufk_index_scan(uint64_t *index, uint32_t n_blocks, uint32_t tile_blocks, uint64_t *tile_sums, uint32_t *status, void *stream) {
    return pack_offsets_launch(
        nullptr, index, kPackIndex, n_blocks, tile_blocks, 1, 0, tile_sums, index, nullptr, reinterpret_cast<uint64_t *>(status),
        (hipStream_t)stream);
}

int hufk_batch_directory(
    const struct hufd_enc_item *items, uint32_t n_items, uint32_t tile_items, uint64_t block_symbols, uint64_t wave_bytes,
    uint64_t tile_blocks, uint64_t capacity, uint64_t *tile_sums, uint64_t *directory, uint64_t *tile_first, uint64_t *summary,
    uint64_t *index, uint32_t *status, void *stream) {
    pack_batch batch{};
    batch.block_symbols = block_symbols;
    batch.tile_blocks = tile_blocks;
    batch.wave_bytes = wave_bytes;
    batch.capacity = capacity;
    batch.index = index;
    batch.status = status;
    const int e = pack_batch_launch(items, kPackBlocks, n_items, tile_items, tile_sums, directory, summary, batch, (hipStream_t)stream);
    if (e || capacity == 0 || n_items == 0) { /* (a size query, or nothing to cut into tiles) */
        return e;
    }
    return pack_batch_launch(items, kPackTiles, n_items, tile_items, tile_sums, tile_first, nullptr, batch, (hipStream_t)stream);
}

int hufk_batch_index_scan(
    uint64_t *index, const uint64_t *device_blocks, uint64_t capacity, uint32_t most_blocks, uint32_t tile_blocks, uint64_t *tile_sums,
    uint32_t *status, void *stream) {
    if (most_blocks == 0 || tile_blocks == 0) {
        return 0;
    }
    pack_batch batch{};
    batch.capacity = capacity;
    batch.count = device_blocks;
    return pack_batch_launch(
        index, kPackIndex, most_blocks, tile_blocks, tile_sums, index, reinterpret_cast<uint64_t *>(status), batch, (hipStream_t)stream);
}

int hufk_pack_offsets_indexed(
    const struct hufd_enc_item *items, uint32_t n_items, uint32_t tile_items, uint64_t align, uint64_t capacity,
    const uint64_t *directory, const uint64_t *index, uint64_t index_capacity, uint64_t *tile_sums, uint64_t *offsets,
    struct hufd_enc_item *packed, uint64_t *summary, void *stream) {
    if (n_items == 0 || tile_items == 0) {
        return 0;
    }
    pack_batch batch{};
    batch.capacity = index_capacity;
    batch.index = const_cast<uint64_t *>(index); /* (read only by this kind) */
    batch.count = directory + 2 * (uint64_t)n_items;
    batch.directory = directory;
    return pack_batch_launch(
        items, kPackIndexed, n_items, tile_items, tile_sums, offsets, summary, batch, (hipStream_t)stream, align, capacity, packed);
}

int hufk_pack_offsets_stored(
    const struct hufd_enc_item *items, const struct hufd_enc_result *lengths, uint32_t n_items, uint32_t tile_items, uint64_t align,
    uint64_t capacity, uint64_t *tile_sums, uint64_t *offsets, struct hufd_enc_item *packed, uint64_t *summary, uint8_t *stored,
    void *stream) {
    if (n_items == 0 || tile_items == 0) {
        return 0;
    }
    pack_batch batch{};
    batch.second = items;
    batch.stored = stored;
    return pack_batch_launch(
        lengths, kPackStored, n_items, tile_items, tile_sums, offsets, summary, batch, (hipStream_t)stream, align, capacity, packed);
}

int hufk_pack_offsets_constant(
    const struct hufd_enc_item *items, const struct hufd_enc_result *lengths, uint32_t n_items, uint32_t tile_items, uint64_t align,
    uint64_t capacity, uint64_t *tile_sums, uint64_t *offsets, struct hufd_enc_item *packed, uint64_t *summary, uint8_t *kinds,
    const uint8_t *differs, void *stream) {
    if (n_items == 0 || tile_items == 0) {
        return 0;
    }
    pack_batch batch{};
    batch.second = items;
    batch.stored = kinds;
    batch.differs = differs;
    return pack_batch_launch(
        lengths, kPackConstant, n_items, tile_items, tile_sums, offsets, summary, batch, (hipStream_t)stream, align, capacity, packed);
}

int hufk_pack_offsets_stored_indexed(
    const struct hufd_enc_item *items, uint32_t n_items, uint32_t tile_items, uint64_t align, uint64_t capacity,
    const uint64_t *directory, const uint64_t *index, uint64_t index_capacity, uint64_t *tile_sums, uint64_t *offsets,
    struct hufd_enc_item *packed, uint64_t *summary, uint8_t *stored, void *stream) {
    if (n_items == 0 || tile_items == 0) {
        return 0;
    }
    pack_batch batch{};
    batch.capacity = index_capacity;
    batch.index = const_cast<uint64_t *>(index); /* (read only by this kind) */
    batch.count = directory + 2 * (uint64_t)n_items;
    batch.directory = directory;
    batch.second = items;
    batch.stored = stored;
    return pack_batch_launch(
        items, kPackStoredIndexed, n_items, tile_items, tile_sums, offsets, summary, batch, (hipStream_t)stream, align, capacity, packed);
}

int hufk_stored_tiles(
    const uint64_t *stored_rec, uint32_t n_items, uint32_t tile_items, uint64_t tile_bytes, uint64_t wave_bytes, uint64_t *tile_sums,
    uint64_t *tile_first, void *stream) {
    if (n_items == 0 || tile_items == 0) {
        return 0;
    }
    pack_batch batch{};
    batch.block_symbols = 1;
    batch.tile_blocks = tile_bytes;
    batch.wave_bytes = wave_bytes;
    return pack_batch_launch(stored_rec, kPackStoredTiles, n_items, tile_items, tile_sums, tile_first, nullptr, batch, (hipStream_t)stream);
}

int hufk_unpack_blank(const struct hufd_dec_item *items, uint32_t n_items, struct hufd_dec_item *packed, void *stream) {
    if (n_items == 0) {
        return 0;
    }
    hipLaunchKernelGGL(
        unpack_records_kernel, dim3((n_items + kPackThreads - 1) / kPackThreads), dim3(kPackThreads), 0, (hipStream_t)stream, items, packed,
        (const hufd_chunk_rec *)nullptr, (hufd_chunk_rec *)nullptr, n_items, pack_scan{});
    return (int)hipGetLastError();
}

int hufk_unpack_offsets(
    const struct hufd_dec_item *items, const struct hufd_dec_result *counts, uint32_t n_items, uint32_t tile_items, uint64_t align,
    uint64_t capacity, uint64_t *tile_sums, uint64_t *offsets, struct hufd_dec_item *packed, uint64_t *summary,
    const struct hufd_chunk_rec *chunk_rec, uint32_t n_chunks, struct hufd_chunk_rec *packed_rec, const uint64_t *stored_rec,
    void *stream) {
    int e = 0;
    if (stored_rec && n_items && tile_items) { /* (a plan with stored items: their packed lengths for their symbols) */
        pack_batch batch{};
        batch.second = items;
        batch.directory = stored_rec;
        e = pack_batch_launch(
            counts, kPackUnstored, n_items, tile_items, tile_sums, offsets, summary, batch, (hipStream_t)stream, align, capacity, packed);
    } else {
        e = pack_offsets_launch(
            items, counts, 1u, n_items, tile_items, align, capacity, tile_sums, offsets, packed, summary, (hipStream_t)stream);
    }
    if (e || n_items == 0 || n_chunks == 0) {
        return e;
    }
    hipLaunchKernelGGL(
        unpack_records_kernel, dim3((n_chunks + kPackThreads - 1) / kPackThreads), dim3(kPackThreads), 0, (hipStream_t)stream,
        (const hufd_dec_item *)nullptr, packed, chunk_rec, packed_rec, n_chunks, pack_scan{});
    return (int)hipGetLastError();
}

int hufk_stored_copy_encode(
    const struct hufd_enc_item *items, uint32_t n_items, const struct hufd_enc_seg *segs, uint32_t n_segs, const uint32_t *solo,
    uint32_t n_solo, const uint32_t *tiny, uint32_t n_tiny, const uint8_t *stored, const uint64_t *offsets, uint64_t capacity,
    const void *input, void *output, struct hufd_enc_result *results, uint64_t *counts, uint8_t *differs, void *stream) {
    if (n_items == 0) {
        return 0;
    }
    const u64 by_items = ((u64)n_items + kStoredThreads - 1) / kStoredThreads;
    const u32 item_blocks = (u32)(by_items < kStoredItemBlocks ? by_items : kStoredItemBlocks);
    const u64 blocks = (u64)n_segs + ((u64)n_solo + kStoredWaves - 1) / kStoredWaves + ((u64)n_tiny + kStoredThreads - 1) / kStoredThreads +
                       item_blocks;
    if (blocks >> 31) {
        return (int)hipErrorInvalidValue;
    }
    stored_job job{};
    job.in = (const u8 *)input;
    job.out = (u8 *)output;
    job.n_items = n_items;
    job.items = items;
    job.segs = segs;
    job.solo = solo;
    job.tiny = tiny;
    job.n_segs = n_segs;
    job.n_solo = n_solo;
    job.n_tiny = n_tiny;
    job.stored = stored;
    job.offsets = offsets;
    job.capacity = capacity;
    job.enc_results = results;
    job.counts = counts;
    job.differs = differs;
    job.item_blocks = item_blocks;
    stored_launch(job, (u32)blocks, (hipStream_t)stream);
    return (int)hipGetLastError();
}

int hufk_constant_detect(
    const struct hufd_enc_item *items, uint32_t n_items, const struct hufd_enc_seg *segs, uint32_t n_segs, const uint32_t *solo,
    uint32_t n_solo, const uint32_t *tiny, uint32_t n_tiny, const void *input, uint8_t *differs, void *stream) {
    const u64 blocks = (u64)n_segs + ((u64)n_solo + kStoredWaves - 1) / kStoredWaves + ((u64)n_tiny + kStoredThreads - 1) / kStoredThreads;
    if (n_items == 0 || blocks == 0) {
        return 0;
    }
    if (blocks >> 31) {
        return (int)hipErrorInvalidValue;
    }
    stored_job job{};
    job.in = (const u8 *)input;
    job.n_items = n_items;
    job.receiver = 4;
    job.items = items;
    job.segs = segs;
    job.solo = solo;
    job.tiny = tiny;
    job.n_segs = n_segs;
    job.n_solo = n_solo;
    job.n_tiny = n_tiny;
    job.differs = differs;
    stored_launch(job, (u32)blocks, (hipStream_t)stream);
    return (int)hipGetLastError();
}

int hufk_stored_copy_decode(
    const uint64_t *stored_rec, const uint64_t *tile_first, uint64_t n_tiles, uint32_t n_items, const struct hufd_dec_item *placed,
    struct hufd_dec_result *results, const void *input, void *output, void *stream) {
    if (n_items == 0) {
        return 0;
    }
    if (!output) { /* (a size query places no item: no workgroup for a tile -- a constant item may count 2^18 of them) */
        n_tiles = 0;
    }
    const u64 blocks = n_tiles + ((u64)n_items + kStoredWaves - 1) / kStoredWaves + ((u64)n_items + kStoredThreads - 1) / kStoredThreads;
    if (n_tiles >> 31 || blocks >> 31) {
        return (int)hipErrorInvalidValue;
    }
    stored_job job{};
    job.in = (const u8 *)input;
    job.out = (u8 *)output;
    job.n_items = n_items;
    job.receiver = 1;
    job.rec = stored_rec;
    job.tile_first = tile_first;
    job.n_tiles = (u32)n_tiles;
    job.placed = placed;
    job.dec_results = results;
    stored_launch(job, (u32)blocks, (hipStream_t)stream);
    return (int)hipGetLastError();
}

int hufk_planes_merge(
    const void *planes, uint64_t plane_stride, uint64_t element_count, uint32_t element_bytes, uint32_t run_elements, void *output,
    uint32_t grid_cap, void *stream) {
    if (element_count == 0) {
        return 0;
    }
    pack_scan scan{};
    scan.pass = 4;
    scan.planes.planes = (const u8 *)planes;
    scan.planes.out = (u8 *)output;
    scan.planes.n = element_count;
    scan.planes.stride = plane_stride;
    scan.planes.element_bytes = element_bytes;
    scan.planes.run_elements = run_elements;
    const u64 step_elements = kPlanesMergeStepBytes / element_bytes;
    const u64 steps = (element_count + step_elements - 1) / step_elements;
    /* sums of differences: the waves' totals of a run, and of the tail's base, go through LDS */
    const u32 lds_bytes = run_elements ? kPlanesMergeSlotBytes : 0u;
    uint32_t grid = hufk_host::persistent_grid(
        unpack_records_kernel, kPackThreads, lds_bytes, (uint32_t)(steps < 0xFFFFFFFFull ? steps : 0xFFFFFFFFull));
    grid = grid_cap && grid_cap < grid ? grid_cap : grid;
    hipLaunchKernelGGL(
        unpack_records_kernel, dim3(grid), dim3(kPackThreads), lds_bytes, (hipStream_t)stream, (const hufd_dec_item *)nullptr,
        (hufd_dec_item *)nullptr, (const hufd_chunk_rec *)nullptr, (hufd_chunk_rec *)nullptr, 0u, scan);
    return (int)hipGetLastError();
}

int hufk_stored_records(
    const uint64_t *offsets, const uint64_t *lengths, const uint8_t *stored, const void *packed, uint32_t n_items,
    uint64_t *stored_rec, void *stream) {
    if (n_items == 0) {
        return 0;
    }
    stored_job job{};
    job.in = (const u8 *)packed;
    job.n_items = n_items;
    job.receiver = 2;
    job.offsets = offsets;
    job.lengths = lengths;
    job.stored = stored;
    job.new_rec = stored_rec;
    stored_launch(job, (n_items + kStoredThreads - 1) / kStoredThreads, (hipStream_t)stream);
    return (int)hipGetLastError();
}

int hufk_stored_range_records(
    const uint64_t *ranges, const uint8_t *stored, const struct hufd_dec_item *items, uint32_t n_items, uint64_t *stored_rec,
    void *stream) {
    if (n_items == 0) {
        return 0;
    }
    stored_job job{};
    job.n_items = n_items;
    job.receiver = 3;
    job.offsets = ranges;
    job.stored = stored;
    job.placed = items;
    job.new_rec = stored_rec;
    stored_launch(job, (n_items + kStoredThreads - 1) / kStoredThreads, (hipStream_t)stream);
    return (int)hipGetLastError();
}

} /* extern "C" */
