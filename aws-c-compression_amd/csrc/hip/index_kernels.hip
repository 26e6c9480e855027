/*
 * Block index of an encoded stream (aws_huffman_amd_block_index, huffman_amd_index.h): from the SYMBOLS of a stream and an
 * engine's encode table in device memory,
 *
 *   index[k] = the sum of the code lengths of symbols [0, min(k * block_symbols, length)),  k = 0 .. n_blocks
 *
 * -- the bit at which block k starts in what the engine encodes of the stream.  Two steps on the caller's stream:
 *
 *   block bits   the hot pass, one read of the symbols: index[k] = the bits of block k alone (index_block_bits.hpp; it runs
 *                as the second body of count_kernel, which reads the same bytes the same way: hufk_block_bits)
 *   scan         reduce, then scan, by the two kernels of pack_kernels.hip as they stand (hufk_index_scan: a third kind of
 *                batch whose "items" are the blocks and whose lengths are the index entries, scanned in place over 64-bit
 *                sums; the last workgroup writes index[n_blocks] and the status)
 *
 * No workgroup waits for another and nothing has to be clear before a launch: the three launches can be captured and
 * replayed.  The index feeds decode plans over ranges of whole blocks (aws_huffman_amd_decode_plan_reset_block_ranges): a
 * range is a kind of item source of the planner (HUFD_ITEMS_BLOCK_RANGES, load_item of plan_kernels.hip), read where every
 * other item record is read.  The feature adds no kernel of its own: the library's kernel census is held at 90.
 *
 * One index over the items of an encode plan (aws_huffman_amd_encode_plan_block_index, huffman_amd_batch_index.h) is the same
 * two steps behind a directory, with every count read on the device: hufk_batch_block_index below.
 */
#include "huffman_kernels.h"

namespace {

constexpr uint64_t kScanTileBlocks = 1024; /* a workgroup's entries: four rounds */
constexpr uint64_t kScanRound = 256;       /* pack_kernels.hip's workgroup */

} /* namespace */

extern "C" {

uint32_t hufk_index_tile_blocks(uint32_t n_blocks, uint32_t asked) {
    /* at most HUFK_INDEX_MAX_TILES tiles, of whole rounds */
    const uint64_t per = ((uint64_t)n_blocks + HUFK_INDEX_MAX_TILES - 1) / HUFK_INDEX_MAX_TILES;
    if (asked && asked >= per) {
        return asked;
    }
    const uint64_t rounded = (per + kScanRound - 1) / kScanRound * kScanRound;
    return (uint32_t)(rounded > kScanTileBlocks ? rounded : kScanTileBlocks);
}

int hufk_block_index(
    const uint64_t *enc_table, const void *input, uint64_t length, uint64_t block_symbols, uint32_t tile_blocks, uint64_t *index,
    uint64_t *tile_sums, uint32_t *status, void *stream) {
    const uint64_t n_blocks = (length + block_symbols - 1) / block_symbols;
    const int e = hufk_block_bits(enc_table, input, length, block_symbols, index, stream);
    return e ? e : hufk_index_scan(index, (uint32_t)n_blocks, tile_blocks, tile_sums, status, stream);
}

/* One index over the items of an encode plan: the directory (and the tiles in front of each item) by the scan kernels, the
 * hot pass, the scan of the entries.  The blocks are counted on the device: most_blocks is what the caller's capacity allows */
int hufk_batch_block_index(const struct hufk_batch_index *job, void *stream) {
    int e = hufk_batch_directory(
        job->items, job->n_items, job->pack_tile_items, job->block_symbols, job->wave_bytes, hufk_batch_tile_blocks(job->block_symbols),
        job->capacity, job->item_tile_sums, job->directory, job->tile_first, job->summary, job->index, job->status, stream);
    if (e || job->capacity < 2 || job->n_items == 0) { /* (no room for a block's entry: the directory's kernel has said so) */
        return e;
    }
    const uint64_t room = job->capacity - 1;
    const uint64_t most_blocks = room < 0xFFFFFFFFull ? room : 0xFFFFFFFFull;
    e = hufk_batch_block_bits(job, most_blocks, stream);
    if (e) {
        return e;
    }
    const uint32_t tile_blocks = hufk_index_tile_blocks((uint32_t)most_blocks, job->index_tile_asked);
    return hufk_batch_index_scan(
        job->index, job->directory + 2 * (uint64_t)job->n_items, job->capacity, (uint32_t)most_blocks, tile_blocks, job->index_tile_sums,
        job->status, stream);
}

} /* extern "C" */
