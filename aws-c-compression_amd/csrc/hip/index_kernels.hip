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

} /* extern "C" */
