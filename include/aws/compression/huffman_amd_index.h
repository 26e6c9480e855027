#ifndef AWS_COMPRESSION_HUFFMAN_AMD_INDEX_H
#define AWS_COMPRESSION_HUFFMAN_AMD_INDEX_H
/*
 * Block index of an encoded stream, made on the device; decode plans over ranges of blocks.
 *
 * A Huffman stream has no markers: symbol number n starts at the bit that is the sum of the code lengths of the n symbols
 * in front of it, and without that number the only way to symbols 700 000 000 .. 700 016 383 of an encoded stream is to
 * decode all of it.  The index is that sum at every multiple of block_symbols:
 *
 *   uint64_t *d_index = aws_huffman_amd_device_alloc(engine, (n_blocks + 1) * sizeof(uint64_t));
 *   aws_huffman_amd_block_index(engine, d_symbols, length, 16384, d_index, d_status, stream);      (beside the encode)
 *   ... later, a reader of blocks 42 713 and 42 714, with the encoded stream (and nothing of the symbols) in d_encoded:
 *   struct aws_huffman_amd_block_range r = {42713, 2, 0};                                          (in device memory)
 *   aws_huffman_amd_decode_plan_reset_block_ranges(plan, d_index, length, 16384, 0, encoded_length, d_ranges, 1, stream);
 *   aws_huffman_amd_decode_plan_launch(plan, d_encoded, d_output, stream);                         (32 768 symbols)
 *
 * The index is 8 bytes a block: 0.05 % of the symbols at 16 384 symbols a block, 12.5 % at 64.
 *
 * Ranges that start or end inside a block: huffman_amd_ranges.h (any range of symbols, located from this index on the
 * device).  One index over the items of a plan: huffman_amd_batch_index.h.  Out of this interface: an index made by the
 * encode launch itself (it would save this second read of the symbols and touches the one-pass encoder), and
 * aws_huffman_amd_shards_*.
 */

#include <aws/compression/huffman_amd.h>

AWS_EXTERN_C_BEGIN

/* what aws_huffman_amd_block_index leaves in *device_status */
#define AWS_HUFFMAN_AMD_INDEX_OK 0u
#define AWS_HUFFMAN_AMD_INDEX_SYMBOL_WITHOUT_CODE 1u /* counted as 0 bits, as aws_huffman_get_encoded_length does */

/*
 * device_index[k] = the sum of the code lengths of symbols [0, min(k * block_symbols, length)) of device_input, for
 * k = 0 .. n_blocks with n_blocks = ceil(length / block_symbols): n_blocks + 1 uint64_t in device memory, 8-byte aligned.
 * device_index[0] = 0; device_index[n_blocks] is the stream's bits, so that (device_index[n_blocks] + 7) / 8 is
 * aws_huffman_get_encoded_length of the stream for a fresh encoder.  length 0: device_index[0] = 0 is written.
 *
 * device_input: the SYMBOLS of one stream in device memory, at any alignment.  block_symbols: a multiple of 64 in
 * [64, 1 << 24]; fewer than 2^32 blocks (256 GiB of symbols in blocks of 64).  device_status (NULL: not wanted; 4-byte aligned): one of the two values above, always written.
 *
 * The lengths are read from the engine's encode table in device memory, so any coder this library encodes works (codes of
 * up to 32 bits), and a fitted engine (huffman_amd_fit.h) indexes behind aws_huffman_amd_engine_fit_counts on the same
 * stream with no host wait: count, fit, index, encode.  Until a fit has been enqueued such an engine raises
 * AWS_ERROR_INVALID_STATE, as its launches do.
 *
 * Asynchronous on `stream` (NULL: the engine's): no host wait, nothing to clear between calls (length 0 alone is two memsets
 * of the stream); it can be captured in a graph and replayed.  The engine's FIRST call allocates the 128 KiB the scan keeps its tile sums in and so cannot be
 * inside a capture; no later call allocates.  That scratch is the engine's: calls of one engine that may run at the same
 * time (on two streams) must be ordered by the caller, as a fit and the launches that use it are.
 *
 * AWS_ERROR_INVALID_ARGUMENT: a NULL engine, a NULL or misaligned device_index, a misaligned device_status, a block_symbols
 * that is not one of the above, 2^32 blocks or more, NULL device_input with length > 0.  AWS_ERROR_UNSUPPORTED_OPERATION without a GPU (nothing
 * is read or written).
 */
AWS_COMPRESSION_API
int aws_huffman_amd_block_index(
    struct aws_huffman_amd_engine *engine,
    const void *device_input,
    uint64_t length,
    uint64_t block_symbols,
    uint64_t *device_index,
    uint32_t *device_status,
    void *stream);

/* blocks first_block .. first_block + block_count - 1 of an indexed stream, decoded to out_offset */
struct aws_huffman_amd_block_range {
    uint64_t first_block;
    uint64_t block_count;
    uint64_t out_offset; /* bytes from the decode launch's output base */
};

/*
 * Makes the plan, on the device, from ranges of whole blocks of ONE indexed stream.  device_index, length and block_symbols
 * are those of aws_huffman_amd_block_index (made by it, or received with the stream); the stream's encoded_length bytes lie
 * encoded_offset bytes behind the input base of the plan's launches.  device_ranges: range_count records in device memory,
 * 8-byte aligned.  With b0 = first_block and b1 = b0 + block_count, item r of the plan is
 *
 *   in_offset    = encoded_offset + index[b0] / 8        first_bit = index[b0] % 8
 *   in_len       = ceil(index[b1] / 8) - index[b0] / 8
 *   out_offset   = the range's own
 *   out_capacity = min(b1 * block_symbols, length) - b0 * block_symbols       (the symbols of the range's blocks)
 *
 * and a plain aws_huffman_amd_decode_plan_launch decodes the ranges; ranges may overlap, repeat and come in any order.
 * block_count 0 is an empty item: nothing read, nothing written, success.
 *
 * Per item the meaning stays "what aws_huffman_decode does for that item" (entered at first_bit, as every item with a
 * first_bit).  Its last byte holds up to 7 bits that are not the range's: the start of the next block's first code, or the
 * stream's padding.  The item has room for exactly the range's symbols, so aws_huffman_amd_decode_plan_results reports
 * success, or AWS_ERROR_SHORT_BUFFER when those bits spell a whole symbol that has nowhere to go.  Either way produced ==
 * out_capacity and the symbols written are the stream's: a reader of ranges takes both verdicts for "decoded".
 *
 * Everything else as aws_huffman_amd_decode_plan_reset_device_items: one wait for a handful of totals, and the same rule
 * about the plan's previous launch.  No item record is written anywhere: the planner reads the ranges and the two index
 * entries at each range's ends where it reads any other plan's item records.  The index and the ranges are read by this
 * call alone; launches of the plan do not need them.
 *
 * AWS_ERROR_INVALID_ARGUMENT, and a plan without items (a launch of it does nothing), as
 * aws_huffman_amd_decode_plan_reset_packed_input refuses offsets that decrease: a range past the last block
 * (first_block + block_count > n_blocks, also where the sum overflows); index[b1] < index[b0]; ceil(index[b1] / 8) >
 * encoded_length -- the check that keeps a received, damaged index from reading outside the buffer; an item of 4 GiB or
 * more; a NULL or misaligned device_index or device_ranges (with range_count > 0), a block_symbols that
 * aws_huffman_amd_block_index refuses.  A range reads the two entries at its ends and no other: an entry damaged strictly
 * inside a range goes unnoticed and does no harm.  AWS_ERROR_UNSUPPORTED_OPERATION without a GPU (nothing is read or
 * changed).
 */
AWS_COMPRESSION_API
int aws_huffman_amd_decode_plan_reset_block_ranges(
    struct aws_huffman_amd_decode_plan *plan,
    const uint64_t *device_index,
    uint64_t length,
    uint64_t block_symbols,
    uint64_t encoded_offset,
    uint64_t encoded_length,
    const struct aws_huffman_amd_block_range *device_ranges,
    size_t range_count,
    void *stream);

/* testing: the blocks one workgroup of the index's scan takes (any number >= 1: a small input then crosses many tile
 * boundaries; one that would need more than 8 192 tiles is ignored); 0: back to the built-in rule (1024, more for streams of
 * many millions of blocks) */
AWS_COMPRESSION_API
void aws_huffman_amd_testing_set_index_tile_blocks(uint32_t blocks);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_INDEX_H */
