#ifndef AWS_COMPRESSION_HUFFMAN_AMD_PACKED_INDEX_H
#define AWS_COMPRESSION_HUFFMAN_AMD_PACKED_INDEX_H
/*
 * A packed encode launch that makes the batch's block index in its length pass.
 *
 * A sender who wants the packed buffer of huffman_amd_packed.h and the one index over it of huffman_amd_batch_index.h can
 * make the two calls of that header's example: the index call reads every symbol once, the packed launch twice more (a
 * length pass, then the encode pass).  The scanned index already holds what the length pass finds out -- with
 * f_i = directory[i].first_block, item i has index[f_{i+1}] - index[f_i] code bits -- so ONE call does both with two reads:
 *
 *   aws_huffman_amd_encode_plan_launch_packed_indexed(plan, d_symbols, d_encoded, capacity, d_offsets, 1,
 *                                                     16384, d_directory, d_index, entries, d_status, stream);
 *
 * `entries` is an upper bound of the blocks plus one (sum of ceil(in_len / block_symbols) + 1), or what a size query through
 * aws_huffman_amd_encode_plan_block_index and aws_huffman_amd_encode_plan_block_index_size has said.
 *
 * The same call for a batch that stores an item raw when its code does not shrink it: huffman_amd_stored_index.h.
 *
 * Out of this interface: an index made by a PLAIN launch (aws_huffman_amd_encode_plan_launch), and aws_huffman_amd_shards_*.
 */

#include <aws/compression/huffman_amd_batch_index.h>
#include <aws/compression/huffman_amd_packed.h>

AWS_EXTERN_C_BEGIN

/*
 * On `stream` (NULL: the engine's), with no host wait and no copy back, the call leaves
 *
 *   in device_directory, device_index and *device_status   exactly what aws_huffman_amd_encode_plan_block_index leaves with
 *                                                          the same plan, device_input, block_symbols, capacity and status
 *   in device_offsets, device_output and the plan's        exactly what aws_huffman_amd_encode_plan_launch_packed leaves with
 *   result records                                         the same plan, input, output, capacity, offsets and align
 *
 * and reads the symbols twice: the index's hot pass, and the encode pass.  The offsets come from the scanned index,
 *
 *   len_i = ceil((index[f_{i+1}] - index[f_i] + the item's carried overflow bits) / 8),    reserved_i = round_up(len_i, align)
 *
 * so the carried bits count towards an item's length and not towards the index, whose meaning is unchanged; a symbol without
 * a code counts 0 bits in both.
 *
 * AN INDEX THAT DOES NOT FIT (total_blocks + 1 > index_capacity, or 2^32 blocks and more): the status says
 * AWS_HUFFMAN_AMD_INDEX_TOO_SMALL, the directory is whole and no word of device_index is written, as for the index call.
 * The device then has no lengths: every word of device_offsets is 0, every item's record is that of aws_huffman_encode into
 * a byte_buf of capacity 0, no byte of device_output is written, and aws_huffman_amd_encode_plan_packed_size reports 0 and
 * 0.  ONLY THE STATUS WORD tells this apart from a batch of empty items: a caller who sizes the index by a bound that may
 * be too small passes device_status and looks at it (aws_huffman_amd_encode_plan_block_index_size says what was needed).
 *
 * Behind the call the plan is as behind both calls: aws_huffman_amd_encode_plan_packed_size,
 * aws_huffman_amd_encode_plan_block_index_size, aws_huffman_amd_encode_plan_results, aws_huffman_amd_encode_plan_road and
 * aws_huffman_amd_decode_plan_from_encode work, and the plan's own layout survives for its next plain launch.  A plan
 * without items: offsets[0] = 0, directory[0] = {0, 0}, index[0] = 0, status OK.
 *
 * Scratch and captures: the union of the two calls' rules.  The plan's first call of this kind, and one after a reset to
 * more items than the plan ever held, allocate and cannot be inside a graph capture; later ones allocate nothing and can be
 * captured and replayed.  The engine's 128 KiB of index scratch is the one aws_huffman_amd_block_index uses: calls of one
 * engine that may run at the same time must be ordered by the caller.
 *
 * AWS_ERROR_INVALID_ARGUMENT: a NULL device_index or index_capacity 0 (a size query goes through
 * aws_huffman_amd_encode_plan_block_index, which then runs the directory only), and every refusal of the two calls -- a NULL
 * plan, an align that is no power of two in 1 .. 4096, a NULL or misaligned device_offsets or device_directory, a
 * misaligned device_index or device_status, a block_symbols that is no multiple of 64 in [64, 1 << 24], NULL device_input
 * for a plan with items, NULL device_output with a capacity.  AWS_ERROR_INVALID_STATE for an engine that was never fitted.
 * AWS_ERROR_UNSUPPORTED_OPERATION without a GPU (nothing is read or written).
 */
AWS_COMPRESSION_API
int aws_huffman_amd_encode_plan_launch_packed_indexed(
    struct aws_huffman_amd_encode_plan *plan,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint32_t align,
    uint64_t block_symbols,
    struct aws_huffman_amd_item_blocks *device_directory,
    uint64_t *device_index,
    uint64_t index_capacity,
    uint32_t *device_status,
    void *stream);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_PACKED_INDEX_H */
