#ifndef AWS_COMPRESSION_HUFFMAN_AMD_PACKED_H
#define AWS_COMPRESSION_HUFFMAN_AMD_PACKED_H
/*
 * Packed batch encode: a plan's items back to back in one output buffer, the offsets made on the device.
 *
 *   uint64_t *d_offsets = aws_huffman_amd_device_alloc(engine, (item_count + 1) * sizeof(uint64_t));
 *   aws_huffman_amd_encode_plan_launch_packed(plan, d_input, d_output, output_capacity, d_offsets, 1, stream);
 *   aws_huffman_amd_encode_plan_packed_size(plan, &total, &longest, stream);     (waits; optional)
 *   aws_huffman_amd_decode_plan_from_encode(decode_plan, plan, stream);          (reads at d_offsets' places)
 *
 * A plain launch writes item i at the out_offset its caller chose, into out_capacity bytes its caller had to guess.  A
 * packed launch runs a length pass, makes the offsets from its lengths, and encodes behind them, all on one stream:
 * no host wait and no copy to the host in between.
 */

#include <aws/compression/huffman_amd.h>

AWS_EXTERN_C_BEGIN

/*
 * Encodes the plan's items back to back into device_output.  Item i's bytes start at device_offsets[i];
 * device_offsets[item_count] is the total.  The items' own out_offset / out_capacity are not used (and are what a later
 * aws_huffman_amd_encode_plan_launch of the same plan uses, as before: the plan keeps its own layout).
 *
 * Item by item, with len_i = aws_huffman_get_encoded_length of item i with its carried overflow bits (what a length_only
 * launch reports; a symbol without a code counts 0 bits):
 *   offsets[0] = 0,  offsets[i + 1] = round_up(offsets[i] + len_i, align)
 *   item i is aws_huffman_encode into a byte_buf of capacity min(offsets[i + 1] - offsets[i], output_capacity - offsets[i])
 *   (0 where that is negative) at device_output + offsets[i].
 * The offsets are always written in full, never clipped: device_offsets[item_count] is what output_capacity had to be.
 * When that fits, every item of a coder that codes every symbol succeeds and produces len_i bytes; an item that stops at
 * a symbol without a code reports AWS_ERROR_COMPRESSION_UNKNOWN_SYMBOL and produced fewer.  When output_capacity is
 * smaller, the items in front of the edge are unchanged, the item across it gets AWS_ERROR_SHORT_BUFFER (with the
 * reference's consumed / produced / overflow for that capacity), the items behind it capacity 0, and nothing at or behind
 * device_output + output_capacity is written.  Bytes in the gaps an alignment leaves are not written.
 * aws_huffman_amd_encode_plan_results / _road report the encode pass as for a plain launch.
 *
 * Asynchronous on `stream` (NULL: the engine's).  device_offsets: item_count + 1 uint64_t in device memory, 8-byte
 * aligned.  align: a power of two, 1 .. 4096.  A plan without items: success, device_offsets[0] = 0 is written.
 *
 * The plan keeps a second array of item records for these launches.  It is allocated by the plan's FIRST packed launch
 * (and again by the first one after a reset to more items than the plan ever held): that launch cannot be inside a graph
 * capture.  Later ones allocate nothing and can be captured and replayed.
 *
 * AWS_ERROR_INVALID_ARGUMENT: NULL device_offsets, an alignment that is not one of the above, NULL device_output with
 * output_capacity > 0.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_encode_plan_launch_packed(
    struct aws_huffman_amd_encode_plan *plan,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint32_t align,
    void *stream);

/*
 * Waits for the plan's last packed launch (made on `stream`).  *total_bytes = device_offsets[item_count], which is also
 * what output_capacity would have had to be; *longest_item_bytes = the largest reserved length (len_i rounded up to the
 * alignment) of one item.  Either pointer may be NULL.
 * AWS_ERROR_INVALID_ARGUMENT: no packed launch since the plan was made or reset.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_encode_plan_packed_size(
    struct aws_huffman_amd_encode_plan *plan,
    uint64_t *total_bytes,
    uint64_t *longest_item_bytes,
    void *stream);

/* testing: the items one workgroup of the offset scan takes (any number >= 1: a small batch then crosses many tile
 * boundaries); 0: back to the built-in rule (1024, more for batches of many millions) */
AWS_COMPRESSION_API
void aws_huffman_amd_testing_set_pack_tile_items(uint32_t items);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_PACKED_H */
