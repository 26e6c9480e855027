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

/*
 * Packed batch decode: the mirror.  A receiver of a packed buffer and its offsets -- from a file, a socket, another GPU --
 * does not know how many symbols an item decodes to; the device finds out and lays the output out itself:
 *
 *   aws_huffman_amd_decode_plan_reset_packed_input(plan, d_in_offsets, NULL, item_count, stream);
 *   aws_huffman_amd_decode_plan_launch_packed(plan, d_input, NULL, 0, d_out_offsets, 1, stream);     (a size query, or
 *   aws_huffman_amd_decode_plan_packed_size(plan, &total, &longest, stream);                          guess a capacity)
 *   aws_huffman_amd_decode_plan_launch_packed(plan, d_input, d_output, total, d_out_offsets, 1, stream);
 *
 * Decodes the plan's items back to back into device_output.  With sym_i = the symbols aws_huffman_decode writes for item
 * i when it never runs out of room (the reference's aws_huffman_decoder_allow_growth: the walk from the item's first_bit
 * to the end of the stream, a code that runs past it, or a window without a code; symbols the padding bits spell count):
 *   offsets[0] = 0,  offsets[i + 1] = round_up(offsets[i] + sym_i, align)
 * always written in full, never clipped: device_offsets[item_count] is what output_capacity had to be.
 * An item whose symbols [offsets[i], offsets[i] + sym_i) all lie in front of output_capacity is aws_huffman_decode into a
 * byte_buf of capacity sym_i at device_output + offsets[i]: success with produced = sym_i, or
 * AWS_ERROR_COMPRESSION_UNKNOWN_SYMBOL.  Any other item gets capacity 0 -- there is no partial room: a caller who ran
 * short allocates device_offsets[item_count] and launches again --: AWS_ERROR_SHORT_BUFFER with produced 0 and
 * bits_consumed 0 where sym_i > 0, the reference's answer for capacity 0 where sym_i = 0.  Nothing at or behind
 * device_output + output_capacity and nothing in the gaps an alignment leaves is written.  The items' own out_offset /
 * out_capacity are neither read nor changed (a later aws_huffman_amd_decode_plan_launch behaves as before).
 * aws_huffman_amd_decode_plan_results after this launch reports against the capacity the launch gave each item.
 *
 * device_output NULL with output_capacity 0 is a size query: the offsets only.
 * Asynchronous on `stream`, no host wait; device_offsets, align, the plan's first packed launch (it allocates, so it
 * cannot be inside a graph capture; later ones can), the empty plan and AWS_ERROR_INVALID_ARGUMENT: as for
 * aws_huffman_amd_encode_plan_launch_packed.
 * The encoded bytes are walked once; only items short enough for a thread or a wave each (and those of a coder with codes
 * of more than 12 bits or of one length) are walked twice, once to count.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_decode_plan_launch_packed(
    struct aws_huffman_amd_decode_plan *plan,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint32_t align,
    void *stream);

/*
 * Waits for the plan's last packed launch (made on `stream`).  *total_symbols = device_offsets[item_count];
 * *longest_item_symbols = the largest reserved length (sym_i rounded up to the alignment) of one item.  Either pointer
 * may be NULL.  AWS_ERROR_INVALID_ARGUMENT: no packed launch since the plan was made or reset.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_decode_plan_packed_size(
    struct aws_huffman_amd_decode_plan *plan,
    uint64_t *total_symbols,
    uint64_t *longest_item_symbols,
    void *stream);

/*
 * Makes the plan, on the device, from a packed input layout: item i reads device_lengths[i] bytes at device_offsets[i],
 * from bit 0.  device_lengths NULL: device_offsets[i + 1] - device_offsets[i] bytes (device_offsets then holds
 * item_count + 1 numbers: what aws_huffman_amd_encode_plan_launch_packed wrote with align 1; with a larger alignment the
 * gap bytes were never written, so the sender ships the lengths, and device_offsets holds item_count numbers).
 * The items' own out_offset and out_capacity are 0: such a plan is meant for packed launches, and a plain launch of it
 * reports AWS_ERROR_SHORT_BUFFER for every item that holds a symbol.
 * Offsets that decrease, or an item of 4 GiB or more: AWS_ERROR_INVALID_ARGUMENT and a plan without items.  Everything
 * else as aws_huffman_amd_decode_plan_reset_device_items (uint64_t arrays in device memory, 8-byte aligned).
 */
AWS_COMPRESSION_API
int aws_huffman_amd_decode_plan_reset_packed_input(
    struct aws_huffman_amd_decode_plan *plan,
    const uint64_t *device_offsets,
    const uint64_t *device_lengths,
    size_t item_count,
    void *stream);

/* testing: the items one workgroup of the offset scan takes (any number >= 1: a small batch then crosses many tile
 * boundaries); 0: back to the built-in rule (1024, more for batches of many millions) */
AWS_COMPRESSION_API
void aws_huffman_amd_testing_set_pack_tile_items(uint32_t items);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_PACKED_H */
