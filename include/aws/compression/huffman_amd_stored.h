#ifndef AWS_COMPRESSION_HUFFMAN_AMD_STORED_H
#define AWS_COMPRESSION_HUFFMAN_AMD_STORED_H
/*
 * Packed batches that store an item raw when its code does not shrink it (huffman_amd_packed.h decides nothing: every item
 * of a packed launch is coded, whatever that costs -- uniform bytes grow by a fifth under the reference's test coder, an
 * item that does not look like its batch by up to a half under a fitted one).  HPACK, the reference's one real consumer,
 * compares aws_huffman_get_encoded_length with the raw length per string and sets the H bit only when the code is strictly
 * shorter; deflate has stored blocks.  Here the decision is made on the device, in the scan a packed launch already runs
 * between its length pass and its encode pass, one flag byte an item; nothing comes to the host.
 *
 *   sender     aws_huffman_amd_encode_plan_launch_packed_stored(plan, d_in, d_out, capacity, d_offsets, d_stored, align, stream);
 *   receiver   aws_huffman_amd_decode_plan_reset_packed_stored_input(dplan, d_offsets, NULL, d_stored, n, stream);
 *              aws_huffman_amd_decode_plan_launch_packed(dplan, d_out, d_back, back_capacity, d_back_offsets, 1, stream);
 *
 * Known cost: the encode pass still reads and codes the symbols of a stored item and throws the result away.
 *
 * With the batch's block index and ranges into stored and coded items alike: huffman_amd_stored_index.h.
 *
 * Out of this interface: aws_huffman_amd_shards_*, the host-pointer calls, coders with symbols without a code made total.
 */

#include <aws/compression/huffman_amd_packed.h>

AWS_EXTERN_C_BEGIN

/*
 * aws_huffman_amd_encode_plan_launch_packed with one rule added.  Let len_i be the encoded length the length pass reports
 * (carried bits + every code bit, rounded up to bytes; a symbol without a code counts 0 bits and is not flagged).  Item i is
 * STORED exactly when in_len_i > 0, it carries no overflow bits in, and len_i >= in_len_i -- a tie is stored.
 *
 *   stored      device_stored[i] = 1, the item's length is in_len_i, and the bytes at device_output + offsets[i] are its
 *               input bytes, unchanged
 *   otherwise   device_stored[i] = 0 and everything is as in a packed launch
 *   offsets[i + 1] = round_up(offsets[i] + (stored ? in_len_i : len_i), align), written in full, never clipped
 *
 * The capacity applies to a stored item as to any: one that fits whole reports success, consumed = produced = in_len_i; one
 * across the edge is copied up to the edge and reports AWS_ERROR_SHORT_BUFFER with consumed = produced = the bytes that
 * fitted; one behind the edge gets nothing; none reports overflow bits.  Nothing at or behind device_output + output_capacity
 * is written, and nothing in alignment gaps.  aws_huffman_amd_encode_plan_packed_size works behind such a launch.
 *
 * No host wait.  The plan's first such launch may allocate, as a first packed launch does; later ones can be captured in a
 * graph and replayed.  A plan without items: offsets[0] = 0 and nothing else.  device_stored: item_count bytes in device
 * memory; NULL is AWS_ERROR_INVALID_ARGUMENT; the other argument checks are those of a packed launch.
 *
 * aws_huffman_amd_decode_plan_from_encode of a plan whose last launch was this one returns AWS_ERROR_INVALID_STATE (it would
 * decode raw bytes as codes): the way back on one device is aws_huffman_amd_decode_plan_reset_packed_stored_input below,
 * given the three device arrays as they lie.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_encode_plan_launch_packed_stored(
    struct aws_huffman_amd_encode_plan *plan,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint8_t *device_stored,
    uint32_t align,
    void *stream);

/*
 * How many items the plan's last launch -- a stored one: AWS_ERROR_INVALID_ARGUMENT otherwise -- stored, and how many input
 * bytes they hold (whatever the capacity let through).  Waits for `stream`, like aws_huffman_amd_encode_plan_packed_size;
 * either pointer may be NULL.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_encode_plan_stored_size(
    struct aws_huffman_amd_encode_plan *plan,
    uint64_t *stored_items,
    uint64_t *stored_bytes,
    void *stream);

/*
 * aws_huffman_amd_decode_plan_reset_packed_input plus the sender's flags.  device_stored == NULL: exactly that call.  A flag
 * byte other than 0 or 1 is refused as decreasing offsets are: AWS_ERROR_INVALID_ARGUMENT and a plan without items; every
 * received word is checked before it is used as an address or a length.  The plan keeps what its launches need of the three
 * arrays: the caller may free them once the reset has run on the stream.
 *
 * aws_huffman_amd_decode_plan_launch_packed of such a plan treats a stored item as sym_i = its packed length: the offsets
 * follow from that; a stored item whose bytes all lie in front of output_capacity is copied to device_output + offsets[i]
 * and reports success, produced = sym_i, bits_consumed = 8 * sym_i; one that does not fit gets the "no partial room" answer
 * a coded item gets.  A NULL output stays a size query.  aws_huffman_amd_decode_plan_launch of a plan that was reset with
 * flags returns AWS_ERROR_INVALID_STATE.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_decode_plan_reset_packed_stored_input(
    struct aws_huffman_amd_decode_plan *plan,
    const uint64_t *device_offsets,
    const uint64_t *device_lengths,
    const uint8_t *device_stored,
    size_t item_count,
    void *stream);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_STORED_H */
