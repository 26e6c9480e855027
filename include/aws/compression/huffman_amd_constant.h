#ifndef AWS_COMPRESSION_HUFFMAN_AMD_CONSTANT_H
#define AWS_COMPRESSION_HUFFMAN_AMD_CONSTANT_H
/*
 * Packed batches that keep an item of one repeated byte as its length and that byte (huffman_amd_stored.h covers the item
 * that does not shrink; nothing there covers the item that hardly carries information: a coder of the fast roads has codes of
 * 4 bits at least, so a plane of zeros -- the high bytes of small integers, padding, masks -- still packs to half its size).
 * A third kind of item beside the coded and the stored one, decided where the stored decision is made: on the device, in the
 * scan a packed launch runs between its length pass and its encode pass, one byte an item; nothing comes to the host.
 *
 *   sender     aws_huffman_amd_encode_plan_launch_packed_constant(plan, d_in, d_out, capacity, d_offsets, d_kinds, align, stream);
 *   receiver   aws_huffman_amd_decode_plan_reset_packed_constant_input(dplan, d_out, d_offsets, NULL, d_kinds, n, stream);
 *              aws_huffman_amd_decode_plan_launch_packed(dplan, d_out, d_back, back_capacity, d_back_offsets, 1, stream);
 *
 * Known cost: the sender reads every item once more (the detection leaves an item at its first group of 16 bytes that
 * differs), and the encode pass still reads and codes the symbols of a constant item and throws the result away.
 *
 * Out of this interface: the indexed launch and the range calls of huffman_amd_stored_index.h (a kind of 2 is refused there
 * as any flag above 1 is), aws_huffman_amd_shards_*, the host-pointer calls.
 */

#include <aws/compression/huffman_amd_stored.h>

/* what device_kinds[i] says of item i */
#define AWS_HUFFMAN_AMD_ITEM_CODED 0
#define AWS_HUFFMAN_AMD_ITEM_STORED 1
#define AWS_HUFFMAN_AMD_ITEM_CONSTANT 2
/* the bytes of a constant item in the packed buffer: its symbols as 8 bytes, little-endian, then the byte they all are */
#define AWS_HUFFMAN_AMD_CONSTANT_BYTES 9
/* the most symbols a receiver takes from a constant item's head: 2^32.  A plan holds fewer than 2^32 items and rounds a
 * length up to 4096 at most, so no sum of the offset scan's (symbols, or the copy's tiles of 16 KiB) over constant items leaves
 * 64 bits */
#define AWS_HUFFMAN_AMD_CONSTANT_MAX_COUNT 0x100000000ull

AWS_EXTERN_C_BEGIN

/*
 * aws_huffman_amd_encode_plan_launch_packed_stored with one rule in front of the stored rule.  With n = in_len_i and len_i
 * the length pass's encoded length (huffman_amd_stored.h), item i is CONSTANT exactly when it carries no overflow bits in,
 * n > 9, len_i > 9 and every byte of the item equals its first -- so a constant item is strictly shorter than both other
 * forms.  Otherwise the stored rule applies unchanged; otherwise the item is coded.  (A symbol without a code counts 0 bits
 * towards len_i, as there.)
 *
 *   constant    device_kinds[i] = 2, the item's length is 9, and the bytes at device_output + offsets[i] are n as 8 bytes,
 *               little-endian, then the value -- written at any alignment
 *   stored      device_kinds[i] = 1, as device_stored[i] = 1 there
 *   coded       device_kinds[i] = 0
 *   offsets[i + 1] = round_up(offsets[i] + (9, in_len_i or len_i), align), written in full, never clipped
 *
 * A constant item whose 9 bytes all lie in front of output_capacity reports success, consumed = n, produced = 9, no overflow
 * bits; one whose 9 bytes do not all fit writes nothing and reports AWS_ERROR_SHORT_BUFFER with consumed = produced = 0.
 * Nothing at or behind device_output + output_capacity is written, and nothing in alignment gaps.
 *
 * Behind such a launch aws_huffman_amd_encode_plan_packed_size works, aws_huffman_amd_encode_plan_stored_size reports the
 * items of kind 1, aws_huffman_amd_encode_plan_constant_size those of kind 2, and aws_huffman_amd_decode_plan_from_encode
 * returns AWS_ERROR_INVALID_STATE.
 *
 * No host wait.  The plan's first such launch may allocate; later ones can be captured in a graph and replayed: the words
 * the detection marks items in are cleared by the launch behind itself, not in front.  A plan without items: offsets[0] = 0
 * and nothing else.  device_kinds: item_count bytes in device memory; NULL is AWS_ERROR_INVALID_ARGUMENT; the other argument
 * checks are those of a packed launch.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_encode_plan_launch_packed_constant(
    struct aws_huffman_amd_encode_plan *plan,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint8_t *device_kinds,
    uint32_t align,
    void *stream);

/*
 * aws_huffman_amd_encode_plan_stored_size for the constant items: how many the plan's last launch -- a constant one:
 * AWS_ERROR_INVALID_ARGUMENT otherwise -- found, and how many input bytes they hold (whatever the capacity let through).
 * Waits for `stream`; either pointer may be NULL.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_encode_plan_constant_size(
    struct aws_huffman_amd_encode_plan *plan,
    uint64_t *constant_items,
    uint64_t *constant_bytes,
    void *stream);

/*
 * aws_huffman_amd_decode_plan_reset_packed_stored_input for all three kinds.  It takes the packed buffer too: the heads of
 * the constant items are read at the reset, so that the plan's records and tiles are all made there, and the launches must
 * be given the same bytes.  device_kinds == NULL: exactly aws_huffman_amd_decode_plan_reset_packed_input.
 *
 * Refused with AWS_ERROR_INVALID_ARGUMENT and a plan without items, as decreasing offsets are: a kind above 2; an offset of
 * 2^63 or more; a constant item whose packed length is not 9; a head that counts 9 symbols or fewer (the sender never makes
 * one) or more than AWS_HUFFMAN_AMD_CONSTANT_MAX_COUNT.  Every received word is checked before it is used as a length or an
 * address; a head is read only where the kind and the packed length say there is one.
 *
 * aws_huffman_amd_decode_plan_launch_packed of such a plan treats a constant item as sym_i = its count: one that fits whole
 * is filled at device_output + offsets[i] and reports success, produced = sym_i, bits_consumed = 72; one that does not fit
 * gets the "no partial room" answer.  Stored and coded items, the size query and the refusal of a plain launch are those of
 * huffman_amd_stored.h.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_decode_plan_reset_packed_constant_input(
    struct aws_huffman_amd_decode_plan *plan,
    const void *device_packed,
    const uint64_t *device_offsets,
    const uint64_t *device_lengths,
    const uint8_t *device_kinds,
    size_t item_count,
    void *stream);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_CONSTANT_H */
