#ifndef AWS_COMPRESSION_HUFFMAN_AMD_STORED_INDEX_H
#define AWS_COMPRESSION_HUFFMAN_AMD_STORED_INDEX_H
/*
 * Indexed packed batches with stored items: one launch for the sender; ranges and locate for the receiver.
 *
 * huffman_amd_stored.h stores an item raw when its code does not shrink it; huffman_amd_packed_index.h makes the batch's block
 * index in the length pass of a packed launch.  Each of the two leaves the other out, so a sender who wants both -- a columnar
 * page store whose incompressible pages must not grow, and random access into the others -- has to call
 * aws_huffman_amd_encode_plan_block_index and then aws_huffman_amd_encode_plan_launch_packed_stored, which read the symbols
 * three times.  The one call below does both with two reads, plus the copy of the stored items:
 *
 *   aws_huffman_amd_encode_plan_launch_packed_stored_indexed(plan, d_symbols, d_encoded, capacity, d_offsets, d_stored, 1,
 *                                                            16384, d_directory, d_index, entries, d_status, stream);
 *
 * A receiver of the packed buffer, its offsets, its flags, the directory and the index reads any blocks or symbols of any item,
 * stored or coded, with the calls of huffman_amd_batch_index.h given the flags as well:
 *
 *   aws_huffman_amd_decode_plan_reset_stored_item_block_ranges(plan, d_directory, d_index, entries, item_count, 16384, d_offsets,
 *                                                              NULL, d_stored, 0, total_bytes, d_ranges, range_count, stream);
 *   aws_huffman_amd_decode_plan_launch(plan, d_encoded, d_output, stream);
 *
 * Out of this interface: aws_huffman_amd_decode_plan_launch_packed of a plan of ranges that holds a stored range; an index made
 * by a PLAIN launch; aws_huffman_amd_decode_plan_from_encode behind a stored launch; aws_huffman_amd_shards_*; the host-pointer
 * calls.
 */

#include <aws/compression/huffman_amd_packed_index.h>
#include <aws/compression/huffman_amd_stored.h>

AWS_EXTERN_C_BEGIN

/*
 * Defined by composition.  On `stream` (NULL: the engine's), with no host wait and no copy back, the call leaves, bit for bit,
 *
 *   in device_directory, device_index and *device_status   what aws_huffman_amd_encode_plan_block_index leaves with the same
 *                                                          plan, device_input, block_symbols, capacity and status
 *   in device_offsets, device_stored, device_output, the   what aws_huffman_amd_encode_plan_launch_packed_stored leaves with
 *   plan's result records and its two sizes                the same plan, input, output, capacity, offsets, flags and align
 *
 * The index keeps its meaning: it counts the code bits of EVERY item, the stored ones too, as one running sum -- the entries of
 * a stored item say what its code would have been --, and a reader of a coded item still subtracts index[first_block].
 *
 * The symbols are read twice (the index's hot pass, which serves as the length pass, and the encode pass) and the stored items
 * once more by their copy.  The scan takes, with f_i = directory[i].first_block,
 *
 *   len_i = ceil((index[f_{i+1}] - index[f_i] + the item's carried overflow bits) / 8)
 *
 * as aws_huffman_amd_encode_plan_launch_packed_indexed does, and applies the rule of huffman_amd_stored.h unchanged: item i is
 * stored exactly when in_len_i > 0, it carries no overflow bits in, and len_i >= in_len_i -- a tie is stored.
 *
 * AN INDEX THAT DOES NOT FIT (total_blocks + 1 > index_capacity, or 2^32 blocks and more): as for
 * aws_huffman_amd_encode_plan_launch_packed_indexed.  The status says AWS_HUFFMAN_AMD_INDEX_TOO_SMALL, the directory is whole
 * and no word of device_index is written; every word of device_offsets is 0, every flag byte is 0, no byte of device_output is
 * written, every item's record is that of aws_huffman_encode into a byte_buf of capacity 0, and
 * aws_huffman_amd_encode_plan_packed_size and aws_huffman_amd_encode_plan_stored_size report zeros.
 *
 * A plan without items: offsets[0] = 0, directory[0] = {0, 0}, index[0] = 0, status OK, and no flag is written.
 *
 * Behind the call aws_huffman_amd_encode_plan_packed_size, _stored_size, _block_index_size, _results and _road work;
 * aws_huffman_amd_decode_plan_from_encode returns AWS_ERROR_INVALID_STATE, as behind any stored launch.  A later launch of any
 * other kind behaves as it always does.
 *
 * Scratch and captures: the union of the two calls' rules.  The plan's first call of this kind, and one after a reset to more
 * items than the plan ever held, allocate and cannot be inside a graph capture; later ones allocate nothing and can be
 * captured and replayed.  The engine's index scratch is the one aws_huffman_amd_block_index uses: calls of one engine that may
 * run at the same time must be ordered by the caller.
 *
 * AWS_ERROR_INVALID_ARGUMENT: a NULL device_stored, a NULL device_index or index_capacity 0, and every refusal of
 * aws_huffman_amd_encode_plan_launch_packed_indexed.  AWS_ERROR_INVALID_STATE for an engine that was never fitted.
 * AWS_ERROR_UNSUPPORTED_OPERATION without a GPU (nothing is read or written).
 */
AWS_COMPRESSION_API
int aws_huffman_amd_encode_plan_launch_packed_stored_indexed(
    struct aws_huffman_amd_encode_plan *plan,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint8_t *device_stored,
    uint32_t align,
    uint64_t block_symbols,
    struct aws_huffman_amd_item_blocks *device_directory,
    uint64_t *device_index,
    uint64_t index_capacity,
    uint32_t *device_status,
    void *stream);

/*
 * The receiver: the three calls of huffman_amd_batch_index.h that address by item, each with the sender's flags --
 * device_stored, item_count bytes in device memory -- behind device_encoded_lengths.  device_stored == NULL: exactly the call
 * without flags.  A range or position in an item whose flag is 0 behaves exactly as there.  In an item whose flag is 1, with
 * n = directory[item].symbols:
 *
 *   the item's packed length (device_encoded_lengths[item], or the difference of its offsets) must equal n; the directory checks
 *   stay (the item exists, its records do not decrease, stay inside index_entries, its blocks are ceil(n / block_symbols)); its
 *   bytes must lie inside encoded_length.  THE INDEX ENTRIES OF SUCH AN ITEM ARE NOT READ: they say what its code would have been.
 *
 *   block range [b0, b1)         lo = b0 * block_symbols, hi = min(b1 * block_symbols, n): the hi - lo bytes at
 *                                encoded_offset + offsets[item] + lo
 *   symbol range [s0, s0 + c)    the c bytes at encoded_offset + offsets[item] + s0
 *   locate s, s <= n             bit = 8 * (offsets[item] + s): a closed form, like the one for coders of one code length; no walk
 *                                is made and the encoded bytes are not read
 *
 * aws_huffman_amd_decode_plan_launch of such a plan decodes the coded ranges as ever and COPIES each stored range to
 * device_output + out_offset, in one launch behind its emit stage: the ranges may come in any order, overlapping or repeated,
 * stored among coded.  A stored range reports success, produced = its bytes, bits_consumed = 8 * its bytes; an empty range is an
 * empty item; nothing outside a range's bytes is written.  The plan keeps what its launches need of the flags and the ranges:
 * the caller may free them once the reset has run on the stream.  aws_huffman_amd_decode_plan_launch_packed of a plan that was
 * reset with flags by one of these two calls returns AWS_ERROR_INVALID_STATE.
 *
 * Refused -- AWS_ERROR_INVALID_ARGUMENT and a plan without items, or AWS_HUFFMAN_AMD_NO_BIT with
 * AWS_HUFFMAN_AMD_LOCATE_NOT_FOUND --: every row of the lists in huffman_amd_batch_index.h; a flag byte above 1 of an item that
 * a range or position names (only the flags of named items are read on the device); a stored item whose packed length is not
 * its symbol count; a range past the item's symbols (sums that overflow count as past).  Every received word is checked before
 * it is used as an address.  For a coder whose plans the host lays out (codes longer than 12 bits, or of one length -- a coder
 * of 256 eight-bit codes stores EVERY item) the flags are copied to the host with the rest and the same rules applied there.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_decode_plan_reset_stored_item_block_ranges(
    struct aws_huffman_amd_decode_plan *plan,
    const struct aws_huffman_amd_item_blocks *device_directory,
    const uint64_t *device_index,
    uint64_t index_entries,
    uint64_t item_count,
    uint64_t block_symbols,
    const uint64_t *device_encoded_offsets,
    const uint64_t *device_encoded_lengths,
    const uint8_t *device_stored,
    uint64_t encoded_offset,
    uint64_t encoded_length,
    const struct aws_huffman_amd_item_block_range *device_ranges,
    size_t range_count,
    void *stream);

AWS_COMPRESSION_API
int aws_huffman_amd_decode_plan_reset_stored_item_symbol_ranges(
    struct aws_huffman_amd_decode_plan *plan,
    const void *device_input,
    const struct aws_huffman_amd_item_blocks *device_directory,
    const uint64_t *device_index,
    uint64_t index_entries,
    uint64_t item_count,
    uint64_t block_symbols,
    const uint64_t *device_encoded_offsets,
    const uint64_t *device_encoded_lengths,
    const uint8_t *device_stored,
    uint64_t encoded_offset,
    uint64_t encoded_length,
    const struct aws_huffman_amd_item_symbol_range *device_ranges,
    size_t range_count,
    void *stream);

AWS_COMPRESSION_API
int aws_huffman_amd_locate_stored_item_symbols(
    struct aws_huffman_amd_engine *engine,
    const void *device_encoded,
    uint64_t encoded_length,
    const struct aws_huffman_amd_item_blocks *device_directory,
    const uint64_t *device_index,
    uint64_t index_entries,
    uint64_t item_count,
    uint64_t block_symbols,
    const uint64_t *device_encoded_offsets,
    const uint64_t *device_encoded_lengths,
    const uint8_t *device_stored,
    const uint64_t *device_items,
    const uint64_t *device_symbols,
    size_t count,
    uint64_t *device_bits,
    uint32_t *device_status,
    void *stream);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_STORED_INDEX_H */
