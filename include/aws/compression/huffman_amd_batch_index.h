#ifndef AWS_COMPRESSION_HUFFMAN_AMD_BATCH_INDEX_H
#define AWS_COMPRESSION_HUFFMAN_AMD_BATCH_INDEX_H
/*
 * One block index over the items of a batch, made on the device.
 *
 * huffman_amd_packed.h encodes the items of a plan back to back with no length ever visiting the host; huffman_amd_index.h
 * indexes ONE stream.  A sender of 65 536 documents in one packed buffer wants both: one index over all of them, from one
 * call, for a plan whose items may be known on the device only.
 *
 *   struct aws_huffman_amd_item_blocks *d_directory = aws_huffman_amd_device_alloc(engine, (item_count + 1) * 16);
 *   aws_huffman_amd_encode_plan_block_index(plan, d_symbols, 16384, d_directory, NULL, 0, NULL, stream);     (a size query)
 *   aws_huffman_amd_encode_plan_block_index_size(plan, &entries, stream);                                    (waits)
 *   uint64_t *d_index = aws_huffman_amd_device_alloc(engine, entries * sizeof(uint64_t));
 *   aws_huffman_amd_encode_plan_block_index(plan, d_symbols, 16384, d_directory, d_index, entries, d_status, stream);
 *   aws_huffman_amd_encode_plan_launch_packed(plan, d_symbols, d_encoded, capacity, d_offsets, 1, stream);
 *
 * A caller who knows an upper bound of the blocks (sum of ceil(in_len / block_symbols) + 1) goes without the query and the
 * wait.  With first = directory[i].first_block, block k of item i starts at bit index[first + k] - index[first] of the item's
 * own encoded bytes, and ceil((index[directory[i + 1].first_block] - index[first]) / 8) is the item's encoded length.
 *
 * A receiver of the packed buffer, its offsets, the directory and the index reads whole blocks of any items with
 *
 *   struct aws_huffman_amd_item_block_range r = {40000, 3, 2, 0};         (item 40 000, its blocks 3 and 4; device memory)
 *   aws_huffman_amd_decode_plan_reset_item_block_ranges(plan, d_directory, d_index, entries, item_count, 16384, d_offsets, NULL,
 *                                                       0, total_bytes, d_ranges, 1, stream);
 *   aws_huffman_amd_decode_plan_launch(plan, d_encoded, d_output, stream);
 *
 * and any symbols of any items with aws_huffman_amd_decode_plan_reset_item_symbol_ranges, as huffman_amd_ranges.h does for
 * one stream; aws_huffman_amd_locate_item_symbols says where a symbol of an item starts.
 *
 * Out of this interface: an index made by a PLAIN encode launch (a packed launch makes it in place of its length pass:
 * aws_huffman_amd_encode_plan_launch_packed_indexed, huffman_amd_packed_index.h, one call for the last two lines above with
 * one read of the symbols fewer), and aws_huffman_amd_shards_*.
 */

#include <aws/compression/huffman_amd_ranges.h>

AWS_EXTERN_C_BEGIN

/* a third value of the status word, beside AWS_HUFFMAN_AMD_INDEX_OK and AWS_HUFFMAN_AMD_INDEX_SYMBOL_WITHOUT_CODE */
#define AWS_HUFFMAN_AMD_INDEX_TOO_SMALL 2u /* the batch has more blocks than index_capacity - 1: no entry was written */

/* directory record i of a batch: the blocks in front of item i, and the item's symbols */
struct aws_huffman_amd_item_blocks {
    uint64_t first_block;
    uint64_t symbols;
};

/*
 * The items are the plan's CURRENT items (their in_offset and in_len, behind device_input as in a launch), however the
 * plan was filled: aws_huffman_amd_encode_plan_new / _reset from host records (the plans of thousands of header-sized items
 * included), _reset_strided, _reset_device_items.  With B = block_symbols and nb_i = ceil(in_len_i / B):
 *
 *   device_directory[i]          = { the sum of nb_j for j < i, in_len_i }       i = 0 .. item_count - 1
 *   device_directory[item_count] = { total_blocks, 0 }
 *   device_index[k]              = the sum of the code lengths of all symbols in the blocks in front of global block k, in
 *                                  item order, k = 0 .. total_blocks: ONE running sum over the batch, device_index[0] = 0
 *
 * An empty item has no blocks.  There is no extra entry per item: a reader subtracts index[first_block of the item].
 * Only the symbols' code bits are counted: an item's carried overflow bits and its eos_padding are not looked at, so the
 * entries describe encoded bytes that start with the first symbol's code at bit 0 -- what a launch writes for an item without
 * carried bits.
 *
 * device_directory: item_count + 1 records in device memory, 8-byte aligned, always written in full.  device_index:
 * index_capacity words, 8-byte aligned.  *device_status (NULL: not wanted; 4-byte aligned) is always written, an OR of
 * AWS_HUFFMAN_AMD_INDEX_OK, AWS_HUFFMAN_AMD_INDEX_SYMBOL_WITHOUT_CODE (such a symbol counts 0 bits) and
 * AWS_HUFFMAN_AMD_INDEX_TOO_SMALL: total_blocks + 1 > index_capacity, or 2^32 blocks and more.  Then the directory is whole, no
 * word of device_index is written, and device_directory[item_count].first_block + 1 is what the capacity had to be.
 * device_index NULL with index_capacity 0 is a size query: the directory, and the status says TOO_SMALL.
 *
 * block_symbols: as for aws_huffman_amd_block_index, a multiple of 64 in [64, 1 << 24].  A fitted engine indexes behind its
 * fit on one stream (AWS_ERROR_INVALID_STATE before any fit has been enqueued).
 *
 * Asynchronous on `stream` (NULL: the engine's), with no host wait: the host does not know the blocks of a plan made on the
 * device, so every launch is sized from index_capacity and the item count and the kernels read the real counts from the
 * directory.  Nothing of the plan is changed and the call is not a launch: results, road and the packed state stay as they
 * were.  The scratch is the plan's (and the 128 KiB of the engine that aws_huffman_amd_block_index uses: calls of one engine
 * that may run at the same time must be ordered by the caller).  It is allocated by the plan's first call, and again after
 * a reset to more items than the plan ever held: such a call cannot be inside a graph capture.  Later calls allocate
 * nothing and can be captured and replayed.
 *
 * AWS_ERROR_INVALID_ARGUMENT: a NULL plan, a NULL or misaligned device_directory, a misaligned device_index or
 * device_status, a NULL device_index with a capacity (or one without), a block_symbols that is not one of the above, NULL
 * device_input for a plan with items.  AWS_ERROR_UNSUPPORTED_OPERATION without a GPU (nothing is read or written).
 */
AWS_COMPRESSION_API
int aws_huffman_amd_encode_plan_block_index(
    struct aws_huffman_amd_encode_plan *plan,
    const void *device_input,
    uint64_t block_symbols,
    struct aws_huffman_amd_item_blocks *device_directory,
    uint64_t *device_index,
    uint64_t index_capacity,
    uint32_t *device_status,
    void *stream);

/* *entries = total_blocks + 1 of the plan's last aws_huffman_amd_encode_plan_block_index on `stream`: what its index needs.
 * Copies one word back and WAITS for the stream, as aws_huffman_amd_encode_plan_packed_size does.
 * AWS_ERROR_INVALID_ARGUMENT where no such call was made since the plan was filled. */
AWS_COMPRESSION_API
int aws_huffman_amd_encode_plan_block_index_size(struct aws_huffman_amd_encode_plan *plan, uint64_t *entries, void *stream);

/* blocks first_block .. first_block + block_count - 1 OF ITEM `item` of an indexed batch, decoded to out_offset */
struct aws_huffman_amd_item_block_range {
    uint64_t item;
    uint64_t first_block; /* counted from the item's first block */
    uint64_t block_count;
    uint64_t out_offset;  /* bytes from the decode launch's output base */
};

/*
 * Makes the plan, on the device, from ranges of whole blocks of the items of ONE indexed batch: what
 * aws_huffman_amd_decode_plan_reset_block_ranges is for one stream.  device_directory (item_count + 1 records),
 * device_index (index_entries words) and block_symbols are those of aws_huffman_amd_encode_plan_block_index, made by it or
 * received with the buffer.  The packed buffer's encoded_length bytes lie encoded_offset bytes behind the input base of the
 * plan's launches, and where an item's bytes lie in it is said as for aws_huffman_amd_decode_plan_reset_packed_input: item
 * j's start device_encoded_offsets[j] bytes into the buffer and are device_encoded_lengths[j] long (NULL:
 * device_encoded_offsets[j + 1] - device_encoded_offsets[j], item_count + 1 offsets) -- what a packed encode launch wrote.
 * The items must have been encoded without carried bits: an item's bytes start with its first symbol's code at bit 0.
 * With fb = directory[item].first_block, b0 = first_block, b1 = b0 + block_count, item r of the plan is
 *
 *   from = index[fb + b0] - index[fb]         to = index[fb + b1] - index[fb]
 *   in_offset    = encoded_offset + offsets[item] + from / 8        first_bit = from % 8
 *   in_len       = ceil(to / 8) - from / 8
 *   out_capacity = min(b1 * block_symbols, directory[item].symbols) - b0 * block_symbols
 *
 * and a plain aws_huffman_amd_decode_plan_launch decodes the ranges, in any order, overlapping or repeated; block_count 0 is
 * an empty item.  The verdicts are those of the single stream's ranges: success, or AWS_ERROR_SHORT_BUFFER where the spare
 * bits of the range's last byte spell a whole symbol; either way produced == out_capacity.  Everything else -- the one wait
 * for the totals, the rule about the plan's previous launch -- as aws_huffman_amd_decode_plan_reset_device_items.
 *
 * AWS_ERROR_INVALID_ARGUMENT, and a plan without items, for what keeps a received, damaged directory or index inside the
 * buffers: item >= item_count; directory[item + 1].first_block below directory[item].first_block, or not below
 * index_entries; an item whose blocks are not ceil(symbols / block_symbols); a range past the item's blocks (sums that
 * overflow count as past); index entries that decrease from the item's first to the range's first to its end; ceil(to / 8)
 * beyond the item's encoded length; the item's bytes beyond encoded_length; an item of 4 GiB or more; and for NULL or
 * misaligned arrays, index_entries 0 or a block_symbols that aws_huffman_amd_block_index refuses.  A range reads its item's
 * two directory records, its item's offset (and the next, or its length) and the index entries at the item's first block and
 * at its own two ends, and no others -- on the device.  For a coder whose plans the host lays out (codes longer than 12
 * bits, or of one length) the call copies the directory, the index, the offsets and the lengths WHOLE to the host, 8 bytes
 * a block and 24 or 32 an item for every reset: keep such a coder's batches or indexes coarse.
 * AWS_ERROR_UNSUPPORTED_OPERATION without a GPU (nothing is read or changed).
 */
AWS_COMPRESSION_API
int aws_huffman_amd_decode_plan_reset_item_block_ranges(
    struct aws_huffman_amd_decode_plan *plan,
    const struct aws_huffman_amd_item_blocks *device_directory,
    const uint64_t *device_index,
    uint64_t index_entries,
    uint64_t item_count,
    uint64_t block_symbols,
    const uint64_t *device_encoded_offsets,
    const uint64_t *device_encoded_lengths,
    uint64_t encoded_offset,
    uint64_t encoded_length,
    const struct aws_huffman_amd_item_block_range *device_ranges,
    size_t range_count,
    void *stream);

/* symbols first_symbol .. first_symbol + symbol_count - 1 OF ITEM `item` of an indexed batch, decoded to out_offset */
struct aws_huffman_amd_item_symbol_range {
    uint64_t item;
    uint64_t first_symbol; /* counted from the item's first symbol */
    uint64_t symbol_count;
    uint64_t out_offset;   /* bytes from the decode launch's output base */
};

/*
 * device_bits[i] = the bit at which symbol device_symbols[i] of item device_items[i] starts, counted from the first byte
 * of the packed buffer at device_encoded: 8 * offsets[item] plus the bit inside the item.  What
 * aws_huffman_amd_locate_symbols is for one stream (the walk, its two roads, the closed form for coders of one code length
 * and AWS_HUFFMAN_AMD_NO_BIT with AWS_HUFFMAN_AMD_LOCATE_NOT_FOUND are the same); the batch is described as for
 * aws_huffman_amd_decode_plan_reset_item_block_ranges, encoded_length being the packed buffer's size.  s equal to the
 * item's symbols is the item's end.  device_items, device_symbols and device_bits: count words each, 8-byte aligned.
 * Not found: an item that is none, directory records that decrease, leave the index or disagree with the item's symbols,
 * a symbol past the item's, index entries that decrease, bits or bytes beyond the item's or the buffer's, a walk that
 * stops in front of the symbol.  Asynchronous on `stream`; allocates nothing, so it can be captured.
 * AWS_ERROR_INVALID_ARGUMENT for NULL or misaligned arrays, index_entries 0 or a block_symbols that
 * aws_huffman_amd_block_index refuses; AWS_ERROR_UNSUPPORTED_OPERATION without a GPU.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_locate_item_symbols(
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
    const uint64_t *device_items,
    const uint64_t *device_symbols,
    size_t count,
    uint64_t *device_bits,
    uint32_t *device_status,
    void *stream);

/*
 * Makes the plan, on the device, from ranges of symbols of the items of one indexed batch: what
 * aws_huffman_amd_decode_plan_reset_symbol_ranges is for one stream, the batch described as for
 * aws_huffman_amd_decode_plan_reset_item_block_ranges; device_input is the input base of the plan's launches (the ends
 * are located in it by this call).  Item r of the plan reads from the byte that holds its first symbol's first bit to
 * the one that holds its last symbol's last, entered at first_bit, with out_capacity = symbol_count; a range of whole
 * blocks makes the item the block range makes.  Verdicts as for the single stream's ranges.
 * AWS_ERROR_INVALID_ARGUMENT, and a plan without items: every row of the block ranges' list, a range past the item's
 * symbols (sums that overflow count as past), and an end that was not located.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_decode_plan_reset_item_symbol_ranges(
    struct aws_huffman_amd_decode_plan *plan,
    const void *device_input,
    const struct aws_huffman_amd_item_blocks *device_directory,
    const uint64_t *device_index,
    uint64_t index_entries,
    uint64_t item_count,
    uint64_t block_symbols,
    const uint64_t *device_encoded_offsets,
    const uint64_t *device_encoded_lengths,
    uint64_t encoded_offset,
    uint64_t encoded_length,
    const struct aws_huffman_amd_item_symbol_range *device_ranges,
    size_t range_count,
    void *stream);

/* testing: items SHORTER than this many symbols are a wave's work, all others are cut into tiles of whole blocks (1: every
 * item with symbols goes to tiles; 65 536 and more: 65 536, the most a wave takes); 0: back to the built-in rule (4 096) */
AWS_COMPRESSION_API
void aws_huffman_amd_testing_set_batch_index_wave_bytes(uint64_t bytes);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_BATCH_INDEX_H */
