#ifndef AWS_COMPRESSION_HUFFMAN_AMD_RANGES_H
#define AWS_COMPRESSION_HUFFMAN_AMD_RANGES_H
/*
 * Symbol numbers as addresses of an indexed stream: where a symbol starts, and decode plans over any range of symbols.
 *
 * The block index (huffman_amd_index.h) says where every block_symbols-th symbol starts.  A reader asks for "symbols
 * 700 000 100 .. 700 000 355", not for blocks: symbol s = b * block_symbols + k starts k codes behind bit index[b], and the
 * device finds that bit by walking those k codes inside the block's own bits.  With the encoded stream, its index and the
 * engine that decodes it (nothing of the symbols):
 *
 *   struct aws_huffman_amd_symbol_range r = {700000100, 256, 0};                                   (in device memory)
 *   aws_huffman_amd_decode_plan_reset_symbol_ranges(plan, d_encoded, d_index, length, 16384, 0, encoded_length, d_ranges, 1, stream);
 *   aws_huffman_amd_decode_plan_launch(plan, d_encoded, d_output, stream);                          (256 symbols)
 *
 * decodes the 256 symbols, reserves 256 bytes of output and reads some 300 bytes of the stream (behind the walk that found
 * the range's ends: at most the two blocks they lie in), where a plan over the covering blocks decodes and reserves
 * 16 384.  The index stays as coarse as it is: 0.05 % of the symbols at 16 384 symbols a block.
 *
 * Out of this interface: an index made by the encode launch itself, and aws_huffman_amd_shards_* (one index over the items
 * of a plan: huffman_amd_batch_index.h).
 */

#include <aws/compression/huffman_amd_index.h>

AWS_EXTERN_C_BEGIN

/* what aws_huffman_amd_locate_symbols leaves in *device_status (OR of) */
#define AWS_HUFFMAN_AMD_LOCATE_OK 0u
#define AWS_HUFFMAN_AMD_LOCATE_NOT_FOUND 1u /* some device_bits[i] is AWS_HUFFMAN_AMD_NO_BIT */
#define AWS_HUFFMAN_AMD_NO_BIT UINT64_MAX

/*
 * device_bits[i] = the bit at which symbol s = device_symbols[i] starts in the stream: the sum of the code lengths of symbols
 * [0, s), i = 0 .. count - 1.  device_encoded: the first byte of the stream's encoded_length bytes; device_index, length and
 * block_symbols: those of aws_huffman_amd_block_index (made by it, or received with the stream).  device_symbols and
 * device_bits: count words each in device memory, 8-byte aligned.  With B = block_symbols, b = s / B and k = s % B:
 *
 *   s == length     index[n_blocks]
 *   k == 0          index[b]: no walk, no read of the stream
 *   otherwise       k codes walked from bit index[b], inside the bits [index[b], index[b + 1]) of the stream
 *
 * AWS_HUFFMAN_AMD_NO_BIT, and AWS_HUFFMAN_AMD_LOCATE_NOT_FOUND in *device_status, for s > length; for index[b + 1] <
 * index[b]; for ceil(index[b + 1] / 8) > encoded_length -- the check that keeps a received, damaged index from reading
 * outside the buffer --; and where the walk stops before k codes: a window without a code, or a code cut by the end of the
 * block's bits.  device_status (NULL: not wanted; 4-byte aligned) is always written; count 0 writes nothing else.
 *
 * The walk reads no byte outside [device_encoded, device_encoded + encoded_length) but the rest of an aligned 16-byte line
 * that holds a byte of the stream, and none outside such lines of the bytes that hold bits [index[b], index[b + 1]).
 *
 * The codes are read from the engine's decode tables in device memory: every coder this library decodes works -- codes of
 * up to 32 bits through linked tables; a coder whose codes all have one length L in closed form, index[b] + k L -- and a
 * fitted engine (huffman_amd_fit.h) locates behind aws_huffman_amd_engine_fit_lengths / _fit_counts on the same stream with
 * no host wait.  Until a fit has been enqueued such an engine raises AWS_ERROR_INVALID_STATE, as its launches do.
 *
 * An index made with status AWS_HUFFMAN_AMD_INDEX_SYMBOL_WITHOUT_CODE counts 0 bits for symbols that are not in the
 * stream: inside the blocks that held such symbols the stream's codes have no symbol numbering, and results there are
 * unspecified (a bit inside the block, or AWS_HUFFMAN_AMD_NO_BIT); no read leaves the bounds above.
 *
 * Asynchronous on `stream` (NULL: the engine's): no host wait, no scratch, no allocation; a memset of the status and one or
 * two launches, which can be captured in a graph and replayed.  A position at most 1 024 codes behind its block's first is
 * one lane's walk; one further behind is a workgroup's, whose lanes share the block's bits.
 *
 * AWS_ERROR_INVALID_ARGUMENT: a NULL engine, a NULL or misaligned device_index, a misaligned device_status, NULL or
 * misaligned device_symbols or device_bits (with count > 0), a block_symbols that aws_huffman_amd_block_index refuses, 2^32
 * blocks or more, NULL device_encoded with length > 0.  AWS_ERROR_UNSUPPORTED_OPERATION for an engine that cannot decode,
 * and without a GPU (nothing is read or written).
 */
AWS_COMPRESSION_API
int aws_huffman_amd_locate_symbols(
    struct aws_huffman_amd_engine *engine,
    const void *device_encoded,
    uint64_t encoded_length,
    const uint64_t *device_index,
    uint64_t length,
    uint64_t block_symbols,
    const uint64_t *device_symbols,
    size_t count,
    uint64_t *device_bits,
    uint32_t *device_status,
    void *stream);

/* symbols first_symbol .. first_symbol + symbol_count - 1 of an indexed stream, decoded to out_offset */
struct aws_huffman_amd_symbol_range {
    uint64_t first_symbol;
    uint64_t symbol_count;
    uint64_t out_offset; /* bytes from the decode launch's output base */
};

/*
 * Makes the plan, on the device, from ranges of symbols of ONE indexed stream.  device_input: the input base the plan's
 * launches will be given; the stream's encoded_length bytes lie encoded_offset bytes behind it (this call reads them: both
 * ends of every range are located as aws_huffman_amd_locate_symbols locates them; an end on a block boundary or at `length`
 * costs no walk).  device_ranges: range_count records in device memory, 8-byte aligned.  With s0 = first_symbol, s1 = s0 +
 * symbol_count and bit(s) the located bit, item r of the plan is
 *
 *   in_offset    = encoded_offset + bit(s0) / 8        first_bit = bit(s0) % 8
 *   in_len       = ceil(bit(s1) / 8) - bit(s0) / 8
 *   out_offset   = the range's own
 *   out_capacity = symbol_count
 *
 * and a plain aws_huffman_amd_decode_plan_launch decodes the ranges; ranges may overlap, repeat and come in any order.
 * symbol_count 0 (with s0 <= length) is an empty item.  Items are tight: the road an item takes is chosen by the range's own
 * size -- 60 symbols are a thread's work whatever the block -- and a range whose ends are the ends of whole blocks comes to
 * exactly the item aws_huffman_amd_decode_plan_reset_block_ranges makes for those blocks.  The verdicts are those of block
 * ranges: success, or AWS_ERROR_SHORT_BUFFER where the spare bits of the item's last byte spell a whole symbol; either way
 * produced == out_capacity and the symbols written are the stream's.
 *
 * Everything else as aws_huffman_amd_decode_plan_reset_block_ranges: one wait for a handful of totals and no other, the
 * same rule about the plan's previous launch.  The located bits live in device memory the plan owns (16 bytes a range).
 * The index, the ranges and the stream are read by this call alone; launches of the plan do not need the first two.
 *
 * AWS_ERROR_INVALID_ARGUMENT, and a plan without items (a launch of it does nothing): a range past the stream's last
 * symbol (s1 > length, also where the sum overflows); an end that is not found (see AWS_HUFFMAN_AMD_NO_BIT above: a
 * damaged index, an encoded_length too short for the end's block, a walk that stops); bit(s1) < bit(s0); an item of 4 GiB or
 * more; a NULL plan; a NULL or misaligned device_index or device_ranges, a NULL device_input (with range_count > 0), a
 * block_symbols that aws_huffman_amd_block_index refuses.  AWS_ERROR_INVALID_STATE for a fitted engine before any fit.
 * AWS_ERROR_UNSUPPORTED_OPERATION without a GPU (nothing is read or changed).
 */
AWS_COMPRESSION_API
int aws_huffman_amd_decode_plan_reset_symbol_ranges(
    struct aws_huffman_amd_decode_plan *plan,
    const void *device_input,
    const uint64_t *device_index,
    uint64_t length,
    uint64_t block_symbols,
    uint64_t encoded_offset,
    uint64_t encoded_length,
    const struct aws_huffman_amd_symbol_range *device_ranges,
    size_t range_count,
    void *stream);

/* testing: the most codes behind its block's first that a position may lie for one lane to walk them alone (any number >= 1;
 * one above the blocks' size: every position); 0: back to the built-in rule (1 024) */
AWS_COMPRESSION_API
void aws_huffman_amd_testing_set_locate_lone_symbols(uint32_t symbols);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_RANGES_H */
