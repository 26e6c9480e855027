#ifndef AWS_COMPRESSION_HUFFMAN_AMD_FIT_H
#define AWS_COMPRESSION_HUFFMAN_AMD_FIT_H
/*
 * A coder fitted on the device: from the 256 counts aws_huffman_amd_symbol_counts leaves in device memory to an engine's
 * encode table and decode table in one kernel launch, with no copy to the host and no wait.  Count, fit, packed encode
 * then run on one stream (or in one captured graph), a fresh code for every batch:
 *
 *   aws_huffman_amd_engine_new_fitted(&engine, -1, 4, 12);                       (once)
 *   aws_huffman_amd_encode_plan_new(&plan, engine, items, n);                    (once: good for every fit)
 *   per batch, all on `stream`:
 *     hipMemsetAsync(d_counts, 0, 256 * sizeof(uint64_t), stream);
 *     aws_huffman_amd_encode_plan_symbol_counts(plan, d_input, d_counts, stream);   (huffman_amd_plan_counts.h: the plan's
 *                                                  items, whatever they cover; aws_huffman_amd_symbol_counts where they tile a range)
 *     aws_huffman_amd_engine_fit_counts(engine, d_counts, d_num_bits, d_status, stream);
 *     aws_huffman_amd_encode_plan_launch_packed(plan, d_input, d_output, capacity, d_offsets, 1, stream);
 *   the receiver, given the 256 bytes of d_num_bits beside the packed buffer and its offsets:
 *     aws_huffman_amd_engine_fit_lengths(engine2, d_num_bits, d_status, stream);
 *     aws_huffman_amd_decode_plan_reset_packed_input(...) + aws_huffman_amd_decode_plan_launch_packed(...)
 *
 * The lengths are exactly those of aws_huffman_amd_code_lengths_from_counts(counts, min_bits, max_bits,
 * AWS_HUFFMAN_AMD_CODE_EVERY_SYMBOL, ...) and the code exactly that of aws_huffman_amd_table_coder_from_lengths
 * (huffman_amd_build.h): whoever holds the 256 lengths -- this library through aws_huffman_amd_engine_fit_lengths or a
 * host-made coder, a stock aws-c-compression build given the .def text of that coder -- decodes what the engine encodes.
 *
 * All 256 symbols are coded with 4 <= min_bits <= length <= max_bits <= 12: the one-pass encoder's rule and the chunked
 * decoder's hold by construction, and no narrower bound is asked for than those fast paths need.
 *
 * The engine keeps the bounds it was made with, whatever range a fit uses: plans, their capacities and the kernels picked
 * depend on the bounds alone, so a plan made before a fit stays valid behind it.  The price is paid by a code narrower
 * than its bounds: all lengths 8 (uniform bytes) in a (4, 12) engine decode through the 12-bit builds of the chunk
 * kernels or their long way -- exact, and slower than the fixed-length road an engine made on the host from the same
 * lengths (aws_huffman_amd_engine_new) takes.  Roads are not switched on the device.
 *
 * Ordering is the caller's: a fit rewrites the tables that launches of the engine's plans read.  Put a fit and the launches
 * that use it, and the launches in front of it that still use the tables before, on one stream, or order them with
 * events.  As for every engine, one host thread at a time calls into one engine.
 *
 * Out of this interface: coders with symbols that have no code, codes of more than 12 bits, the host-pointer calls of
 * huffman.h and aws_huffman_amd_shards_* (they find engines by coder; a fitted engine has none).
 */

#include <aws/compression/huffman_amd.h>

AWS_EXTERN_C_BEGIN

/*
 * An engine without a coder.  Its tables are made on the device, for codes of min_bits .. max_bits for all 256 symbols.
 * Bounds: 4 <= min_bits <= 8 <= max_bits <= 12, and min_bits < max_bits.  device -1 = current.
 * With min_bits == 8 or max_bits == 8 a fit from counts can only ever yield the flat code of 8 bits a symbol (Kraft, 256
 * coded symbols: none may be shorter than 8 under max_bits 8, none need be longer over min_bits 8): such an engine is
 * accepted, and never compresses.  Bounds that leave the fit a choice have min_bits < 8 < max_bits.
 * Until a fit has been enqueued, launches of its plans raise AWS_ERROR_INVALID_STATE.
 * AWS_ERROR_INVALID_ARGUMENT: bounds outside the range, a NULL pointer, a device that does not exist;
 * AWS_ERROR_UNSUPPORTED_OPERATION without a GPU.  *engine is written on success only.
 * aws_huffman_amd_engine_destroy frees it; aws_huffman_amd_engine_max_code_bits is the declared max_bits.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_engine_new_fitted(struct aws_huffman_amd_engine **engine, int device, uint32_t min_bits, uint32_t max_bits);

/* what a fit leaves in *device_status; anything but 0: the tables are as they were */
#define AWS_HUFFMAN_AMD_FIT_OK 0u
#define AWS_HUFFMAN_AMD_FIT_COUNTS_TOO_LARGE 1u     /* counts that sum to 2^58 or more (the host function's own limit) */
#define AWS_HUFFMAN_AMD_FIT_LENGTH_ZERO 2u          /* a symbol without a code */
#define AWS_HUFFMAN_AMD_FIT_LENGTH_OUT_OF_BOUNDS 3u /* a length outside the engine's min_bits .. max_bits */
#define AWS_HUFFMAN_AMD_FIT_KRAFT_ABOVE_ONE 4u      /* lengths no prefix code has */

/*
 * counts (256 uint64_t in device memory, 8-byte aligned, as aws_huffman_amd_symbol_counts leaves them)
 *   -> code lengths -> canonical code -> the engine's encode table and decode table.
 * One kernel launch on `stream` (NULL: the engine's own).  No host wait, no allocation, no memset: it can be captured in a
 * graph.
 * device_num_bits: 256 bytes in device memory that receive the lengths (NULL: not wanted).
 * device_status: one uint32_t in device memory, 4-byte aligned (NULL: not wanted), AWS_HUFFMAN_AMD_FIT_*.
 * AWS_ERROR_INVALID_ARGUMENT: NULL or misaligned pointers, an engine not made by aws_huffman_amd_engine_new_fitted.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_engine_fit_counts(
    struct aws_huffman_amd_engine *engine,
    const uint64_t *device_counts,
    uint8_t *device_num_bits,
    uint32_t *device_status,
    void *stream);

/*
 * The receiver's half: tables from 256 code lengths that lie in device memory.  A length of 0, a length outside the
 * engine's bounds and a Kraft sum above 1 are refused (status); a Kraft sum below 1 is accepted, and the decode table's
 * windows that no code owns are 0 -- no code, as in every other engine.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_engine_fit_lengths(
    struct aws_huffman_amd_engine *engine,
    const uint8_t *device_num_bits,
    uint32_t *device_status,
    void *stream);

/* made by aws_huffman_amd_engine_new_fitted */
AWS_COMPRESSION_API
bool aws_huffman_amd_engine_is_fitted(const struct aws_huffman_amd_engine *engine);

/*
 * testing: the engine's two device tables copied to the host.  Waits for the engine's stream.
 * enc_table[s] = length << 32 | code; dec_lut[w] = symbol << 8 | length for the window w of
 * aws_huffman_amd_engine_max_code_bits bits, 0: no code; dec_lut_entries must be 1 << that number.
 * (Any engine whose longest code has at most 12 bits.)
 */
AWS_COMPRESSION_API
int aws_huffman_amd_testing_engine_tables(
    struct aws_huffman_amd_engine *engine,
    uint64_t enc_table[256],
    uint16_t *dec_lut,
    size_t dec_lut_entries);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_FIT_H */
