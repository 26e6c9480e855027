#ifndef AWS_COMPRESSION_HUFFMAN_AMD_BUILD_H
#define AWS_COMPRESSION_HUFFMAN_AMD_BUILD_H
/*
 * Coders built from data: count the symbols of bytes in device memory, make length-limited code lengths for those
 * counts, make the canonical coder of those lengths, and write its table as .def text.
 *
 *   uint64_t *d_counts = aws_huffman_amd_device_alloc(engine, 256 * sizeof(uint64_t));
 *   aws_huffman_amd_device_fill(engine, d_counts, 0, 256 * sizeof(uint64_t));
 *   aws_huffman_amd_symbol_counts(-1, d_input, length, d_counts, aws_huffman_amd_engine_stream(engine));
 *   aws_huffman_amd_copy_to_host(engine, counts, d_counts, sizeof(counts));  (on the same stream, and waits for it)
 *   aws_huffman_amd_code_lengths_from_counts(counts, 4, 12, AWS_HUFFMAN_AMD_CODE_EVERY_SYMBOL, num_bits);
 *   coder = aws_huffman_amd_table_coder_from_lengths(num_bits);
 *
 * Lengths in [4, 12] for all 256 symbols meet the one-pass encoder's rule (every symbol coded, 4 .. 15 bits) and the
 * chunked decoder's (at most 12 bits) by construction.  The coder is a table coder like any other
 * (aws_huffman_amd_table_coder_destroy frees it); aws_huffman_amd_table_coder_to_def writes its table in the input
 * format of the reference's generator, so that a stock aws-c-compression build can decode what it encodes.
 */

#include <aws/compression/huffman_amd.h>

AWS_EXTERN_C_BEGIN

/*
 * counts[b] += number of bytes equal to b in device_input[0 .. length), for b in 0..255.
 * Asynchronous on `stream` (NULL: the device's null stream); no host wait, no allocation, no memset: it can be captured
 * in a graph.  device_counts: 256 uint64_t in device memory, 8-byte aligned, ADDED to (the caller zeroes them, e.g.
 * aws_huffman_amd_device_fill), with device-scope atomics, so calls on several streams into one array sum correctly.
 * Any address alignment, any length (0: nothing enqueued, success).  device -1 = current; the caller's current device
 * is unchanged on return.
 * AWS_ERROR_INVALID_ARGUMENT: NULL pointers with length > 0, a device that does not exist;
 * AWS_ERROR_UNSUPPORTED_OPERATION without a GPU.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_symbol_counts(
    int device,
    const void *device_input,
    uint64_t length,
    uint64_t *device_counts,
    void *stream);

#define AWS_HUFFMAN_AMD_CODE_EVERY_SYMBOL 1u /* symbols counted 0 times get a code too */

/*
 * Optimal prefix-code lengths for these counts with min_bits <= length <= max_bits (1 <= min <= max <= 32).
 * Coded symbols: count > 0, or all 256 with EVERY_SYMBOL; others get 0.  Minimises sum(counts[s] * num_bits[s])
 * subject to Kraft <= 1.  Deterministic; a higher count never gets a longer code, and equal counts give lengths
 * non-decreasing in symbol value.  One coded symbol gets min_bits.  AWS_ERROR_INVALID_ARGUMENT: no coded symbol,
 * more coded symbols than 2^max_bits, bounds out of range, unknown flags, counts summing to 2^58 or more.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_code_lengths_from_counts(
    const uint64_t counts[256],
    uint32_t min_bits,
    uint32_t max_bits,
    uint32_t flags,
    uint8_t num_bits[256]);

/*
 * The canonical code for these lengths (RFC 1951 section 3.2.2: by (length, symbol), the shortest starting at 0;
 * pattern in the low bits as struct aws_huffman_code says).  0 = no code.  NULL + AWS_ERROR_INVALID_ARGUMENT when
 * Kraft > 1 or a length > 32.  A table coder (aws_huffman_amd_table_coder_new of its rows).
 */
AWS_COMPRESSION_API
struct aws_huffman_symbol_coder *aws_huffman_amd_table_coder_from_lengths(const uint8_t num_bits[256]);

/*
 * The coder's encode table as .def text in the reference generator's input format, one
 * HUFFMAN_CODE(sym, "bits", 0xpattern, num_bits) row per coded symbol (256 encode calls: any coder).
 * *length = bytes needed; AWS_ERROR_SHORT_BUFFER (nothing promised in `text`) when capacity is smaller.
 * No terminating zero is written or counted.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_table_coder_to_def(
    struct aws_huffman_symbol_coder *coder,
    char *text,
    size_t capacity,
    size_t *length);

/* testing: what one workgroup of the counting kernel reads at most between two flushes of its 32-bit LDS counts
 * (rounded down to a multiple of 32 KiB, at least 32 KiB); 0: back to the default, 1 GiB */
AWS_COMPRESSION_API
void aws_huffman_amd_testing_set_count_flush_bytes(uint64_t bytes);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_BUILD_H */
