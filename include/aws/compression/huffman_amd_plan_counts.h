#ifndef AWS_COMPRESSION_HUFFMAN_AMD_PLAN_COUNTS_H
#define AWS_COMPRESSION_HUFFMAN_AMD_PLAN_COUNTS_H
/*
 * Symbol counts of the items of an encode plan, made on the device: the first link of a coder fitted to a batch
 * (huffman_amd_fit.h) where the batch is not one contiguous range.
 *
 * aws_huffman_amd_symbol_counts (huffman_amd_build.h) counts ONE range.  A plan's items need not tile a range: a strided
 * plan with in_stride > in_len has gaps (rows with padding, records with headers), a plan made by
 * aws_huffman_amd_encode_plan_reset_device_items has offsets and lengths the host never sees, and a host-made plan may skip
 * bytes, repeat them or list its items in any order.  This call reads the plan's current items, however the plan was
 * filled, and counts exactly the symbols the next launch of that plan encodes:
 *
 *   hipMemsetAsync(d_counts, 0, 256 * sizeof(uint64_t), stream);
 *   aws_huffman_amd_encode_plan_symbol_counts(plan, d_input, d_counts, stream);
 *   aws_huffman_amd_engine_fit_counts(engine, d_counts, NULL, NULL, stream);
 *   aws_huffman_amd_encode_plan_launch_packed(plan, d_input, d_encoded, capacity, d_offsets, 1, stream);
 *
 * Out of this interface: decode plans, aws_huffman_amd_shards_*, counts per item or per group.
 */

#include <aws/compression/huffman_amd.h>

AWS_EXTERN_C_BEGIN

/*
 * device_counts[b] += the sum, over the plan's current items i, of the bytes device_input[in_offset_i + k], k < in_len_i,
 * that equal b.  An item that lists a byte twice counts it twice, and so do two items that overlap; bytes between the items
 * are not counted; carried overflow bits and eos_padding are not symbols and are not counted.
 *
 * device_counts: 256 uint64_t in device memory, 8-byte aligned, ADDED to with device-scope 64-bit atomic adds, as
 * aws_huffman_amd_symbol_counts adds: the caller clears the array, and calls for several plans, on several streams, and of
 * both kinds into one array sum.
 *
 * Asynchronous on `stream` (NULL: the engine's): no host wait, no allocation and no memset, the plan's first such call
 * included, so the call can be captured in a graph.  It reads no table: it works on an engine made by
 * aws_huffman_amd_engine_new_fitted that was never fitted.  It works on every plan -- host-made, strided, from device
 * items -- and changes nothing a later launch or fetch of the plan can see.  A plan without items: success, nothing is
 * enqueued, the counts are untouched.  The plan's records are read on `stream`: whoever gets the plan's arrays next
 * waits for the call as for a launch.
 *
 * AWS_ERROR_INVALID_ARGUMENT: a NULL plan, a NULL or misaligned device_counts, NULL device_input for a plan with items.
 * AWS_ERROR_UNSUPPORTED_OPERATION without a GPU (nothing is read or written).
 */
AWS_COMPRESSION_API
int aws_huffman_amd_encode_plan_symbol_counts(
    struct aws_huffman_amd_encode_plan *plan,
    const void *device_input,
    uint64_t *device_counts,
    void *stream);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_PLAN_COUNTS_H */
