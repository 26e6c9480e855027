#ifndef AWS_COMPRESSION_HUFFMAN_AMD_PLANES_H
#define AWS_COMPRESSION_HUFFMAN_AMD_PLANES_H
/*
 * Byte planes of arrays of multi-byte elements, made on the device: the transposition in front of a coder a plane.
 *
 * The bytes of bf16, f32, ids and offsets have very different distributions by their position within the element: the sign
 * and exponent byte of N(0, 1) holds 2.6 bits of entropy, a mantissa byte 8.  Interleaved, such bytes do not code; by planes,
 * with an engine fitted to each plane (huffman_amd_fit.h) and the stored rule for the planes that do not shrink
 * (huffman_amd_stored.h), they do.  The split takes the 256 counts of every plane in the same read, so a fit needs no pass of
 * its own over the planes:
 *
 *   hipMemsetAsync(d_counts, 0, element_bytes * 256 * sizeof(uint64_t), stream);
 *   aws_huffman_amd_planes_split(-1, d_elements, n, element_bytes, d_planes, stride, d_counts, stream);
 *   for every plane p:
 *       aws_huffman_amd_engine_fit_counts(engine[p], d_counts + 256 * p, d_bits[p], NULL, stream);
 *       aws_huffman_amd_encode_plan_launch_packed_stored(plan[p], d_planes + p * stride, ...);   (a strided plan over the plane)
 *   ... and the receiver: fit_lengths, the packed decode a plane, then
 *   aws_huffman_amd_planes_merge(-1, d_planes, stride, n, element_bytes, d_elements, stream);
 *
 * Both calls take a device number and no engine, as aws_huffman_amd_symbol_counts (huffman_amd_build.h) does.  They are
 * asynchronous on `stream` (NULL: the device's null stream): no host wait, no allocation, no scratch, no memset, the first call
 * included, so they can be captured in a graph.  device -1 = current; the caller's current device is unchanged on return.
 *
 * element_bytes is 1, 2, 4 or 8 (1: a copy, counted if asked).  The elements, the planes and the stride may have any
 * alignment; the only condition is plane_stride >= element_count.  (16-byte aligned addresses and strides are the fast case.)
 *
 * AWS_ERROR_INVALID_ARGUMENT: any other element_bytes; a NULL input, planes or output with element_count > 0;
 * plane_stride < element_count; element_count * element_bytes or (element_bytes - 1) * plane_stride + element_count that does
 * not fit 64 bits; a device that does not exist; device_counts that is not 8-byte aligned; a source range and a destination
 * range that overlap (checked on the host from the pointers).  element_count == 0: success, nothing is enqueued.
 * AWS_ERROR_UNSUPPORTED_OPERATION without a GPU (nothing is read or written).
 *
 * Out of this interface: other element sizes, bit planes, a container for the per-plane buffers, host pointers.
 * (Sorted and slowly moving integers -- offsets, running sums, ids: the planes of their differences, huffman_amd_planes_delta.h.)
 */

#include <aws/compression/huffman_amd.h>

AWS_EXTERN_C_BEGIN

/*
 * device_planes[p * plane_stride + j] = device_input[j * element_bytes + p] for p < element_bytes and j < element_count.
 * Nothing else is written: the bytes between element_count and plane_stride of a plane stay as they were, and so does
 * everything in front of and behind the planes.
 *
 * device_counts (NULL: nothing is counted): element_bytes * 256 uint64_t in device memory, 8-byte aligned;
 * device_counts[p * 256 + b] is ADDED the number of bytes of plane p equal to b, with device-scope 64-bit atomic adds, as
 * aws_huffman_amd_symbol_counts adds: the caller clears the array, and calls on several streams into one array sum.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_planes_split(
    int device,
    const void *device_input,
    uint64_t element_count,
    uint32_t element_bytes,
    void *device_planes,
    uint64_t plane_stride,
    uint64_t *device_counts,
    void *stream);

/*
 * The inverse: device_output[j * element_bytes + p] = device_planes[p * plane_stride + j].  Exactly
 * element_count * element_bytes bytes are written.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_planes_merge(
    int device,
    const void *device_planes,
    uint64_t plane_stride,
    uint64_t element_count,
    uint32_t element_bytes,
    void *device_output,
    void *stream);

/* testing: the most workgroups either call launches (0: back to the default, as many as are resident), so that a few
 * hundred KiB take a workgroup through its grid-stride loop several times.  aws_huffman_amd_testing_set_count_flush_bytes
 * (huffman_amd_build.h) applies to the counted split as to the other counting calls. */
AWS_COMPRESSION_API
void aws_huffman_amd_testing_set_planes_grid(uint32_t workgroups);

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_PLANES_H */
