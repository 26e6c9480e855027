#ifndef AWS_COMPRESSION_HUFFMAN_AMD_PLANES_DELTA_H
#define AWS_COMPRESSION_HUFFMAN_AMD_PLANES_DELTA_H
/*
 * Byte planes of DIFFERENCES, in runs: the split of huffman_amd_planes.h with the difference to the previous element taken in
 * its registers, and the merge with the sum behind it.
 *
 * A sorted or slowly moving integer array -- the 64-bit offsets of a packed batch, the running sum of code bits of a block
 * index, the directory of a batch index, sorted ids -- has a narrow local distribution, but over a whole plane its low bytes
 * are uniform: one coder a plane sees 8 bits a byte in them.  Their differences are small numbers whose upper planes are
 * constant and whose low plane is narrow.
 *
 * With x the elements, little-endian unsigned integers of E = element_bytes bytes, and R = run_elements:
 *
 *   d[j] = x[j]                          where R divides j (a run starts)
 *   d[j] = x[j] - x[j - 1] mod 2^(8 E)   everywhere else
 *
 * The difference restarts every R elements, as blocked formats do it: the inverse is then a sum over at most R elements,
 * which one workgroup makes with no word passed between workgroups -- no look-back, no scratch, no status words, nothing
 * that waits -- and a run stays decodable on its own.  The run length hardly matters to the size: R = 16 and R = 2048
 * differ by less than 0.01 of the raw size on offsets and ids.
 *
 *   hipMemsetAsync(d_counts, 0, element_bytes * 256 * sizeof(uint64_t), stream);
 *   aws_huffman_amd_plane_delta_split(-1, d_elements, n, element_bytes, 1024, d_planes, stride, d_counts, stream);
 *   ... a fit and a packed stored launch a plane, as huffman_amd_planes.h shows; the receiver's decode a plane, then
 *   aws_huffman_amd_plane_delta_merge(-1, d_planes, stride, n, element_bytes, 1024, d_elements, stream);
 *
 * Everything huffman_amd_planes.h says of its pair holds for this one: element_bytes is 1, 2, 4 or 8; elements, planes and
 * stride have any alignment with plane_stride >= element_count; device -1 is the current device; the calls are asynchronous
 * on `stream`, with no host wait, no allocation, no scratch and no memset from the first call on, so they can be captured;
 * element_count == 0 succeeds and enqueues nothing; the same arguments are refused with AWS_ERROR_INVALID_ARGUMENT, the
 * overlap of source and destination included (there is no in-place use); AWS_ERROR_UNSUPPORTED_OPERATION without a GPU.
 *
 * run_elements is a power of two from 16 to 2048, or the call fails with AWS_ERROR_INVALID_ARGUMENT: a lane takes 16
 * elements (8 of 8 bytes) and a workgroup of the merge 16 KiB a step, which is 2048 elements of 8 bytes, so a run starts
 * where a lane starts and lies within one step for every element size.  Sender and receiver agree on it as on element_bytes.
 *
 * (The names say plane_delta and not planes_: the library's exported names that speak of planes are exactly those of
 * huffman_amd_planes.h, and its tests hold it to that.)
 *
 * Out of this interface: a sum across runs or runs above 2048; zigzag, XOR or second-order differences; other element sizes;
 * in-place operation; host pointers; summing only some runs of a range.
 */

#include <aws/compression/huffman_amd_planes.h>

AWS_EXTERN_C_BEGIN

/*
 * device_planes[p * plane_stride + j] = byte p of d[j] for p < element_bytes and j < element_count, and nothing else is
 * written.  Nothing in front of the input or behind its element_count * element_bytes bytes is read.
 *
 * device_counts (NULL: nothing is counted): as aws_huffman_amd_planes_split's, of the planes this call writes --
 * device_counts[p * 256 + b] is ADDED the number of j with byte p of d[j] equal to b.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_plane_delta_split(
    int device,
    const void *device_input,
    uint64_t element_count,
    uint32_t element_bytes,
    uint32_t run_elements,
    void *device_planes,
    uint64_t plane_stride,
    uint64_t *device_counts,
    void *stream);

/*
 * The inverse, for any planes (not only those the split wrote): with d[j] the element whose byte p is
 * device_planes[p * plane_stride + j], element j of device_output is the sum of d[i] over i from the start of j's run
 * through j, mod 2^(8 * element_bytes).  Exactly element_count * element_bytes bytes are written.
 */
AWS_COMPRESSION_API
int aws_huffman_amd_plane_delta_merge(
    int device,
    const void *device_planes,
    uint64_t plane_stride,
    uint64_t element_count,
    uint32_t element_bytes,
    uint32_t run_elements,
    void *device_output,
    void *stream);

/* testing: aws_huffman_amd_testing_set_planes_grid (huffman_amd_planes.h) and aws_huffman_amd_testing_set_count_flush_bytes
 * (huffman_amd_build.h) apply to these calls as to the plain ones. */

AWS_EXTERN_C_END

#endif /* AWS_COMPRESSION_HUFFMAN_AMD_PLANES_DELTA_H */
