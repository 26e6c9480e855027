/*
 * Items stored raw in a packed batch (huffman_amd_stored.h): the copy of their bytes, and their result records -- bodies that
 * unpack_records_kernel (pack_kernels.hip, which includes this file inside its namespace) hosts beside the scan's, chosen by
 * its launch argument: the library links 90 kernels and is held to that many (tests/test_library_boundary.py).
 *
 * Sender (aws_huffman_amd_encode_plan_launch_packed_stored): the scan between the length pass and the encode pass has decided
 * which items are stored (pack_kernels.hip, kPackStored: the caller's flags, and no room for them in the encode pass's
 * records).  Behind the encode pass ONE launch copies them, distributed by the plan's own lists, which cover every item
 * exactly once, as the fourth body of count_kernel distributes them: a workgroup a segment, a wave an item a wave encodes, a
 * lane an item a thread encodes.  Work whose item is not flagged leaves at once.  Its last workgroups, a thread an item,
 * rewrite the stored items' result records (the encode pass has written "no room" there) and count them.
 *
 * Receiver (aws_huffman_amd_decode_plan_launch_packed of a plan reset with flags): a stored item has no encoded bytes in the
 * plan's item records, so no decode kernel touches it; the plan owns {source offset, length} of every stored item and the
 * tiles of the long ones, scanned (pack_kernels.hip, kPackStoredTiles).  Behind the emit stage the same kernel copies them: a
 * workgroup a tile, found by a search over the scanned tiles, a wave an item shorter than a tile's quarter; and rewrites
 * their result records.
 *
 * Ranges of an indexed batch with stored items (huffman_amd_stored_index.h): the plan of such a reset holds a range in a stored
 * item as {in_off = where its bytes start, in_len = 0, out_off = the caller's, out_cap = their number}.  The reset makes the
 * same records and tiles from these, a thread a range, and a PLAIN launch runs the receiver's copy behind its emit stage with
 * the plan's own item records for the places: destinations come from the ranges, in any order, not from a scan.
 *
 * Constant items (huffman_amd_constant.h), three more jobs of the same bodies.  The sender's detection, in front of the scan
 * (receiver == 4): the sender's distribution once more, every unit compares its bytes with the item's first byte in groups of
 * 16 loaded at any alignment -- a group that ends on the range's last byte for what is left over, so nothing outside the item
 * is read -- and a unit that meets a difference marks the item in differs[] and leaves: a wave after its first group, which
 * for every wave of a workgroup is among the segment's first 64, so data that is not constant costs 1 KiB a segment from
 * memory.  Items that cannot be constant (carried bits, 9 bytes or fewer) are not read.
 * The scan reads the marks; the sender's record pass writes the 9 bytes of a constant item, its record and its counts, and
 * clears every mark again: a launch leaves the words as it found them, nothing is cleared in front.  The receiver's records
 * hold {kStoredConstant | value, count} for a constant item, read from its head at the reset, and the copy's tile and wave arms
 * fill from the broadcast byte where they would copy.
 *
 * A range is copied at any source and destination address: up to 15 bytes one by one until the destination is 16-byte
 * aligned, whole 16-byte groups -- loaded at any alignment, stored aligned, four a thread in flight --, then up to 15 bytes
 * one by one.  Nothing outside the range is read or written.  (A lone lane's range: stored_copy_lane.)
 */

constexpr u32 kStoredThreads = 256;
constexpr u32 kStoredWaves = kStoredThreads / kWave;
constexpr u32 kStoredItemBlocks = 256; /* workgroups of the sender's record pass at most */
constexpr u32 kStoredLdsBytes = 2 * kStoredWaves * sizeof(u64);
constexpr u32 kStoredUnroll = 4; /* 16-byte groups a thread has in flight: a workgroup's turn is a segment */
static_assert(kStoredThreads == kPackThreads && kStoredLdsBytes <= kPackLdsBytes, "hosted by unpack_records_kernel");
static_assert(kStoredThreads * kStoredUnroll * 16u == HUFD_ENC_SEG_BYTES, "a segment is one turn of a workgroup");
static_assert(HUFK_STORED_TILE_BYTES == HUFD_ENC_SEG_BYTES, "the receiver's tile is the sender's segment");

struct stored_job {
    const u8 *in;
    u8 *out;
    u32 n_items;
    u32 receiver; /* 0: the sender's copy, 1: the receiver's, 2: the receiver's records at a reset, 3: those of a reset to ranges, 4: the sender's detection of constant items (the same in every thread of the launch) */
    /* sender: the plan's records and lists, the flags and offsets the scan wrote, the caller's capacity */
    const hufd_enc_item *items;
    const hufd_enc_seg *segs;
    const u32 *solo, *tiny;
    u32 n_segs, n_solo, n_tiny;
    const u8 *stored;
    const u64 *offsets;
    u64 capacity;
    hufd_enc_result *enc_results;
    u64 *counts; /* [2]: the stored items, their bytes; with differs [4]: then the constant items, their bytes */
    u8 *differs; /* a constant launch (NULL: a stored one): [n_items], 1 where the detection met a byte that is not the item's first */
    u32 item_blocks; /* the workgroups that rewrite records and count, a thread an item in turns */
    /* receiver: the plan's stored records and scanned tiles, the records the offsets pass placed */
    const u64 *rec;        /* [n_items][2]: source offset, length or HUFK_NOT_STORED */
    const u64 *tile_first; /* [n_items + 1] */
    u32 n_tiles;
    const hufd_dec_item *placed;
    hufd_dec_result *dec_results;
    /* the receiver's reset: the sender's lengths (NULL: up to the next offset; `offsets`, `stored`: the other two arrays) and
     * the records to write.  A reset to ranges: `offsets` is the ranges, four words each, the first the item; `stored` the
     * batch's flags; `placed` the plan's item records */
    const u64 *lengths;
    u64 *new_rec;
};

/* `len` bytes from src to dst by `g` threads, this one number t of them */
__device__ __forceinline__ void stored_copy_range(const u8 *src, u8 *dst, u32 len, u32 t, u32 g) {
    const u32 to_aligned = (16u - (u32)((uintptr_t)dst & 15u)) & 15u;
    const u32 head = to_aligned < len ? to_aligned : len;
    for (u32 b = t; b < head; b += g) {
        dst[b] = src[b];
    }
    const u32 n_vec = (len - head) / 16u;
    const u8 *s = src + head;
    u8 *d = dst + head;
    for (u32 first = 0; first < n_vec; first += g * kStoredUnroll) {
        uint4 v[kStoredUnroll];
        bool ok[kStoredUnroll];
#pragma unroll
        for (u32 u = 0; u < kStoredUnroll; ++u) {
            const u32 a = first + u * g + t;
            ok[u] = a < n_vec;
            v[u] = uint4{0u, 0u, 0u, 0u};
            if (ok[u]) {
                const unaligned_uint4 w = *reinterpret_cast<const unaligned_uint4 *>(s + (u64)a * 16u);
                v[u] = uint4{w.x, w.y, w.z, w.w};
            }
        }
#pragma unroll
        for (u32 u = 0; u < kStoredUnroll; ++u) {
            const u32 a = first + u * g + t;
            if (ok[u]) {
                *reinterpret_cast<uint4 *>(d + (u64)a * 16u) = v[u];
            }
        }
    }
    for (u32 b = head + n_vec * 16u + t; b < len; b += g) {
        dst[b] = src[b];
    }
}

/* The same by ONE lane, for an item a thread encodes: a lane's byte loops are round trips one after the other (fifteen at
 * either end were 0.53 ms for a million items of 16 to 80 bytes), so there is no head -- the groups are stored at any
 * alignment as they are loaded -- and the last len % 16 bytes of a range of 16 or more go as one more group that ends on the
 * range's last byte, over bytes the group in front has written with the same values.  Only a range below 16 bytes goes byte
 * by byte. */
__device__ __forceinline__ void stored_copy_lane(const u8 *src, u8 *dst, u32 len) {
    const u32 n_vec = len / 16u;
    for (u32 first = 0; first < n_vec; first += kStoredUnroll) {
        uint4 v[kStoredUnroll]; /* (field by field: an array of the packed records went through scratch memory) */
#pragma unroll
        for (u32 u = 0; u < kStoredUnroll; ++u) {
            const u32 a = first + u < n_vec ? first + u : first;
            const unaligned_uint4 w = *reinterpret_cast<const unaligned_uint4 *>(src + a * 16u);
            v[u] = uint4{w.x, w.y, w.z, w.w};
        }
#pragma unroll
        for (u32 u = 0; u < kStoredUnroll; ++u) {
            if (first + u < n_vec) {
                *reinterpret_cast<unaligned_uint4 *>(dst + (first + u) * 16u) = unaligned_uint4{v[u].x, v[u].y, v[u].z, v[u].w};
            }
        }
    }
    if (len & 15u) {
        if (n_vec) {
            *reinterpret_cast<unaligned_uint4 *>(dst + len - 16u) = *reinterpret_cast<const unaligned_uint4 *>(src + len - 16u);
        } else {
            for (u32 b = 0; b < len; ++b) {
                dst[b] = src[b];
            }
        }
    }
}


constexpr u64 kStoredConstant = HUFK_CONSTANT; /* in a receiver's record: the source "offset" of a constant item is this | its value */
constexpr u32 kStoredConstantBytes = HUFK_CONSTANT_BYTES;

/* `len` bytes at dst, each the byte v32 repeats, by `g` threads, this one number t of them: as the copy, bytes until the
 * destination is aligned, aligned groups, bytes */
__device__ __forceinline__ void stored_fill_range(u8 *dst, u32 len, u32 v32, u32 t, u32 g) {
    const u32 to_aligned = (16u - (u32)((uintptr_t)dst & 15u)) & 15u;
    const u32 head = to_aligned < len ? to_aligned : len;
    for (u32 b = t; b < head; b += g) {
        dst[b] = (u8)v32;
    }
    const u32 n_vec = (len - head) / 16u;
    u8 *d = dst + head;
    for (u32 a = t; a < n_vec; a += g) {
        *reinterpret_cast<uint4 *>(d + (u64)a * 16u) = uint4{v32, v32, v32, v32};
    }
    for (u32 b = head + n_vec * 16u + t; b < len; b += g) {
        dst[b] = (u8)v32;
    }
}

/* whether the 16 bytes at `at` are not all the byte v32 repeats */
__device__ __forceinline__ bool constant_group_differs(const u8 *at, u32 v32) {
    const unaligned_uint4 w = *reinterpret_cast<const unaligned_uint4 *>(at);
    return ((w.x ^ v32) | (w.y ^ v32) | (w.z ^ v32) | (w.w ^ v32)) != 0u;
}

/* Whether some byte of src[0 .. len) is not that byte, by the `g` threads of whole waves (every lane of them calls), the
 * same answer in every lane of a wave: group a < len / 16 lies at 16 a, one more ends on the last byte.  A wave leaves behind
 * its first group where one of its lanes met a difference; what is left goes kStoredUnroll groups a thread in flight. */
__device__ __forceinline__ bool constant_range_differs(const u8 *src, u32 len, u32 v32, u32 t, u32 g) {
    bool differs = false;
    if (len < 16u) {
        for (u32 b = t; b < len; b += g) {
            differs |= src[b] != (u8)v32;
        }
        return __any(differs) != 0;
    }
    const u32 n_vec = len / 16u, groups = n_vec + ((len & 15u) ? 1u : 0u);
    /* (every wave of a workgroup looks at the range's FIRST 64 groups: what data that is not constant costs is 1 KiB a
     * segment from memory -- the waves' own first groups were 4 KiB of it, 0.11 ms for a 1 GiB item) */
    const u32 lane = t & (kWave - 1);
    if (lane < groups) {
        differs = constant_group_differs(src + (lane < n_vec ? lane * 16u : len - 16u), v32);
    }
    if (__any(differs)) {
        return true;
    }
    for (u32 first = kWave; first < groups; first += g * kStoredUnroll) { /* (the same trips in every thread) */
#pragma unroll
        for (u32 u = 0; u < kStoredUnroll; ++u) {
            const u32 a = first + u * g + t;
            if (a < groups) {
                differs |= constant_group_differs(src + (a < n_vec ? a * 16u : len - 16u), v32);
            }
        }
        if (__any(differs)) {
            return true;
        }
    }
    return false;
}

/* the same by ONE lane, for an item a thread encodes: it leaves at its first group that differs */
__device__ __forceinline__ bool constant_lane_differs(const u8 *src, u32 len, u32 v32) {
    if (len < 16u) {
        for (u32 b = 0; b < len; ++b) {
            if (src[b] != (u8)v32) {
                return true;
            }
        }
        return false;
    }
    const u32 n_vec = len / 16u, groups = n_vec + ((len & 15u) ? 1u : 0u);
    if (constant_group_differs(src, v32)) {
        return true;
    }
    for (u32 first = 1; first < groups; first += kStoredUnroll) {
        bool differs = false;
#pragma unroll
        for (u32 u = 0; u < kStoredUnroll; ++u) {
            const u32 a = first + u < groups ? first + u : first;
            differs |= constant_group_differs(src + (a < n_vec ? a * 16u : len - 16u), v32);
        }
        if (differs) {
            return true;
        }
    }
    return false;
}

/* detection: bytes [at, at + len) of item `item` against the item's first byte; a unit that meets a difference marks the item.
 * An item the rule of huffman_amd_constant.h never makes constant is not read (the same in every thread of the unit). */
__device__ __forceinline__ void constant_detect(const stored_job &job, u32 item, u64 at, u32 len, u32 t, u32 g) {
    const hufd_enc_item *it = job.items + item;
    if (it->ovf_bits != 0 || it->in_len <= kStoredConstantBytes) {
        return;
    }
    const u8 *base = job.in + it->in_off;
    const u32 v32 = (u32)base[0] * 0x01010101u;
    const bool differs = g == 1 ? constant_lane_differs(base + at, len, v32) : constant_range_differs(base + at, len, v32, t, g);
    if (differs && (t & (kWave - 1)) == 0) { /* (a lone lane is given t = 0) */
        job.differs[item] = 1;
    }
}

/* sender: bytes [at, at + len) of item `item`, where it is stored, as far as they lie in front of the capacity */
__device__ __forceinline__ void stored_send(const stored_job &job, u32 item, u64 at, u32 len, u32 t, u32 g) {
    if (job.stored[item] != 1) {
        return;
    }
    const u64 off = job.offsets[item] + at;
    if (off >= job.capacity) {
        return;
    }
    const u64 room = job.capacity - off;
    const u8 *src = job.in + job.items[item].in_off + at;
    const u32 fitted = room < len ? (u32)room : len;
    if (g == 1) {
        stored_copy_lane(src, job.out + off, fitted);
    } else {
        stored_copy_range(src, job.out + off, fitted, t, g);
    }
}

/* the sender's work on a unit of the plan's lists: the detection, or the copy of what the scan has flagged stored */
__device__ __forceinline__ void stored_unit(const stored_job &job, u32 item, u64 at, u32 len, u32 t, u32 g) {
    if (job.receiver == 4) { /* (the same in every thread of the launch) */
        constant_detect(job, item, at, len, t, g);
    } else {
        stored_send(job, item, at, len, t, g);
    }
}

__device__ __forceinline__ u64 stored_wave_sum(u64 v) {
#pragma unroll
    for (u32 d = kWave / 2; d > 0; d >>= 1) {
        v += __shfl_xor(v, d);
    }
    return v;
}

/* counts[0] += the workgroup's sum of `one`, counts[1] += that of `bytes` -- ONE pair of atomic adds a workgroup: a pair a wave
 * were 32 768 of them on two words for a million items, one after the other at the memory side, 0.39 ms.  `slots`:
 * 2 * kStoredWaves words of LDS, free again behind the call */
__device__ __forceinline__ void stored_block_count(u64 one, u64 bytes, u64 *counts, u64 *slots) {
    const u32 t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    one = stored_wave_sum(one);
    bytes = stored_wave_sum(bytes);
    if (lane == 0) {
        slots[wave] = one;
        slots[kStoredWaves + wave] = bytes;
    }
    __syncthreads();
    if (t == 0) {
        one = bytes = 0;
        for (u32 w = 0; w < kStoredWaves; ++w) {
            one += slots[w];
            bytes += slots[kStoredWaves + w];
        }
        if (one) {
            atomicAdd(&counts[0], one);
            atomicAdd(&counts[1], bytes);
        }
    }
    __syncthreads();
}

/* the plan's stored records from the three arrays a receiver was given (checked by the planner's pass in front) */
__device__ __forceinline__ void stored_records_body(const stored_job &job) {
    const u32 i = blockIdx.x * kStoredThreads + threadIdx.x;
    if (i >= job.n_items) {
        return;
    }
    const u64 at = job.offsets[i];
    const u32 kind = job.stored[i];
    if (kind == 2 && job.in) { /* (a reset with the packed buffer: the head of a constant item, its count and its value) */
        const u8 *head = job.in + at;
        u64 count = 0;
        for (u32 k = 0; k < 8; ++k) {
            count |= (u64)head[k] << (8 * k);
        }
        job.new_rec[2 * (u64)i] = kStoredConstant | head[8];
        job.new_rec[2 * (u64)i + 1] = count;
        return;
    }
    job.new_rec[2 * (u64)i] = at;
    job.new_rec[2 * (u64)i + 1] = kind == 1 ? (job.lengths ? job.lengths[i] : job.offsets[(u64)i + 1] - at) : HUFK_NOT_STORED;
}

/* ... and from the item records of a plan of ranges (the planner's pass in front has checked every range, its item and
 * that item's flag): a range of no bytes is an empty item, not a stored one */
__device__ __forceinline__ void stored_range_records_body(const stored_job &job) {
    const u32 i = blockIdx.x * kStoredThreads + threadIdx.x;
    if (i >= job.n_items) {
        return;
    }
    const u64 item = job.offsets[4 * (u64)i];
    const u64 len = job.placed[i].out_cap;
    job.new_rec[2 * (u64)i] = job.placed[i].in_off;
    job.new_rec[2 * (u64)i + 1] = job.stored[item] == 1 && len ? len : HUFK_NOT_STORED;
}

__device__ __forceinline__ void stored_copy_body(const stored_job &job) {
    if (job.receiver == 2 || job.receiver == 3) { /* (the same in every thread of the launch) */
        if (job.receiver == 2) {
            stored_records_body(job);
        } else {
            stored_range_records_body(job);
        }
        return;
    }
    const u32 t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    u32 b = blockIdx.x;
    if (job.receiver != 1) { /* (0 or 4: the sender's distribution) */
        if (b < job.n_segs) { /* a workgroup a segment */
            const hufd_enc_seg *seg = job.segs + b;
            const u32 item = seg->item;
            stored_unit(job, item, seg->in_off - job.items[item].in_off, seg->len, t, kStoredThreads);
            return;
        }
        b -= job.n_segs;
        const u32 solo_blocks = (job.n_solo + kStoredWaves - 1) / kStoredWaves;
        if (b < solo_blocks) { /* a wave an item of at most a segment */
            const u32 k = b * kStoredWaves + wave;
            if (k < job.n_solo) {
                const u32 item = job.solo[k];
                stored_unit(job, item, 0, (u32)job.items[item].in_len, lane, kWave);
            }
            return;
        }
        b -= solo_blocks;
        const u32 tiny_blocks = (job.n_tiny + kStoredThreads - 1) / kStoredThreads;
        if (b < tiny_blocks) { /* a lane an item a thread encodes */
            const u32 k = b * kStoredThreads + t;
            if (k < job.n_tiny) {
                const u32 item = job.tiny[k];
                stored_unit(job, item, 0, (u32)job.items[item].in_len, 0, 1);
            }
            return;
        }
        b -= tiny_blocks;
        if (job.receiver == 4) { /* (the detection has no record pass: its grid ends with the lists) */
            return;
        }
        /* a thread an item, the workgroups in turns: the record of a stored item (whole: success; across the edge: what
         * fitted, and AWS_ERROR_SHORT_BUFFER; never overflow bits), and the counts.  A constant launch: also the 9 bytes of a
         * constant item, all of them or none, its record and its counts, and every mark of the detection cleared again */
        u64 one = 0, bytes = 0, constant_one = 0, constant_bytes = 0;
        for (u64 i = (u64)b * kStoredThreads + t; i < job.n_items; i += (u64)job.item_blocks * kStoredThreads) {
            if (job.differs && job.differs[i]) {
                job.differs[i] = 0;
            }
            const u32 kind = job.stored[i];
            if (!kind) {
                continue;
            }
            const u64 len = job.items[i].in_len, off = job.offsets[i];
            const u64 room = job.capacity > off ? job.capacity - off : 0;
            hufd_enc_result *r = job.enc_results + i;
            r->ovf_pattern = 0;
            r->ovf_bits = 0;
            r->reserved = 0;
            if (kind == 2) {
                const bool fits = room >= kStoredConstantBytes;
                if (fits) {
                    u8 *to = job.out + off;
                    for (u32 k = 0; k < 8; ++k) {
                        to[k] = (u8)(len >> (8 * k));
                    }
                    to[8] = job.in[job.items[i].in_off];
                }
                r->status = fits ? HUFD_ENC_OK : HUFD_ENC_SHORT;
                r->consumed = fits ? len : 0;
                r->produced = fits ? kStoredConstantBytes : 0;
                constant_one += 1;
                constant_bytes += len;
                continue;
            }
            const u64 fitted = room < len ? room : len;
            r->status = fitted < len ? HUFD_ENC_SHORT : HUFD_ENC_OK;
            r->consumed = fitted;
            r->produced = fitted;
            one += 1;
            bytes += len;
        }
        u64 *slots = reinterpret_cast<u64 *>(dyn_lds);
        stored_block_count(one, bytes, job.counts, slots);
        if (job.differs) { /* (the same in every thread of the launch) */
            stored_block_count(constant_one, constant_bytes, job.counts + 2, slots);
        }
        return;
    }
    if (b < job.n_tiles) { /* a workgroup a tile: the last item whose tiles start at or in front of it */
        u32 lo = 0, hi = job.n_items;
        while (hi - lo > 1) {
            const u32 mid = lo + (hi - lo) / 2;
            if (job.tile_first[mid] <= b) {
                lo = mid;
            } else {
                hi = mid;
            }
        }
        const u64 len = job.rec[2 * (u64)lo + 1];
        const u64 at = ((u64)b - job.tile_first[lo]) * HUFK_STORED_TILE_BYTES;
        const hufd_dec_item *to = job.placed + lo;
        /* (a record that says a tile past its item's end: nothing) */
        if (len == HUFK_NOT_STORED || at >= len || to->out_cap != len) {
            return;
        }
        const u64 left = len - at, from = job.rec[2 * (u64)lo];
        const u32 n = left < HUFK_STORED_TILE_BYTES ? (u32)left : HUFK_STORED_TILE_BYTES;
        if (from & kStoredConstant) { /* (a constant item: the source is its byte) */
            stored_fill_range(job.out + to->out_off + at, n, (u32)(from & 0xFFu) * 0x01010101u, t, kStoredThreads);
        } else {
            stored_copy_range(job.in + from + at, job.out + to->out_off + at, n, t, kStoredThreads);
        }
        return;
    }
    b -= job.n_tiles;
    const u32 wave_blocks = (job.n_items + kStoredWaves - 1) / kStoredWaves;
    if (b < wave_blocks) { /* a wave an item too short for tiles */
        const u32 i = b * kStoredWaves + wave;
        if (i < job.n_items) {
            const u64 len = job.rec[2 * (u64)i + 1];
            const hufd_dec_item *to = job.placed + i;
            if (len < HUFK_STORED_WAVE_BYTES && to->out_cap == len) {
                const u64 from = job.rec[2 * (u64)i];
                if (from & kStoredConstant) {
                    stored_fill_range(job.out + to->out_off, (u32)len, (u32)(from & 0xFFu) * 0x01010101u, lane, kWave);
                } else {
                    stored_copy_range(job.in + from, job.out + to->out_off, (u32)len, lane, kWave);
                }
            }
        }
        return;
    }
    b -= wave_blocks;
    /* a thread an item: the record of a stored item -- sym = its packed length, all of them or none (the record the offsets
     * pass placed says which) */
    const u32 i = b * kStoredThreads + t;
    if (i < job.n_items) {
        const u64 len = job.rec[2 * (u64)i + 1];
        if (len != HUFK_NOT_STORED) {
            hufd_dec_result *r = job.dec_results + i;
            r->total_symbols = len;
            r->stop_bit = (job.rec[2 * (u64)i] & kStoredConstant) ? 8u * kStoredConstantBytes : 8 * len;
            r->cap_bit = 0;
            r->stop_kind = HUFD_STOP_END;
            r->reserved = 0;
        }
    }
}
