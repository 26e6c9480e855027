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
    u32 receiver; /* 0: the sender's copy, 1: the receiver's, 2: the receiver's records at a reset, 3: those of a reset to ranges (the same in every thread of the launch) */
    /* sender: the plan's records and lists, the flags and offsets the scan wrote, the caller's capacity */
    const hufd_enc_item *items;
    const hufd_enc_seg *segs;
    const u32 *solo, *tiny;
    u32 n_segs, n_solo, n_tiny;
    const u8 *stored;
    const u64 *offsets;
    u64 capacity;
    hufd_enc_result *enc_results;
    u64 *counts; /* [2]: the stored items, their bytes */
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

/* sender: bytes [at, at + len) of item `item`, where it is stored, as far as they lie in front of the capacity */
__device__ __forceinline__ void stored_send(const stored_job &job, u32 item, u64 at, u32 len, u32 t, u32 g) {
    if (!job.stored[item]) {
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

__device__ __forceinline__ u64 stored_wave_sum(u64 v) {
#pragma unroll
    for (u32 d = kWave / 2; d > 0; d >>= 1) {
        v += __shfl_xor(v, d);
    }
    return v;
}

/* the plan's stored records from the three arrays a receiver was given (checked by the planner's pass in front) */
__device__ __forceinline__ void stored_records_body(const stored_job &job) {
    const u32 i = blockIdx.x * kStoredThreads + threadIdx.x;
    if (i >= job.n_items) {
        return;
    }
    const u64 at = job.offsets[i];
    job.new_rec[2 * (u64)i] = at;
    job.new_rec[2 * (u64)i + 1] = job.stored[i] == 1 ? (job.lengths ? job.lengths[i] : job.offsets[(u64)i + 1] - at) : HUFK_NOT_STORED;
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
    if (job.receiver >= 2) { /* (the same in every thread of the launch) */
        if (job.receiver == 2) {
            stored_records_body(job);
        } else {
            stored_range_records_body(job);
        }
        return;
    }
    const u32 t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
    u32 b = blockIdx.x;
    if (!job.receiver) {
        if (b < job.n_segs) { /* a workgroup a segment */
            const hufd_enc_seg *seg = job.segs + b;
            const u32 item = seg->item;
            stored_send(job, item, seg->in_off - job.items[item].in_off, seg->len, t, kStoredThreads);
            return;
        }
        b -= job.n_segs;
        const u32 solo_blocks = (job.n_solo + kStoredWaves - 1) / kStoredWaves;
        if (b < solo_blocks) { /* a wave an item of at most a segment */
            const u32 k = b * kStoredWaves + wave;
            if (k < job.n_solo) {
                const u32 item = job.solo[k];
                stored_send(job, item, 0, (u32)job.items[item].in_len, lane, kWave);
            }
            return;
        }
        b -= solo_blocks;
        const u32 tiny_blocks = (job.n_tiny + kStoredThreads - 1) / kStoredThreads;
        if (b < tiny_blocks) { /* a lane an item a thread encodes */
            const u32 k = b * kStoredThreads + t;
            if (k < job.n_tiny) {
                const u32 item = job.tiny[k];
                stored_send(job, item, 0, (u32)job.items[item].in_len, 0, 1);
            }
            return;
        }
        b -= tiny_blocks;
        /* a thread an item, the workgroups in turns: the record of a stored item (whole: success; across the edge: what
         * fitted, and AWS_ERROR_SHORT_BUFFER; never overflow bits), and the counts -- ONE pair of atomic adds a workgroup: a
         * pair a wave were 32 768 of them on two words for a million items, one after the other at the memory side, 0.39 ms */
        u64 one = 0, bytes = 0;
        for (u64 i = (u64)b * kStoredThreads + t; i < job.n_items; i += (u64)job.item_blocks * kStoredThreads) {
            if (!job.stored[i]) {
                continue;
            }
            const u64 len = job.items[i].in_len, off = job.offsets[i];
            const u64 room = job.capacity > off ? job.capacity - off : 0;
            const u64 fitted = room < len ? room : len;
            hufd_enc_result *r = job.enc_results + i;
            r->status = fitted < len ? HUFD_ENC_SHORT : HUFD_ENC_OK;
            r->ovf_pattern = 0;
            r->ovf_bits = 0;
            r->reserved = 0;
            r->consumed = fitted;
            r->produced = fitted;
            one += 1;
            bytes += len;
        }
        u64 *slots = reinterpret_cast<u64 *>(dyn_lds);
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
                atomicAdd(&job.counts[0], one);
                atomicAdd(&job.counts[1], bytes);
            }
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
        const u64 left = len - at;
        stored_copy_range(
            job.in + job.rec[2 * (u64)lo] + at, job.out + to->out_off + at, left < HUFK_STORED_TILE_BYTES ? (u32)left : HUFK_STORED_TILE_BYTES,
            t, kStoredThreads);
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
                stored_copy_range(job.in + job.rec[2 * (u64)i], job.out + to->out_off, (u32)len, lane, kWave);
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
            r->stop_bit = 8 * len;
            r->cap_bit = 0;
            r->stop_kind = HUFD_STOP_END;
            r->reserved = 0;
        }
    }
}
