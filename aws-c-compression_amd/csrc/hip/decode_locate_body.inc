/*
 * Where a symbol of an indexed stream starts (aws_huffman_amd_locate_symbols and the ends of
 * aws_huffman_amd_decode_plan_reset_symbol_ranges, huffman_amd_ranges.h): symbol s = b * block_symbols + k starts k codes
 * behind bit index[b], and this body walks them.  It is a further body of dec_deep_kernel (decode_items_kernels.hip, which
 * includes this file behind stream_reader, deep_entry, deep_shared and lane_memo), chosen by a launch argument
 * (hufd_locate::bits != NULL), not a kernel of its own: it stages the same tables in the same LDS, settles lanes by the same
 * fixed point, and the library's kernel census is held at 90.
 *
 * What bounds it.  A walk is given the span of its block, bits [index[b], index[b + 1]) of the stream: the reader is started
 * at the byte that holds the span's first bit with the bytes up to the one that holds its last, so nothing is loaded outside
 * the aligned 16-byte lines that hold a byte of the span, and a code that does not end inside the span is cut
 * (HUFD_STOP_INCOMPLETE), whatever the bits behind it say.  Before any walk: s <= length, index[b + 1] >= index[b] and
 * ceil(index[b + 1] / 8) <= encoded_length; a position that fails one of them, or whose walk stops before k codes (a window
 * without a code, a code cut by the span's end), gets HUFD_NO_BIT and raises bit 0 of *status.  s == length and k == 0 are
 * index entries: no walk, no read of the stream.  A coder whose codes all have one length L: index[b] + k L, no walk.
 *
 * Two launches, each position taken by exactly one of them:
 *   coop 0   a lane a position, for k <= lone_symbols (and everything that needs no walk): the lane walks k codes.
 *   coop 1   a workgroup a position, for k > lone_symbols.  Code k starts at most 32 k bits behind the span's first, so the
 *            lanes split the bytes from the span's first to there (or to its end) evenly, walk count-only from a guessed
 *            entry (where a walk over the 256 bits in front of the lane crosses into it; lane 0: the span's true first bit) and take the exit of the lane in front for
 *            their entry until nothing changes -- dec_deep_kernel's fixed point with dec_wide_settle's rule for walks that
 *            stop: lane 0's entry is true and every round settles at least one more lane, so it is exact also for streams whose walks never fall into step, which need
 *            up to as many rounds as lanes (a lane's last four entries are remembered: such a round costs a look).  The
 *            counts of the lanes on the true path are scanned, and the one lane that holds code number k walks to it.
 */

constexpr u32 kLocateLaneMinBytes = 64; /* a cooperating lane's share of a short span: fewer lanes, fewer rounds */
constexpr u32 kLocateGuessBits = 256;   /* the bits in front of a lane its first guess is walked over (dec_wide_settle's 32 bytes) */

struct locate_walked {
    u64 pos;   /* where the walk ended */
    u32 count; /* codes that start in [from, pos) */
    u32 why;   /* HUFD_STOP_NONE: it reached `to`, the span's end or code number `want` */
};

/* follows the codes from stream bit `from` (bits from byte 0 of `in`) while they start in front of `to` and of the span's
 * end `rem`, up to code number `want` (~0u: all of them) */
template <bool DEEP, bool GUESS = false> /* GUESS: a window without a code is stepped over a bit at a time (a walk that only looks for where the codes fall into step) */
__device__ __forceinline__ locate_walked locate_walk(
    const u32 *deep, const u16 *lut, u32 lut_bits, const u8 *in, u64 rem, u64 from, u64 to, u32 want) {
    const u64 end_byte = rem / 8 + (rem % 8 ? 1 : 0);
    stream_reader sr = {};
    if (from < rem) {
        sr.start(in + (from >> 3), end_byte - (from >> 3), (u32)(from & 7));
    }
    locate_walked r;
    r.pos = from;
    r.count = 0;
    r.why = HUFD_STOP_NONE;
    const u64 stop = to < rem ? to : rem;
    while (r.pos < stop && r.count != want) {
        const u32 entry = DEEP ? deep_entry(deep, sr.peek()) : lut[sr.peek() >> (32 - lut_bits)];
        const u32 len = entry & 0xFFu;
        if (len == 0) {
            if (GUESS) {
                sr.skip(1);
                r.pos += 1;
                continue;
            }
            r.why = HUFD_STOP_INVALID;
            break;
        }
        if (r.pos + len > rem) {
            r.why = HUFD_STOP_INCOMPLETE;
            break;
        }
        ++r.count;
        sr.skip(len);
        r.pos += len;
    }
    return r;
}

struct locate_position {
    u64 bit;      /* walk == 0: the answer */
    u64 from, to; /* walk != 0: the span of the symbol's block */
    u32 k;        /* ... and the codes between its first bit and the symbol */
    u32 walk;
};

/* The item arm: (item, symbol) to the absolute span of the symbol's block, bits from the packed buffer's first byte.  The
 * single stream's rule with the entries taken relative to the item's first and moved to the item's place; every word of a
 * received directory, index or offset array is checked before it is an address (the rows of load_item's item kinds): what
 * fails is not found.  The walk, both of its roads and the closed form for one-length coders are the caller's as they are */
__device__ __forceinline__ locate_position locate_item_position_of(const hufd_locate &loc, u64 i, u32 fixed_bits) {
    u64 item, s;
    if (loc.items == nullptr) { /* (the ends of ranges) */
        const hufd_item_symbol_range g = loc.item_ranges[i >> 1];
        item = g.item;
        s = g.first_symbol;
        if (i & 1u) {
            s += g.symbol_count;
            s = s < g.first_symbol ? ~0ull : s; /* (the sum overflows: past every item) */
        }
    } else {
        item = loc.items[i];
        s = loc.symbols[i];
    }
    locate_position p;
    p.bit = HUFD_NO_BIT;
    p.from = p.to = 0;
    p.k = 0;
    p.walk = 0;
    if (item >= loc.item_count) {
        return p;
    }
    const u64 first = loc.directory[2 * item], symbols = loc.directory[2 * item + 1], next = loc.directory[2 * item + 2];
    const u64 blocks = symbols / loc.block_symbols + (symbols % loc.block_symbols ? 1u : 0u);
    const u64 at = loc.offsets[item];
    u64 bytes;
    bool placed = true;
    if (loc.lengths) {
        bytes = loc.lengths[item];
    } else {
        const u64 behind = loc.offsets[item + 1];
        placed = behind >= at;
        bytes = behind - at;
    }
    if (next < first || next >= loc.index_entries || next - first != blocks || s > symbols || !placed || at > loc.encoded_length ||
        bytes > loc.encoded_length - at) {
        return p;
    }
    if (loc.stored) { /* (the same in every thread of the launch) */
        /* an item stored raw: a byte a symbol, a closed form like the one for coders of one code length -- no index entry and
         * no encoded byte is read; its packed length must be its symbols, and a flag that is neither 0 nor 1 is not found */
        const u32 flag = loc.stored[item];
        if (flag) {
            p.bit = flag == 1u && bytes == symbols ? 8 * (at + s) : HUFD_NO_BIT;
            return p;
        }
    }
    const u64 base = loc.index[first];
    const u64 b = s / loc.block_symbols;
    const u32 k = (u32)(s - b * loc.block_symbols);
    const u64 x0 = loc.index[first + b]; /* (s == symbols on a block's edge: b == blocks, the item's last entry) */
    if (x0 < base || (x0 - base + 7) / 8 > bytes) {
        return p;
    }
    const u64 from = 8 * at + (x0 - base);
    if (k == 0) {
        p.bit = from;
        return p;
    }
    const u64 x1 = loc.index[first + b + 1]; /* (k != 0: b < blocks) */
    if (x1 < x0 || (x1 - base + 7) / 8 > bytes) {
        return p;
    }
    const u64 to = 8 * at + (x1 - base);
    if (s == symbols) { /* the end of a ragged last block: the item's last entry */
        p.bit = to;
        return p;
    }
    if (fixed_bits) {
        const u64 bit = from + (u64)k * fixed_bits;
        p.bit = bit <= to ? bit : HUFD_NO_BIT;
        return p;
    }
    p.from = from;
    p.to = to;
    p.k = k;
    p.walk = 1;
    return p;
}

__device__ __forceinline__ locate_position locate_position_of(const hufd_locate &loc, u64 i, u32 fixed_bits) {
    if (loc.directory) { /* (the same in every thread of the launch) */
        return locate_item_position_of(loc, i, fixed_bits);
    }
    u64 s;
    if (loc.ranges) {
        const hufd_symbol_range g = loc.ranges[i >> 1];
        s = g.first_symbol;
        if (i & 1u) {
            s += g.symbol_count;
            s = s < g.first_symbol ? ~0ull : s; /* (the sum overflows: past every stream) */
        }
    } else {
        s = loc.symbols[i];
    }
    locate_position p;
    p.bit = HUFD_NO_BIT;
    p.from = p.to = 0;
    p.k = 0;
    p.walk = 0;
    if (s > loc.length) {
        return p;
    }
    if (s == loc.length) {
        p.bit = loc.index[loc.n_blocks];
        return p;
    }
    const u64 b = s / loc.block_symbols;
    const u32 k = (u32)(s - b * loc.block_symbols);
    const u64 from = loc.index[b];
    if (k == 0) {
        p.bit = from;
        return p;
    }
    const u64 to = loc.index[b + 1];
    if (to < from || to / 8 + (to % 8 ? 1 : 0) > loc.encoded_length) {
        return p;
    }
    if (fixed_bits) {
        const u64 at = from + (u64)k * fixed_bits;
        p.bit = at <= to ? at : HUFD_NO_BIT;
        return p;
    }
    p.from = from;
    p.to = to;
    p.k = k;
    p.walk = 1;
    return p;
}

__device__ __forceinline__ void locate_answer(const hufd_locate &loc, u64 i, u64 bit) {
    loc.bits[i] = bit;
    if (bit == HUFD_NO_BIT && loc.status) {
        atomicOr(loc.status, 1u);
    }
}

template <bool DEEP>
__device__ __forceinline__ void locate_body(const hufd_tables &tb, const hufd_locate &loc) {
    deep_shared &sh = *reinterpret_cast<deep_shared *>(dyn_lds);
    u32 *deep = reinterpret_cast<u32 *>(dyn_lds + sizeof(deep_shared));
    u16 *lut = reinterpret_cast<u16 *>(dyn_lds + sizeof(deep_shared));
    const u32 l = threadIdx.x, lanes = blockDim.x;
    locate_position p;
    u64 i;
    if (loc.coop) {
        /* (the same position in every lane: the workgroup leaves together) */
        i = loc.first + blockIdx.x;
        p = locate_position_of(loc, i, tb.fixed_bits);
        if (!p.walk || p.k <= loc.lone_symbols) {
            return;
        }
    }
    if (DEEP) {
        for (u32 e = l; e < tb.deep_entries; e += lanes) {
            deep[e] = tb.deep_lut[e];
        }
    } else {
        for (u32 e = l; e < (1u << tb.lut_bits); e += lanes) {
            lut[e] = tb.dec_lut[e];
        }
    }
    if (l == 0) {
        sh.stop_kind = lanes; /* (coop: the first lane whose settled walk stops) */
    }
    __syncthreads();
    if (!loc.coop) {
        i = loc.first + (u64)blockIdx.x * lanes + l;
        if (i >= loc.count) {
            return;
        }
        p = locate_position_of(loc, i, tb.fixed_bits);
        if (!p.walk) {
            locate_answer(loc, i, p.bit);
        } else if (p.k <= loc.lone_symbols) {
            const locate_walked r = locate_walk<DEEP>(deep, lut, tb.lut_bits, loc.encoded, p.to, p.from, p.to, p.k);
            locate_answer(loc, i, r.why == HUFD_STOP_NONE && r.count == p.k ? r.pos : HUFD_NO_BIT);
        }
        return;
    }
    const u8 *in = loc.encoded;
    const u64 rem = p.to;
    const u32 k = p.k;
    const u64 reach = 32ull * k + 1; /* code number k starts fewer than this many bits behind the span's first */
    const u64 cover = rem - p.from > reach ? p.from + reach : rem;
    const u64 first_byte = p.from / 8, bytes = cover / 8 + (cover % 8 ? 1 : 0) - first_byte;
    u64 lane_bytes = ((bytes + lanes - 1) / lanes + 7) & ~7ull;
    lane_bytes = lane_bytes < kLocateLaneMinBytes ? kLocateLaneMinBytes : lane_bytes;
    const u32 n_lanes = bytes ? (u32)((bytes + lane_bytes - 1) / lane_bytes) : 1u; /* (an empty span: lane 0 finds nothing) */
    const bool active = l < n_lanes;
    const u64 lane_from = (first_byte + (u64)l * lane_bytes) * 8, lane_to = lane_from + lane_bytes * 8;
    u32 start = l == 0 ? (u32)(p.from % 8) : 0u, my_exit = kDeepStop, my_count = 0;
    bool walk = active;
    if (active && l > 0) {
        /* the first guess: where a walk from anywhere over the bits in front of the lane (from the span's first bit, where
         * that is nearer: then it is no guess) crosses into it */
        const u64 back = lane_from - p.from < kLocateGuessBits ? p.from : lane_from - kLocateGuessBits;
        const locate_walked g = locate_walk<DEEP, true>(deep, lut, tb.lut_bits, in, rem, back, lane_from, ~0u);
        start = g.why == HUFD_STOP_NONE && g.pos >= lane_from ? (u32)(g.pos - lane_from) : 0u;
    }
    lane_memo memo;
    memo.clear();
    /* (as dec_wide_settle: a walk that stops says nothing to the lane behind it while entries are guesses -- under a coder
     * with windows without a code most walks from a wrong entry stop --; of the settled lanes the first that stops ends
     * the true path) */
    for (;;) {
        if (walk && !memo.find(start, my_exit, my_count)) {
            const locate_walked r = locate_walk<DEEP>(deep, lut, tb.lut_bits, in, rem, lane_from + start, lane_to, ~0u);
            /* (a walk the span's end stops in front of lane_to has no lane behind it: its exit is not looked at) */
            my_exit = r.why == HUFD_STOP_NONE ? (r.pos > lane_to ? (u32)(r.pos - lane_to) : 0u) : kDeepStop;
            my_count = r.count;
            memo.put(start, my_exit, my_count);
        }
        sh.exit_of[l] = active ? my_exit : kDeepStop;
        if (l == 0) {
            sh.changed = 0;
        }
        __syncthreads();
        walk = false;
        if (active && l > 0) {
            const u32 prev = sh.exit_of[l - 1];
            if (prev != kDeepStop && prev != start) {
                start = prev;
                walk = true;
                sh.changed = 1;
            }
        }
        __syncthreads();
        const bool again = sh.changed != 0;
        __syncthreads(); /* everyone has seen the flag and the exits before they are written again */
        if (!again) {
            break;
        }
    }
    if (active && my_exit == kDeepStop) {
        atomicMin(&sh.stop_kind, l); /* (the word holds the first lane that stops) */
    }
    __syncthreads();
    const bool reached = active && l <= sh.stop_kind;
    /* the codes in front of each lane: an exclusive scan of the counts of the lanes on the true path */
    const u32 mine = reached ? my_count : 0u;
    u32 total = 0;
    const u32 before = block_exclusive_sum<kDeepThreads>(mine, sh.scan, total); /* (a locate launch has kDeepThreads lanes) */
    if (mine && before <= k && k < before + mine) {
        /* (the one lane that holds code number k) */
        const locate_walked r = locate_walk<DEEP>(deep, lut, tb.lut_bits, in, rem, lane_from + start, lane_to, k - before);
        locate_answer(loc, i, r.pos);
    }
    if (total == k) {
        /* no lane holds it, and its k codes are whole: it starts where the true path's last walk ended -- at the window or the
         * cut code that stopped it, or on the span's last bit */
        if (reached && (my_exit == kDeepStop || l == n_lanes - 1)) {
            const locate_walked r = locate_walk<DEEP>(deep, lut, tb.lut_bits, in, rem, lane_from + start, lane_to, ~0u);
            locate_answer(loc, i, r.pos);
        }
    } else if (l == 0 && total < k) {
        locate_answer(loc, i, HUFD_NO_BIT); /* the true path stops in front of it */
    }
}
