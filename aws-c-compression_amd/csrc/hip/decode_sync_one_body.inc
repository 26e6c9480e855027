/*
 * The body of dec_sync_one for ONE chunk, as text: included into the kernels of decode_sync_kernels.hip that take such chunks
 * (dec_sync_one_kernel<.., TAIL>, and twice into dec_sync_one_mixed_kernel), each of which has, where it includes this,
 *   constexpr bool TAIL   -- a chunk its stream ends in;
 *   constexpr bool FOLLOW -- (TAIL only) the workgroup's first thread also follows the stream from where the last whole lane
 *                            leaves it to where it stops: dec_sync_tail's work for this chunk;
 *   const u32 c           -- the chunk;
 * the kernel's parameters under dec_sync_one_kernel's names, and `return` ending the kernel.
 * Text and not a function: the same lines as a __device__ function called from the kernels cost the compiler its grip on the
 * sub-chunk's words (it folds pairs of them into 8-byte loads of its own, re-loads them row by row, and spills 15 .. 34
 * vector registers at the 64 that eight waves a SIMD allow -- measured; as the kernel's own lines: 54, none).
 */

    static_assert(TAIL || !FOLLOW, "only a chunk its stream ends in has an end to follow");
    HUFD_STAMP(0, 0);
    one_shared<LB> &sh = *reinterpret_cast<one_shared<LB> *>(dyn_lds);
    const u32 ns = tb.n_states;
    const u32 lane = threadIdx.x;
    const hufd_chunk_rec rec = chunk_rec[c];
    const u64 valid = rec.valid;
    const u8 *src = d_in + rec.src_off;
    if (!TAIL && valid < (u64)HUFD_DEC_CHUNK_BYTES + 8u) {
        return; /* holds the end of its stream: the other instantiation's */
    }
    /* the lanes whose sub-chunk and the 8 bytes behind it lie inside the stream */
    const u32 n_full = !TAIL ? HUFD_DEC_LANES : (valid >= 8u ? (u32)((valid - 8u) / HUFD_DEC_SUB_BYTES) : 0u);
    const bool active = !TAIL || lane < n_full;
    if (TAIL && n_full == 0 && tb.lut_bits <= HUFD_DEC_MAX_LUT_BITS) {
        if (lane == 0) {
            chunk_regular[c] = 3; /* fewer than 136 bytes: one thread's work in dec_sync_tail / dec_emit_tail */
        }
        if (FOLLOW) {
            /* ... dec_sync_tail's, done here: the chunk's whole transfer function, a walk an entry state (one, the item's
             * first bit, where the chunk is the item's first) */
            u16 *lut = reinterpret_cast<u16 *>(sh.wlut);
            for (u32 i = lane; i < (1u << tb.lut_bits); i += HUFD_DEC_LANES) {
                lut[i] = tb.dec_lut[i];
            }
            __syncthreads();
            if (lane == 0) {
                u32 *tiny = sh.tiny;
                load_be32_run(tiny, src, valid, kTailWords);
                const bool only = rec.entry_bit != HUFD_NONE32;
                for (u32 st = only ? rec.entry_bit : 0u; st < (only ? rec.entry_bit + 1u : ns); ++st) {
                    u32 stop_pos = 0, stop_why = 0;
                    const tail_walk tw = tail_follow(tiny, lut, tb.lut_bits, st, (u32)(valid * 8), 2 * HUFD_DEC_SUB_BITS, nullptr, &stop_pos, &stop_why);
                    chunk_fn[(u64)c * ns + st] = wide_pack(true, 0, tw.count[0] + tw.count[1]); /* the stream ends here whatever the entry */
                }
            }
        }
        return;
    }
    const one_walk ow(LB);
    u32 table = lds_offset_of(sh.wlut);
    opaque(table); /* (in a register of its own: a constant the compiler knows it writes anew in front of every row's loop) */
    const bool eligible = n_full >= 1 && tb.lut_bits <= LB && tb.max_bits <= HUFD_DEC_MAX_LUT_BITS &&
                          row_walk(LB, tb.max_bits).sure >= SURE && (table & ((4u << LB) - 1u)) == 0;
    if (!eligible) {
        if (lane == 0) {
            chunk_regular[c] = 0;
            long_list[atomicAdd(long_count, 1u)] = c;
        }
        return;
    }
    constexpr u32 kLutPerLane = (1u << LB) / HUFD_DEC_LANES, kLutBatch = 4;
    const auto table_share = [&](u32 j0) {
        u32 lut_raw[kLutBatch];
#pragma unroll
        for (u32 j = 0; j < kLutBatch; ++j) {
            lut_raw[j] = tb.dec_lut[(lane + (j0 + j) * HUFD_DEC_LANES) >> (LB - tb.lut_bits)];
        }
#pragma unroll
        for (u32 j = 0; j < kLutBatch; ++j) {
            sh.wlut[lane + (j0 + j) * HUFD_DEC_LANES] = one_walk::entry_of(lut_raw[j] & 0xFFu);
        }
    };
    if (TAIL && lane >= kWave && (lane & ~(kWave - 1)) >= n_full) {
        /* a wave wholly behind the stream's whole lanes: its share of the table done, it leaves: the barriers below count the waves that are still there */
#pragma unroll
        for (u32 j0 = 0; j0 < kLutPerLane; j0 += kLutBatch) {
            table_share(j0);
        }
        /* (FOLLOW: the records of the one or two lanes the stream ends in are the following thread's to write) */
        if (!FOLLOW || (lane != n_full && lane != n_full + 1)) {
            lane_rec_store(lane_rec, c, lane, lane_rec_unreached());
        }
        return;
    }
    u32 w[kFastRows];
    {
        /* (TAIL: a lane behind the stream's whole lanes reads sub-chunk 0 again: words that are codes, never looked at) */
        const u32 mine = active ? lane : 0u;
        const unaligned_uint4 *line = reinterpret_cast<const unaligned_uint4 *>(src + (u64)mine * HUFD_DEC_SUB_BYTES);
#pragma unroll
        for (u32 q = 0; q < kSubWords / 4; ++q) {
            const unaligned_uint4 v = line[q];
            w[4 * q + 0] = v.x;
            w[4 * q + 1] = v.y;
            w[4 * q + 2] = v.z;
            w[4 * q + 3] = v.w;
        }
        w[kSubWords] = reinterpret_cast<const unaligned_u32 *>(src + (u64)(mine + 1) * HUFD_DEC_SUB_BYTES)->x;
    }
#pragma unroll
    for (u32 j0 = 0; j0 < kLutPerLane; j0 += kLutBatch) {
        table_share(j0);
    }
    if (lane == 0) {
        sh.bad = 0;
        sh.decided0 = 0;
        sh.moved = 0;
        sh.bad_mine = 0;
#pragma unroll
        for (u32 wv = 0; wv < HUFD_DEC_LANES / kWave; ++wv) {
            sh.wave_sum[wv] = 0; /* (TAIL: of the waves that have left) */
        }
    }
    /* the words as the rows take them (one_walk::shifted): from the last one down, each from its own bytes swapped and those of
     * the word in front of it; nothing in front of the sub-chunk's first word is ever looked at */
    {
        u32 behind = __builtin_bswap32(w[kFastRows - 1]);
#pragma unroll
        for (u32 r = kFastRows - 1; r >= 1; --r) {
            const u32 front = __builtin_bswap32(w[r - 1]);
            w[r] = one_walk::shifted<LB>(front, behind);
            behind = front;
        }
        w[0] = one_walk::shifted<LB>(0u, behind);
    }
    if (lane == 0) {
#pragma unroll
        for (u32 r = 0; r <= kOneMaxMerge0; ++r) {
            sh.sub0[r] = w[r]; /* (sub-chunk 0's, for the threads that try its entry states) */
        }
    }
    __syncthreads();
    HUFD_STAMP(0, 1);
    HUFD_STAMP(0, 2);

    /* the guessed walk's states at the kept boundaries: in registers (48 + 12 of 64 -- since the rows go through a funnel shift and
     * need no register pair put together, the chunks streams end in have them to spare too: 55; in LDS they cost that
     * instantiation two dozen LDS instructions a lane, 4 us of config 4's 0.54 ms) */
    u32 kept_r[kOneRecs + kQuarters - 1];
#pragma unroll
    for (u32 q = 0; q < kOneRecs + kQuarters - 1; ++q) {
        kept_r[q] = 0;
    }
    auto kept_set = [&](u32 q, u32 v) { kept_r[q] = v; };
    auto kept_get = [&](u32 q) -> u32 { return kept_r[q]; };

    /* R: one walk from bit 0, a guess, over the whole sub-chunk; its state kept at a few row boundaries */
    u32 state = ow.state_at(0);
    bool hopeless = false; /* (the same for the wave) */
#pragma unroll
    for (u32 r = 0; r < kSubWords; ++r) {
        if (!hopeless) {
            if (one_rec_index(r) < kOneRecs) {
                kept_set(one_rec_index(r), state);
            }
            if (r != 0 && r % (kSubWords / kQuarters) == 0) {
                kept_set(kOneRecs + r / (kSubWords / kQuarters) - 1, state);
            }
            state = ow.template row<SURE>(state, w[r], w[r + 1], table) + 32u;
            if (r + 1 == kOneGarbageRow) {
                /* dozens of windows without a code in four rows: bytes that are no stream of this coder (a walk over them
                 * steps a bit at a time) -- the long way says where the first one is */
                hopeless = __any(active && one_walk::dead_of(state) > kOneGarbageDead);
            }
        }
    }
    const u32 last = state;
    kept_set(kOneRecs - 1, last); /* (the boundary behind the last row: the sub-chunk's end) */
    if (lane == 0) {
        sh.last0 = last; /* (what the candidates of sub-chunk 0 ask of lane 0's walk) */
    }
    u32 ref_exit = ow.offset_of(last); /* (how the lane leaves: the guessed walk's way, unless the true walk never met it) */
    bool ok = !hopeless; /* what speaks against the chunk whatever its lanes' entries are ... */
    bool ok_mine = !active || ref_exit < ns; /* ... and what may change for a lane when the lane in front of it leaves another way */
    sh.exit_state[lane] = ref_exit;
    HUFD_STAMP(0, 3);
    __syncthreads();
    HUFD_STAMP(0, 4);

    /* H: my own sub-chunk from my true entry state, until I stand where my guessed walk stood */
    u32 entry = lane ? sh.exit_state[lane - 1] : 0u;
    u32 count = 0, meet_row = 0;
    u32 head_cp[kQuarters - 1] = {0, 0, 0}; /* the walk from the true entry where it enters the second, third and fourth quarter */
    {
        u32 st = ow.state_at(entry < ns ? entry : 0u);
        bool met = !active || lane == 0; /* (lane 0's entry is only known to dec_scan: the candidates below) */
        u32 h_at = 0, r_at = 0;
        bool done = false; /* (the same for the wave) */
        constexpr u32 kInRegisters = 24; /* the rows H walks out of the lane's registers: behind them the words come from memory again */
#pragma unroll
        for (u32 r = 0; r <= kInRegisters; ++r) {
            if (!done && !hopeless) {
                if (r != 0 && r % (kSubWords / kQuarters) == 0) {
                    head_cp[r / (kSubWords / kQuarters) - 1] = st;
                }
                if (one_rec_index(r) < kOneRecs) {
                    const u32 there = kept_get(one_rec_index(r));
                    if (!met && ((st ^ there) & one_walk::kPos) == 0) {
                        met = true;
                        h_at = st;
                        r_at = there;
                        meet_row = r;
                    }
                    done = __all(met);
                    if (one_rec_index(r) == 0) {
                        if (!done) {
                            /* most of the wave's lanes still apart after six rows: a stream whose walks do not fall into step
                             * (one symbol over and over) -- no regular chunk, and no more rows spent on finding that out */
                            hopeless = __popcll(__ballot(!met)) > kWave - kWave / 8;
                        }
                    }
                }
                if (r < kInRegisters) {
                    if (!done && !hopeless) {
                        st = ow.template row<SURE>(st, w[r], w[r + 1], table) + 32u;
                    }
                }
            }
        }
        if (!done && !hopeless) {
            /* rare (a wave in a hundred): a lane still apart from its guessed walk after 24 rows.  On to the sub-chunk's end,
             * the words from memory (kept in registers for this they cost the kernel its eight waves a SIMD); a walk that
             * has covered the whole sub-chunk from the true entry needs the guessed one only to leave the same way. */
            const u8 *mine = src + (u64)(active ? lane : 0u) * HUFD_DEC_SUB_BYTES;
            u32 word = __builtin_bswap32(reinterpret_cast<const unaligned_u32 *>(mine + 4 * kInRegisters)->x);
            u32 hi = one_walk::shifted<LB>(__builtin_bswap32(reinterpret_cast<const unaligned_u32 *>(mine + 4 * (kInRegisters - 1))->x), word);
            for (u32 r = kInRegisters; r < kSubWords && !done; ++r) {
                const u32 next = __builtin_bswap32(reinterpret_cast<const unaligned_u32 *>(mine + 4 * (r + 1))->x);
                const u32 lo = one_walk::shifted<LB>(word, next);
                word = next;
                st = ow.template row<0>(st, hi, lo, table) + 32u;
                hi = lo;
                if (r + 1 == one_rec_row(kOneRecs - 2) || r + 1 == one_rec_row(kOneRecs - 1)) {
                    const u32 there = r + 1 == one_rec_row(kOneRecs - 2) ? kept_get(kOneRecs - 2) : kept_get(kOneRecs - 1);
                    if (!met && ((st ^ there) & one_walk::kPos) == 0) {
                        met = true;
                        h_at = st;
                        r_at = there;
                        meet_row = r + 1;
                    }
                    done = __all(met);
                }
            }
        }
        if (active && lane && !hopeless && !met && entry < ns) {
            /* Never met (a lane in some hundred thousand; the loop above has then run to the sub-chunk's end): the walk from
             * the true entry has covered the whole sub-chunk -- the records are all its own, and it leaves as IT does, which
             * is not how the lane behind this one thought: that one walks again below (a chunk given up for this cost the
             * launches behind this kernel 30 us of dec_sync_guess, for two dozen chunks of the 1 GiB stream). */
            met = true;
            h_at = st;
            r_at = last;
            meet_row = kSubWords;
            ref_exit = ow.offset_of(st);
            sh.exit_state[lane] = ref_exit; /* (read again behind the next barrier only) */
            sh.moved = 1;
        }
        if (active && lane) {
            /* met, no window without a code on the true path (H's part, R's part), my entry a state, my exit too */
            ok_mine = !hopeless && met && entry < ns && ref_exit < ns && one_walk::dead_of(h_at) == 0 &&
                      one_walk::dead_of(last) == one_walk::dead_of(r_at);
            count = one_walk::count_of(h_at) + one_walk::count_of(last) - one_walk::count_of(r_at);
        }
    }

    HUFD_STAMP(0, 7);
    /* What every wave has to say is said here, IN FRONT of the walks of sub-chunk 0's candidates, which are wave 0's alone
     * and the tail of a workgroup's life (a seventh of it): the other waves used to stand at the barrier behind those walks.
     * Now they leave their records and go -- their wave slots are the next workgroup's that much earlier.  (Records of a
     * chunk that wave 0 then finds irregular are never looked at: chunk_regular says so, and the kernels that take the
     * chunk write them again.  When a lane's exit moved -- rare -- everybody stays for the rounds below.) */
    {
        const u32 wsum0 = wave_sum(lane ? count : 0u);
        if ((lane & (kWave - 1)) == 0) {
            sh.wave_sum[lane / kWave] = wsum0;
        }
        if (!ok) {
            sh.bad = 1;
        }
        if (!ok_mine) {
            sh.bad_mine = 1;
        }
    }
    __syncthreads();
    const bool stay = sh.moved != 0; /* (the same for the workgroup) */
    /* my sub-chunk's record, one store: the checkpoints, how the lane is entered and left, its symbols */
    auto lane_record = [&](u32 merged, u32 symbols) {
        if (active) {
            u32 cps[kQuarters - 1];
#pragma unroll
            for (u32 qq = 0; qq + 1 < kQuarters; ++qq) {
                /* a checkpoint in front of the meeting row is not on the guessed walk's true part: it is taken from the walk
                 * from the true entry, which passed it (not for lane 0, whose true entry is only known to dec_scan: its first
                 * checkpoint may be missing, dec_emit_fast walks on through that quarter) */
                const u32 boundary = (qq + 1) * (kSubWords / kQuarters);
                bool have = boundary >= meet_row;
                const u32 at_boundary = kept_get(kOneRecs + qq);
                u32 tail = one_walk::count_of(last) - one_walk::count_of(at_boundary), bits = ow.offset_of(at_boundary);
                if (!have && lane != 0) {
                    tail = count - one_walk::count_of(head_cp[qq]);
                    bits = ow.offset_of(head_cp[qq]);
                    have = true;
                }
                cps[qq] = have ? 0x8000u | (bits << 11) | tail : 0u;
            }
            lane_rec_store(lane_rec, c, lane, lane_rec_pack(cps[0], cps[1], cps[2], merged, symbols));
        } else if (!FOLLOW || (lane != n_full && lane != n_full + 1)) {
            /* (TAIL) behind the whole lanes, in a wave that has some: as for the waves that left */
            lane_rec_store(lane_rec, c, lane, lane_rec_unreached());
        }
        if (TAIL && lane + 1 == n_full) {
            tail_entry[c] = ref_exit;
        }
    };
    if (!stay && lane >= kWave) {
        if (!sh.bad && !sh.bad_mine) {
            lane_record((1u << entry) | (ref_exit << 12), count);
        }
        return;
    }
    /* H: sub-chunk 0 from every entry state the chunk may be entered in (threads 0 .. ns-1): each dies at a window without a
     * code (the count up to there has to be right) or meets lane 0's guessed walk -- which the wave's last thread walks
     * AGAIN beside them, a row at a time, so that they can meet it at any row boundary (two rows on average; met at the
     * kept boundaries only, every candidate walked six rows at least, and these walks are the tail of the workgroup's
     * life: the other waves wait for them) */
    u32 cand_count = 0, cand_dead = 0, meet_row0 = 0, ref_count0 = 0;
    bool cand_reached = false;
    u64 cand_alive = 0;
    if (lane < kWave) {
        constexpr u32 kTwin = kWave - 1;
        const bool twin = lane == kTwin;
        const u32 last0 = sh.last0;
        u32 st = ow.state_at(lane < ns ? lane : 0u);
        /* (an item's first chunk is only ever entered at the item's first bit: one candidate, not ns -- every chunk of
         * BASELINE configs[3]; the other states' entries of the chunk function are never asked for) */
        const u32 only = rec.entry_bit; /* (a scalar: the record is the same for the workgroup) */
        bool dd = only == HUFD_NONE32 ? lane >= ns : lane != only, met = false;
        u32 c_at = 0, r_at = 0;
        u32 at0 = st, latest = 0; /* lane 0's walk where the last candidate met it, and the row (the same in every thread) */
        u32 hi = sh.sub0[0];
        for (u32 r = 0; !hopeless; ++r) {
            /* (lane 0's walk started on a guess: while it is on a wrong phase it may step over a window without a code.  A
             * candidate that stands where that walk stands IN FRONT of such a window does not join it: it walks on by
             * itself, the same way, and dies at that window with the count that is right) */
            const u32 there = __shfl(st, kTwin);
            const bool now = !twin && !dd && !met && ((st ^ there) & one_walk::kPos) == 0 && one_walk::dead_of(last0) == one_walk::dead_of(there);
            if (now) {
                met = true;
                c_at = st;
                r_at = there;
            }
            if (__any(now)) {
                at0 = there;
                latest = r;
            }
            if (__all(dd || met || twin) || r == kSubWords) {
                break;
            }
            const u32 lo = sh.sub0[r + 1];
            if (twin) {
                st = ow.template row<SURE>(st, hi, lo, table); /* (as phase R took the row: the marks are part of the state) */
            } else if (!dd && !met) {
                /* the row as the other walks take it; a window without a code in it (a walk on a wrong phase: within a
                 * row or two) and the row is taken again, step by step, for the count up to that window */
                const u32 before = st;
                st = ow.template row<SURE>(st, hi, lo, table);
                if (one_walk::dead_of(st)) {
                    st = before;
                    for (;;) {
                        const u32 e = ow.look(st, hi, lo, table);
                        if (e == one_walk::entry_of(0)) {
                            break;
                        }
                        st += e;
                    }
                    dd = true;
                    cand_dead = one_walk::count_of(st); /* (the step that found no code is not a symbol) */
                }
            }
            st += 32u;
            hi = lo;
        }
        const bool decided = !hopeless && __all(dd || met || twin);
        cand_reached = met && lane < ns;
        cand_alive = __ballot(cand_reached);
        /* where the last of them met it: from that row on lane 0's walk is the true one whatever the chunk's entry */
        meet_row0 = latest;
        cand_count = one_walk::count_of(c_at) + one_walk::count_of(last0) - one_walk::count_of(r_at);
        if (lane == 0) {
            sh.decided0 = decided;
        }
        ok = ok && decided && cand_alive != 0;
        if (lane == 0) {
            meet_row = meet_row0;
            ref_count0 = one_walk::count_of(last0) - one_walk::count_of(at0);
        }
    }

    HUFD_STAMP(0, 5);
    if (!ok) {
        sh.bad = 1; /* (wave 0: what the candidates' walks said) */
    }
    if (stay) {
        __syncthreads(); /* (everybody is still here) */
    }
    if (!stay && sh.bad_mine) {
        sh.bad = 1; /* (every thread that gets here writes the same) */
    }
    if (stay && !sh.bad) {
        /* Rare.  A lane's exit moved: the lane behind it walks its sub-chunk again from the entry that is now known, the
         * words from memory, until it stands where its guessed walk stood -- or to the end, and then ITS exit may move.
         * A few rounds of that, one lane at work in each; a chunk that is not settled by then is not regular. */
        constexpr u32 kRounds = 4;
        u32 round = 0;
        for (; round < kRounds; ++round) {
            __syncthreads(); /* (everybody has read `moved`) */
            if (lane == 0) {
                sh.moved = 0;
            }
            __syncthreads();
            const u32 entry_now = lane ? sh.exit_state[lane - 1] : 0u;
            if (active && lane && entry_now != entry) {
                entry = entry_now;
                bool fine = entry < ns;
                if (fine) {
                    const u8 *mine = src + (u64)lane * HUFD_DEC_SUB_BYTES;
                    u32 st = ow.state_at(entry), h_at = 0, r_at = 0;
                    bool met = false;
                    u32 word = __builtin_bswap32(reinterpret_cast<const unaligned_u32 *>(mine)->x);
                    u32 hi = one_walk::shifted<LB>(0u, word);
                    for (u32 r = 0;; ++r) {
#pragma unroll
                        for (u32 qq = 0; qq + 1 < kQuarters; ++qq) {
                            head_cp[qq] = r == (qq + 1) * (kSubWords / kQuarters) ? st : head_cp[qq];
                        }
                        const u32 j = one_rec_index(r);
                        u32 there = 0;
#pragma unroll
                        for (u32 q = 0; q < kOneRecs; ++q) {
                            there = j == q ? kept_get(q) : there;
                        }
                        if (j < kOneRecs && ((st ^ there) & one_walk::kPos) == 0) {
                            met = true;
                            h_at = st;
                            r_at = there;
                            meet_row = r;
                        }
                        if (met || r == kSubWords) {
                            break;
                        }
                        const u32 next = __builtin_bswap32(reinterpret_cast<const unaligned_u32 *>(mine + 4 * (r + 1))->x);
                        const u32 lo = one_walk::shifted<LB>(word, next);
                        word = next;
                        st = ow.template row<0>(st, hi, lo, table) + 32u;
                        hi = lo;
                    }
                    if (!met) {
                        h_at = st;
                        r_at = last;
                        meet_row = kSubWords;
                    }
                    const u32 exit_now = met ? ow.offset_of(last) : ow.offset_of(st);
                    if (exit_now != ref_exit) {
                        ref_exit = exit_now;
                        sh.exit_state[lane] = exit_now;
                        sh.moved = 1;
                    }
                    fine = ref_exit < ns && one_walk::dead_of(h_at) == 0 && one_walk::dead_of(last) == one_walk::dead_of(r_at);
                    count = one_walk::count_of(h_at) + one_walk::count_of(last) - one_walk::count_of(r_at);
                }
                ok_mine = fine;
            }
            __syncthreads();
            if (!sh.moved) {
                break;
            }
        }
        if (round == kRounds || !ok_mine) {
            sh.bad = 1; /* (a lane whose first walk went wrong on a wrong entry and was never asked to walk again: its entry stood) */
        }
        const u32 wsum_now = wave_sum(lane ? count : 0u);
        if ((lane & (kWave - 1)) == 0) {
            sh.wave_sum[lane / kWave] = wsum_now;
        }
        __syncthreads();
    }
    if (sh.bad) {
        if (lane == 0) {
            chunk_regular[c] = 0;
            if (TAIL || !sh.decided0) {
                long_list[atomicAdd(long_count, 1u)] = c;
            } else {
                slow_list[atomicAdd(slow_count, 1u)] = c;
            }
        }
        return;
    }

    /* the tables dec_scan and dec_emit read (the regular chunks' format) */
    u16 *fn_out = fn_tab + (u64)c * ns * HUFD_DEC_LANES;
    /* (lane 0: its symbols from where its walk is the true one, and the entry states that get there) */
    lane_record((lane ? 1u << entry : (u32)cand_alive) | (ref_exit << 12), lane ? count : ref_count0);
    if (lane == 0) {
        chunk_regular[c] = TAIL ? 2 : 1;
    }
    /* FOLLOW: the stream's last symbols, from where the last whole lane leaves it to where it stops -- what dec_sync_tail
     * does for such a chunk, a thread of its own, in a kernel of its own behind this one: here by the workgroup's first
     * thread (~100 dependent steps; a launch folds a FEW such chunks in among many inside streams, and their workgroups
     * are the grid's first).  Wave 0 is the only one left (or everybody is through with the walk table): the decode
     * table and the stream's last words take the table's place. */
    u32 follow_exit = 0, follow_count = 0, follow_stop = 2;
    if (FOLLOW && lane < kWave) {
        u16 *lut = reinterpret_cast<u16 *>(sh.wlut);
        u32 *words = sh.wlut + (1u << LB) / 2; /* (behind the 2-byte entries) */
        const u32 entry_t = sh.exit_state[n_full - 1];
        wave_step(); /* (the walk table is overwritten: nobody of this wave reads it any more) */
        for (u32 i = lane; i < (1u << tb.lut_bits); i += kWave) {
            lut[i] = tb.dec_lut[i];
        }
        tail_walk tw = {{0, 0}, 0, 2};
        if (lane == 0) {
            const u8 *tsrc = src + (u64)n_full * HUFD_DEC_SUB_BYTES;
            const u64 tail_bytes = valid - (u64)n_full * HUFD_DEC_SUB_BYTES; /* 8 .. 135 */
            load_be32_run(words, tsrc, tail_bytes, kTailWords);
        }
        wave_step();
        if (lane == 0) {
            const u64 tail_bytes = valid - (u64)n_full * HUFD_DEC_SUB_BYTES;
            const u32 limit = (n_full + 1 < HUFD_DEC_LANES ? 2u : 1u) * HUFD_DEC_SUB_BITS; /* the last lane's walk ends with the chunk */
            u32 stop_pos = 0, stop_why = 0;
            tw = tail_follow(words, lut, tb.lut_bits, entry_t, (u32)(tail_bytes * 8), limit, nullptr, &stop_pos, &stop_why);
            /* the records of the one or two lanes the true path gets to; a lane it does not get to: nothing in it */
            for (u32 k = 0; k < 2; ++k) {
                const u32 ln = n_full + k;
                if (ln >= HUFD_DEC_LANES) {
                    break;
                }
                const bool reached = k == 0 || tw.stop != 0;
                if (reached) {
                    const u32 my_entry = k == 0 ? entry_t : tw.exit;
                    const bool stops_here = tw.stop == k;
                    fn_out[(u64)my_entry * HUFD_DEC_LANES + ln] =
                        stops_here ? fn_pack(true, 0, tw.count[k] & 0x7FFu) : fn_pack(false, tw.exit, tw.count[k] & 0x7FFu);
                    lane_rec_store(lane_rec, c, ln, lane_rec_pack(0, 0, 0, (1u << my_entry) | ((stops_here ? kExitStop : tw.exit) << 12), tw.count[k]));
                } else {
                    lane_rec_store(lane_rec, c, ln, lane_rec_unreached());
                }
            }
        }
        follow_exit = __shfl(tw.exit, 0);
        follow_count = __shfl(tw.count[0] + tw.count[1], 0);
        follow_stop = __shfl(tw.stop, 0);
    }
    if (lane < ns) {
        u32 rest = 0;
#pragma unroll
        for (u32 wv = 0; wv < HUFD_DEC_LANES / kWave; ++wv) {
            rest += sh.wave_sum[wv];
        }
        const u32 first_exit = sh.exit_state[0];
        const u32 last_exit = sh.exit_state[HUFD_DEC_LANES - 1];
        fn_out[(u64)lane * HUFD_DEC_LANES] =
            cand_reached ? fn_pack(false, first_exit, cand_count & 0x7FFu) : fn_pack(true, 0, cand_dead);
        /* (TAIL: symbols of the whole lanes only, and no exit yet: dec_sync_tail adds the stream's last symbols and how it ends
         * -- FOLLOW: added here, every walk that gets through sub-chunk 0 goes on to the end of the stream) */
        const bool stops = follow_stop != 2u;
        chunk_fn[(u64)c * ns + lane] =
            cand_reached ? (FOLLOW ? wide_pack(stops, stops ? 0u : follow_exit, cand_count + rest + follow_count)
                                   : wide_pack(false, TAIL ? 0u : last_exit, cand_count + rest))
                         : wide_pack(true, 0, cand_dead);
    }
    HUFD_STAMP(0, 6);
