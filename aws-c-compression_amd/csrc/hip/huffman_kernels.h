#ifndef HUFFMAN_AMD_KERNELS_H
#define HUFFMAN_AMD_KERNELS_H
/*
 * C interface of the kernel file: argument packs and launch wrappers.  The
 * pointers are device pointers; the launches are asynchronous on `stream`
 * (a hipStream_t carried as void *).  Return value: 0 or a hipError_t.
 */
#include <stdint.h>

#include "device_types.h"

#ifdef __cplusplus
extern "C" {
#endif

struct hufk_encode_args {
    struct hufd_tables tables;
    const struct hufd_enc_item *items;
    uint32_t n_items;
    const struct hufd_enc_seg *segs; /* [n_segs] */
    uint32_t n_segs;
    const uint32_t *large_items; /* [n_large] items with more than HUFD_SCAN_SMALL_MAX segments */
    uint32_t n_large;
    const uint32_t *tiny_items;  /* [n_tiny] items of at most HUFD_ENC_TINY_BYTES symbols: no segments, one thread each */
    uint32_t n_tiny;
    const uint32_t *solo_items;  /* [n_solo] items of one tile at most (hufd_enc_item.tiny == 2): no segments, one wave each */
    uint32_t n_solo;
    uint32_t length_only; /* stop after the scan */
    const void *d_in;
    void *d_out;
    uint32_t *seg_bits;   /* [n_segs] scratch */
    uint32_t *wave_bits;  /* [n_segs][4] scratch: bits of each quarter (4 KiB of symbols) of a segment */
    uint32_t *seg_unk;    /* [n_segs] scratch */
    uint64_t *seg_bitoff; /* [n_segs] scratch */
    uint32_t *careful_list;  /* [2 * n_items] scratch: segments for the per-symbol packer */
    uint32_t *careful_count; /* [1] scratch */
    /* one-pass path (every symbol coded, codes of 4 .. 15 bits): */
    void *zero_block;        /* hufk_encode_zero_bytes(n_segs, n_items) bytes, clear when the launch starts and when it is
                              * through: the control words (word 0 the way back's tickets, word 1 "a wait ran out", word 2
                              * careful_count, word 4 word 1 of the last launch), then the look-back tables, twice */
    uint32_t zero_is_clear;  /* 1: the block is known to be clear (the plan's last launch left it so); 0: the launch clears it first */
    uint64_t zero_bytes;     /* all of the block (what a clearing takes when the layout of the launch that dirtied it is not known) */
    uint8_t *seg_unk_seen;   /* [n_segs] scratch */
    uint64_t *item_total;    /* [n_items] scratch */
    uint32_t single_pass;    /* 1: one kernel reads the symbols once (enc_onepass) instead of count / scan / pack */
    uint32_t fail_tile;      /* 1: a wave of enc_onepass is made to give up (the way back, for tests: aws_huffman_amd_testing_set_encode_road) */
    struct hufd_enc_item_state *states; /* [n_items] scratch */
    struct hufd_enc_result *results;    /* [n_items] */
    void **stage_events; /* NULL, or 4 hipEvent_t: before count, after count, after scan, after pack */
};

struct hufk_wide_item {
    uint32_t slot;         /* of the item's index in deep_items */
    uint32_t n_blocks;     /* 32 KiB blocks (HUFD_WIDE_BLOCK_BYTES) */
    uint64_t block_offset; /* of its scratch in wide_block */
};

/* hufk_decode_args.counters: */
#define HUFK_DEC_COUNT_SLOW 0u      /* slow_list: the chunks dec_sync_one / dec_sync_pack leave to dec_sync_guess (or, without one, to dec_sync) */
#define HUFK_DEC_COUNT_LONG 1u      /* emit_list: the chunks for the long way (dec_sync_few's and dec_sync's list) */
#define HUFK_DEC_COUNT_FEW 2u       /* slow_list again: dec_sync_few's chunks, for dec_sync_true */
#define HUFK_DEC_COUNT_EMIT 3u      /* emit_list again: the chunks dec_emit_fast leaves to dec_emit */
#define HUFK_DEC_COUNT_DENSE 4u     /* dense_list */
#define HUFK_DEC_COUNTERS 8u

struct hufk_decode_args {
    struct hufd_tables tables;
    const struct hufd_dec_item *items;
    uint32_t n_items;
    const uint32_t *chunk_item; /* [n_chunks] */
    uint32_t n_chunks;
    const uint32_t *tail_chunks; /* [n_tail] chunks with fewer than HUFD_DEC_CHUNK_BYTES + 8 bytes of their item left: the end of a stream is in them */
    uint32_t n_tail;
    const uint32_t *tiny_items;  /* [n_tiny] items of at most HUFD_DEC_TINY_BYTES encoded bytes: no chunks, one thread each */
    uint32_t n_tiny;
    const uint32_t *deep_items;  /* [n_deep] longer items of a coder with codes of more than HUFD_DEC_MAX_LUT_BITS bits: no chunks, one workgroup each */
    uint32_t n_deep;
    /* the deep items of at least wide_from bytes: every 32 KiB block of one is a workgroup's (dec_wide_*) */
    const struct hufk_wide_item *wide; /* [n_wide], HOST memory */
    uint32_t n_wide;
    uint64_t wide_from;
    void *wide_block; /* scratch: hufk_decode_wide_bytes(blocks) each, at the offsets in `wide` */
    uint32_t wide_fails; /* 1: they give up (tests of the way back); 2: and dec_wide_fn_* behind them as well */
    uint32_t few_walks;  /* 1: the chunks inside streams whose walks do not fall into step go to dec_sync_few / dec_sync_true; 0: the long way */
    /* a coder with codes of one length (tables.fixed_bits): its items beyond a thread's work, 16 KiB blocks of them */
    const uint32_t *fixed_blocks; /* [n_fixed_blocks][2]: item, block of HUFD_FIXED_BLOCK_BYTES inside it */
    uint32_t n_fixed_blocks;
    const uint32_t *large_items; /* per item with more than HUFD_SCAN_SMALL_MAX chunks: item index, its first run */
    uint32_t n_large;
    const uint32_t *runs;        /* per run of HUFD_SCAN_RUN_CHUNKS chunks of a large item: item index, run number */
    uint32_t n_runs;
    uint32_t *run_fn;            /* [n_runs][n_states] scratch */
    const void *d_in;
    void *d_out;
    uint16_t *fn_tab;      /* [n_chunks][n_states][HUFD_DEC_LANES] scratch */
    struct hufd_lane_rec *lane_rec; /* [n_chunks][HUFD_DEC_LANES] scratch: a sub-chunk's walk checkpoints, merged-state word and symbols */
    uint32_t *chunk_fn;    /* [n_chunks][n_states] scratch */
    uint32_t *slow_list;   /* [n_chunks] scratch: chunks that take the long way through dec_sync */
    uint32_t *emit_list;   /* [n_chunks] scratch: chunks left to dec_emit by dec_emit_fast */
    uint32_t *dense_list;  /* [n_chunks] scratch: chunks dec_emit_fast leaves to dec_emit_dense */
    uint32_t *counters;    /* [HUFK_DEC_COUNTERS] scratch: how many entries the lists hold, one word for every use a launch
                            * makes of a list (the arrays take turns, the words do not).  Clear when the plan gets them, and
                            * every launch leaves them as it needs them itself (so that a launch captured in a graph can be
                            * replayed): the sync stage's words are cleared by the launch's LAST kernel (dec_emit, the long
                            * way: nobody reads them behind the sync stage), the emit stage's by the last kernel of the
                            * sync stage (dec_sync, the long way: nobody has touched them yet) -- both run in every launch
                            * with chunks.  A clearing command in front of every launch was ~4 us of its own. */
    uint32_t counters_self_cleared; /* 1: as above; 0: cleared by a command in front of the launch */
    uint32_t *summary;       /* NULL, or [HUFK_DEC_COUNTERS]: the launch's last kernel leaves its counters here (in front of the
                              * result records: one copy fetches both) -- what the host reads `quiet` from */
    uint32_t quiet;          /* 1: the plan's last fetched launch listed no chunk for any kernel but the regular ones: this
                              * launch goes without the kernels that only make listed chunks FASTER (dec_sync_guess, _few,
                              * _true, dec_emit_big -- an empty launch is ~4 us each); whatever is listed takes the long way
                              * (dec_sync, dec_emit: exact for every chunk), and the counters say so at the next fetch */
    uint8_t *chunk_regular; /* [n_chunks] scratch */
    uint32_t *tail_entry;   /* [n_chunks] scratch: state in which the last whole lane of an end-of-stream chunk leaves */
    uint32_t *chunk_entry; /* [n_chunks] scratch */
    uint64_t *chunk_base;  /* [n_chunks] scratch */
    struct hufd_emit_rec *emit_rec; /* [n_chunks] scratch: the scan stage's record of every chunk for dec_emit_fast */
    const struct hufd_chunk_rec *chunk_rec; /* [n_chunks] built with the plan */
    void *side_stream;  /* NULL, or a stream of the engine's for the kernels of the chunks streams end in ... */
    void *fork_event;   /* ... and two events to fork it off the launch's stream and join it again */
    void *join_event;
    struct hufd_dec_item_state *states; /* [n_items] scratch */
    struct hufd_dec_result *results;    /* [n_items] */
    uint32_t tail_stage_bytes; /* the most symbols a chunk that holds the end of a stream can decode to, +32 (0: unknown) */
    uint32_t tail_lanes;       /* the most whole lanes (sub-chunks with 8 more bytes behind them) a NARROW such chunk has */
    uint32_t tail_wide_lanes;  /* ... and a wide one (0: not known -- as many as a chunk has) */
    uint32_t n_tail_narrow;    /* the first so many of tail_chunks have at most HUFD_DEC_PACK_LANES whole lanes: they may share workgroups */
    uint32_t one_chunk_a_workgroup; /* 1: the chunks streams end in get a workgroup each, however short and many (tests: the road a plan of
                                     * few such chunks takes, for a plan of many) */
    uint32_t tails_apart;           /* 1: ... and kernels of their own even where they are few among many chunks inside streams (tests:
                                     * such a launch folds them into the big kernels' grids) */
    void **stage_events; /* NULL, or 4 hipEvent_t: before sync, after sync, after scan, after emit */
    /* a plan of ranges that holds ranges of items stored raw (huffman_amd_stored_index.h; NULL: none), for a PLAIN launch: their
     * records and the tiles of the long ones, as hufk_decode_pack has them; `items` say where each goes */
    const uint64_t *stored_rec;        /* [n_items][2] */
    const uint64_t *stored_tile_first; /* [n_items + 1] */
    uint64_t stored_tiles;
};

/* one-time per-process kernel attribute setup (dynamic LDS above 64 KiB) */
int hufk_init(void);

uint32_t hufk_enc_image_words(uint32_t max_bits);
/* whether the one-pass encoder takes this coder, and the size of the block it wants zeroed per launch */
int hufk_encode_one_pass_applies(const struct hufd_tables *tables);
uint64_t hufk_encode_zero_bytes(uint32_t n_segs, uint32_t n_items);
int hufk_encode_launch(const struct hufk_encode_args *args, void *stream);
int hufk_decode_launch(const struct hufk_decode_args *args, void *stream);
/* A packed launch (huffman_amd_packed.h): the plan's items decoded back to back, each to as many symbols as its stream
 * holds.  The sync stage, the scans, the offsets from the scans' symbol counts (hufk_unpack_offsets), the emit stage behind
 * them: the walk over the encoded bytes runs once.  The items without chunks, whose kernels walk and write in one go, run
 * twice: against no room at all for their counts, then against their places. */
struct hufk_decode_pack {
    uint32_t tile_items; /* hufk_pack_tile_items */
    uint32_t tail_stage_bytes; /* hufk_decode_args.tail_stage_bytes for the packed capacities (the plan's own is for its own) */
    uint64_t align, capacity;
    uint64_t *tile_sums; /* scratch: 2 * hufk_pack_tiles() words */
    uint64_t *offsets;   /* [n_items + 1], the caller's */
    uint64_t *summary;   /* [2]: the total, the largest rounded count */
    struct hufd_dec_item *items;      /* [n_items] the second record array: args->items with out_off / out_cap rewritten */
    struct hufd_chunk_rec *chunk_rec; /* [n_chunks] ... and args->chunk_rec with the same */
    /* a plan with stored items (huffman_amd_stored.h; NULL: none): their records, the tiles of the long ones */
    const uint64_t *stored_rec;        /* [n_items][2] */
    const uint64_t *stored_tile_first; /* [n_items + 1] */
    uint64_t stored_tiles;
};
int hufk_decode_launch_packed(const struct hufk_decode_args *args, const struct hufk_decode_pack *pack, void *stream);
/* a plan of items that are all one thread's work: the kernels' item records and the list of such items (= all of them) from
 * the caller's records, copied to the device as they are (struct hufd_raw_dec_item / hufd_raw_enc_item) */
int hufk_decode_plan_tiny_items(const void *raw_items, uint32_t n_items, struct hufd_dec_item *items, uint32_t *tiny_list, void *stream);
/* items[i] = the encoded output of encode item i as its result record on the device describes it, decoded back to where its symbols came from */
int hufk_decode_plan_from_encode(
    const struct hufd_enc_item *enc_items, const struct hufd_enc_result *enc_results, uint32_t n_items, struct hufd_dec_item *items,
    uint32_t *tiny_list, void *stream);
int hufk_encode_plan_tiny_items(const void *raw_items, uint32_t n_items, struct hufd_enc_item *items, uint32_t *tiny_list, void *stream);
/* fills chunk_item[n_chunks] and chunk_rec[n_chunks] of a decode plan from its item records, on the device */
int hufk_decode_plan_chunks(
    const struct hufd_dec_item *items, uint32_t n_items, uint32_t n_chunks, uint32_t *chunk_item, struct hufd_chunk_rec *chunk_rec,
    void *stream);
/* Plans made on the device from items the host never looks at (plan_kernels.hip).  _count: what the items come to -- statistics,
 * the thread-per-item rule, counts per item scanned into positions; copies the totals back and WAITS for the stream (the sizes
 * of the plan's arrays and of the launch's grids are the host's to know).  _fill: the records and lists, from the same scratch. */
struct hufk_plan_totals {
    uint64_t totals[8]; /* decode: chunks, thread items, wave items, large items, runs, narrow / wide end-of-stream chunks, items
                         * with chunks; encode: segments, thread items, one-tile items, large items, -, -, -, items with segments */
    uint64_t tiny_limit;
    uint64_t shortest, longest, largest_out_cap, tail_stage, tail_lanes, wide_lanes;
    uint32_t worst_bits, invalid;
};
uint64_t hufk_plan_scratch_bytes(uint64_t n_items);
int hufk_decode_plan_count(
    const struct hufd_item_source *src, uint32_t n_items, uint64_t per_byte, uint32_t shortest_code_bits, void *scratch,
    struct hufk_plan_totals *totals, void *stream);
int hufk_decode_plan_fill(
    const struct hufd_item_source *src, uint32_t n_items, uint32_t shortest_code_bits, const void *scratch, struct hufd_dec_item *items,
    uint32_t *tiny_list, uint32_t *tail_list, uint32_t *large_list, uint32_t *run_list, void *stream);
int hufk_encode_plan_count(
    const struct hufd_item_source *src, uint32_t n_items, uint64_t class0, uint64_t class1, uint64_t per_byte, uint64_t solo_limit,
    void *scratch, struct hufk_plan_totals *totals, void *stream);
int hufk_encode_plan_fill(
    const struct hufd_item_source *src, uint32_t n_items, uint32_t n_segs, uint64_t solo_limit, const void *scratch,
    struct hufd_enc_item *items, struct hufd_enc_seg *segs, uint32_t *tiny_list, uint32_t *large_list, uint32_t *solo_list, void *stream);
/* one short item whose record already sits in device memory (the host-pointer calls' small-input road): one launch */
int hufk_encode_one_tiny(
    const struct hufd_tables *tables, const struct hufd_enc_item *item, const uint32_t *zero, const void *d_in, void *d_out,
    struct hufd_enc_result *result, uint32_t length_only, void *stream);
int hufk_decode_one_tiny(
    const struct hufd_tables *tables, const struct hufd_dec_item *item, const uint32_t *zero, const void *d_in, void *d_out,
    struct hufd_dec_item_state *state, struct hufd_dec_result *result, void *stream);
/* scratch bytes of one wide item of n_blocks blocks */
uint64_t hufk_decode_wide_bytes(uint64_t n_blocks);
/* the same for an item of up to HUFD_DEC_COOP_BYTES encoded bytes (any size with long codes): dec_deep, one launch */
int hufk_decode_one_coop(
    const struct hufd_tables *tables, const struct hufd_dec_item *item, const uint32_t *zero, const void *d_in, void *d_out,
    struct hufd_dec_item_state *state, struct hufd_dec_result *result, void *stream);
/* the same for an item of up to HUFD_DEC_BLOCK_MAX_BYTES encoded bytes of a coder without long codes: one workgroup, one
 * launch (dec_block_kernel); item = the record, in HOST memory (it travels with the launch) */
int hufk_decode_one_block(
    const struct hufd_tables *tables, const struct hufd_dec_item *item, const void *d_in, void *d_out,
    struct hufd_dec_item_state *state, struct hufd_dec_result *result, void *stream);
/* one item of up to HUFD_ENC_BLOCK_MAX_BYTES symbols, one workgroup, one launch (enc_block_kernel); `symbols` = the
 * item's in_len (the record itself is in device memory); _fits: whether such an item of this coder is taken */
int hufk_encode_one_block_fits(const struct hufd_tables *tables, uint64_t symbols);
int hufk_encode_one_block(
    const struct hufd_tables *tables, const struct hufd_enc_item *item, uint32_t symbols, const void *d_in, void *d_out,
    struct hufd_enc_result *result, uint32_t length_only, void *stream);
int hufk_fill_splitmix64(void *dst, uint64_t len, uint64_t seed, void *stream);
/* counts[b] += the bytes of input[0 .. length) equal to b, u64 agent-scope atomic adds (count_kernels.hip); flush_bytes:
 * what a workgroup reads at most between two flushes of its 32-bit LDS counts (rounded down to 32 KiB, at least that) */
int hufk_symbol_counts(const void *input, uint64_t length, uint64_t *counts, uint64_t flush_bytes, void *stream);
/* the same sums over the items of an encode plan, through the plan's own lists, which cover every item once: its segments,
 * the items a wave encodes (solo) and the items a thread encodes (tiny; none of them longer than thread_limit), the last
 * two as numbers of items[]; `input` is the base the items' in_off count from.  One launch, or none for a plan without
 * items; the same adds, the same flush_bytes */
int hufk_plan_symbol_counts(
    const struct hufd_enc_item *items, const struct hufd_enc_seg *segs, uint32_t n_segs, const uint32_t *solo, uint32_t n_solo,
    const uint32_t *tiny, uint32_t n_tiny, uint64_t thread_limit, const void *input, uint64_t *counts, uint64_t flush_bytes,
    void *stream);
/* Byte planes of element_count elements of element_bytes (1, 2, 4 or 8) bytes (huffman_amd_planes.h; planes.hpp):
 *   _split   planes[p * plane_stride + j] = input[j * element_bytes + p], and with counts != NULL counts[p * 256 + b] += the
 *            bytes of plane p equal to b, the adds and flush_bytes as hufk_symbol_counts (a body of count_kernel)
 *   _merge   output[j * element_bytes + p] = planes[p * plane_stride + j] (a body of unpack_records_kernel)
 * One launch each, none for no elements.  grid_cap: the most workgroups (the tests'; 0: what is resident)
 * run_elements (0: as above; else a power of two from 16 to 2048, huffman_amd_planes_delta.h): the planes are those of
 * d[j] = element j - element j - 1, d[j] = element j where run_elements divides j -- made by the split and counted, summed
 * by the merge */
int hufk_planes_split(
    const void *input, uint64_t element_count, uint32_t element_bytes, uint32_t run_elements, void *planes, uint64_t plane_stride,
    uint64_t *counts, uint64_t flush_bytes, uint32_t grid_cap, void *stream);
int hufk_planes_merge(
    const void *planes, uint64_t plane_stride, uint64_t element_count, uint32_t element_bytes, uint32_t run_elements, void *output,
    uint32_t grid_cap, void *stream);
/* Between the length pass and the encode pass of a packed launch (pack_kernels.hip): from the length pass's records
 * `lengths`, offsets[i] = the sum of round_up((total_bits + 7) / 8, align) of the items in front of i, offsets[n_items] the
 * total; packed[i] = items[i] with out_off = offsets[i] and out_cap = what of the item's rounded length lies in front of
 * `capacity`; summary[0] = the total, summary[1] = the largest rounded length.  tile_sums: scratch of 2 * hufk_pack_tiles()
 * words; tile_items: the items a workgroup scans, from hufk_pack_tile_items (asked: the tests' own number, 0: the rule). */
uint32_t hufk_pack_tile_items(uint32_t n_items, uint32_t asked);
uint32_t hufk_pack_tiles(uint32_t n_items, uint32_t tile_items);
int hufk_pack_offsets(
    const struct hufd_enc_item *items, const struct hufd_enc_result *lengths, uint32_t n_items, uint32_t tile_items, uint64_t align,
    uint64_t capacity, uint64_t *tile_sums, uint64_t *offsets, struct hufd_enc_item *packed, uint64_t *summary, void *stream);
/* The same for a packed decode launch, from the scans' records `counts`: offsets[i + 1] = round_up(offsets[i] +
 * total_symbols_i, align); packed[i] = items[i] with out_off = offsets[i] and out_cap = total_symbols_i where the item's
 * symbols all lie in front of `capacity`, 0 where not; packed_rec[c] = chunk_rec[c] with its item's new out_off / out_cap.
 * _blank: packed[i] = items[i] with no room (what the walk that only counts is given). */
int hufk_unpack_blank(const struct hufd_dec_item *items, uint32_t n_items, struct hufd_dec_item *packed, void *stream);
int hufk_unpack_offsets(
    const struct hufd_dec_item *items, const struct hufd_dec_result *counts, uint32_t n_items, uint32_t tile_items, uint64_t align,
    uint64_t capacity, uint64_t *tile_sums, uint64_t *offsets, struct hufd_dec_item *packed, uint64_t *summary,
    const struct hufd_chunk_rec *chunk_rec, uint32_t n_chunks, struct hufd_chunk_rec *packed_rec, const uint64_t *stored_rec,
    void *stream);
/* Items stored raw in a packed batch (huffman_amd_stored.h; pack_kernels.hip, stored_copy.hpp).
 *   _pack_offsets_stored  hufk_pack_offsets with len_i = in_len_i for a stored item (in_len_i > 0, no carried bits, a coded
 *                         length that is no shorter); also stored[i] = 0 / 1, packed[i].out_cap = 0 for a stored item,
 *                         summary[2] = summary[3] = 0 (summary: four words)
 *   _stored_copy_encode   behind the encode pass over `packed`: the stored items' bytes to output + offsets[i], as far as they
 *                         lie in front of `capacity`, distributed by the plan's lists as hufk_plan_symbol_counts is; their
 *                         result records; counts[0] += the stored items, counts[1] += their bytes
 *   _stored_records       a receiver's records: stored_rec[i] = {offsets[i], the packed length of a stored item or
 *                         HUFK_NOT_STORED}, from arrays the planner's pass has checked (lengths NULL: up to the next offset)
 *   _stored_tiles         tile_first[0 .. n_items]: the tiles of tile_bytes in front of each item, none for an item that is
 *                         not stored or shorter than wave_bytes; tile_sums: 2 * hufk_pack_tiles() words
 *   hufk_unpack_offsets   with stored_rec != NULL: sym_i = the packed length of a stored item
 *   _stored_copy_decode   behind the emit stage: every stored item whose placed record has room for it copied to its place, a
 *                         workgroup a tile or a wave an item; the stored items' result records */
#define HUFK_NOT_STORED 0xFFFFFFFFFFFFFFFFull
#define HUFK_STORED_TILE_BYTES 16384u
#define HUFK_STORED_WAVE_BYTES 4096u
int hufk_pack_offsets_stored(
    const struct hufd_enc_item *items, const struct hufd_enc_result *lengths, uint32_t n_items, uint32_t tile_items, uint64_t align,
    uint64_t capacity, uint64_t *tile_sums, uint64_t *offsets, struct hufd_enc_item *packed, uint64_t *summary, uint8_t *stored,
    void *stream);
int hufk_stored_copy_encode(
    const struct hufd_enc_item *items, uint32_t n_items, const struct hufd_enc_seg *segs, uint32_t n_segs, const uint32_t *solo,
    uint32_t n_solo, const uint32_t *tiny, uint32_t n_tiny, const uint8_t *stored, const uint64_t *offsets, uint64_t capacity,
    const void *input, void *output, struct hufd_enc_result *results, uint64_t *counts, uint8_t *differs, void *stream);
int hufk_stored_records(
    const uint64_t *offsets, const uint64_t *lengths, const uint8_t *stored, const void *packed, uint32_t n_items,
    uint64_t *stored_rec, void *stream);
/* Constant items (huffman_amd_constant.h; the same bodies).
 *   _constant_detect        in front of the scan, distributed by the plan's lists as the copy is: differs[i] = 1 where a byte
 *                           of item i is not its first byte (items with carried bits or of 9 bytes or fewer are not read);
 *                           differs[] must be clear in front, and the copy clears it again
 *   _pack_offsets_constant  hufk_pack_offsets_stored with the constant rule in front: kinds[i] = 0 / 1 / 2, len_i = 9 for a
 *                           constant item, summary[2 .. 5] = 0 (summary: six words)
 *   _stored_copy_encode     with differs != NULL: stored[] holds kinds; also the 9 bytes of every constant item that fits
 *                           whole, its record, counts[2] += the constant items, counts[3] += their bytes, differs[] cleared
 *   _stored_records         with packed != NULL: stored[] holds kinds, and a constant item's record is {HUFK_CONSTANT | value,
 *                           count}, read from its head at packed + offsets[i] (checked by the planner's pass in front)
 *   _stored_copy_decode     fills such an item where it would copy */
#define HUFK_CONSTANT (1ull << 63)
#define HUFK_CONSTANT_BYTES 9u
#define HUFK_CONSTANT_MAX_COUNT 0x100000000ull
int hufk_constant_detect(
    const struct hufd_enc_item *items, uint32_t n_items, const struct hufd_enc_seg *segs, uint32_t n_segs, const uint32_t *solo,
    uint32_t n_solo, const uint32_t *tiny, uint32_t n_tiny, const void *input, uint8_t *differs, void *stream);
int hufk_pack_offsets_constant(
    const struct hufd_enc_item *items, const struct hufd_enc_result *lengths, uint32_t n_items, uint32_t tile_items, uint64_t align,
    uint64_t capacity, uint64_t *tile_sums, uint64_t *offsets, struct hufd_enc_item *packed, uint64_t *summary, uint8_t *kinds,
    const uint8_t *differs, void *stream);
/* ... of a plan of ranges of an indexed batch (huffman_amd_stored_index.h): stored_rec[r] = {items[r].in_off, items[r].out_cap}
 * for a range of bytes in an item flagged 1, {.., HUFK_NOT_STORED} for any other; ranges: four words each, the first the item */
int hufk_stored_range_records(
    const uint64_t *ranges, const uint8_t *stored, const struct hufd_dec_item *items, uint32_t n_items, uint64_t *stored_rec,
    void *stream);
int hufk_stored_tiles(
    const uint64_t *stored_rec, uint32_t n_items, uint32_t tile_items, uint64_t tile_bytes, uint64_t wave_bytes, uint64_t *tile_sums,
    uint64_t *tile_first, void *stream);
int hufk_stored_copy_decode(
    const uint64_t *stored_rec, const uint64_t *tile_first, uint64_t n_tiles, uint32_t n_items, const struct hufd_dec_item *placed,
    struct hufd_dec_result *results, const void *input, void *output, void *stream);
/* A coder fitted on the device (fit_kernels.hip, huffman_amd_fit.h): ONE launch of one workgroup writes enc_table[256] and
 * dec_lut[1 << max_bits] -- from 256 counts (from_lengths 0: package-merge lengths in min_bits .. max_bits for all 256
 * symbols, also left in num_bits_out where that is not NULL), or from 256 lengths (from_lengths 1) -- and *status (NULL: not
 * wanted): 0, or why the tables were left as they were.  4 <= min_bits <= 8 <= max_bits <= 12, min_bits < max_bits. */
#define HUFK_FIT_COUNTS_TOO_LARGE 1u     /* counts that sum to 2^58 or more */
#define HUFK_FIT_LENGTH_ZERO 2u          /* a symbol without a code */
#define HUFK_FIT_LENGTH_OUT_OF_BOUNDS 3u /* a length outside min_bits .. max_bits */
#define HUFK_FIT_KRAFT_ABOVE_ONE 4u      /* not a prefix code */
int hufk_fit_tables(
    uint32_t from_lengths, const uint64_t *counts, const uint8_t *lengths, uint32_t min_bits, uint32_t max_bits, uint64_t *enc_table,
    uint16_t *dec_lut, uint8_t *num_bits_out, uint32_t *status, void *stream);

/* The block index of a stream (index_kernels.hip, huffman_amd_index.h): index[k] = the code bits of symbols
 * [0, min(k * block_symbols, length)) under enc_table, k = 0 .. n_blocks = ceil(length / block_symbols), 1 <= n_blocks < 2^32;
 * *status (NULL: not wanted) says whether a symbol without a code was met (it counts 0 bits).  block_symbols: a multiple of
 * 64 up to 1 << 24.  tile_sums: scratch of 2 * HUFK_INDEX_MAX_TILES words; tile_blocks: the entries a workgroup of the scan
 * takes, from hufk_index_tile_blocks (asked: the tests' own number, 0: the rule; never more than HUFK_INDEX_MAX_TILES tiles).
 * Its two steps: _block_bits (count_kernels.hip) leaves index[k] = the bits of block k alone, bit 63 set on some entry where
 * a symbol without a code was met; _index_scan (pack_kernels.hip) sums them in place and writes index[n_blocks] and *status. */
#define HUFK_INDEX_OK 0u
#define HUFK_INDEX_SYMBOL_WITHOUT_CODE 1u
#define HUFK_INDEX_MAX_TILES 8192u
uint32_t hufk_index_tile_blocks(uint32_t n_blocks, uint32_t asked);
int hufk_block_index(
    const uint64_t *enc_table, const void *input, uint64_t length, uint64_t block_symbols, uint32_t tile_blocks, uint64_t *index,
    uint64_t *tile_sums, uint32_t *status, void *stream);
int hufk_block_bits(
    const uint64_t *enc_table, const void *input, uint64_t length, uint64_t block_symbols, uint64_t *index, void *stream);
int hufk_index_scan(uint64_t *index, uint32_t n_blocks, uint32_t tile_blocks, uint64_t *tile_sums, uint32_t *status, void *stream);

/* One block index over the items of an encode plan (index_kernels.hip, huffman_amd_batch_index.h): the directory -- record i
 * = {the blocks in front of item i, its symbols}, record n_items = {all blocks, 0}, two words each -- and index[k] = the code
 * bits in front of global block k, one running sum over the batch.  The host knows the capacity of the index, not the
 * blocks: every grid is sized from `capacity` and n_items, and the kernels read the counts the directory scan left.
 *   _batch_directory   the directory, summary[0] = all blocks, tile_first[0 .. n_items] (the tiles of the hot pass in front
 *                      of each item; not for a size query, capacity 0), and where the batch has no block or its index does
 *                      not fit, the status (and index[0] = 0); tile_sums: 2 * hufk_pack_tiles(n_items, tile_items) words
 *   _batch_block_bits  the hot pass (count_kernel's body, index_block_bits.hpp): items shorter than wave_bytes a wave each,
 *                      the others in tiles of whole blocks
 *   _batch_index_scan  hufk_index_scan over the blocks *device_blocks says, at most most_blocks of them */
#define HUFK_INDEX_TOO_SMALL 2u
#define HUFK_BATCH_WAVE_MAX_BYTES 65536u /* the longest item a wave takes: its groups of 16 symbols are numbered below 2^12 */
struct hufk_batch_index {
    const uint64_t *enc_table;
    const struct hufd_enc_item *items; /* the plan's records: in_off and in_len are read */
    uint32_t n_items;
    const void *input;
    uint64_t block_symbols;
    uint64_t wave_bytes;       /* 1 .. HUFK_BATCH_WAVE_MAX_BYTES */
    uint32_t pack_tile_items;  /* hufk_pack_tile_items */
    uint32_t index_tile_asked; /* the tests' own number for hufk_index_tile_blocks (0: the rule) */
    uint64_t *directory;       /* the caller's: 2 * (n_items + 1) words */
    uint64_t *index;           /* the caller's: `capacity` words (NULL with capacity 0: a size query) */
    uint64_t capacity;
    uint32_t *status;          /* NULL: not wanted */
    uint64_t *tile_first;      /* scratch: n_items + 1 words */
    uint64_t *item_tile_sums;  /* scratch: 2 * hufk_pack_tiles(n_items, pack_tile_items) words */
    uint64_t *summary;         /* [1]: all blocks */
    uint64_t *index_tile_sums; /* scratch: 2 * HUFK_INDEX_MAX_TILES words */
};
int hufk_batch_block_index(const struct hufk_batch_index *job, void *stream);
int hufk_batch_directory(
    const struct hufd_enc_item *items, uint32_t n_items, uint32_t tile_items, uint64_t block_symbols, uint64_t wave_bytes,
    uint64_t tile_blocks, uint64_t capacity, uint64_t *tile_sums, uint64_t *directory, uint64_t *tile_first, uint64_t *summary,
    uint64_t *index, uint32_t *status, void *stream);
uint32_t hufk_batch_tile_blocks(uint64_t block_symbols);
int hufk_batch_block_bits(const struct hufk_batch_index *job, uint64_t most_blocks, void *stream);
int hufk_batch_index_scan(
    uint64_t *index, const uint64_t *device_blocks, uint64_t capacity, uint32_t most_blocks, uint32_t tile_blocks, uint64_t *tile_sums,
    uint32_t *status, void *stream);

/* The offsets of a packed launch from the batch's block index in place of a length pass (pack_kernels.hip,
 * huffman_amd_packed_index.h): behind hufk_batch_block_index on the same stream, with f_i = directory[2 i],
 * len_i = ceil((index[f_{i+1}] - index[f_i] + items[i].ovf_bits) / 8), and offsets, packed and summary from these as
 * hufk_pack_offsets makes them from a length pass's records.  Where the batch's blocks (directory[2 n_items]) have no index in
 * index_capacity entries, every len_i is 0: offsets and summary all 0, packed[i] with no room. */
int hufk_pack_offsets_indexed(
    const struct hufd_enc_item *items, uint32_t n_items, uint32_t tile_items, uint64_t align, uint64_t capacity,
    const uint64_t *directory, const uint64_t *index, uint64_t index_capacity, uint64_t *tile_sums, uint64_t *offsets,
    struct hufd_enc_item *packed, uint64_t *summary, void *stream);
/* The two together (huffman_amd_stored_index.h): hufk_pack_offsets_stored with the coded length hufk_pack_offsets_indexed
 * reads out of the scanned index.  An index that does not fit: every length 0, so also every flag. */
int hufk_pack_offsets_stored_indexed(
    const struct hufd_enc_item *items, uint32_t n_items, uint32_t tile_items, uint64_t align, uint64_t capacity,
    const uint64_t *directory, const uint64_t *index, uint64_t index_capacity, uint64_t *tile_sums, uint64_t *offsets,
    struct hufd_enc_item *packed, uint64_t *summary, uint8_t *stored, void *stream);

/* Where symbols of an indexed stream start (decode_locate_body.inc, huffman_amd_ranges.h): job->bits[i] for the positions
 * [0, job->count) of `job` (its `first` and `coop` are the launches' own), under the decode tables of `tables`.  One launch
 * of a lane a position; walks_coop != 0: a second of a workgroup a position, for the positions more than job->lone_symbols
 * codes behind their block's first.  *job->status is ORed into: the caller clears it in front. */
int hufk_locate_symbols(const struct hufd_tables *tables, const struct hufd_locate *job, uint32_t walks_coop, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* HUFFMAN_AMD_KERNELS_H */
