/*
 * Host layer (C99) of libaws-c-compression-amd: engines, plans and the
 * translation between the reference's call semantics and the device records.
 * All symbol work happens in the HIP kernels (the *_kernels.hip files of csrc/hip);
 * this file tabulates coders, lays out items, launches, and reads results back.
 * There is no CPU implementation of encode or decode here.
 */
#include "engine.h"
#include "arena.h"

#include <aws/compression/huffman_amd_batch_index.h>
#include <aws/compression/huffman_amd_packed_index.h>
#include <aws/compression/huffman_amd_build.h>
#include <aws/compression/huffman_amd_fit.h>
#include <aws/compression/huffman_amd_index.h>
#include <aws/compression/huffman_amd_packed.h>
#include <aws/compression/huffman_amd_plan_counts.h>
#include <aws/compression/huffman_amd_planes.h>
#include <aws/compression/huffman_amd_planes_delta.h>
#include <aws/compression/huffman_amd_ranges.h>
#include <aws/compression/huffman_amd_constant.h>
#include <aws/compression/huffman_amd_stored.h>
#include <aws/compression/huffman_amd_stored_index.h>

#include <assert.h>
#include <stdlib.h>
#include <string.h>

/* the tests' switches (huffman_amd.h "testing hooks"): process-wide words, read with the plans and launches that follow */
static uint32_t s_testing_encode_road = 0, s_testing_decode_road = 0;
static uint64_t s_testing_per_byte[2] = {0, 0}; /* [0] encode, [1] decode */

void aws_huffman_amd_testing_set_encode_road(uint32_t flags) {
    __atomic_store_n(&s_testing_encode_road, flags, __ATOMIC_RELAXED);
}
void aws_huffman_amd_testing_set_decode_road(uint32_t flags) {
    __atomic_store_n(&s_testing_decode_road, flags, __ATOMIC_RELAXED);
}
void aws_huffman_amd_testing_set_items_per_byte(uint64_t encode, uint64_t decode) {
    __atomic_store_n(&s_testing_per_byte[0], encode, __ATOMIC_RELAXED);
    __atomic_store_n(&s_testing_per_byte[1], decode, __ATOMIC_RELAXED);
}
static uint32_t testing_encode_road(void) {
    return __atomic_load_n(&s_testing_encode_road, __ATOMIC_RELAXED);
}
static uint32_t testing_decode_road(void) {
    return __atomic_load_n(&s_testing_decode_road, __ATOMIC_RELAXED);
}


/* ------------------------------------------------------------------ small helpers */

/* behind a plan's launch: what a later owner of the plan's device arrays waits for.  On a caller's stream an event (the
 * stream may be gone by then); on the engine's own stream nothing -- that stream lives as long as the engine and is
 * waited for itself (an event record is a packet of its own on the queue: ~4 us behind every launch) */
static int plan_mark_done(void **event, bool *on_engine_stream, const struct aws_huffman_amd_engine *eng, void *stream) {
    if (!stream || stream == eng->stream) {
        *on_engine_stream = true;
        return 0;
    }
    if (!*event) {
        *event = hufs_event_create_untimed();
        if (!*event) {
            return 2;
        }
    }
    return hufs_event_record(*event, stream);
}

static int plan_wait_done(void *event, bool on_engine_stream, const struct aws_huffman_amd_engine *eng) {
    int err = on_engine_stream ? hufs_stream_sync(eng->stream) : 0;
    if (!err && event) {
        err = hufs_event_sync(event);
    }
    return err;
}

/*
 * The calling thread's current HIP device is the caller's business: every entry point that works on an engine's device
 * switches to it for its own duration and leaves the thread where it found it (a library call that moves a thread to
 * another GPU makes the caller's next kernel launch, or the next engine picked by the current device, land there).
 */
struct device_scope {
    int previous; /* < 0: nothing to go back to */
};
static struct device_scope device_scope_enter(int device) {
    struct device_scope sc = {-1};
    int now = -1;
    if (hufs_get_device(&now) == 0 && now != device) {
        sc.previous = now;
    }
    hufs_set_device(device);
    return sc;
}
static void device_scope_leave(struct device_scope *sc) {
    if (sc->previous >= 0) {
        hufs_set_device(sc->previous);
    }
}
#define HUFS_PASTE2(a, b) a##b
#define HUFS_PASTE(a, b) HUFS_PASTE2(a, b)
#define ON_DEVICE(device)                                                                                              \
    struct device_scope HUFS_PASTE(device_scope_, __LINE__) __attribute__((cleanup(device_scope_leave), unused)) =     \
        device_scope_enter(device)

static int raise_hip(int hip_error) {
    (void)hip_error;
    return aws_raise_error(AWS_ERROR_UNKNOWN);
}

/* the few words a launch's scan left for the host (a plan's size getters): copied back on `st`, which is waited for.
 * src NULL: nothing was left (a plan without items) -- the wait alone, the words stay as they are */
static int plan_read_words(int device, const uint64_t *src, uint64_t *words, size_t n, void *st) {
    ON_DEVICE(device);
    int err = src ? hufs_copy_d2h(words, src, n * sizeof(uint64_t), st) : 0;
    if (!err) {
        err = hufs_stream_sync(st);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

static void *device_upload(const void *host, size_t size, void *stream, int *err) {
    void *d = hufs_malloc(size);
    if (!d) {
        *err = 2; /* hipErrorOutOfMemory */
        return NULL;
    }
    *err = hufs_copy_h2d(d, host, size, stream);
    if (!*err) {
        *err = hufs_stream_sync(stream);
    }
    if (*err) {
        hufs_free(d);
        return NULL;
    }
    return d;
}

/* ------------------------------------------------------------------ engine */


/*
 * Decode tables for a coder with codes of more than HUFD_DEC_MAX_LUT_BITS bits: a root table indexed by the
 * first HUFD_DEEP_ROOT_BITS bits of the window, whose entries either answer (symbol, length / no code) or
 * link to a table indexed by the next few bits, and so on down to bit 32.  Filled by asking the decode
 * callback (reference huffman.h:48) about every index with the bits below it all zero and all one: the same
 * answer, no longer than the bits looked at, is an entry; anything else depends on later bits and gets a
 * table of its own.  Every code of the encode table must then come back out of the tables.
 *
 * A linked table is made HUFD_DEEP_SUB_BITS wide and, when none of its entries is a link, narrowed to the
 * bits its answers depend on: entries that repeat in runs of 2^k lose k index bits (the link carries the
 * width).  Only answers are asked for, so a decode-only coder gets the same tables.  The levels stay where
 * they were (bits 10, 18, 26), so a look-up takes as many steps as before the narrowing.
 *
 * Size, for a canonical code (aws_huffman_amd_table_coder_from_lengths: codes in order of length, so the codes
 * of one length are one run of the code space, and room that is left lies behind the last code).  Call the
 * runs of lengths 11 .. 32 and the room left "classes"; a class of length L ends on a multiple of 2^(32-L).
 *   - A table whose span holds one class of length L is either all codes (narrowed to L - depth bits: one
 *     entry per code) or all links with at least one code below each: at most one entry per code and level,
 *     3 * 256 = 768 entries.
 *   - A table whose span holds the end of a class of length L inside it lies at a depth below L.  There are
 *     at most 22 such ends (L = 11 .. 32), each inside one table per level: 22 tables at depth 10, 14 at depth
 *     18 (L >= 19), of at most 256 entries, and 6 at depth 26 (L >= 27) of 64: 9600 entries.
 * With the root's 1024 that is 11 392 <= HUFD_DEEP_MAX_ENTRIES for every canonical code of 1 .. 256 symbols and
 * lengths up to 32 (what the data gives is nearer 1024 plus a few hundred).  Other prefix codes
 * (aws_huffman_amd_table_coder_new with patterns of the caller's own) can need more -- 256 codes of 32 bits
 * under 256 different 10-bit prefixes need about 150 000 entries: those stay without decode
 * (aws_huffman_amd_engine_can_decode() == false), as huffman_amd.h and INTEGRATION.md say.
 */
struct deep_builder {
    struct aws_huffman_symbol_coder *coder;
    uint32_t *tab; /* HUFD_DEEP_MAX_ENTRIES, and room for the one table that is not narrowed yet */
    uint32_t used;
    bool ok;
};

/* how many index bits the link-free table of 1 << width entries at tab can lose: the largest k < width with every run of
 * 2^k entries the same */
static uint32_t deep_table_spare_bits(const uint32_t *tab, uint32_t width) {
    uint32_t k = 0;
    while (k + 1 < width) {
        const uint32_t half = 1u << k;
        for (uint32_t i = 0; i < (1u << width); i += 2 * half) {
            if (tab[i] != tab[i + half]) {
                return k;
            }
        }
        ++k;
    }
    return k;
}

static void deep_table_fill(struct deep_builder *b, uint32_t base, uint32_t prefix, uint32_t depth, uint32_t width) {
    const uint32_t low = 32 - depth - width; /* window bits below this table's index */
    const uint32_t fill = low ? (uint32_t)((1ull << low) - 1) : 0;
    for (uint32_t w = 0; w < (1u << width) && b->ok; ++w) {
        const uint32_t bits = prefix | (uint32_t)((uint64_t)w << low);
        uint8_t s0 = 0, s1 = 0;
        const uint8_t n0 = b->coder->decode(bits, &s0, b->coder->userdata);
        const uint8_t n1 = b->coder->decode(bits | fill, &s1, b->coder->userdata);
        if (n0 == n1 && n0 <= depth + width && (n0 == 0 || s0 == s1)) {
            b->tab[base + w] = n0 ? ((uint32_t)s0 << 8) | n0 : 0;
        } else if (low == 0) {
            b->ok = false; /* an answer longer than the window */
        } else {
            uint32_t sub = low < HUFD_DEEP_SUB_BITS ? low : HUFD_DEEP_SUB_BITS;
            /* (a table is opened full-width and narrowed afterwards, so `used` may run up to 1 << HUFD_DEEP_SUB_BITS entries
             * past the maximum here -- the room deep_table_build allocates on top -- and deep_table_build's check of the
             * final size decides) */
            if (b->used > HUFD_DEEP_MAX_ENTRIES) {
                b->ok = false; /* more tables than the kernels keep in LDS */
                return;
            }
            const uint32_t at = b->used;
            b->used += 1u << sub;
            deep_table_fill(b, at, bits, depth + width, sub);
            if (b->ok && b->used == at + (1u << sub)) {
                /* no table below this one: its entries are answers, and it is the last one made */
                const uint32_t spare = deep_table_spare_bits(b->tab + at, sub);
                for (uint32_t i = 0; i < (1u << (sub - spare)); ++i) {
                    b->tab[at + i] = b->tab[at + (i << spare)];
                }
                sub -= spare;
                b->used = at + (1u << sub);
            }
            b->tab[base + w] = HUFD_DEEP_LINK | (sub << 16) | at;
        }
    }
}

static uint32_t deep_table_lookup(const uint32_t *tab, uint32_t window) {
    uint32_t e = tab[window >> (32 - HUFD_DEEP_ROOT_BITS)], used = HUFD_DEEP_ROOT_BITS;
    while (e & HUFD_DEEP_LINK) {
        const uint32_t width = (e >> 16) & 0xFFu;
        e = tab[(e & 0xFFFFu) + ((window << used) >> (32 - width))];
        used += width;
    }
    return e;
}

static int deep_table_build(struct aws_huffman_amd_engine *eng, struct aws_huffman_symbol_coder *coder) {
    struct deep_builder b = {
        coder, malloc((HUFD_DEEP_MAX_ENTRIES + (1u << HUFD_DEEP_SUB_BITS)) * sizeof(uint32_t)), 1u << HUFD_DEEP_ROOT_BITS, true};
    if (!b.tab) {
        return aws_raise_error(AWS_ERROR_OOM);
    }
    deep_table_fill(&b, 0, 0, 0, HUFD_DEEP_ROOT_BITS);
    b.ok = b.ok && b.used <= HUFD_DEEP_MAX_ENTRIES;
    /* the longest and the shortest code the decoder knows (an encoder may know fewer, or none) */
    for (uint32_t i = 0; i < b.used && b.ok; ++i) {
        const uint32_t e = b.tab[i];
        if (!(e & HUFD_DEEP_LINK) && (e & 0xFFu)) {
            const uint32_t len = e & 0xFFu;
            eng->tables.max_bits = len > eng->tables.max_bits ? len : eng->tables.max_bits;
            eng->tables.min_bits = len < eng->tables.min_bits ? len : eng->tables.min_bits;
        }
    }
    eng->tables.n_states = eng->tables.max_bits > 8 ? eng->tables.max_bits : 8;
    for (int sym = 0; sym < 256 && b.ok && coder->encode; ++sym) {
        const uint32_t len = (uint32_t)(eng->enc_table[sym] >> 32);
        if (len) {
            const uint32_t code = (uint32_t)eng->enc_table[sym] << (32 - len);
            const uint32_t fill = len < 32 ? (1u << (32 - len)) - 1u : 0u;
            const uint32_t want = ((uint32_t)sym << 8) | len;
            b.ok = deep_table_lookup(b.tab, code) == want && deep_table_lookup(b.tab, code | fill) == want;
        }
    }
    if (!b.ok) {
        free(b.tab); /* not a table-shaped decoder: decode stays unavailable */
        return AWS_OP_SUCCESS;
    }
    eng->deep_lut_host = b.tab;
    eng->tables.deep_entries = b.used;
    eng->tables.lut_bits = 0;
    eng->can_decode = true;
    return AWS_OP_SUCCESS;
}

/* the engine's own stream, and the second stream with its two events; 0 or a HIP error */
static int engine_streams_create(struct aws_huffman_amd_engine *eng) {
    const int err = hufs_stream_create(&eng->stream);
    if (!err && hufs_stream_create(&eng->side_stream) == 0) {
        eng->fork_event = hufs_event_create_untimed();
        eng->join_event = hufs_event_create_untimed();
        if (!eng->fork_event || !eng->join_event) {
            /* (no overlap then: the kernels run one after the other on the one stream) */
            hufs_event_destroy(eng->fork_event);
            hufs_event_destroy(eng->join_event);
            hufs_stream_destroy(eng->side_stream);
            eng->fork_event = eng->join_event = eng->side_stream = NULL;
        }
    } else {
        eng->side_stream = NULL;
    }
    return err;
}

int aws_huffman_amd_engine_new(
    struct aws_huffman_amd_engine **out_engine,
    struct aws_huffman_symbol_coder *coder,
    int device) {

    *out_engine = NULL;
    /* (a coder may lack one of its two callbacks: the reference's encoder only ever calls `encode`, its decoder only
     * `decode` -- source/huffman.c:60,235 -- and an engine is then good for that half) */
    if (!coder || (!coder->encode && !coder->decode)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (hufs_device_count() <= 0) {
        /* fail loudly: there is no CPU path to fall back to */
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    if (device < 0) {
        if (hufs_get_device(&device)) {
            return aws_raise_error(AWS_ERROR_UNKNOWN);
        }
    }
    if (device >= hufs_device_count()) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    ON_DEVICE(device);
    {
        const int e = hufk_init(); /* per device, once; safe from several threads */
        if (e) {
            return raise_hip(e);
        }
    }

    struct aws_huffman_amd_engine *eng = calloc(1, sizeof(*eng));
    if (!eng) {
        return aws_raise_error(AWS_ERROR_OOM);
    }
    pthread_mutex_init(&eng->one_lock, NULL);
    pthread_mutex_init(&eng->spare_lock, NULL);
    eng->device = device;
    eng->coder = coder;
    eng->key_encode = (void *)coder->encode;
    eng->key_decode = (void *)coder->decode;
    eng->key_userdata = coder->userdata;
    eng->fingerprint = aws_huffman_amd_coder_fingerprint(coder);

    /* encode table: one callback per symbol (reference huffman.h:37) */
    uint32_t max_bits = 0, min_bits = 33;
    eng->can_encode = coder->encode != NULL;
    for (int sym = 0; sym < 256 && coder->encode; ++sym) {
        const struct aws_huffman_code code = coder->encode((uint8_t)sym, coder->userdata);
        if (code.num_bits > 32) {
            free(eng);
            return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
        }
        const uint32_t masked =
            code.num_bits == 0 ? 0 : (code.num_bits == 32 ? code.pattern : code.pattern & ((1u << code.num_bits) - 1u));
        eng->enc_table[sym] = ((uint64_t)code.num_bits << 32) | masked;
        if (code.num_bits) {
            max_bits = code.num_bits > max_bits ? code.num_bits : max_bits;
            min_bits = code.num_bits < min_bits ? code.num_bits : min_bits;
        }
    }
    eng->tables.all_coded = 1;
    for (int sym = 0; sym < 256; ++sym) {
        if ((eng->enc_table[sym] >> 32) == 0) {
            eng->tables.all_coded = 0;
        }
    }
    {
        const uint32_t road = testing_encode_road();
        /* one pass over the input where the coder allows it (hufk_encode_one_pass_applies); the tests can ask for count /
         * scan / pack, the road every other coder takes */
        eng->single_pass = !(road & AWS_HUFFMAN_AMD_TEST_ENCODE_THREE_KERNEL);
        /* ... or for a wave of the one-pass kernel that gives up, as if a look-back wait had run out: the three-kernel
         * road queued behind it on the stream does the launch over */
        eng->encode_fails = (road & AWS_HUFFMAN_AMD_TEST_ENCODE_ONE_PASS_FAILS) != 0;
    }
    /* decode tables from the DECODE callback alone (the reference's decoder knows nothing else: source/huffman.c:235-238;
     * reference huffman.h:48).  Every window of HUFD_DEC_MAX_LUT_BITS bits is asked twice, the bits behind it all zero
     * and all one: the same answer both times, no longer than the window, for every window = a coder whose codes have at
     * most that many bits, and its table (exhaustive: nothing is inferred).  Otherwise codes are longer: the linked
     * tables (deep_table_build), checked against the encode table where there is one. */
    eng->can_decode = false;
    uint32_t dec_max = 0, dec_min = 33;
    if (coder->decode) {
        const uint32_t wide = HUFD_DEC_MAX_LUT_BITS, windows = 1u << wide;
        const uint32_t fill = (1u << (32 - wide)) - 1u;
        uint16_t *probe = malloc(windows * sizeof(uint16_t));
        if (!probe) {
            free(eng);
            return aws_raise_error(AWS_ERROR_OOM);
        }
        bool tabular = true;
        for (uint32_t w = 0; w < windows && tabular; ++w) {
            uint8_t s0 = 0, s1 = 0;
            const uint32_t bits = w << (32 - wide);
            const uint8_t n0 = coder->decode(bits, &s0, coder->userdata);
            const uint8_t n1 = coder->decode(bits | fill, &s1, coder->userdata);
            if (n0 != n1 || n0 > wide || (n0 && s0 != s1)) {
                tabular = false;
            }
            probe[w] = n0 ? (uint16_t)(((uint16_t)s0 << 8) | n0) : 0;
            if (n0) {
                dec_max = n0 > dec_max ? n0 : dec_max;
                dec_min = n0 < dec_min ? n0 : dec_min;
            }
        }
        /* (a code of n bits must own all windows that start with it: a callback that answers from more bits than it
         * says is not a prefix code's) */
        for (uint32_t w = 0; w < windows && tabular; ++w) {
            const uint32_t n = probe[w] & 0xFFu;
            if (n && n < wide) {
                const uint32_t first = w >> (wide - n) << (wide - n);
                tabular = probe[first] == probe[w] && probe[first + (1u << (wide - n)) - 1u] == probe[w];
            }
        }
        if (tabular && dec_max >= 1) {
            uint16_t *lut = malloc(((size_t)1 << dec_max) * sizeof(uint16_t));
            if (!lut) {
                free(probe);
                free(eng);
                return aws_raise_error(AWS_ERROR_OOM);
            }
            for (uint32_t w = 0; w < (1u << dec_max); ++w) {
                lut[w] = probe[w << (wide - dec_max)];
            }
            eng->dec_lut_host = lut;
            eng->tables.lut_bits = dec_max;
            eng->can_decode = true;
        } else if (tabular) {
            dec_min = 33; /* a decoder without a single code: every stream stops at its first window, as the reference's would */
            uint16_t *lut = calloc(2, sizeof(uint16_t));
            if (!lut) {
                free(probe);
                free(eng);
                return aws_raise_error(AWS_ERROR_OOM);
            }
            eng->dec_lut_host = lut;
            eng->tables.lut_bits = 1;
            eng->can_decode = true;
        }
        free(probe);
    }
    /* two sets of code-length bounds: the encode table's own size images and stages and pick the packer; the decode
     * kernels' entry states, walk tables and certain steps follow what the DECODE table knows -- an encoder with codes of
     * 13..32 bits beside a decoder whose table has 12 or fewer must not give the chunk kernels more entry states than
     * they have registers for (they hold HUFD_DEC_MAX_LUT_BITS, or 16 on the long way) */
    eng->tables.enc_max_bits = max_bits;
    eng->tables.enc_min_bits = min_bits > 32 ? 1 : min_bits;
    if (eng->can_decode && dec_max) {
        max_bits = dec_max;
        min_bits = dec_min;
    }
    eng->tables.max_bits = max_bits;
    eng->tables.min_bits = min_bits; /* (33: no code known yet) */
    eng->tables.n_states = max_bits > 8 ? max_bits : 8;
    /* every code the DECODE table knows has one length: symbol k starts at bit k * length (dec_fixed_*) */
    eng->tables.fixed_bits = eng->can_decode && dec_max && dec_min == dec_max && dec_max <= HUFD_DEC_MAX_LUT_BITS ? dec_max : 0;
    eng->tables.fixed_complete = 0;
    if (eng->tables.fixed_bits && eng->dec_lut_host) {
        /* ... and every window is one (256 codes of 8 bits): no stream has a symbol without a code to look for */
        eng->tables.fixed_complete = 1;
        for (uint32_t i = 0; i < (1u << eng->tables.lut_bits); ++i) {
            if ((eng->dec_lut_host[i] & 0xFFu) == 0) {
                eng->tables.fixed_complete = 0;
                break;
            }
        }
    }

    if (!eng->can_decode && coder->decode) {
        if (deep_table_build(eng, coder)) {
            free(eng);
            return AWS_OP_ERR;
        }
    }
    if (eng->tables.min_bits > 32) {
        eng->tables.min_bits = 1;
    }

    int err = engine_streams_create(eng);
    if (!err && eng->deep_lut_host) {
        eng->d_deep_lut =
            device_upload(eng->deep_lut_host, (size_t)eng->tables.deep_entries * sizeof(uint32_t), eng->stream, &err);
    }
    if (!err) {
        eng->d_enc_table = device_upload(eng->enc_table, sizeof(eng->enc_table), eng->stream, &err);
    }
    if (!err && eng->dec_lut_host) {
        eng->d_dec_lut =
            device_upload(eng->dec_lut_host, (size_t)sizeof(uint16_t) << eng->tables.lut_bits, eng->stream, &err);
    }
    if (err) {
        aws_huffman_amd_engine_destroy(eng);
        return raise_hip(err);
    }
    eng->tables.enc_table = eng->d_enc_table;
    eng->tables.dec_lut = eng->d_dec_lut;
    eng->tables.deep_lut = eng->d_deep_lut;
    *out_engine = eng;
    return AWS_OP_SUCCESS;
}

void aws_huffman_amd_engine_destroy(struct aws_huffman_amd_engine *eng) {
    if (!eng) {
        return;
    }
    ON_DEVICE(eng->device);
    if (eng->one_enc) {
        aws_huffman_amd_encode_plan_destroy(eng->one_enc);
    }
    if (eng->one_dec) {
        aws_huffman_amd_decode_plan_destroy(eng->one_dec);
    }
    /* (the plans destroyed last, kept for the next *_plan_new: gone for good now) */
    {
        struct aws_huffman_amd_encode_plan *se = eng->spare_enc;
        struct aws_huffman_amd_decode_plan *sd = eng->spare_dec;
        eng->spare_enc = NULL;
        eng->spare_dec = NULL;
        eng->retiring = true;
        if (se) {
            aws_huffman_amd_encode_plan_destroy(se);
        }
        if (sd) {
            aws_huffman_amd_decode_plan_destroy(sd);
        }
    }
    hufs_free(eng->one_in);
    hufs_free(eng->one_out);
    hufs_free(eng->mini_dev);
    hufs_host_free(eng->mini_host);
    hufs_free(eng->d_enc_table);
    hufs_free(eng->d_dec_lut);
    hufs_free(eng->d_deep_lut);
    hufs_free(eng->d_index_tile_sums);
    hufs_event_destroy(eng->fork_event);
    hufs_event_destroy(eng->join_event);
    if (eng->side_stream) {
        hufs_stream_destroy(eng->side_stream);
    }
    hufs_stream_destroy(eng->stream);
    free(eng->dec_lut_host);
    free(eng->deep_lut_host);
    pthread_mutex_destroy(&eng->one_lock);
    pthread_mutex_destroy(&eng->spare_lock);
    free(eng);
}

int aws_huffman_amd_engine_device(const struct aws_huffman_amd_engine *eng) {
    return eng->device;
}

int aws_huffman_amd_current_device(void) {
    int device = -1;
    return hufs_get_device(&device) ? -1 : device;
}

uint32_t aws_huffman_amd_engine_max_code_bits(const struct aws_huffman_amd_engine *eng) {
    return eng->tables.max_bits > eng->tables.enc_max_bits ? eng->tables.max_bits : eng->tables.enc_max_bits;
}

bool aws_huffman_amd_engine_can_decode(const struct aws_huffman_amd_engine *eng) {
    return eng->can_decode;
}

void *aws_huffman_amd_engine_stream(struct aws_huffman_amd_engine *eng) {
    return eng->stream;
}

/* ------------------------------------------------------------------ engines fitted on the device (huffman_amd_fit.h) */

_Static_assert(AWS_HUFFMAN_AMD_FIT_COUNTS_TOO_LARGE == HUFK_FIT_COUNTS_TOO_LARGE, "fit status");
_Static_assert(AWS_HUFFMAN_AMD_FIT_LENGTH_ZERO == HUFK_FIT_LENGTH_ZERO, "fit status");
_Static_assert(AWS_HUFFMAN_AMD_FIT_LENGTH_OUT_OF_BOUNDS == HUFK_FIT_LENGTH_OUT_OF_BOUNDS, "fit status");
_Static_assert(AWS_HUFFMAN_AMD_FIT_KRAFT_ABOVE_ONE == HUFK_FIT_KRAFT_ABOVE_ONE, "fit status");

int aws_huffman_amd_engine_new_fitted(struct aws_huffman_amd_engine **out_engine, int device, uint32_t min_bits, uint32_t max_bits) {
    /* (the caller's pointer is written on success only) */
    if (!out_engine || min_bits < 4 || min_bits > 8 || max_bits < 8 || max_bits > HUFD_DEC_MAX_LUT_BITS || min_bits >= max_bits) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION); /* no GPU: there is no CPU path */
    }
    if (device < 0 && hufs_get_device(&device)) {
        return aws_raise_error(AWS_ERROR_UNKNOWN);
    }
    if (device >= hufs_device_count()) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    ON_DEVICE(device);
    {
        const int e = hufk_init();
        if (e) {
            return raise_hip(e);
        }
    }
    struct aws_huffman_amd_engine *eng = calloc(1, sizeof(*eng));
    if (!eng) {
        return aws_raise_error(AWS_ERROR_OOM);
    }
    pthread_mutex_init(&eng->one_lock, NULL);
    pthread_mutex_init(&eng->spare_lock, NULL);
    eng->device = device;
    eng->fitted = true;
    /* no coder, no key: huffman.c's cache never holds such an engine.  Every decision the host makes from a coder reads
     * one of these bounds (row_walk's certain steps, image and stage sizes, the one-pass rule, the capacity sums), and a
     * fit keeps within them: plans made before a fit stay good behind it */
    eng->can_encode = eng->can_decode = true;
    eng->tables.enc_min_bits = eng->tables.min_bits = min_bits;
    eng->tables.enc_max_bits = eng->tables.max_bits = eng->tables.lut_bits = max_bits;
    eng->tables.n_states = max_bits > 8 ? max_bits : 8;
    eng->tables.all_coded = 1;
    {
        const uint32_t road = testing_encode_road();
        eng->single_pass = !(road & AWS_HUFFMAN_AMD_TEST_ENCODE_THREE_KERNEL);
        eng->encode_fails = (road & AWS_HUFFMAN_AMD_TEST_ENCODE_ONE_PASS_FAILS) != 0;
    }
    int err = engine_streams_create(eng);
    if (!err) {
        eng->d_enc_table = hufs_malloc(256 * sizeof(uint64_t));
        eng->d_dec_lut = hufs_malloc((size_t)sizeof(uint16_t) << max_bits);
        err = eng->d_enc_table && eng->d_dec_lut ? 0 : 2;
    }
    if (err) {
        aws_huffman_amd_engine_destroy(eng);
        return raise_hip(err);
    }
    eng->tables.enc_table = eng->d_enc_table;
    eng->tables.dec_lut = eng->d_dec_lut;
    *out_engine = eng;
    return AWS_OP_SUCCESS;
}

bool aws_huffman_amd_engine_is_fitted(const struct aws_huffman_amd_engine *eng) {
    return eng && eng->fitted;
}

static int engine_fit(
    struct aws_huffman_amd_engine *eng, const uint64_t *device_counts, const uint8_t *device_lengths, uint8_t *device_num_bits,
    uint32_t *device_status, void *stream) {
    const uint32_t lo = eng->tables.min_bits, hi = eng->tables.max_bits;
    /* what the selection of the kernel (and of coder_build.c) stands on: X = 256 - 2^lo symbols too many for lo bits
     * (none at 8), and the 2 X items it takes of the first list are there -- that list has 512 - 2^(9 - D) items */
    assert(lo >= 4 && lo <= 8 && hi >= 8 && hi <= 12 && lo < hi);
    assert(lo == 8 || 2u * (256u - (1u << lo)) <= 512u - (512u >> (hi - lo)));
    ON_DEVICE(eng->device);
    const int err = hufk_fit_tables(
        device_lengths != NULL, device_counts, device_lengths, lo, hi, eng->d_enc_table, eng->d_dec_lut, device_num_bits, device_status,
        stream ? stream : eng->stream);
    if (err) {
        return raise_hip(err);
    }
    eng->fit_enqueued = true;
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_engine_fit_counts(
    struct aws_huffman_amd_engine *eng, const uint64_t *device_counts, uint8_t *device_num_bits, uint32_t *device_status, void *stream) {
    if (!eng || !eng->fitted || !device_counts || ((uintptr_t)device_counts & 7u) || ((uintptr_t)device_status & 3u)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    return engine_fit(eng, device_counts, NULL, device_num_bits, device_status, stream);
}

int aws_huffman_amd_engine_fit_lengths(
    struct aws_huffman_amd_engine *eng, const uint8_t *device_num_bits, uint32_t *device_status, void *stream) {
    if (!eng || !eng->fitted || !device_num_bits || ((uintptr_t)device_status & 3u)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    return engine_fit(eng, NULL, device_num_bits, NULL, device_status, stream);
}

int aws_huffman_amd_testing_engine_tables(
    struct aws_huffman_amd_engine *eng, uint64_t enc_table[256], uint16_t *dec_lut, size_t dec_lut_entries) {
    if (!eng || !enc_table || !dec_lut || !eng->d_enc_table || !eng->d_dec_lut ||
        dec_lut_entries != (size_t)1 << eng->tables.lut_bits) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    ON_DEVICE(eng->device);
    int err = hufs_copy_d2h(enc_table, eng->d_enc_table, 256 * sizeof(uint64_t), eng->stream);
    if (!err) {
        err = hufs_copy_d2h(dec_lut, eng->d_dec_lut, dec_lut_entries * sizeof(uint16_t), eng->stream);
    }
    if (!err) {
        err = hufs_stream_sync(eng->stream);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

/* a plan of an engine whose tables nobody has written yet is not launched */
static bool engine_never_fitted(const struct aws_huffman_amd_engine *eng) {
    return eng->fitted && !eng->fit_enqueued;
}

/* ------------------------------------------------------------------ encode plans */

#define ENC_PLAN_ARRAYS(X, ci, cs, cl, ct)                                                                                 \
    X(d_items, (ci) * sizeof(struct hufd_enc_item))                                                                    \
    X(d_segs, (cs) * sizeof(struct hufd_enc_seg))                                                                      \
    X(d_large, (cl) * sizeof(uint32_t))                                                                                \
    X(d_tiny, (ct) * sizeof(uint32_t))                                                                                 \
    X(d_solo, (ci) * sizeof(uint32_t))                                                                                 \
    X(d_seg_bits, (cs) * sizeof(uint32_t))                                                                             \
    X(d_wave_bits, (cs) * 4 * sizeof(uint32_t))                                                                        \
    X(d_seg_unk, (cs) * sizeof(uint32_t))                                                                              \
    X(d_seg_bitoff, (cs) * sizeof(uint64_t))                                                                           \
    /* the scan lists up to two segments an item, the wave packer any segment it leaves */                              \
    X(d_careful, (2 * (ci) + (cs) + 4) * sizeof(uint32_t))                                                             \
    X(d_zero, hufk_encode_zero_bytes((uint32_t)(cs), (uint32_t)(ci)))                                                  \
    X(d_unk_seen, (cs))                                                                                                \
    X(d_item_total, (ci) * sizeof(uint64_t))                                                                           \
    X(d_states, (ci) * sizeof(struct hufd_enc_item_state))                                                             \
    X(d_results, (ci) * sizeof(struct hufd_enc_result))

static void enc_plan_release_device(struct aws_huffman_amd_encode_plan *p) {
    hufs_free(p->d_arena);
    p->d_arena = NULL;
#define ENC_FORGET(name, bytes) p->name = NULL;
    ENC_PLAN_ARRAYS(ENC_FORGET, 0, 0, 0, 0)
#undef ENC_FORGET
    p->cap_items = p->cap_segs = p->cap_large = p->cap_tiny = 0;
}

/* short items with anything to write (symbols or carried bits) are one thread's work, without segments */
/* fewer items than this: the host's loop over them costs less than an allocation and a launch */
#define PLAN_ON_DEVICE_MIN_ITEMS 4096u

/* items per byte of the longest item from which a length class goes to a thread per item (HUFD_*_TINY_PER_BYTE; the tests
 * set other numbers: aws_huffman_amd_testing_set_items_per_byte) */
static uint64_t tiny_per_byte(bool decode) {
    const uint64_t asked = __atomic_load_n(&s_testing_per_byte[decode], __ATOMIC_RELAXED);
    return asked ? asked : (decode ? HUFD_DEC_TINY_PER_BYTE : HUFD_ENC_TINY_PER_BYTE);
}

/* ... and for an encoder that packs ragged tiles in one pass (a wave a tile: ~1.6 ns an item whatever its length, where a lone
 * thread needs ~0.7 us a symbol of the LONGEST item): the thread road pays from ~430 items per byte on -- measured,
 * profiles/tools/mid_items.py: 447 K items of 300 B 1.02 ms by threads against 2.82 by tiles, but BASELINE configs[3]'s
 * 16 384 resume items of ~320 symbols 251 us by threads where tiles take a tenth */
static uint64_t enc_tiny_per_byte(const struct aws_huffman_amd_engine *eng) {
    const uint64_t asked = __atomic_load_n(&s_testing_per_byte[0], __ATOMIC_RELAXED);
    if (asked || !aws_huffman_amd_engine_encodes_in_one_pass(eng)) {
        return tiny_per_byte(false);
    }
    return HUFD_ENC_TINY_PER_BYTE_ONE_PASS;
}

struct item_stats { /* of a plan's items, from the pass that finds the thread-per-item limit */
    uint64_t shortest, longest;
    uint32_t worst_bits; /* largest first_bit (decode) / overflow_in.num_bits (encode) */
    uint64_t largest_out_cap; /* (encode) */
};

/* the caller's records go to the device as they are when every item of a plan is one thread's work: the kernels that
 * read them there (hufk_*_plan_tiny_items) see these layouts */
_Static_assert(sizeof(struct aws_huffman_amd_decode_item) == sizeof(struct hufd_raw_dec_item), "decode item layout");
_Static_assert(offsetof(struct aws_huffman_amd_decode_item, first_bit) == offsetof(struct hufd_raw_dec_item, first_bit), "decode item layout");
_Static_assert(offsetof(struct aws_huffman_amd_decode_item, out_offset) == offsetof(struct hufd_raw_dec_item, out_offset), "decode item layout");
_Static_assert(offsetof(struct aws_huffman_amd_decode_item, out_capacity) == offsetof(struct hufd_raw_dec_item, out_capacity), "decode item layout");
_Static_assert(sizeof(struct aws_huffman_amd_encode_item) == sizeof(struct hufd_raw_enc_item), "encode item layout");
_Static_assert(offsetof(struct aws_huffman_amd_encode_item, out_capacity) == offsetof(struct hufd_raw_enc_item, out_capacity), "encode item layout");
_Static_assert(offsetof(struct aws_huffman_amd_encode_item, overflow_in) == offsetof(struct hufd_raw_enc_item, ovf_pattern), "encode item layout");
_Static_assert(offsetof(struct aws_huffman_amd_encode_item, overflow_in) + offsetof(struct aws_huffman_code, num_bits) ==
                   offsetof(struct hufd_raw_enc_item, ovf_bits), "encode item layout");
_Static_assert(offsetof(struct aws_huffman_amd_encode_item, eos_padding) == offsetof(struct hufd_raw_enc_item, eos_padding), "encode item layout");

static bool enc_item_is_tiny(const struct aws_huffman_amd_encode_item *it, uint64_t limit) {
    return it->in_len <= limit && (it->in_len > 0 || it->overflow_in.num_bits);
}

/* the longest item a lone thread takes in this plan: see HUFD_ENC_TINY_PER_BYTE */
static uint64_t enc_tiny_limit(
    const struct aws_huffman_amd_engine *eng, const struct aws_huffman_amd_encode_item *items, size_t n_items, struct item_stats *st) {
    /* (the one-pass kernel packs ragged tiles at full speed: measured, a wave beats a thread from about 1 KiB an item) */
    const uint64_t classes[2] = {
        aws_huffman_amd_engine_encodes_in_one_pass(eng) ? HUFD_ENC_TINY_WAVE_BYTES : HUFD_TINY_MANY_BYTES, HUFD_ENC_TINY_BYTES};
    uint64_t count[2] = {0, 0}, longest[2] = {0, 0}; /* (one pass over the items for both classes) */
    st->shortest = UINT64_MAX;
    st->longest = 0;
    st->worst_bits = 0;
    st->largest_out_cap = 0;
    for (size_t i = 0; i < n_items; ++i) {
        const uint64_t len = items[i].in_len;
        st->shortest = len < st->shortest ? len : st->shortest;
        st->longest = len > st->longest ? len : st->longest;
        st->worst_bits = items[i].overflow_in.num_bits > st->worst_bits ? items[i].overflow_in.num_bits : st->worst_bits;
        st->largest_out_cap = items[i].out_capacity > st->largest_out_cap ? items[i].out_capacity : st->largest_out_cap;
        for (int c = 0; c < 2; ++c) {
            if (len <= classes[c]) {
                ++count[c];
                longest[c] = len > longest[c] ? len : longest[c];
            }
        }
    }
    for (int c = 0; c < 2; ++c) {
        if (longest[c] > HUFD_TINY_FEW_BYTES && count[c] >= enc_tiny_per_byte(eng) * longest[c]) {
            return classes[c];
        }
    }
    return HUFD_TINY_FEW_BYTES;
}

/* the longest item that is one wave's work without segments (enc_onepass<.., SOLO>: the one-pass packer, waiting for nobody) */
static uint64_t enc_solo_limit(const struct aws_huffman_amd_engine *eng, size_t n_items) {
    if (!aws_huffman_amd_engine_encodes_in_one_pass(eng)) {
        return 0;
    }
    return n_items >= HUFD_ENC_SOLO_MANY_ITEMS ? HUFD_ENC_SOLO_MANY_BYTES : HUFD_ENC_SOLO_BYTES;
}

static bool enc_item_is_solo(const struct aws_huffman_amd_encode_item *it, uint64_t tiny_limit, uint64_t solo_limit) {
    return !enc_item_is_tiny(it, tiny_limit) && it->in_len > 0 && it->in_len <= solo_limit;
}

static uint64_t enc_item_segments(const struct aws_huffman_amd_encode_item *it, uint64_t tiny_limit, uint64_t solo_limit) {
    if (enc_item_is_tiny(it, tiny_limit) || enc_item_is_solo(it, tiny_limit, solo_limit)) {
        return 0; /* one thread encodes it (enc_tiny), or one wave */
    }
    return (it->in_len + HUFD_ENC_SEG_BYTES - 1) / HUFD_ENC_SEG_BYTES;
}

/* (Re)fills a plan from host items, growing its device arrays when needed. */
/* the plan's device arrays for this many items, segments, large and thread-per-item items (grown, never shrunk); 0 or a HIP error */
static int enc_plan_reserve(struct aws_huffman_amd_encode_plan *p, size_t n_items, size_t n_segs, size_t n_large, size_t n_tiny) {
    if (n_items > p->cap_items || n_segs > p->cap_segs || n_large > p->cap_large || n_tiny > p->cap_tiny) {
        enc_plan_release_device(p);
        const size_t ci = n_items ? n_items : 1, cs = n_segs ? n_segs : 1, cl = n_large ? n_large : 1, ct = n_tiny ? n_tiny : 1;
#define ENC_PART(name, bytes) {&p->name, (bytes)},
        const struct arena_part parts[] = {ENC_PLAN_ARRAYS(ENC_PART, ci, cs, cl, ct)};
#undef ENC_PART
        if (arena_alloc(&p->d_arena, ARENA_PARTS(parts))) {
            return 2;
        }
        p->cap_items = ci;
        p->cap_segs = cs;
        p->cap_large = cl;
        p->cap_tiny = ct;
        /* the one-pass encoder's look-back block starts out clear; from then on every launch clears it behind itself */
        int e = hufs_memset(p->d_zero, 0, (size_t)hufk_encode_zero_bytes((uint32_t)cs, (uint32_t)ci), p->engine->stream);
        if (!e) {
            e = hufs_stream_sync(p->engine->stream);
        }
        if (e) {
            return e;
        }
        p->zero_is_clear = true;
    }
    return 0;
}

static int enc_plan_fill(
    struct aws_huffman_amd_encode_plan *p,
    const struct aws_huffman_amd_encode_item *items,
    size_t n_items) {

    struct aws_huffman_amd_engine *eng = p->engine;
    if (!eng->can_encode) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION); /* a coder without an encode callback: good for decoding only */
    }
    struct item_stats stats;
    const uint64_t tiny_limit = enc_tiny_limit(eng, items, n_items, &stats);
    /* a failed refill must not leave counts of the fill before behind (the device arrays may be gone or too small) */
    p->n_items = p->n_segs = p->n_large = p->n_tiny = p->n_solo = 0;
    p->launched = false; /* (the records of a launch of other items say nothing about these) */
    memset(&p->stats, 0, sizeof(p->stats));
    p->largest_out_cap = stats.largest_out_cap;
    p->most_overflow_bits = stats.worst_bits;
    p->longest_in_len = stats.longest;
    p->packed = p->packed_sized = p->stored = p->constant = false;
    p->block_indexed = false;
    if (n_items >= PLAN_ON_DEVICE_MIN_ITEMS && n_items < 0xFFFFFFFFull && stats.shortest >= 1 && stats.longest <= tiny_limit &&
        stats.worst_bits <= 32) {
        /* every item is one thread's work (enc_item_is_tiny): no segments, no lists to make -- the caller's records go to the
         * device as they are and become the kernels' there (hufk_encode_plan_tiny_items) */
        ON_DEVICE(eng->device);
        int e = enc_plan_reserve(p, n_items, 0, 0, n_items);
        void *d_raw = e ? NULL : hufs_malloc(n_items * sizeof(*items));
        if (!e && !d_raw) {
            e = 2;
        }
        if (!e) {
            e = hufs_copy_h2d(d_raw, items, n_items * sizeof(*items), eng->stream);
        }
        if (!e) {
            e = hufk_encode_plan_tiny_items(d_raw, (uint32_t)n_items, p->d_items, p->d_tiny, eng->stream);
        }
        if (!e) {
            e = hufs_stream_sync(eng->stream);
        }
        hufs_free(d_raw);
        if (e) {
            return raise_hip(e);
        }
        p->n_items = (uint32_t)n_items;
        p->n_tiny = (uint32_t)n_items;
        p->stats.items = p->stats.by_thread = n_items;
        p->stats.thread_limit = tiny_limit;
        return AWS_OP_SUCCESS;
    }
    const uint64_t solo_limit = enc_solo_limit(eng, n_items);
    uint64_t n_segs = 0, n_large = 0, n_tiny = 0, n_cut = 0, n_solo = 0;
    for (size_t i = 0; i < n_items; ++i) {
        if (items[i].overflow_in.num_bits > 32) {
            return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
        }
        const uint64_t segs = enc_item_segments(&items[i], tiny_limit, solo_limit);
        n_segs += segs;
        n_large += segs > HUFD_SCAN_SMALL_MAX;
        n_tiny += enc_item_is_tiny(&items[i], tiny_limit);
        n_solo += enc_item_is_solo(&items[i], tiny_limit, solo_limit);
        n_cut += segs != 0;
    }
    if (n_segs >= 0xFFFFFFFFull || n_items >= 0xFFFFFFFFull || n_solo >= (1ull << 30)) { /* (tile numbers are 32 bits: four tiles a wave's item) */
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }

    struct hufd_enc_item *h_items = malloc((n_items ? n_items : 1) * sizeof(*h_items));
    struct hufd_enc_seg *h_segs = malloc((n_segs ? n_segs : 1) * sizeof(*h_segs));
    uint32_t *h_large = malloc((n_large ? n_large : 1) * sizeof(uint32_t));
    uint32_t *h_tiny = malloc((n_tiny ? n_tiny : 1) * sizeof(uint32_t));
    uint32_t *h_solo = malloc((n_solo ? n_solo : 1) * sizeof(uint32_t));
    if (!h_items || !h_segs || !h_large || !h_tiny || !h_solo) {
        free(h_items);
        free(h_segs);
        free(h_large);
        free(h_tiny);
        free(h_solo);
        return aws_raise_error(AWS_ERROR_OOM);
    }
    uint32_t seg = 0, large = 0, tiny = 0, solo = 0;
    for (size_t i = 0; i < n_items; ++i) {
        const struct aws_huffman_amd_encode_item *src = &items[i];
        struct hufd_enc_item *dst = &h_items[i];
        const uint32_t segs = (uint32_t)enc_item_segments(src, tiny_limit, solo_limit);
        const uint32_t ob = src->overflow_in.num_bits;
        dst->in_off = src->in_offset;
        dst->in_len = src->in_len;
        dst->out_off = src->out_offset;
        dst->out_cap = src->out_capacity;
        dst->ovf_bits = ob;
        dst->ovf_pattern = ob == 0 ? 0 : (ob == 32 ? src->overflow_in.pattern : src->overflow_in.pattern & ((1u << ob) - 1u));
        dst->eos_padding = src->eos_padding;
        dst->first_seg = seg;
        dst->n_segs = segs;
        dst->tiny = enc_item_is_tiny(src, tiny_limit) ? 1u : (enc_item_is_solo(src, tiny_limit, solo_limit) ? 2u : 0u);
        if (dst->tiny == 1) {
            h_tiny[tiny++] = (uint32_t)i;
        } else if (dst->tiny == 2) {
            h_solo[solo++] = (uint32_t)i;
        }
        for (uint32_t k = 0; k < segs; ++k) {
            struct hufd_enc_seg *sd = &h_segs[seg++];
            const uint64_t off = (uint64_t)k * HUFD_ENC_SEG_BYTES;
            const uint64_t left = src->in_len > off ? src->in_len - off : 0;
            const uint64_t after = left > HUFD_ENC_SEG_BYTES ? left - HUFD_ENC_SEG_BYTES : 0;
            sd->in_off = src->in_offset + off;
            sd->len = (uint32_t)(left < HUFD_ENC_SEG_BYTES ? left : HUFD_ENC_SEG_BYTES);
            sd->item = (uint32_t)i;
            sd->index = k;
            sd->flags = (k == 0 ? 1u : 0u) | (k + 1 == segs ? 2u : 0u);
            sd->next_len = (uint32_t)(after < HUFD_ENC_SEG_BYTES ? after : HUFD_ENC_SEG_BYTES);
            sd->reserved = 0;
        }
        if (segs > HUFD_SCAN_SMALL_MAX) {
            h_large[large++] = (uint32_t)i;
        }
    }

    int err = 0;
    ON_DEVICE(eng->device);
    err = enc_plan_reserve(p, n_items, n_segs, n_large, n_tiny);
    if (!err) {
        err = hufs_copy_h2d(p->d_items, h_items, n_items * sizeof(*h_items), eng->stream);
    }
    if (!err) {
        err = hufs_copy_h2d(p->d_segs, h_segs, n_segs * sizeof(*h_segs), eng->stream);
    }
    if (!err) {
        err = hufs_copy_h2d(p->d_large, h_large, n_large * sizeof(uint32_t), eng->stream);
    }
    if (!err) {
        err = hufs_copy_h2d(p->d_tiny, h_tiny, n_tiny * sizeof(uint32_t), eng->stream);
    }
    if (!err) {
        err = hufs_copy_h2d(p->d_solo, h_solo, n_solo * sizeof(uint32_t), eng->stream);
    }
    if (!err) {
        err = hufs_stream_sync(eng->stream);
    }
    free(h_items);
    free(h_segs);
    free(h_large);
    free(h_tiny);
    free(h_solo);
    if (err) {
        return raise_hip(err);
    }
    p->n_items = (uint32_t)n_items;
    p->n_segs = (uint32_t)n_segs;
    p->n_large = (uint32_t)n_large;
    p->n_tiny = (uint32_t)n_tiny;
    p->n_solo = (uint32_t)n_solo;
    p->stats.items = n_items;
    p->stats.thread_limit = tiny_limit;
    p->stats.by_thread = n_tiny;
    p->stats.by_wave = n_solo;
    p->stats.by_pieces = n_cut;
    p->stats.pieces = n_segs;
    p->stats.empty = n_items - n_tiny - n_solo - n_cut;
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_encode_plan_stats(const struct aws_huffman_amd_encode_plan *plan, struct aws_huffman_amd_plan_stats *stats) {
    *stats = plan->stats;
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_decode_plan_stats(const struct aws_huffman_amd_decode_plan *plan, struct aws_huffman_amd_plan_stats *stats) {
    *stats = plan->stats;
    return AWS_OP_SUCCESS;
}

bool aws_huffman_amd_engine_encodes_in_one_pass(const struct aws_huffman_amd_engine *eng) {
    return eng->single_pass && hufk_encode_one_pass_applies(&eng->tables);
}

int aws_huffman_amd_encode_plan_new(
    struct aws_huffman_amd_encode_plan **out_plan,
    struct aws_huffman_amd_engine *eng,
    const struct aws_huffman_amd_encode_item *items,
    size_t item_count) {

    *out_plan = NULL;
    /* the plan destroyed last, if the engine kept it: its device arrays serve again where they are large enough */
    pthread_mutex_lock(&eng->spare_lock);
    struct aws_huffman_amd_encode_plan *p = eng->spare_enc;
    eng->spare_enc = NULL;
    pthread_mutex_unlock(&eng->spare_lock);
    if (p) {
        /* its last launch may still run on the caller's stream (freeing the arrays used to wait for it): waited for by the
         * event that launch left behind -- not for every stream of the device, on which other threads' batches may run */
        ON_DEVICE(eng->device);
        if (plan_wait_done(p->done_event, p->done_on_engine_stream, eng)) {
            p->unkeepable = true; /* (freed, not parked again for the next caller to fail on) */
            aws_huffman_amd_encode_plan_destroy(p);
            return aws_raise_error(AWS_ERROR_UNKNOWN);
        }
        p->done_on_engine_stream = false;
        p->last_input = NULL;
        p->last_output = NULL;
        p->launched = false;
        p->last_single_pass = false;
        p->last_timed_out = false;
        p->look_back_timed_out = false;
    } else {
        p = calloc(1, sizeof(*p));
        if (!p) {
            return aws_raise_error(AWS_ERROR_OOM);
        }
        p->engine = eng;
    }
    if (enc_plan_fill(p, items, item_count)) {
        aws_huffman_amd_encode_plan_destroy(p);
        return AWS_OP_ERR;
    }
    *out_plan = p;
    return AWS_OP_SUCCESS;
}

/* the scratch a planning pass on the device wants, grown as needed */
static int plan_scratch_reserve(void **scratch, size_t *cap, size_t n_items) {
    const size_t want = (size_t)hufk_plan_scratch_bytes(n_items);
    if (want > *cap) {
        hufs_free(*scratch);
        *scratch = hufs_malloc(want);
        *cap = *scratch ? want : 0;
    }
    return *scratch ? 0 : 2;
}

/* A plan from items the host does not look at (plan_kernels.hip): described by a stride, or lying in device memory.  Three
 * small launches count, one copy brings a few totals back (the wait of the call), then the records are written on `stream`:
 * the plan is good for launches on that stream, or on another once this one has been waited for. */
static int enc_plan_fill_on_device(struct aws_huffman_amd_encode_plan *p, const struct hufd_item_source *src, size_t n_items, void *stream) {
    struct aws_huffman_amd_engine *eng = p->engine;
    if (!eng->can_encode) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    p->n_items = p->n_segs = p->n_large = p->n_tiny = p->n_solo = 0;
    p->launched = false;
    p->look_back_timed_out = false;
    memset(&p->stats, 0, sizeof(p->stats));
    p->largest_out_cap = 0;
    p->most_overflow_bits = 0;
    p->longest_in_len = 0;
    p->packed = p->packed_sized = p->stored = p->constant = false;
    p->block_indexed = false;
    if (n_items == 0) {
        return AWS_OP_SUCCESS;
    }
    if (n_items >= 0xFFFFFFFFull) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    void *st = stream ? stream : eng->stream;
    ON_DEVICE(eng->device);
    struct hufk_plan_totals t;
    int e = plan_scratch_reserve(&p->d_plan_scratch, &p->cap_plan_scratch, n_items);
    if (!e) {
        const uint64_t class0 = aws_huffman_amd_engine_encodes_in_one_pass(eng) ? HUFD_ENC_TINY_WAVE_BYTES : HUFD_TINY_MANY_BYTES;
        e = hufk_encode_plan_count(
            src, (uint32_t)n_items, class0, HUFD_ENC_TINY_BYTES, enc_tiny_per_byte(eng), enc_solo_limit(eng, n_items), p->d_plan_scratch, &t, st);
    }
    if (e) {
        return raise_hip(e);
    }
    if (t.invalid || t.totals[0] >= 0xFFFFFFFFull || t.totals[2] >= (1ull << 30)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    e = enc_plan_reserve(p, n_items, (size_t)t.totals[0], (size_t)t.totals[3], (size_t)t.totals[1]);
    if (!e) {
        e = hufk_encode_plan_fill(
            src, (uint32_t)n_items, (uint32_t)t.totals[0], enc_solo_limit(eng, n_items), p->d_plan_scratch, p->d_items, p->d_segs, p->d_tiny,
            p->d_large, p->d_solo, st);
    }
    if (e) {
        return raise_hip(e);
    }
    p->n_items = (uint32_t)n_items;
    p->n_segs = (uint32_t)t.totals[0];
    p->n_large = (uint32_t)t.totals[3];
    p->n_tiny = (uint32_t)t.totals[1];
    p->n_solo = (uint32_t)t.totals[2];
    p->largest_out_cap = t.largest_out_cap;
    p->most_overflow_bits = t.worst_bits;
    p->longest_in_len = t.longest;
    p->stats.items = n_items;
    p->stats.thread_limit = t.tiny_limit;
    p->stats.by_thread = t.totals[1];
    p->stats.by_wave = t.totals[2];
    p->stats.by_pieces = t.totals[7];
    p->stats.pieces = t.totals[0];
    p->stats.empty = n_items - t.totals[1] - t.totals[2] - t.totals[7];
    /* the record-writing kernels run on `st` behind the one wait above: whoever gets this plan's arrays next (a plan
     * destroyed before any launch is the engine's spare) waits for them as for a launch */
    e = plan_mark_done(&p->done_event, &p->done_on_engine_stream, eng, stream);
    return e ? raise_hip(e) : AWS_OP_SUCCESS;
}

static void strided_source(struct hufd_item_source *src, const struct aws_huffman_amd_strided_items *items) {
    memset(src, 0, sizeof(*src));
    src->kind = HUFD_ITEMS_STRIDED;
    src->first_bit = items->first_bit;
    src->eos_padding = items->eos_padding;
    src->in_offset = items->in_offset;
    src->in_stride = items->in_stride;
    src->in_len = items->in_len;
    src->out_offset = items->out_offset;
    src->out_stride = items->out_stride;
    src->out_capacity = items->out_capacity;
}

int aws_huffman_amd_encode_plan_reset_strided(
    struct aws_huffman_amd_encode_plan *p, const struct aws_huffman_amd_strided_items *items, void *stream) {
    struct hufd_item_source src;
    strided_source(&src, items);
    return enc_plan_fill_on_device(p, &src, (size_t)items->count, stream);
}

int aws_huffman_amd_encode_plan_reset_device_items(
    struct aws_huffman_amd_encode_plan *p, const struct aws_huffman_amd_encode_item *device_items, size_t item_count, void *stream) {
    struct hufd_item_source src;
    memset(&src, 0, sizeof(src));
    src.kind = HUFD_ITEMS_DEVICE_ARRAY;
    src.raw = device_items;
    return enc_plan_fill_on_device(p, &src, item_count, stream);
}

int aws_huffman_amd_encode_plan_reset(
    struct aws_huffman_amd_encode_plan *p,
    const struct aws_huffman_amd_encode_item *items,
    size_t item_count) {
    p->look_back_timed_out = false;
    return enc_plan_fill(p, items, item_count); /* (device arrays are kept where they are large enough) */
}

void aws_huffman_amd_encode_plan_destroy(struct aws_huffman_amd_encode_plan *p) {
    if (p) {
        struct aws_huffman_amd_engine *eng = p->engine;
        /* the engine keeps ONE destroyed plan with its device arrays for the next aws_huffman_amd_encode_plan_new */
        pthread_mutex_lock(&eng->spare_lock);
        const bool keep = !eng->retiring && !eng->spare_enc && p->cap_items && p != eng->one_enc && !p->unkeepable;
        if (keep) {
            eng->spare_enc = p;
        }
        pthread_mutex_unlock(&eng->spare_lock);
        if (keep) {
            return;
        }
        ON_DEVICE(eng->device);
        enc_plan_release_device(p);
        hufs_free(p->d_packed_arena);
        hufs_free(p->d_block_index_arena);
        hufs_free(p->d_plan_scratch);
        hufs_event_destroy(p->done_event);
        free(p);
    }
}

int aws_huffman_amd_encode_plan_launch(
    struct aws_huffman_amd_encode_plan *p,
    const void *device_input,
    void *device_output,
    bool length_only,
    void *stream) {
    return aws_huffman_amd_encode_plan_launch_staged(p, device_input, device_output, length_only, stream, NULL);
}

/* one launch of the plan's lists over `items`: the plan's own records, or the ones a packed launch has rewritten */
static int enc_plan_launch_items(
    struct aws_huffman_amd_encode_plan *p,
    const struct hufd_enc_item *items,
    const void *device_input,
    void *device_output,
    bool length_only,
    void *stream,
    void **stage_events) {

    struct hufk_encode_args a;
    memset(&a, 0, sizeof(a));
    a.tables = p->engine->tables;
    a.items = items;
    a.n_items = p->n_items;
    a.segs = p->d_segs;
    a.n_segs = p->n_segs;
    a.large_items = p->d_large;
    a.tiny_items = p->d_tiny;
    a.n_tiny = p->n_tiny;
    a.solo_items = p->d_solo;
    a.n_solo = p->n_solo;
    a.n_large = p->n_large;
    a.length_only = length_only;
    a.d_in = device_input;
    a.d_out = device_output;
    a.seg_bits = p->d_seg_bits;
    a.wave_bits = p->d_wave_bits;
    a.seg_unk = p->d_seg_unk;
    a.seg_bitoff = p->d_seg_bitoff;
    a.careful_list = p->d_careful;
    a.zero_block = p->d_zero;
    a.zero_is_clear = p->zero_is_clear;
    a.zero_bytes = hufk_encode_zero_bytes((uint32_t)p->cap_segs, (uint32_t)p->cap_items);
    a.careful_count = (uint32_t *)p->d_zero + 2;
    a.seg_unk_seen = p->d_unk_seen;
    a.item_total = p->d_item_total;
    a.single_pass = p->engine->single_pass && !p->look_back_timed_out;
    a.fail_tile = p->engine->encode_fails;
    p->last_input = device_input;
    p->last_output = device_output;
    if (!length_only) {
        p->stored = p->constant = false; /* (a stored launch says so behind its encode pass) */
    }
    p->launched = !length_only; /* (a length query leaves lengths in the records and no output: nothing to chain a decode to) */
    p->last_single_pass =
        a.single_pass && (p->n_segs || p->n_solo) && !length_only && hufk_encode_one_pass_applies(&p->engine->tables);
    a.states = p->d_states;
    a.results = p->d_results;
    a.stage_events = stage_events;
    ON_DEVICE(p->engine->device);
    int err = hufk_encode_launch(&a, stream ? stream : p->engine->stream);
    if (p->last_single_pass) {
        p->zero_is_clear = !err; /* (the launch leaves the block clear behind itself -- unless it could not be queued whole) */
    }
    if (!err) {
        err = plan_mark_done(&p->done_event, &p->done_on_engine_stream, p->engine, stream);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

int aws_huffman_amd_encode_plan_launch_staged(
    struct aws_huffman_amd_encode_plan *p,
    const void *device_input,
    void *device_output,
    bool length_only,
    void *stream,
    void **stage_events) {
    if (engine_never_fitted(p->engine)) {
        return aws_raise_error(AWS_ERROR_INVALID_STATE);
    }
    if (!length_only) {
        p->packed = false; /* (the output lies where the plan's own records say) */
    }
    return enc_plan_launch_items(p, p->d_items, device_input, device_output, length_only, stream, stage_events);
}

/* ------------------------------------------------------------------ packed launches (huffman_amd_packed.h) */

static uint32_t s_pack_tile_items = 0;

void aws_huffman_amd_testing_set_pack_tile_items(uint32_t items) {
    __atomic_store_n(&s_pack_tile_items, items, __ATOMIC_RELAXED);
}

/* the second record array, the scan's tile sums and its summary words for this many items and tiles (grown, never
 * shrunk): an allocation, so not inside a graph capture -- the first packed launch of a plan, or of more items */
static int enc_plan_reserve_packed(struct aws_huffman_amd_encode_plan *p, size_t n_items, size_t n_tiles) {
    if (p->d_packed_arena && n_items <= p->cap_packed_items && n_tiles <= p->cap_pack_tiles) {
        return 0;
    }
    p->cap_packed_items = p->cap_pack_tiles = 0;
    const size_t ci = n_items > p->cap_items ? n_items : p->cap_items; /* as many as the plan's own array: a reset within it allocates nothing */
    const struct arena_part parts[] = {
        {&p->d_packed_items, ci * sizeof(struct hufd_enc_item)},
        {&p->d_pack_tile_sums, 2 * n_tiles * sizeof(uint64_t)},
        {&p->d_pack_summary, 6 * sizeof(uint64_t)}, /* (the last four: a stored launch's counts, a constant launch's) */
        {&p->d_pack_differs, ci}};
    p->pack_differs_clear = false;
    if (arena_alloc(&p->d_packed_arena, ARENA_PARTS(parts))) {
        return 2;
    }
    p->cap_packed_items = ci;
    p->cap_pack_tiles = n_tiles;
    return 0;
}

/* what a packed launch asks of its own arguments (the plan is not looked into) */
static bool packed_launch_args_ok(
    const struct aws_huffman_amd_encode_plan *p, const void *device_output, uint64_t output_capacity, const uint64_t *device_offsets,
    uint32_t align) {
    return p && device_offsets && !((uintptr_t)device_offsets & 7u) && align != 0 && align <= 4096 && !(align & (align - 1)) &&
           (device_output || !output_capacity);
}

/* what a launch that makes the batch's block index on the way is given for it (huffman_amd_packed_index.h), and
 * aws_huffman_amd_encode_plan_block_index as well */
struct enc_plan_index_args {
    uint64_t block_symbols;
    struct aws_huffman_amd_item_blocks *directory;
    uint64_t *index;
    uint64_t index_capacity;
    uint32_t *status;
};
static bool enc_plan_block_index_args_ok(
    const struct aws_huffman_amd_encode_plan *p, const void *device_input, const struct enc_plan_index_args *ix);
static int enc_plan_block_index_enqueue(
    struct aws_huffman_amd_encode_plan *p, const void *device_input, const struct enc_plan_index_args *ix, void *stream);

/* the tail of a stored launch (huffman_amd_stored.h), behind the encode pass over the second record array: the copy of the
 * stored items and their records, and the plan's state */
static int enc_plan_launch_stored_copy(
    struct aws_huffman_amd_encode_plan *p,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    const uint64_t *device_offsets,
    const uint8_t *device_stored,
    bool constant, /* device_stored holds kinds: the 9 bytes and the records of the constant items, and the detection's marks cleared */
    void *stream) {

    ON_DEVICE(p->engine->device);
    int e = hufk_stored_copy_encode(
        p->d_items, p->n_items, p->d_segs, p->n_segs, p->d_solo, p->n_solo, p->d_tiny, p->n_tiny, device_stored, device_offsets,
        output_capacity, device_input, device_output, p->d_results, p->d_pack_summary + 2, constant ? p->d_pack_differs : NULL,
        stream ? stream : p->engine->stream);
    if (constant) {
        p->pack_differs_clear = !e;
    }
    if (!e) {
        e = plan_mark_done(&p->done_event, &p->done_on_engine_stream, p->engine, stream);
    }
    if (e) {
        /* (raw items were not placed: neither the records, nor the layout, nor the sizes are what a fetch, a chained plan or
         * a size query should read) */
        p->launched = p->packed = p->packed_sized = false;
        return raise_hip(e);
    }
    p->stored = true;
    p->constant = constant;
    return AWS_OP_SUCCESS;
}

/*
 * Every packed launch of an encode plan; the caller has checked the arguments.  Three stages on one stream:
 *   - the lengths: a length pass into the plan's result records, or (ix) the batch's block index, whose hot pass reads the
 *     symbols once and leaves the coded lengths in the index;
 *   - the scan: the offsets and the second record array from those lengths; with `device_stored` it also decides which items
 *     are stored raw, flags them and gives them no room in the second record array; `constant` (huffman_amd_constant.h): the
 *     detection of constant items runs in front of the scan, whose flags are then kinds;
 *   - the encode pass over that array (its records replace the lengths), and behind it the copy of the stored items.
 */
static int enc_plan_launch_packed_any(
    struct aws_huffman_amd_encode_plan *p,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint32_t align,
    uint8_t *device_stored, /* NULL: no item is stored */
    bool constant, /* (with device_stored, without ix) */
    const struct enc_plan_index_args *ix, /* NULL: no index is made */
    void *stream) {

    if (engine_never_fitted(p->engine)) {
        return aws_raise_error(AWS_ERROR_INVALID_STATE);
    }
    void *st = stream ? stream : p->engine->stream;
    uint32_t tile_items = 0;
    if (p->n_items) {
        /* the scan's tile, with the second record array and the scan's scratch reserved: before anything is enqueued */
        tile_items = hufk_pack_tile_items(p->n_items, __atomic_load_n(&s_pack_tile_items, __ATOMIC_RELAXED));
        ON_DEVICE(p->engine->device);
        const int e = enc_plan_reserve_packed(p, p->n_items, hufk_pack_tiles(p->n_items, tile_items));
        if (e) {
            return raise_hip(e);
        }
    }
    /* (a plan without items still gets its index: the directory's one record, index[0] and the status) */
    if (ix ? enc_plan_block_index_enqueue(p, device_input, ix, stream)
           : (p->n_items && enc_plan_launch_items(p, p->d_items, device_input, device_output, true, stream, NULL))) {
        return AWS_OP_ERR;
    }
    ON_DEVICE(p->engine->device);
    if (p->n_items == 0) { /* offsets[0] = 0, and a size of nothing */
        int e = hufs_memset(device_offsets, 0, sizeof(uint64_t), st);
        if (e) {
            return raise_hip(e);
        }
        p->packed = false;
        p->packed_sized = true;
        p->stored = device_stored != NULL;
        p->constant = constant;
        /* (the index read the plan's records and scratch on this stream: whoever gets its arrays next waits, as for a launch) */
        e = ix ? plan_mark_done(&p->done_event, &p->done_on_engine_stream, p->engine, stream) : 0;
        return e ? raise_hip(e) : AWS_OP_SUCCESS;
    }
    const uint64_t *directory = ix ? (const uint64_t *)ix->directory : NULL;
    if (constant) {
        /* the marks: clear from the launch in front, or cleared here (a fresh array, a launch that failed half way) */
        int e = p->pack_differs_clear ? 0 : hufs_memset(p->d_pack_differs, 0, p->cap_packed_items, st);
        p->pack_differs_clear = false; /* (until the copy behind the encode pass has been queued) */
        if (!e) {
            e = hufk_constant_detect(
                p->d_items, p->n_items, p->d_segs, p->n_segs, p->d_solo, p->n_solo, p->d_tiny, p->n_tiny, device_input,
                p->d_pack_differs, st);
        }
        if (e) {
            return raise_hip(e);
        }
    }
    const int e =
        constant ? hufk_pack_offsets_constant(
                       p->d_items, p->d_results, p->n_items, tile_items, align, output_capacity, p->d_pack_tile_sums, device_offsets,
                       p->d_packed_items, p->d_pack_summary, device_stored, p->d_pack_differs, st) :
        ix ? (device_stored ? hufk_pack_offsets_stored_indexed(
                                  p->d_items, p->n_items, tile_items, align, output_capacity, directory, ix->index, ix->index_capacity,
                                  p->d_pack_tile_sums, device_offsets, p->d_packed_items, p->d_pack_summary, device_stored, st)
                            : hufk_pack_offsets_indexed(
                                  p->d_items, p->n_items, tile_items, align, output_capacity, directory, ix->index, ix->index_capacity,
                                  p->d_pack_tile_sums, device_offsets, p->d_packed_items, p->d_pack_summary, st))
           : (device_stored ? hufk_pack_offsets_stored(
                                  p->d_items, p->d_results, p->n_items, tile_items, align, output_capacity, p->d_pack_tile_sums,
                                  device_offsets, p->d_packed_items, p->d_pack_summary, device_stored, st)
                            : hufk_pack_offsets(
                                  p->d_items, p->d_results, p->n_items, tile_items, align, output_capacity, p->d_pack_tile_sums,
                                  device_offsets, p->d_packed_items, p->d_pack_summary, st));
    if (e) {
        return raise_hip(e);
    }
    if (enc_plan_launch_items(p, p->d_packed_items, device_input, device_output, false, stream, NULL)) {
        return AWS_OP_ERR;
    }
    p->packed = true;
    p->packed_sized = true;
    if (!device_stored) {
        return AWS_OP_SUCCESS;
    }
    return enc_plan_launch_stored_copy(p, device_input, device_output, output_capacity, device_offsets, device_stored, constant, stream);
}

int aws_huffman_amd_encode_plan_launch_packed(
    struct aws_huffman_amd_encode_plan *p,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint32_t align,
    void *stream) {

    if (!packed_launch_args_ok(p, device_output, output_capacity, device_offsets, align)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    return enc_plan_launch_packed_any(p, device_input, device_output, output_capacity, device_offsets, align, NULL, false, NULL, stream);
}

int aws_huffman_amd_encode_plan_launch_packed_constant(
    struct aws_huffman_amd_encode_plan *p,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint8_t *device_kinds,
    uint32_t align,
    void *stream) {

    if (!packed_launch_args_ok(p, device_output, output_capacity, device_offsets, align) || !device_kinds) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    return enc_plan_launch_packed_any(p, device_input, device_output, output_capacity, device_offsets, align, device_kinds, true, NULL, stream);
}

int aws_huffman_amd_encode_plan_launch_packed_stored(
    struct aws_huffman_amd_encode_plan *p,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint8_t *device_stored,
    uint32_t align,
    void *stream) {

    if (!packed_launch_args_ok(p, device_output, output_capacity, device_offsets, align) || !device_stored) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    return enc_plan_launch_packed_any(p, device_input, device_output, output_capacity, device_offsets, align, device_stored, false, NULL, stream);
}

int aws_huffman_amd_encode_plan_launch_packed_indexed(
    struct aws_huffman_amd_encode_plan *p,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint32_t align,
    uint64_t block_symbols,
    struct aws_huffman_amd_item_blocks *device_directory,
    uint64_t *device_index,
    uint64_t index_capacity,
    uint32_t *device_status,
    void *stream) {

    const struct enc_plan_index_args ix = {block_symbols, device_directory, device_index, index_capacity, device_status};
    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION); /* no GPU: there is no CPU path */
    }
    if (!packed_launch_args_ok(p, device_output, output_capacity, device_offsets, align) || !device_index ||
        !enc_plan_block_index_args_ok(p, device_input, &ix)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    return enc_plan_launch_packed_any(p, device_input, device_output, output_capacity, device_offsets, align, NULL, false, &ix, stream);
}

int aws_huffman_amd_encode_plan_launch_packed_stored_indexed(
    struct aws_huffman_amd_encode_plan *p,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint8_t *device_stored,
    uint32_t align,
    uint64_t block_symbols,
    struct aws_huffman_amd_item_blocks *device_directory,
    uint64_t *device_index,
    uint64_t index_capacity,
    uint32_t *device_status,
    void *stream) {

    const struct enc_plan_index_args ix = {block_symbols, device_directory, device_index, index_capacity, device_status};
    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION); /* no GPU: there is no CPU path */
    }
    if (!packed_launch_args_ok(p, device_output, output_capacity, device_offsets, align) || !device_stored || !device_index ||
        !enc_plan_block_index_args_ok(p, device_input, &ix)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    return enc_plan_launch_packed_any(p, device_input, device_output, output_capacity, device_offsets, align, device_stored, false, &ix, stream);
}

int aws_huffman_amd_encode_plan_stored_size(
    struct aws_huffman_amd_encode_plan *p,
    uint64_t *stored_items,
    uint64_t *stored_bytes,
    void *stream) {

    if (!p || !p->packed_sized || !p->stored) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    uint64_t counts[2] = {0, 0};
    if (plan_read_words(p->engine->device, p->n_items ? p->d_pack_summary + 2 : NULL, counts, 2, stream ? stream : p->engine->stream)) {
        return AWS_OP_ERR;
    }
    if (stored_items) {
        *stored_items = counts[0];
    }
    if (stored_bytes) {
        *stored_bytes = counts[1];
    }
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_encode_plan_constant_size(
    struct aws_huffman_amd_encode_plan *p,
    uint64_t *constant_items,
    uint64_t *constant_bytes,
    void *stream) {

    if (!p || !p->packed_sized || !p->constant) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    uint64_t counts[2] = {0, 0};
    if (plan_read_words(p->engine->device, p->n_items ? p->d_pack_summary + 4 : NULL, counts, 2, stream ? stream : p->engine->stream)) {
        return AWS_OP_ERR;
    }
    if (constant_items) {
        *constant_items = counts[0];
    }
    if (constant_bytes) {
        *constant_bytes = counts[1];
    }
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_encode_plan_packed_size(
    struct aws_huffman_amd_encode_plan *p,
    uint64_t *total_bytes,
    uint64_t *longest_item_bytes,
    void *stream) {

    if (!p || !p->packed_sized) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    uint64_t summary[2] = {0, 0};
    if (plan_read_words(p->engine->device, p->n_items ? p->d_pack_summary : NULL, summary, 2, stream ? stream : p->engine->stream)) {
        return AWS_OP_ERR;
    }
    if (total_bytes) {
        *total_bytes = summary[0];
    }
    if (longest_item_bytes) {
        *longest_item_bytes = summary[1];
    }
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_encode_plan_raw_results(
    struct aws_huffman_amd_encode_plan *p,
    struct hufd_enc_result *raw,
    void *stream) {
    void *st = stream ? stream : p->engine->stream;
    ON_DEVICE(p->engine->device);
    int err = 0;
    /* The one-pass kernel's waves wait for each other's totals; every wait is bounded, and one that ran out raises a
     * flag.  The kernels of the three-kernel road (no waits between workgroups) are queued behind it on the same
     * stream and look at that flag first: the output and these records are whole when the stream gets here, whichever
     * road made them.  The flag comes back with the results only so that the plan stays on the three-kernel road
     * from then on (a wait that ran out once -- the grid was not resident as a whole: another kernel on the device --
     * is likely to run out again, and costs milliseconds). */
    uint32_t timed_out = 0;
    if (p->last_single_pass) {
        err = hufs_copy_d2h(&timed_out, p->d_zero + 4 * sizeof(uint32_t), sizeof(timed_out), st); /* (enc_finish's copy of the word) */
    }
    if (!err) {
        err = hufs_copy_d2h(raw, p->d_results, (size_t)p->n_items * sizeof(*raw), st);
    }
    if (!err) {
        err = hufs_stream_sync(st);
    }
    if (!err && timed_out && !p->engine->encode_fails) {
        p->look_back_timed_out = true;
    }
    p->last_timed_out = !err && timed_out;
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

int aws_huffman_amd_encode_plan_road(const struct aws_huffman_amd_encode_plan *p, uint32_t *road) {
    *road = !p->last_single_pass ? AWS_HUFFMAN_AMD_ROAD_TWO_PASS
                                 : (p->last_timed_out ? AWS_HUFFMAN_AMD_ROAD_ONE_PASS_GAVE_UP : AWS_HUFFMAN_AMD_ROAD_ONE_PASS);
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_encode_plan_encoded_lengths(struct aws_huffman_amd_encode_plan *p, uint64_t *lengths, void *stream) {
    struct hufd_enc_result *raw = malloc((p->n_items ? p->n_items : 1) * sizeof(*raw));
    if (!raw) {
        return aws_raise_error(AWS_ERROR_OOM);
    }
    if (aws_huffman_amd_encode_plan_raw_results(p, raw, stream)) {
        free(raw);
        return AWS_OP_ERR;
    }
    for (uint32_t i = 0; i < p->n_items; ++i) {
        lengths[i] = (raw[i].total_bits + 7) / 8; /* source/huffman.c:121-128 */
    }
    free(raw);
    return AWS_OP_SUCCESS;
}

void aws_huffman_amd_encode_result_from_raw(
    const struct hufd_enc_result *raw,
    struct aws_huffman_amd_encode_result *out) {
    out->consumed = raw->consumed;
    out->produced = raw->produced;
    out->overflow_out.pattern = raw->ovf_pattern;
    out->overflow_out.num_bits = (uint8_t)raw->ovf_bits;
    switch (raw->status) {
        case HUFD_ENC_OK:
            out->rc = AWS_OP_SUCCESS;
            out->error = 0;
            break;
        case HUFD_ENC_SHORT:
            out->rc = AWS_OP_ERR;
            out->error = AWS_ERROR_SHORT_BUFFER;
            break;
        case HUFD_ENC_UNKNOWN:
            out->rc = AWS_OP_ERR;
            out->error = AWS_ERROR_COMPRESSION_UNKNOWN_SYMBOL;
            break;
        default:
            out->rc = AWS_OP_ERR;
            out->error = AWS_ERROR_INVALID_STATE;
            break;
    }
}

int aws_huffman_amd_encode_plan_results(
    struct aws_huffman_amd_encode_plan *p,
    struct aws_huffman_amd_encode_result *results,
    void *stream) {

    struct hufd_enc_result *raw = malloc((p->n_items ? p->n_items : 1) * sizeof(*raw));
    if (!raw) {
        return aws_raise_error(AWS_ERROR_OOM);
    }
    if (aws_huffman_amd_encode_plan_raw_results(p, raw, stream)) {
        free(raw);
        return AWS_OP_ERR;
    }
    for (uint32_t i = 0; i < p->n_items; ++i) {
        aws_huffman_amd_encode_result_from_raw(&raw[i], &results[i]);
    }
    free(raw);
    return AWS_OP_SUCCESS;
}

/* ------------------------------------------------------------------ decode plans */

#define DEC_SUMMARY_BYTES 256u
#define DEC_PLAN_ARRAYS(X, ci, cc, cl, cr, ns)                                                                            \
    X(d_items, (ci) * sizeof(struct hufd_dec_item))                                                                    \
    X(d_chunk_item, (cc) * sizeof(uint32_t))                                                                           \
    X(d_tail, (ci) * 2 * sizeof(uint32_t))                                                                             \
    X(d_tiny, (ci) * sizeof(uint32_t))                                                                                 \
    X(d_large, (cl) * 2 * sizeof(uint32_t))                                                                            \
    X(d_runs, (cr) * 2 * sizeof(uint32_t))                                                                             \
    X(d_run_fn, (cr) * (ns) * sizeof(uint32_t))                                                                        \
    X(d_fn_tab, (cc) * (ns) * HUFD_DEC_LANES * sizeof(uint16_t))                                                       \
    X(d_lane_rec, (cc) * HUFD_DEC_LANES * sizeof(struct hufd_lane_rec)) /* (16-byte records: every cut is 256-aligned) */ \
    X(d_chunk_fn, (cc) * (ns) * sizeof(uint32_t))                                                                      \
    X(d_slow_list, ((cc) + 1) * sizeof(uint32_t)) /* [0] count, [1..] chunks */                                        \
    X(d_emit_list, ((cc) + 1) * sizeof(uint32_t))                                                                      \
    X(d_dense_list, ((cc) + 1) * sizeof(uint32_t))                                                                     \
    X(d_counters, HUFK_DEC_COUNTERS * sizeof(uint32_t))                                                                \
    X(d_chunk_regular, (cc))                                                                                           \
    X(d_tail_entry, (cc) * sizeof(uint32_t))                                                                           \
    X(d_chunk_entry, (cc) * sizeof(uint32_t))                                                                          \
    X(d_chunk_base, (cc) * sizeof(uint64_t))                                                                           \
    X(d_emit_rec, (cc) * sizeof(struct hufd_emit_rec))                                                                 \
    X(d_chunk_rec, (cc) * sizeof(struct hufd_chunk_rec))                                                               \
    X(d_states, (ci) * sizeof(struct hufd_dec_item_state))                                                             \
    /* the list counters as the launch's last kernel found them, one arena cut (256 bytes) in front of the records:    \
     * ONE copy brings both to the host */                                                                             \
    X(d_summary, DEC_SUMMARY_BYTES)                                                                                    \
    X(d_results, (ci) * sizeof(struct hufd_dec_result))

_Static_assert(sizeof(struct hufd_lane_rec) == 16, "a sub-chunk's record is one 16-byte load or store");

static void dec_plan_release_device(struct aws_huffman_amd_decode_plan *p) {
    hufs_free(p->d_arena);
    p->d_arena = NULL;
#define DEC_FORGET(name, bytes) p->name = NULL;
    DEC_PLAN_ARRAYS(DEC_FORGET, 0, 0, 0, 0, 0)
#undef DEC_FORGET
    p->cap_items = p->cap_chunks = p->cap_large = p->cap_runs = 0;
}

/* short items are one thread's work, without chunks */
/* short items are one thread's work, without chunks; with codes too long for the chunked decoder's tables the
 * longer items are one workgroup's, without chunks either */
static bool dec_item_is_tiny(const struct aws_huffman_amd_decode_item *it, uint64_t limit) {
    return it->in_len > 0 && it->in_len <= limit;
}

/* the longest item a lone thread takes in this plan: see HUFD_DEC_TINY_PER_BYTE */
static uint64_t dec_tiny_limit(const struct aws_huffman_amd_decode_item *items, size_t n_items, struct item_stats *st) {
    /* (round 4: the upper class ended at 3 KiB of encoded bytes; since several short chunks share a workgroup -- dec_sync_pack,
     * dec_emit_pack -- items above what one wave takes decode 1.8 .. 2.8 times faster through the chunk kernels than a thread each:
     * 1 KiB items 0.82 -> 0.45 ms, 1.5 KiB 1.13 -> 0.41 ms per 128 MiB) */
    static const uint64_t classes[2] = {HUFD_DEC_COOP_BYTES, HUFD_DEC_TINY_BYTES};
    /* (one pass over the items for both classes: a plan of a million header-sized items is read from memory once here) */
    uint64_t count[2] = {0, 0}, longest[2] = {0, 0};
    st->shortest = UINT64_MAX;
    st->longest = 0;
    st->worst_bits = 0;
    for (size_t i = 0; i < n_items; ++i) {
        const uint64_t len = items[i].in_len;
        st->shortest = len < st->shortest ? len : st->shortest;
        st->longest = len > st->longest ? len : st->longest;
        st->worst_bits = items[i].first_bit > st->worst_bits ? items[i].first_bit : st->worst_bits;
        for (int c = 0; c < 2; ++c) {
            if (len <= classes[c]) {
                ++count[c];
                longest[c] = len > longest[c] ? len : longest[c];
            }
        }
    }
    for (int c = 0; c < 2; ++c) {
        if (longest[c] > HUFD_TINY_FEW_BYTES && count[c] >= tiny_per_byte(true) * longest[c]) {
            return classes[c];
        }
    }
    return HUFD_TINY_FEW_BYTES;
}

/* Items of a coder with long codes of at least this many encoded bytes go across the chip, seven launches each
 * (dec_wide_*): from HUFD_WIDE_MIN_BYTES on when the batch's items do not fill the chip a workgroup each, from
 * HUFD_WIDE_MANY_MIN_BYTES on when they do.  Tests set one limit for both. */
static uint64_t s_wide_min_bytes = 0;

void aws_huffman_amd_testing_set_wide_min_bytes(uint64_t bytes) {
    s_wide_min_bytes = bytes;
}

static uint64_t wide_min_bytes(size_t deep_items) {
    if (s_wide_min_bytes) {
        return s_wide_min_bytes;
    }
    return deep_items < HUFD_WIDE_FEW_ITEMS ? HUFD_WIDE_MIN_BYTES : HUFD_WIDE_MANY_MIN_BYTES;
}

static bool dec_item_is_deep(
    const struct aws_huffman_amd_engine *eng, const struct aws_huffman_amd_decode_item *it, uint64_t tiny_limit) {
    /* (the same kernel, as one wave, takes every coder's items that are too short to be worth a chunk's workgroup) */
    return it->in_len > tiny_limit && (eng->tables.deep_entries || it->in_len <= HUFD_DEC_COOP_BYTES);
}

/* (codes of one length: no chunks, no walks to bring into step) */
static bool dec_item_is_fixed(
    const struct aws_huffman_amd_engine *eng, const struct aws_huffman_amd_decode_item *it, uint64_t tiny_limit) {
    return eng->tables.fixed_bits && it->in_len > tiny_limit;
}

static uint64_t dec_item_chunks(
    const struct aws_huffman_amd_engine *eng, const struct aws_huffman_amd_decode_item *it, uint64_t tiny_limit) {
    if (dec_item_is_tiny(it, tiny_limit) || dec_item_is_fixed(eng, it, tiny_limit) || dec_item_is_deep(eng, it, tiny_limit)) {
        return 0;
    }
    return (it->in_len + HUFD_DEC_CHUNK_BYTES - 1) / HUFD_DEC_CHUNK_BYTES;
}

/* the plan's device arrays for this many items, chunks, large items and runs (grown, never shrunk); 0 or a HIP error */
/* whole lanes of a chunk with `left` bytes of its item from its first byte on: sub-chunks with 8 more bytes behind them */
static uint64_t whole_lanes_of(uint64_t left) {
    const uint64_t in_chunk = left < HUFD_DEC_CHUNK_BYTES + 8u ? left : HUFD_DEC_CHUNK_BYTES + 8u;
    return in_chunk >= 8 ? (in_chunk - 8) / HUFD_DEC_SUB_BYTES : 0;
}

static int dec_plan_reserve(struct aws_huffman_amd_decode_plan *p, size_t n_items, size_t n_chunks, size_t n_large, size_t n_runs) {
    const uint32_t ns = p->engine->tables.n_states;
    if (n_items > p->cap_items || n_chunks > p->cap_chunks || n_large > p->cap_large || n_runs > p->cap_runs) {
        dec_plan_release_device(p);
        const size_t ci = n_items ? n_items : 1, cc = n_chunks ? n_chunks : 1, cl = n_large ? n_large : 1;
        const size_t cr = n_runs ? n_runs : 1;
#define DEC_PART(name, bytes) {&p->name, (bytes)},
        const struct arena_part parts[] = {DEC_PLAN_ARRAYS(DEC_PART, ci, cc, cl, cr, ns)};
#undef DEC_PART
        if (arena_alloc(&p->d_arena, ARENA_PARTS(parts))) {
            return 2;
        }
        p->cap_items = ci;
        p->cap_chunks = cc;
        p->cap_large = cl;
        p->cap_runs = cr;
        /* the list counters start out clear; from then on every launch clears them for itself and for the one behind it (hufk_decode_args.counters) */
        int e = hufs_memset(p->d_counters, 0, HUFK_DEC_COUNTERS * sizeof(uint32_t), p->engine->stream);
        if (!e) { /* (... and what a fetch reads of the last launch's lists, before any launch: nothing listed, nothing known) */
            e = hufs_memset(p->d_summary, 0, DEC_SUMMARY_BYTES, p->engine->stream);
        }
        if (!e) {
            e = hufs_stream_sync(p->engine->stream);
        }
        if (e) {
            return e;
        }
        p->launches_with_chunks = 0;
        if ((uint8_t *)p->d_results != (uint8_t *)p->d_summary + DEC_SUMMARY_BYTES) {
            return 1; /* (the one copy of aws_huffman_amd_decode_plan_results counts on it: cuts are 256 bytes apart) */
        }
    }
    return 0;
}

static int dec_plan_fill(
    struct aws_huffman_amd_decode_plan *p,
    const struct aws_huffman_amd_decode_item *items,
    size_t n_items) {

    struct aws_huffman_amd_engine *eng = p->engine;
    if (!eng->can_decode) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    struct item_stats stats;
    const uint64_t tiny_limit = dec_tiny_limit(items, n_items, &stats);
    /* a failed refill must not leave counts of the fill before behind (the device arrays may be gone or too small) */
    p->n_items = p->n_chunks = p->n_large = p->n_runs = p->n_tail = p->n_fixed = p->n_wide = 0;
    p->quiet = false; /* (other items: nothing is known of what their launches list) */
    p->launches_with_chunks = 0; /* (... and no launch of these has left a summary to read it from) */
    p->packed = p->packed_sized = p->stored = p->stored_ranges = false;
    p->longest_in_len = 0;
    p->n_tiny = p->n_deep = 0;
    memset(&p->stats, 0, sizeof(p->stats));
    p->chained = false;
    if (n_items >= PLAN_ON_DEVICE_MIN_ITEMS && n_items < 0xFFFFFFFFull && stats.shortest >= 1 && stats.longest <= tiny_limit &&
        stats.worst_bits <= 7) {
        /* every item is one thread's work (dec_item_is_tiny): no chunks, no lists to make -- the caller's records go to the
         * device as they are and become the kernels' there (hufk_decode_plan_tiny_items) */
        ON_DEVICE(eng->device);
        int e = dec_plan_reserve(p, n_items, 0, 0, 0);
        void *d_raw = e ? NULL : hufs_malloc(n_items * sizeof(*items));
        if (!e && !d_raw) {
            e = 2;
        }
        if (!e) {
            e = hufs_copy_h2d(d_raw, items, n_items * sizeof(*items), eng->stream);
        }
        if (!e) {
            e = hufk_decode_plan_tiny_items(d_raw, (uint32_t)n_items, p->d_items, p->d_tiny, eng->stream);
        }
        struct aws_huffman_amd_decode_item *keep = e ? NULL : realloc(p->h_items, n_items * sizeof(*keep));
        if (!e && !keep) {
            e = 2;
        }
        if (!e) {
            memcpy(keep, items, n_items * sizeof(*keep)); /* (while the copy and the kernel run) */
            p->h_items = keep;
            e = hufs_stream_sync(eng->stream);
        }
        hufs_free(d_raw);
        if (e) {
            return raise_hip(e);
        }
        p->wide_from = wide_min_bytes(0);
        p->tail_stage_bytes = 0;
        p->tail_lanes = 0;
    p->tail_wide_lanes = 0;
        p->tail_wide_lanes = 0;
        p->n_tail_narrow = 0;
        p->n_items = (uint32_t)n_items;
        p->n_tiny = (uint32_t)n_items;
        p->stats.items = p->stats.by_thread = n_items;
        p->stats.thread_limit = tiny_limit;
        p->longest_in_len = stats.longest;
        return AWS_OP_SUCCESS;
    }
    uint64_t n_chunks = 0, n_large = 0, n_runs = 0, n_cut = 0;
    for (size_t i = 0; i < n_items; ++i) {
        /* symbol counts in the scan's function entries are 26-bit; 4 GiB of encoded bytes per item is the limit */
        if (items[i].first_bit > 7 || items[i].in_len > 0xFFFFFFFFull) {
            return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
        }
        const uint64_t chunks = dec_item_chunks(eng, &items[i], tiny_limit);
        n_chunks += chunks;
        n_cut += chunks != 0;
        n_large += chunks > HUFD_SCAN_SMALL_MAX;
        n_runs += chunks > HUFD_SCAN_SMALL_MAX ? (chunks + HUFD_SCAN_RUN_CHUNKS - 1) / HUFD_SCAN_RUN_CHUNKS : 0;
    }
    if (n_chunks >= 0xFFFFFFFFull || n_items >= 0xFFFFFFFFull) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }

    struct hufd_dec_item *h_items = malloc((n_items ? n_items : 1) * sizeof(*h_items));
    uint32_t *h_large = malloc((n_large ? n_large : 1) * 2 * sizeof(uint32_t));
    uint32_t *h_runs = malloc((n_runs ? n_runs : 1) * 2 * sizeof(uint32_t));
    uint32_t *h_tail = malloc((n_items ? n_items : 1) * 2 * sizeof(uint32_t));
    uint32_t *h_tiny = malloc((n_items ? n_items : 1) * sizeof(uint32_t));
    if (!h_items || !h_large || !h_runs || !h_tail || !h_tiny) {
        free(h_tail);
        free(h_tiny);
        free(h_runs);
        free(h_items);
        free(h_large);
        return aws_raise_error(AWS_ERROR_OOM);
    }
    uint32_t chunk = 0, large = 0, run = 0, tail = 0, narrow = 0, wide = 0, tiny = 0, deep = 0;
    size_t deep_items = 0;
    for (size_t i = 0; i < n_items && eng->tables.deep_entries; ++i) {
        deep_items += !dec_item_is_tiny(&items[i], tiny_limit) && dec_item_is_deep(eng, &items[i], tiny_limit);
    }
    const uint64_t wide_from = wide_min_bytes(deep_items);
    uint32_t *h_fixed = NULL;
    uint64_t n_fixed = 0, fixed_items = 0;
    struct hufk_wide_item *h_wide = NULL;
    uint32_t n_wide = 0;
    uint64_t wide_bytes = 0;
    bool wide_oom = false;
    uint64_t tail_stage = 0; /* the most symbols a chunk that holds the end of a stream can decode to */
    uint64_t tail_lanes = 0; /* ... and the most whole lanes it has */
    uint64_t wide_lanes = 0; /* ... and a wide one has (dec_emit_fast<TAIL>'s workgroup size) */
    for (size_t i = 0; i < n_items; ++i) {
        const struct aws_huffman_amd_decode_item *src = &items[i];
        struct hufd_dec_item *dst = &h_items[i];
        const uint32_t chunks = (uint32_t)dec_item_chunks(eng, src, tiny_limit);
        dst->in_off = src->in_offset;
        dst->in_len = src->in_len;
        dst->out_off = src->out_offset;
        dst->out_cap = src->out_capacity;
        dst->first_bit = src->first_bit;
        dst->first_chunk = chunk;
        dst->n_chunks = chunks;
        dst->tiny = 0;
        if (dec_item_is_tiny(src, tiny_limit)) {
            dst->tiny = 1;
            h_tiny[tiny++] = (uint32_t)i;
        } else if (dec_item_is_fixed(eng, src, tiny_limit)) {
            dst->tiny = 2;
            ++fixed_items;
            const uint64_t blocks = (src->in_len + HUFD_FIXED_BLOCK_BYTES - 1) / HUFD_FIXED_BLOCK_BYTES;
            uint32_t *more = realloc(h_fixed, (n_fixed + blocks) * 2 * sizeof(uint32_t));
            if (!more) {
                wide_oom = true;
            } else {
                h_fixed = more;
                for (uint64_t k = 0; k < blocks; ++k) {
                    h_fixed[2 * (n_fixed + k)] = (uint32_t)i;
                    h_fixed[2 * (n_fixed + k) + 1] = (uint32_t)k;
                }
                n_fixed += blocks;
            }
        } else if (dec_item_is_deep(eng, src, tiny_limit)) {
            dst->tiny = 1;
            h_tiny[n_items - ++deep] = (uint32_t)i;
            if (eng->tables.deep_entries && src->in_len >= wide_from) {
                struct hufk_wide_item *more = realloc(h_wide, (n_wide + 1) * sizeof(*more));
                if (!more) {
                    wide_oom = true;
                } else {
                    h_wide = more;
                    h_wide[n_wide].slot = deep; /* from the back of the list, for now */
                    h_wide[n_wide].n_blocks = (uint32_t)((src->in_len + HUFD_WIDE_BLOCK_BYTES - 1) / HUFD_WIDE_BLOCK_BYTES);
                    h_wide[n_wide].block_offset = wide_bytes;
                    wide_bytes += hufk_decode_wide_bytes(h_wide[n_wide].n_blocks);
                    ++n_wide;
                }
            }
        }
        /* the chunks that hold the end of the stream, or lie just behind it: fewer than a chunk + 8 bytes left from their
         * first byte on -- the item's last chunk, and the one in front of it when the last one holds less than 8 bytes.
         * (chunk -> item and the records per chunk are made on the device: hufk_decode_plan_chunks) */
        for (uint32_t k = chunks > 2 ? chunks - 2 : 0; k < chunks; ++k) {
            if (src->in_len - (uint64_t)k * HUFD_DEC_CHUNK_BYTES < (uint64_t)HUFD_DEC_CHUNK_BYTES + 8u) {
                const uint64_t left = src->in_len - (uint64_t)k * HUFD_DEC_CHUNK_BYTES;
                /* (the chunks with few whole lanes first: several of those share a workgroup, dec_sync_pack) */
                if (whole_lanes_of(left) <= HUFD_DEC_PACK_LANES) {
                    h_tail[narrow++] = chunk + k;
                } else {
                    h_tail[2 * (n_items ? n_items : 1) - ++wide] = chunk + k;
                }
                ++tail;
                const uint32_t shortest = eng->tables.min_bits ? eng->tables.min_bits : 1;
                uint64_t holds = left * 8 / shortest + 1;
                holds = holds < src->out_capacity ? holds : src->out_capacity;
                tail_stage = holds > tail_stage ? holds : tail_stage;
                const uint64_t whole = whole_lanes_of(left);
                if (whole <= HUFD_DEC_PACK_LANES) {
                    tail_lanes = whole > tail_lanes ? whole : tail_lanes;
                } else {
                    wide_lanes = whole > wide_lanes ? whole : wide_lanes;
                }
            }
        }
        chunk += chunks;
        if (chunks > HUFD_SCAN_SMALL_MAX) {
            h_large[2 * large] = (uint32_t)i;
            h_large[2 * large + 1] = run;
            ++large;
            for (uint32_t k = 0; k * HUFD_SCAN_RUN_CHUNKS < chunks; ++k) {
                h_runs[2 * run] = (uint32_t)i;
                h_runs[2 * run + 1] = k;
                ++run;
            }
        }
    }

    int err = wide_oom ? 2 : 0;
    ON_DEVICE(eng->device);
    for (uint32_t k = 0; k < n_wide; ++k) {
        h_wide[k].slot = deep - h_wide[k].slot; /* the deep items are the last `deep` of d_tiny, filled from the back */
    }
    if (!err && n_fixed > 0xFFFFFFFFull) {
        err = 2;
    }
    if (!err && n_fixed > p->cap_fixed) {
        hufs_free(p->d_fixed);
        p->d_fixed = hufs_malloc(n_fixed * 2 * sizeof(uint32_t));
        p->cap_fixed = p->d_fixed ? n_fixed : 0;
        err = p->d_fixed ? 0 : 2;
    }
    if (!err && n_fixed) {
        err = hufs_copy_h2d(p->d_fixed, h_fixed, n_fixed * 2 * sizeof(uint32_t), eng->stream);
        if (!err) {
            err = hufs_stream_sync(eng->stream); /* (h_fixed is freed below) */
        }
    }
    free(h_fixed);
    if (!err && wide_bytes > p->cap_wide_block) {
        hufs_free(p->d_wide_block);
        p->d_wide_block = hufs_malloc(wide_bytes);
        p->cap_wide_block = p->d_wide_block ? wide_bytes : 0;
        err = p->d_wide_block ? 0 : 2;
    }
    if (!err) {
        err = dec_plan_reserve(p, n_items, n_chunks, n_large, n_runs);
    }
    if (!err) {
        err = hufs_copy_h2d(p->d_items, h_items, n_items * sizeof(*h_items), eng->stream);
    }
    if (!err) {
        err = hufs_copy_h2d(p->d_runs, h_runs, n_runs * 2 * sizeof(uint32_t), eng->stream);
    }
    /* (the wide chunks were listed from the back, last one first: behind the narrow ones, in their order) */
    if (wide) {
        /* (the two blocks may overlap when nearly every slot of the list is taken: turn the back block round where it
         * lies, then move it down as a whole -- a copy entry by entry overwrote wide chunks it had not read yet) */
        uint32_t *back = h_tail + (2 * (n_items ? n_items : 1) - wide);
        for (uint32_t lo = 0, hi = wide - 1; lo < hi; ++lo, --hi) {
            const uint32_t t = back[lo];
            back[lo] = back[hi];
            back[hi] = t;
        }
        memmove(h_tail + narrow, back, (size_t)wide * sizeof(uint32_t));
    }
    if (!err) {
        err = hufs_copy_h2d(p->d_tail, h_tail, tail * sizeof(uint32_t), eng->stream);
    }
    if (!err) {
        err = hufs_copy_h2d(p->d_tiny, h_tiny, (tiny || deep ? n_items : 0) * sizeof(uint32_t), eng->stream);
    }
    if (!err) {
        err = hufk_decode_plan_chunks(p->d_items, (uint32_t)n_items, (uint32_t)n_chunks, p->d_chunk_item, p->d_chunk_rec, eng->stream);
    }
    if (!err) {
        err = hufs_copy_h2d(p->d_large, h_large, n_large * 2 * sizeof(uint32_t), eng->stream);
    }
    if (!err) {
        err = hufs_stream_sync(eng->stream);
    }
    /* keep what the result translation needs */
    if (!err) {
        struct aws_huffman_amd_decode_item *keep = realloc(p->h_items, (n_items ? n_items : 1) * sizeof(*keep));
        if (!keep) {
            err = 2;
        } else {
            if (n_items) { /* (a plan of no items may be given no array: memcpy wants a pointer even for nothing) */
                memcpy(keep, items, n_items * sizeof(*keep));
            }
            p->h_items = keep;
        }
    }
    free(h_items);
    free(h_large);
    free(h_runs);
    free(h_tail);
    free(h_tiny);
    if (err) {
        free(h_wide);
        return raise_hip(err);
    }
    free(p->h_wide);
    p->h_wide = h_wide;
    p->n_wide = n_wide;
    p->wide_from = wide_from;
    p->n_fixed = (uint32_t)n_fixed;
    p->n_items = (uint32_t)n_items;
    p->n_chunks = (uint32_t)n_chunks;
    p->n_large = (uint32_t)n_large;
    p->n_runs = (uint32_t)n_runs;
    p->n_tail = tail;
    p->tail_stage_bytes = tail_stage + 32 < 0xFFFFFFFFu ? (uint32_t)tail_stage + 32u : 0u;
    p->tail_lanes = tail_lanes < HUFD_DEC_LANES ? (uint32_t)tail_lanes : HUFD_DEC_LANES;
    p->tail_wide_lanes = wide_lanes < HUFD_DEC_LANES ? (uint32_t)wide_lanes : HUFD_DEC_LANES;
    p->n_tail_narrow = narrow;
    p->n_tiny = tiny;
    p->n_deep = deep;
    {
        const bool packs = narrow >= HUFD_DEC_PACK_MIN_CHUNKS && p->tail_lanes + 2u <= HUFD_DEC_LANES / 2;
        p->stats.items = n_items;
        p->stats.thread_limit = tiny_limit;
        p->longest_in_len = stats.longest;
        p->stats.by_thread = tiny;
        p->stats.by_blocks = n_wide + fixed_items;
        p->stats.by_wave = eng->tables.deep_entries ? 0 : deep;
        p->stats.by_workgroup = eng->tables.deep_entries ? deep - n_wide : 0;
        p->stats.by_pieces = n_cut;
        p->stats.pieces = n_chunks;
        /* (a few among many chunks inside streams: workgroups of the big kernels' own grids -- hufk_host::tails_are_folded) */
        const bool folded = tail && tail < n_chunks && (uint64_t)tail * 8 <= n_chunks;
        p->stats.end_pieces_folded = folded ? tail : 0;
        p->stats.end_pieces_packed = packs && !folded ? narrow : 0;
        p->stats.end_pieces_single = tail - p->stats.end_pieces_packed - p->stats.end_pieces_folded;
        p->stats.empty = n_items - tiny - deep - fixed_items - n_cut;
    }
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_decode_plan_new(
    struct aws_huffman_amd_decode_plan **out_plan,
    struct aws_huffman_amd_engine *eng,
    const struct aws_huffman_amd_decode_item *items,
    size_t item_count) {

    *out_plan = NULL;
    pthread_mutex_lock(&eng->spare_lock);
    struct aws_huffman_amd_decode_plan *p = eng->spare_dec;
    eng->spare_dec = NULL;
    pthread_mutex_unlock(&eng->spare_lock);
    if (p) {
        /* (as for an encode plan: the spare's last launch is waited for by its own event) */
        ON_DEVICE(eng->device);
        if (plan_wait_done(p->done_event, p->done_on_engine_stream, eng)) {
            p->unkeepable = true;
            aws_huffman_amd_decode_plan_destroy(p);
            return aws_raise_error(AWS_ERROR_UNKNOWN);
        }
        p->done_on_engine_stream = false;
    } else {
        p = calloc(1, sizeof(*p));
        if (!p) {
            return aws_raise_error(AWS_ERROR_OOM);
        }
        p->engine = eng;
    }
    if (dec_plan_fill(p, items, item_count)) {
        aws_huffman_amd_decode_plan_destroy(p);
        return AWS_OP_ERR;
    }
    *out_plan = p;
    return AWS_OP_SUCCESS;
}

/* the items of a source the device planner does not take (a coder with codes of more than 12 bits or of one length: their plans
 * hold what only the host lays out), brought to the host: the loop over them makes the plan */
static int dec_items_to_host(
    struct aws_huffman_amd_decode_plan *p, const struct hufd_item_source *src, size_t n_items, void *st, struct aws_huffman_amd_decode_item **out) {
    struct aws_huffman_amd_decode_item *items = calloc(n_items ? n_items : 1, sizeof(*items));
    if (!items) {
        return 2;
    }
    int e = 0;
    if (src->kind == HUFD_ITEMS_STRIDED) {
        for (size_t i = 0; i < n_items; ++i) {
            items[i].in_offset = src->in_offset + i * src->in_stride;
            items[i].in_len = src->in_len;
            items[i].first_bit = (uint8_t)src->first_bit;
            items[i].out_offset = src->out_offset + i * src->out_stride;
            items[i].out_capacity = src->out_capacity;
        }
    } else if (src->kind == HUFD_ITEMS_DEVICE_ARRAY) {
        e = hufs_copy_d2h(items, src->raw, n_items * sizeof(*items), st);
        if (!e) {
            e = hufs_stream_sync(st);
        }
    } else if (src->kind == HUFD_ITEMS_PACKED_INPUT || src->kind == HUFD_ITEMS_PACKED_STORED_INPUT ||
               src->kind == HUFD_ITEMS_PACKED_CONSTANT_INPUT) {
        const size_t n_offsets = src->packed_lengths ? n_items : n_items + 1;
        const bool kinds = src->kind == HUFD_ITEMS_PACKED_CONSTANT_INPUT;
        const bool flagged = src->kind == HUFD_ITEMS_PACKED_STORED_INPUT || kinds;
        uint64_t *at = malloc((n_offsets ? n_offsets : 1) * sizeof(*at));
        uint64_t *len = malloc((n_items ? n_items : 1) * sizeof(*len));
        uint8_t *flag = calloc(n_items ? n_items : 1, 1);
        e = at && len && flag ? 0 : 2;
        if (!e && n_items && flagged) {
            e = hufs_copy_d2h(flag, src->packed_stored, n_items, st);
        }
        if (!e && n_items) {
            e = hufs_copy_d2h(at, src->packed_offsets, n_offsets * sizeof(*at), st);
        }
        if (!e && n_items && src->packed_lengths) {
            e = hufs_copy_d2h(len, src->packed_lengths, n_items * sizeof(*len), st);
        }
        if (!e) {
            e = hufs_stream_sync(st);
        }
        for (size_t i = 0; i < n_items && !e; ++i) {
            /* (offsets that decrease: a length no plan takes, as the device planner's `invalid`) */
            bool bad = (src->packed_lengths ? (i > 0 && at[i - 1] > at[i]) : at[i + 1] < at[i]) || flag[i] > (kinds ? 2 : 1);
            const uint64_t bytes = bad ? 0 : (src->packed_lengths ? len[i] : at[i + 1] - at[i]);
            if (kinds && !bad) {
                /* (load_item of plan_kernels.hip is the rule this restates: the head of a constant item, read where the kind
                 * and the length say there is one -- eight bytes at a time: only coders whose plans the host lays out come here) */
                bad = at[i] >> 63;
                if (flag[i] == 2 && !bad) {
                    uint64_t count = 0;
                    if (bytes == HUFK_CONSTANT_BYTES) {
                        uint8_t head[8];
                        e = hufs_copy_d2h(head, src->packed_bytes + at[i], sizeof(head), st);
                        if (!e) {
                            e = hufs_stream_sync(st);
                        }
                        for (size_t k = 0; k < 8 && !e; ++k) {
                            count |= (uint64_t)head[k] << (8 * k);
                        }
                    }
                    bad = count <= HUFK_CONSTANT_BYTES || count > HUFK_CONSTANT_MAX_COUNT;
                }
            }
            items[i].in_offset = at[i];
            /* (an item stored raw, or a constant one: nothing for the decode kernels) */
            items[i].in_len = bad ? UINT64_MAX : (flag[i] ? 0 : bytes);
        }
        free(at);
        free(len);
        free(flag);
    } else if (src->kind == HUFD_ITEMS_BLOCK_RANGES) {
        /* (the index whole: 8 bytes a block; load_item of plan_kernels.hip is the rule this loop restates) */
        struct hufd_block_range *ranges = malloc((n_items ? n_items : 1) * sizeof(*ranges));
        uint64_t *index = malloc(((size_t)src->n_blocks + 1) * sizeof(*index));
        e = ranges && index ? 0 : 2;
        if (!e && n_items) {
            e = hufs_copy_d2h(ranges, src->block_ranges, n_items * sizeof(*ranges), st);
        }
        if (!e && n_items) {
            e = hufs_copy_d2h(index, src->block_index, ((size_t)src->n_blocks + 1) * sizeof(*index), st);
        }
        if (!e) {
            e = hufs_stream_sync(st);
        }
        for (size_t i = 0; i < n_items && !e; ++i) {
            const uint64_t b0 = ranges[i].first_block, count = ranges[i].block_count;
            items[i].out_offset = ranges[i].out_offset;
            items[i].in_len = UINT64_MAX; /* (a length no plan takes) */
            if (b0 <= src->n_blocks && count <= src->n_blocks - b0) {
                const uint64_t from = index[b0], to = index[b0 + count];
                const uint64_t first_byte = from / 8, end_byte = to / 8 + (to % 8 ? 1 : 0);
                if (to >= from && end_byte <= src->encoded_length) {
                    const uint64_t lo = b0 * src->block_symbols, hi = (b0 + count) * src->block_symbols;
                    items[i].in_len = count ? end_byte - first_byte : 0;
                    items[i].in_offset = count ? src->encoded_offset + first_byte : 0;
                    items[i].first_bit = count ? (uint8_t)(from % 8) : 0;
                    items[i].out_capacity = count ? (hi < src->stream_symbols ? hi : src->stream_symbols) - lo : 0;
                }
            }
        }
        free(ranges);
        free(index);
    } else if (src->kind == HUFD_ITEMS_SYMBOL_RANGES) {
        /* (load_item of plan_kernels.hip is the rule this loop restates) */
        struct hufd_symbol_range *ranges = malloc((n_items ? n_items : 1) * sizeof(*ranges));
        uint64_t *bits = malloc((n_items ? n_items : 1) * 2 * sizeof(*bits));
        e = ranges && bits ? 0 : 2;
        if (!e && n_items) {
            e = hufs_copy_d2h(ranges, src->symbol_ranges, n_items * sizeof(*ranges), st);
        }
        if (!e && n_items) {
            e = hufs_copy_d2h(bits, src->located_bits, n_items * 2 * sizeof(*bits), st);
        }
        if (!e) {
            e = hufs_stream_sync(st);
        }
        for (size_t i = 0; i < n_items && !e; ++i) {
            const uint64_t s0 = ranges[i].first_symbol, count = ranges[i].symbol_count;
            items[i].out_offset = ranges[i].out_offset;
            items[i].in_len = UINT64_MAX; /* (a length no plan takes) */
            if (s0 <= src->stream_symbols && count <= src->stream_symbols - s0) {
                const uint64_t from = bits[2 * i], to = bits[2 * i + 1];
                const uint64_t first_byte = from / 8, end_byte = to / 8 + (to % 8 ? 1 : 0);
                if (from != HUFD_NO_BIT && to != HUFD_NO_BIT && to >= from && end_byte <= src->encoded_length) {
                    items[i].in_len = count ? end_byte - first_byte : 0;
                    items[i].in_offset = count ? src->encoded_offset + first_byte : 0;
                    items[i].first_bit = count ? (uint8_t)(from % 8) : 0;
                    items[i].out_capacity = count;
                }
            }
        }
        free(ranges);
        free(bits);
    } else if (src->kind == HUFD_ITEMS_ITEM_BLOCK_RANGES) {
        /* (the directory, the index and the offsets whole; load_item of plan_kernels.hip is the rule this loop restates) */
        const size_t n_batch = (size_t)src->batch_items, n_entries = (size_t)src->index_entries;
        const size_t n_offsets = src->packed_lengths ? n_batch : n_batch + 1;
        struct hufd_item_block_range *ranges = malloc((n_items ? n_items : 1) * sizeof(*ranges));
        uint64_t *dir = malloc((n_batch + 1) * 2 * sizeof(*dir));
        uint64_t *index = malloc((n_entries ? n_entries : 1) * sizeof(*index));
        uint64_t *at = malloc((n_offsets ? n_offsets : 1) * sizeof(*at));
        uint64_t *len = malloc((n_batch ? n_batch : 1) * sizeof(*len));
        uint8_t *flag = calloc(n_batch ? n_batch : 1, 1); /* (all 0 without the sender's flags) */
        e = ranges && dir && index && at && len && flag ? 0 : 2;
        if (!e && n_items && n_batch && src->packed_stored) {
            e = hufs_copy_d2h(flag, src->packed_stored, n_batch, st);
        }
        if (!e && n_items) {
            e = hufs_copy_d2h(ranges, src->item_block_ranges, n_items * sizeof(*ranges), st);
        }
        if (!e && n_items) {
            e = hufs_copy_d2h(dir, src->batch_directory, (n_batch + 1) * 2 * sizeof(*dir), st);
        }
        if (!e && n_items && n_entries) {
            e = hufs_copy_d2h(index, src->block_index, n_entries * sizeof(*index), st);
        }
        if (!e && n_items && n_offsets) {
            e = hufs_copy_d2h(at, src->packed_offsets, n_offsets * sizeof(*at), st);
        }
        if (!e && n_items && n_batch && src->packed_lengths) {
            e = hufs_copy_d2h(len, src->packed_lengths, n_batch * sizeof(*len), st);
        }
        if (!e) {
            e = hufs_stream_sync(st);
        }
        for (size_t i = 0; i < n_items && !e; ++i) {
            const uint64_t item = ranges[i].item, b0 = ranges[i].first_block, count = ranges[i].block_count;
            items[i].out_offset = ranges[i].out_offset;
            items[i].in_len = UINT64_MAX; /* (a length no plan takes) */
            if (item >= src->batch_items) {
                continue;
            }
            const uint64_t first = dir[2 * item], symbols = dir[2 * item + 1], next = dir[2 * item + 2];
            const uint64_t blocks = symbols / src->block_symbols + (symbols % src->block_symbols ? 1u : 0u);
            const uint64_t off = at[item];
            const bool placed = src->packed_lengths || at[item + 1] >= off;
            const uint64_t bytes = src->packed_lengths ? len[item] : at[item + 1] - off;
            const bool framed = next >= first && next < src->index_entries && next - first == blocks && b0 <= blocks &&
                                count <= blocks - b0 && placed && off <= src->encoded_length && bytes <= src->encoded_length - off;
            if (flag[item] == 1) {
                /* (an item stored raw: its bytes as they lie, nothing for the decode kernels, no index entry read) */
                if (framed && bytes == symbols) {
                    const uint64_t lo = b0 * src->block_symbols;
                    const uint64_t hi = b0 + count == blocks ? symbols : lo + count * src->block_symbols;
                    items[i].in_len = 0;
                    items[i].in_offset = count ? src->encoded_offset + off + lo : 0;
                    items[i].first_bit = 0;
                    items[i].out_capacity = count ? hi - lo : 0;
                }
            } else if (flag[item] == 0 && framed) {
                const uint64_t base = index[first], x0 = index[first + b0], x1 = index[first + b0 + count];
                const uint64_t from = x0 - base, to = x1 - base;
                const uint64_t first_byte = from / 8, end_byte = to / 8 + (to % 8 ? 1 : 0);
                if (x0 >= base && x1 >= x0 && end_byte <= bytes) {
                    const uint64_t lo = b0 * src->block_symbols, hi = (b0 + count) * src->block_symbols;
                    items[i].in_len = count ? end_byte - first_byte : 0;
                    items[i].in_offset = count ? src->encoded_offset + off + first_byte : 0;
                    items[i].first_bit = count ? (uint8_t)(from % 8) : 0;
                    items[i].out_capacity = count ? (hi < symbols ? hi : symbols) - lo : 0;
                }
            }
        }
        free(ranges);
        free(dir);
        free(index);
        free(at);
        free(len);
        free(flag);
    } else if (src->kind == HUFD_ITEMS_ITEM_SYMBOL_RANGES) {
        /* (the directory and the offsets whole; load_item of plan_kernels.hip is the rule this loop restates) */
        const size_t n_batch = (size_t)src->batch_items;
        const size_t n_offsets = src->packed_lengths ? n_batch : n_batch + 1;
        struct hufd_item_symbol_range *ranges = malloc((n_items ? n_items : 1) * sizeof(*ranges));
        uint64_t *bits = malloc((n_items ? n_items : 1) * 2 * sizeof(*bits));
        uint64_t *dir = malloc((n_batch + 1) * 2 * sizeof(*dir));
        uint64_t *at = malloc((n_offsets ? n_offsets : 1) * sizeof(*at));
        uint64_t *len = malloc((n_batch ? n_batch : 1) * sizeof(*len));
        uint8_t *flag = calloc(n_batch ? n_batch : 1, 1); /* (all 0 without the sender's flags) */
        e = ranges && bits && dir && at && len && flag ? 0 : 2;
        if (!e && n_items && n_batch && src->packed_stored) {
            e = hufs_copy_d2h(flag, src->packed_stored, n_batch, st);
        }
        if (!e && n_items) {
            e = hufs_copy_d2h(ranges, src->item_symbol_ranges, n_items * sizeof(*ranges), st);
        }
        if (!e && n_items) {
            e = hufs_copy_d2h(bits, src->located_bits, n_items * 2 * sizeof(*bits), st);
        }
        if (!e && n_items) {
            e = hufs_copy_d2h(dir, src->batch_directory, (n_batch + 1) * 2 * sizeof(*dir), st);
        }
        if (!e && n_items && n_offsets) {
            e = hufs_copy_d2h(at, src->packed_offsets, n_offsets * sizeof(*at), st);
        }
        if (!e && n_items && n_batch && src->packed_lengths) {
            e = hufs_copy_d2h(len, src->packed_lengths, n_batch * sizeof(*len), st);
        }
        if (!e) {
            e = hufs_stream_sync(st);
        }
        for (size_t i = 0; i < n_items && !e; ++i) {
            const uint64_t item = ranges[i].item, s0 = ranges[i].first_symbol, count = ranges[i].symbol_count;
            items[i].out_offset = ranges[i].out_offset;
            items[i].in_len = UINT64_MAX; /* (a length no plan takes) */
            if (item >= src->batch_items) {
                continue;
            }
            const uint64_t symbols = dir[2 * item + 1], off = at[item];
            const bool placed = src->packed_lengths || at[item + 1] >= off;
            const uint64_t bytes = src->packed_lengths ? len[item] : at[item + 1] - off;
            const uint64_t from = bits[2 * i], to = bits[2 * i + 1];
            const uint64_t first_byte = from / 8, end_byte = to / 8 + (to % 8 ? 1 : 0);
            /* (an item stored raw: the locate body's closed form left the ends, a byte a symbol) */
            const bool raw_ok =
                flag[item] == 0 || (flag[item] == 1 && bytes == symbols && from % 8 == 0 && to - from == 8 * count);
            if (s0 <= symbols && count <= symbols - s0 && placed && off <= src->encoded_length && bytes <= src->encoded_length - off &&
                from != HUFD_NO_BIT && to != HUFD_NO_BIT && to >= from && first_byte >= off && end_byte <= off + bytes && raw_ok) {
                items[i].in_len = count && !flag[item] ? end_byte - first_byte : 0;
                items[i].in_offset = count ? src->encoded_offset + first_byte : 0;
                items[i].first_bit = count ? (uint8_t)(from % 8) : 0;
                items[i].out_capacity = count;
            }
        }
        free(ranges);
        free(bits);
        free(dir);
        free(at);
        free(len);
        free(flag);
    } else {
        struct hufd_enc_item *ei = malloc((n_items ? n_items : 1) * sizeof(*ei));
        struct hufd_enc_result *er = malloc((n_items ? n_items : 1) * sizeof(*er));
        e = ei && er ? 0 : 2;
        if (!e) {
            e = hufs_copy_d2h(ei, src->enc_items, n_items * sizeof(*ei), st);
        }
        if (!e) {
            e = hufs_copy_d2h(er, src->enc_results, n_items * sizeof(*er), st);
        }
        if (!e) {
            e = hufs_stream_sync(st);
        }
        for (size_t i = 0; i < n_items && !e; ++i) {
            items[i].in_offset = ei[i].out_off;
            items[i].in_len = er[i].produced < ei[i].out_cap ? er[i].produced : ei[i].out_cap;
            items[i].out_offset = ei[i].in_off;
            items[i].out_capacity = ei[i].in_len;
        }
        free(ei);
        free(er);
    }
    (void)p;
    if (e) {
        free(items);
        return e;
    }
    *out = items;
    return 0;
}

/* as enc_plan_fill_on_device: chunks, lists and per-chunk records of the items of `src`, made on the device */
static int dec_plan_fill_on_device(struct aws_huffman_amd_decode_plan *p, const struct hufd_item_source *src, size_t n_items, void *stream) {
    struct aws_huffman_amd_engine *eng = p->engine;
    if (!eng->can_decode) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    void *st = stream ? stream : eng->stream;
    if (eng->tables.deep_entries || eng->tables.fixed_bits) {
        struct aws_huffman_amd_decode_item *items = NULL;
        ON_DEVICE(eng->device);
        const int e = dec_items_to_host(p, src, n_items, st, &items);
        if (e) {
            return raise_hip(e);
        }
        const int rc = dec_plan_fill(p, items, n_items);
        free(items);
        return rc;
    }
    p->n_items = p->n_chunks = p->n_large = p->n_runs = p->n_tail = p->n_fixed = p->n_wide = 0;
    p->quiet = false; /* (other items: nothing is known of what their launches list) */
    p->launches_with_chunks = 0; /* (... and no launch of these has left a summary to read it from) */
    p->packed = p->packed_sized = p->stored = p->stored_ranges = false;
    p->longest_in_len = 0;
    p->n_tiny = p->n_deep = 0;
    memset(&p->stats, 0, sizeof(p->stats));
    p->chained = false;
    p->wide_from = wide_min_bytes(0);
    p->tail_stage_bytes = 0;
    p->tail_lanes = 0;
    p->tail_wide_lanes = 0;
    p->n_tail_narrow = 0;
    if (n_items == 0) {
        return AWS_OP_SUCCESS;
    }
    if (n_items >= 0xFFFFFFFFull) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    ON_DEVICE(eng->device);
    struct hufk_plan_totals t;
    int e = plan_scratch_reserve(&p->d_plan_scratch, &p->cap_plan_scratch, n_items);
    if (!e) {
        e = hufk_decode_plan_count(src, (uint32_t)n_items, tiny_per_byte(true), eng->tables.min_bits, p->d_plan_scratch, &t, st);
    }
    if (e) {
        return raise_hip(e);
    }
    if (t.invalid || t.totals[0] >= 0xFFFFFFFFull) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    const uint64_t n_chunks = t.totals[0], tiny = t.totals[1], coop = t.totals[2], n_large = t.totals[3], n_runs = t.totals[4];
    const uint64_t narrow = t.totals[5], wide = t.totals[6];
    e = dec_plan_reserve(p, n_items, (size_t)n_chunks, (size_t)n_large, (size_t)n_runs);
    if (!e) {
        e = hufk_decode_plan_fill(
            src, (uint32_t)n_items, eng->tables.min_bits, p->d_plan_scratch, p->d_items, p->d_tiny, p->d_tail, p->d_large, p->d_runs, st);
    }
    if (!e) {
        e = hufk_decode_plan_chunks(p->d_items, (uint32_t)n_items, (uint32_t)n_chunks, p->d_chunk_item, p->d_chunk_rec, st);
    }
    if (e) {
        return raise_hip(e);
    }
    p->n_items = (uint32_t)n_items;
    p->n_chunks = (uint32_t)n_chunks;
    p->n_large = (uint32_t)n_large;
    p->n_runs = (uint32_t)n_runs;
    p->n_tail = (uint32_t)(narrow + wide);
    p->n_tail_narrow = (uint32_t)narrow;
    p->n_tiny = (uint32_t)tiny;
    p->n_deep = (uint32_t)coop;
    p->tail_stage_bytes = t.tail_stage + 32 < 0xFFFFFFFFu ? (uint32_t)t.tail_stage + 32u : 0u;
    p->tail_lanes = t.tail_lanes < HUFD_DEC_LANES ? (uint32_t)t.tail_lanes : HUFD_DEC_LANES;
    p->tail_wide_lanes = t.wide_lanes < HUFD_DEC_LANES ? (uint32_t)t.wide_lanes : HUFD_DEC_LANES;
    p->chained = true; /* (the items are known on the device only: the results are translated from its records) */
    {
        const bool packs = narrow >= HUFD_DEC_PACK_MIN_CHUNKS && p->tail_lanes + 2u <= HUFD_DEC_LANES / 2;
        p->stats.items = n_items;
        p->stats.thread_limit = t.tiny_limit;
        p->longest_in_len = t.longest;
        p->stats.by_thread = tiny;
        p->stats.by_wave = coop;
        p->stats.by_pieces = t.totals[7];
        p->stats.pieces = n_chunks;
        const bool folded = narrow + wide && narrow + wide < n_chunks && (narrow + wide) * 8 <= n_chunks;
        p->stats.end_pieces_folded = folded ? narrow + wide : 0;
        p->stats.end_pieces_packed = packs && !folded ? narrow : 0;
        p->stats.end_pieces_single = narrow + wide - p->stats.end_pieces_packed - p->stats.end_pieces_folded;
        p->stats.empty = n_items - tiny - coop - t.totals[7];
    }
    e = plan_mark_done(&p->done_event, &p->done_on_engine_stream, eng, stream); /* (as enc_plan_fill_on_device) */
    return e ? raise_hip(e) : AWS_OP_SUCCESS;
}

int aws_huffman_amd_decode_plan_reset_strided(
    struct aws_huffman_amd_decode_plan *p, const struct aws_huffman_amd_strided_items *items, void *stream) {
    struct hufd_item_source src;
    strided_source(&src, items);
    return dec_plan_fill_on_device(p, &src, (size_t)items->count, stream);
}

int aws_huffman_amd_decode_plan_reset_device_items(
    struct aws_huffman_amd_decode_plan *p, const struct aws_huffman_amd_decode_item *device_items, size_t item_count, void *stream) {
    struct hufd_item_source src;
    memset(&src, 0, sizeof(src));
    src.kind = HUFD_ITEMS_DEVICE_ARRAY;
    src.raw = device_items;
    return dec_plan_fill_on_device(p, &src, item_count, stream);
}

int aws_huffman_amd_decode_plan_reset(
    struct aws_huffman_amd_decode_plan *p,
    const struct aws_huffman_amd_decode_item *items,
    size_t item_count) {
    return dec_plan_fill(p, items, item_count);
}

void aws_huffman_amd_decode_plan_destroy(struct aws_huffman_amd_decode_plan *p) {
    if (p) {
        struct aws_huffman_amd_engine *eng = p->engine;
        pthread_mutex_lock(&eng->spare_lock);
        const bool keep = !eng->retiring && !eng->spare_dec && p->cap_items && p != eng->one_dec && !p->unkeepable;
        if (keep) {
            eng->spare_dec = p;
        }
        pthread_mutex_unlock(&eng->spare_lock);
        if (keep) {
            return;
        }
        ON_DEVICE(p->engine->device);
        dec_plan_release_device(p);
        hufs_free(p->d_packed_arena);
        hufs_free(p->d_plan_scratch);
        hufs_event_destroy(p->done_event);
        hufs_free(p->d_wide_block);
        hufs_free(p->d_fixed);
        hufs_free(p->d_range_bits);
        hufs_free(p->d_stored_arena);
        free(p->h_wide);
        free(p->h_items);
        free(p);
    }
}

int aws_huffman_amd_decode_plan_launch(
    struct aws_huffman_amd_decode_plan *p,
    const void *device_input,
    void *device_output,
    void *stream) {
    return aws_huffman_amd_decode_plan_launch_staged(p, device_input, device_output, stream, NULL);
}

/* what a launch of the plan hands the kernels */
static void dec_plan_launch_args(
    struct aws_huffman_amd_decode_plan *p,
    struct hufk_decode_args *args,
    const void *device_input,
    void *device_output,
    void **stage_events) {

    struct hufk_decode_args a;
    memset(&a, 0, sizeof(a));
    a.tables = p->engine->tables;
    a.items = p->d_items;
    a.n_items = p->n_items;
    a.chunk_item = p->d_chunk_item;
    a.n_chunks = p->n_chunks;
    a.tail_chunks = p->d_tail;
    a.n_tail = p->n_tail;
    a.tail_stage_bytes = p->tail_stage_bytes;
    a.tail_lanes = p->tail_lanes;
    a.tail_wide_lanes = p->tail_wide_lanes;
    a.n_tail_narrow = p->n_tail_narrow;
    a.deep_items = p->d_tiny + (p->n_items - p->n_deep);
    a.n_deep = p->n_deep;
    a.wide = p->h_wide;
    a.n_wide = p->n_wide;
    a.wide_from = p->wide_from;
    a.wide_block = p->d_wide_block;
    a.fixed_blocks = p->d_fixed;
    a.n_fixed_blocks = p->n_fixed;
    a.tiny_items = p->d_tiny;
    a.n_tiny = p->n_tiny;
    a.large_items = p->d_large;
    a.n_large = p->n_large;
    a.runs = p->d_runs;
    a.n_runs = p->n_runs;
    a.run_fn = p->d_run_fn;
    a.d_in = device_input;
    a.d_out = device_output;
    a.fn_tab = p->d_fn_tab;
    a.lane_rec = p->d_lane_rec;
    a.chunk_fn = p->d_chunk_fn;
    a.slow_list = p->d_slow_list + 1;
    a.emit_list = p->d_emit_list + 1;
    a.dense_list = p->d_dense_list + 1;
    a.counters = p->d_counters;
    a.counters_self_cleared = 1;
    a.summary = p->d_summary;
    a.quiet = p->quiet && !(testing_decode_road() & AWS_HUFFMAN_AMD_TEST_DECODE_ALL_KERNELS);
    a.chunk_regular = p->d_chunk_regular;
    a.tail_entry = p->d_tail_entry;
    a.chunk_entry = p->d_chunk_entry;
    a.chunk_base = p->d_chunk_base;
    a.emit_rec = p->d_emit_rec;
    a.chunk_rec = p->d_chunk_rec;
    a.side_stream = p->engine->side_stream;
    a.fork_event = p->engine->fork_event;
    a.join_event = p->engine->join_event;
    a.states = p->d_states;
    a.results = p->d_results;
    {
        const uint32_t road = testing_decode_road();
        a.one_chunk_a_workgroup = (road & AWS_HUFFMAN_AMD_TEST_DECODE_ONE_CHUNK_A_WORKGROUP) != 0;
        a.tails_apart = (road & AWS_HUFFMAN_AMD_TEST_DECODE_TAILS_APART) != 0;
        /* dec_wide_* give every long item of a coder with long codes up: dec_wide_fn_*, the road for such an item by
         * transfer functions, takes it -- or gives it up as well, and dec_deep takes it (the ways back) */
        a.wide_fails = road & AWS_HUFFMAN_AMD_TEST_DECODE_WIDE_FN_FAILS ? 2u : (road & AWS_HUFFMAN_AMD_TEST_DECODE_WIDE_FAILS ? 1u : 0u);
        /* the chunks whose walks do not fall into step through dec_sync and dec_emit (not dec_sync_few / _true) */
        a.few_walks = road & AWS_HUFFMAN_AMD_TEST_DECODE_LONG_WAY ? 0u : 1u;
    }
    a.stage_events = stage_events;
    if (p->stored_ranges) { /* (a plain launch copies them; a packed one is refused in front of this) */
        a.stored_rec = p->d_stored_rec;
        a.stored_tile_first = p->d_stored_tile_first;
        a.stored_tiles = p->stored_tiles;
    }
    *args = a;
}

int aws_huffman_amd_decode_plan_launch_staged(
    struct aws_huffman_amd_decode_plan *p,
    const void *device_input,
    void *device_output,
    void *stream,
    void **stage_events) {

    if (engine_never_fitted(p->engine) || p->stored) { /* (stored items have no place of their own: such a plan is for packed launches) */
        return aws_raise_error(AWS_ERROR_INVALID_STATE);
    }
    struct hufk_decode_args a;
    dec_plan_launch_args(p, &a, device_input, device_output, stage_events);
    p->packed = false; /* (the results are results for the plan's own capacities) */
    ON_DEVICE(p->engine->device);
    int err = hufk_decode_launch(&a, stream ? stream : p->engine->stream);
    if (!err && p->n_chunks) {
        ++p->launches_with_chunks; /* (queued whole: its last kernel leaves the lists' lengths in d_summary) */
    }
    if (!err) {
        err = plan_mark_done(&p->done_event, &p->done_on_engine_stream, p->engine, stream);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

/* ------------------------------------------------------------------ packed decode launches (huffman_amd_packed.h) */

/* as enc_plan_reserve_packed: the second record arrays, the scan's tile sums and its summary words (grown, never shrunk);
 * an allocation, so not inside a graph capture -- the first packed launch of a plan, or of more items or chunks */
static int dec_plan_reserve_packed(struct aws_huffman_amd_decode_plan *p, size_t n_items, size_t n_chunks, size_t n_tiles) {
    if (p->d_packed_arena && n_items <= p->cap_packed_items && n_chunks <= p->cap_packed_chunks && n_tiles <= p->cap_pack_tiles) {
        return 0;
    }
    p->cap_packed_items = p->cap_packed_chunks = p->cap_pack_tiles = 0;
    /* as many as the plan's own arrays: a reset within them allocates nothing */
    const size_t ci = n_items > p->cap_items ? n_items : p->cap_items;
    const size_t cc = n_chunks > p->cap_chunks ? n_chunks : p->cap_chunks;
    const struct arena_part parts[] = {
        {&p->d_packed_items, ci * sizeof(struct hufd_dec_item)},
        {&p->d_packed_chunk_rec, (cc ? cc : 1) * sizeof(struct hufd_chunk_rec)},
        {&p->d_pack_tile_sums, 2 * n_tiles * sizeof(uint64_t)},
        {&p->d_pack_summary, 2 * sizeof(uint64_t)}};
    if (arena_alloc(&p->d_packed_arena, ARENA_PARTS(parts))) {
        return 2;
    }
    p->cap_packed_items = ci;
    p->cap_packed_chunks = cc;
    p->cap_pack_tiles = n_tiles;
    return 0;
}

int aws_huffman_amd_decode_plan_launch_packed(
    struct aws_huffman_amd_decode_plan *p,
    const void *device_input,
    void *device_output,
    uint64_t output_capacity,
    uint64_t *device_offsets,
    uint32_t align,
    void *stream) {

    if (!p || !device_offsets || ((uintptr_t)device_offsets & 7u) || align == 0 || align > 4096 || (align & (align - 1)) ||
        (!device_output && output_capacity)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (engine_never_fitted(p->engine) || p->stored_ranges) { /* (ranges of stored items go where their ranges say: such a plan is for plain launches) */
        return aws_raise_error(AWS_ERROR_INVALID_STATE);
    }
    void *st = stream ? stream : p->engine->stream;
    if (p->n_items == 0) {
        ON_DEVICE(p->engine->device);
        const int e = hufs_memset(device_offsets, 0, sizeof(uint64_t), st);
        if (e) {
            return raise_hip(e);
        }
        p->packed = false;
        p->packed_sized = true;
        return AWS_OP_SUCCESS;
    }
    struct hufk_decode_pack pk;
    memset(&pk, 0, sizeof(pk));
    pk.tile_items = hufk_pack_tile_items(p->n_items, __atomic_load_n(&s_pack_tile_items, __ATOMIC_RELAXED));
    ON_DEVICE(p->engine->device);
    int err = dec_plan_reserve_packed(p, p->n_items, p->n_chunks, hufk_pack_tiles(p->n_items, pk.tile_items));
    if (err) {
        return raise_hip(err);
    }
    /* the most symbols a chunk that holds the end of a stream can decode to, + 32, as the plan's own number -- but that
     * one is cut to the items' own capacities, which a packed launch does not use */
    {
        const uint64_t in_chunk = p->longest_in_len < HUFD_DEC_CHUNK_BYTES + 8u ? p->longest_in_len : HUFD_DEC_CHUNK_BYTES + 8u;
        const uint32_t shortest = p->engine->tables.min_bits ? p->engine->tables.min_bits : 1u;
        pk.tail_stage_bytes = p->longest_in_len ? (uint32_t)(in_chunk * 8 / shortest + 1 + 32) : 0u;
    }
    pk.align = align;
    pk.capacity = output_capacity;
    pk.tile_sums = p->d_pack_tile_sums;
    pk.offsets = device_offsets;
    pk.summary = p->d_pack_summary;
    pk.items = p->d_packed_items;
    pk.chunk_rec = p->d_packed_chunk_rec;
    if (p->stored) {
        pk.stored_rec = p->d_stored_rec;
        pk.stored_tile_first = p->d_stored_tile_first;
        pk.stored_tiles = p->stored_tiles;
    }
    struct hufk_decode_args a;
    dec_plan_launch_args(p, &a, device_input, device_output, NULL);
    err = hufk_decode_launch_packed(&a, &pk, st);
    if (!err && p->n_chunks) {
        ++p->launches_with_chunks;
    }
    if (!err) {
        err = plan_mark_done(&p->done_event, &p->done_on_engine_stream, p->engine, stream);
    }
    if (err) {
        return raise_hip(err);
    }
    p->packed = true;
    p->packed_sized = true;
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_decode_plan_packed_size(
    struct aws_huffman_amd_decode_plan *p,
    uint64_t *total_symbols,
    uint64_t *longest_item_symbols,
    void *stream) {

    if (!p || !p->packed_sized) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    uint64_t summary[2] = {0, 0};
    if (plan_read_words(p->engine->device, p->n_items ? p->d_pack_summary : NULL, summary, 2, stream ? stream : p->engine->stream)) {
        return AWS_OP_ERR;
    }
    if (total_symbols) {
        *total_symbols = summary[0];
    }
    if (longest_item_symbols) {
        *longest_item_symbols = summary[1];
    }
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_decode_plan_reset_packed_input(
    struct aws_huffman_amd_decode_plan *p,
    const uint64_t *device_offsets,
    const uint64_t *device_lengths,
    size_t item_count,
    void *stream) {

    if (!p) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if ((!device_offsets && item_count) || ((uintptr_t)device_offsets & 7u) || ((uintptr_t)device_lengths & 7u)) {
        p->quiet = false; /* (as a refused aws_huffman_amd_decode_plan_from_encode) */
        p->launches_with_chunks = 0;
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    struct hufd_item_source src;
    memset(&src, 0, sizeof(src));
    src.kind = HUFD_ITEMS_PACKED_INPUT;
    src.packed_offsets = device_offsets;
    src.packed_lengths = device_lengths;
    return dec_plan_fill_on_device(p, &src, item_count, stream);
}

/* ------------------------------------------------------------------ items stored raw, the receiver (huffman_amd_stored.h) */

/* the plan's stored records, the tiles in front of each item and the tile sums of their scan (grown, never shrunk) */
static int dec_plan_reserve_stored(struct aws_huffman_amd_decode_plan *p, size_t n_items, size_t n_tiles) {
    if (p->d_stored_arena && n_items <= p->cap_stored_items && n_tiles <= p->cap_stored_tiles) {
        return 0;
    }
    p->cap_stored_items = p->cap_stored_tiles = 0;
    const struct arena_part parts[] = {
        {&p->d_stored_rec, 2 * n_items * sizeof(uint64_t)},
        {&p->d_stored_tile_first, (n_items + 1) * sizeof(uint64_t)},
        {&p->d_stored_tile_sums, 2 * n_tiles * sizeof(uint64_t)}};
    if (arena_alloc(&p->d_stored_arena, ARENA_PARTS(parts))) {
        return 2;
    }
    p->cap_stored_items = n_items;
    p->cap_stored_tiles = n_tiles;
    return 0;
}

/* What the launches of a plan with stored items need: {source offset, length} of every stored item -- from the three arrays
 * of a packed input, or (ranges != NULL) from the item records of a plan of ranges and the batch's flags --, and the tiles the
 * copy cuts the long ones into, scanned; their number comes back (the reset has waited for the planner's totals already).
 * What fails leaves a plan without items. */
static int dec_plan_stored_records(
    struct aws_huffman_amd_decode_plan *p,
    const uint64_t *device_offsets,
    const uint64_t *device_lengths,
    const uint8_t *device_stored,
    const void *device_ranges,
    const void *device_packed, /* != NULL: device_stored holds kinds, and a constant item's record comes from its head (huffman_amd_constant.h) */
    void *stream) {

    void *st = stream ? stream : p->engine->stream;
    const uint32_t tile_items = hufk_pack_tile_items(p->n_items, __atomic_load_n(&s_pack_tile_items, __ATOMIC_RELAXED));
    uint64_t tiles = 0;
    ON_DEVICE(p->engine->device);
    int e = dec_plan_reserve_stored(p, p->n_items, hufk_pack_tiles(p->n_items, tile_items));
    if (!e) {
        e = device_ranges
                ? hufk_stored_range_records((const uint64_t *)device_ranges, device_stored, p->d_items, p->n_items, p->d_stored_rec, st)
                : hufk_stored_records(device_offsets, device_lengths, device_stored, device_packed, p->n_items, p->d_stored_rec, st);
    }
    if (!e) {
        e = hufk_stored_tiles(
            p->d_stored_rec, p->n_items, tile_items, HUFK_STORED_TILE_BYTES, HUFK_STORED_WAVE_BYTES, p->d_stored_tile_sums,
            p->d_stored_tile_first, st);
    }
    if (!e) {
        e = hufs_copy_d2h(&tiles, p->d_stored_tile_first + p->n_items, sizeof(tiles), st);
    }
    if (!e) {
        e = hufs_stream_sync(st);
    }
    if (e || tiles >= 0x7FFFFFFFull) {
        p->n_items = p->n_chunks = p->n_large = p->n_runs = p->n_tail = p->n_tiny = p->n_deep = p->n_fixed = p->n_wide = 0; /* (no plan) */
        p->n_tail_narrow = 0;
        p->packed = p->packed_sized = false;
        memset(&p->stats, 0, sizeof(p->stats));
        return e ? raise_hip(e) : aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    p->stored_tiles = tiles;
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_decode_plan_reset_packed_stored_input(
    struct aws_huffman_amd_decode_plan *p,
    const uint64_t *device_offsets,
    const uint64_t *device_lengths,
    const uint8_t *device_stored,
    size_t item_count,
    void *stream) {

    if (!device_stored) {
        return aws_huffman_amd_decode_plan_reset_packed_input(p, device_offsets, device_lengths, item_count, stream);
    }
    if (!p) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if ((!device_offsets && item_count) || ((uintptr_t)device_offsets & 7u) || ((uintptr_t)device_lengths & 7u)) {
        p->quiet = false; /* (as a refused aws_huffman_amd_decode_plan_reset_packed_input) */
        p->launches_with_chunks = 0;
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    struct hufd_item_source src;
    memset(&src, 0, sizeof(src));
    src.kind = HUFD_ITEMS_PACKED_STORED_INPUT;
    src.packed_offsets = device_offsets;
    src.packed_lengths = device_lengths;
    src.packed_stored = device_stored;
    /* the planner's pass checks every offset, length and flag; a stored item comes out of it without encoded bytes */
    if (dec_plan_fill_on_device(p, &src, item_count, stream)) {
        return AWS_OP_ERR;
    }
    if (p->n_items == 0) {
        return AWS_OP_SUCCESS;
    }
    if (dec_plan_stored_records(p, device_offsets, device_lengths, device_stored, NULL, NULL, stream)) {
        return AWS_OP_ERR;
    }
    p->stored = true;
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_decode_plan_reset_packed_constant_input(
    struct aws_huffman_amd_decode_plan *p,
    const void *device_packed,
    const uint64_t *device_offsets,
    const uint64_t *device_lengths,
    const uint8_t *device_kinds,
    size_t item_count,
    void *stream) {

    if (!device_kinds) {
        return aws_huffman_amd_decode_plan_reset_packed_input(p, device_offsets, device_lengths, item_count, stream);
    }
    if (!p) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if ((!device_offsets && item_count) || (!device_packed && item_count) || ((uintptr_t)device_offsets & 7u) ||
        ((uintptr_t)device_lengths & 7u)) {
        p->quiet = false; /* (as a refused aws_huffman_amd_decode_plan_reset_packed_input) */
        p->launches_with_chunks = 0;
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    struct hufd_item_source src;
    memset(&src, 0, sizeof(src));
    src.kind = HUFD_ITEMS_PACKED_CONSTANT_INPUT;
    src.packed_offsets = device_offsets;
    src.packed_lengths = device_lengths;
    src.packed_stored = device_kinds;
    src.packed_bytes = (const uint8_t *)device_packed;
    /* the planner's pass checks every offset, length, kind and head; a stored or constant item comes out of it without encoded
     * bytes, and the records of the copy -- for a constant item {its value, its count} -- are made behind it */
    if (dec_plan_fill_on_device(p, &src, item_count, stream)) {
        return AWS_OP_ERR;
    }
    if (p->n_items == 0) {
        return AWS_OP_SUCCESS;
    }
    if (dec_plan_stored_records(p, device_offsets, device_lengths, device_kinds, NULL, device_packed, stream)) {
        return AWS_OP_ERR;
    }
    p->stored = true;
    return AWS_OP_SUCCESS;
}

/* ------------------------------------------------------------------ block index and range plans (huffman_amd_index.h) */

_Static_assert(AWS_HUFFMAN_AMD_INDEX_OK == HUFK_INDEX_OK, "index status");
_Static_assert(AWS_HUFFMAN_AMD_INDEX_SYMBOL_WITHOUT_CODE == HUFK_INDEX_SYMBOL_WITHOUT_CODE, "index status");
_Static_assert(sizeof(struct aws_huffman_amd_block_range) == sizeof(struct hufd_block_range), "block range layout");
_Static_assert(offsetof(struct aws_huffman_amd_block_range, block_count) == offsetof(struct hufd_block_range, block_count), "block range layout");
_Static_assert(offsetof(struct aws_huffman_amd_block_range, out_offset) == offsetof(struct hufd_block_range, out_offset), "block range layout");

static uint32_t s_index_tile_blocks = 0;

void aws_huffman_amd_testing_set_index_tile_blocks(uint32_t blocks) {
    __atomic_store_n(&s_index_tile_blocks, blocks, __ATOMIC_RELAXED);
}

static bool index_block_symbols_ok(uint64_t block_symbols) {
    return block_symbols >= 64 && block_symbols <= (1ull << 24) && block_symbols % 64 == 0;
}

int aws_huffman_amd_block_index(
    struct aws_huffman_amd_engine *eng,
    const void *device_input,
    uint64_t length,
    uint64_t block_symbols,
    uint64_t *device_index,
    uint32_t *device_status,
    void *stream) {

    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION); /* no GPU: there is no CPU path */
    }
    if (!eng || !device_index || ((uintptr_t)device_index & 7u) || ((uintptr_t)device_status & 3u) ||
        !index_block_symbols_ok(block_symbols) || (length && !device_input)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    const uint64_t n_blocks = (length + block_symbols - 1) / block_symbols;
    if (n_blocks > 0xFFFFFFFFull) { /* (the scan numbers blocks in 32 bits: 256 GiB of symbols in blocks of 64) */
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (engine_never_fitted(eng)) {
        return aws_raise_error(AWS_ERROR_INVALID_STATE);
    }
    ON_DEVICE(eng->device);
    pthread_mutex_lock(&eng->spare_lock);
    if (!eng->d_index_tile_sums) { /* (the engine's first call: an allocation, so not inside a graph capture) */
        eng->d_index_tile_sums = hufs_malloc(2 * (size_t)HUFK_INDEX_MAX_TILES * sizeof(uint64_t));
    }
    uint64_t *tile_sums = eng->d_index_tile_sums;
    pthread_mutex_unlock(&eng->spare_lock);
    if (!tile_sums) {
        return raise_hip(2);
    }
    void *st = stream ? stream : eng->stream;
    int err;
    if (length == 0) { /* (no block, no launch: index[0] = 0 and the status, two memset nodes) */
        err = hufs_memset(device_index, 0, sizeof(uint64_t), st);
        if (!err && device_status) {
            err = hufs_memset(device_status, 0, sizeof(uint32_t), st);
        }
    } else {
        const uint32_t tile_blocks = hufk_index_tile_blocks((uint32_t)n_blocks, __atomic_load_n(&s_index_tile_blocks, __ATOMIC_RELAXED));
        err = hufk_block_index(eng->d_enc_table, device_input, length, block_symbols, tile_blocks, device_index, tile_sums, device_status, st);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

/* ------------------------------------------------------------------ one index over a plan's items (huffman_amd_batch_index.h) */

_Static_assert(AWS_HUFFMAN_AMD_INDEX_TOO_SMALL == HUFK_INDEX_TOO_SMALL, "index status");
_Static_assert(sizeof(struct aws_huffman_amd_item_blocks) == 2 * sizeof(uint64_t), "directory layout");
_Static_assert(offsetof(struct aws_huffman_amd_item_blocks, symbols) == sizeof(uint64_t), "directory layout");

#define BATCH_INDEX_WAVE_BYTES 4096u /* items shorter than this are a wave's work */

static uint64_t s_batch_index_wave_bytes = 0;

void aws_huffman_amd_testing_set_batch_index_wave_bytes(uint64_t bytes) {
    __atomic_store_n(&s_batch_index_wave_bytes, bytes, __ATOMIC_RELAXED);
}

/* the call's scratch for this many items and tiles of the scans over them (grown, never shrunk): an allocation, so not
 * inside a graph capture -- the plan's first call, or one of more items */
static int enc_plan_reserve_block_index(struct aws_huffman_amd_encode_plan *p, size_t n_items, size_t n_tiles) {
    if (p->d_block_index_arena && n_items <= p->cap_block_index_items && n_tiles <= p->cap_block_index_tiles) {
        return 0;
    }
    p->cap_block_index_items = p->cap_block_index_tiles = 0;
    const size_t ci = n_items > p->cap_items ? n_items : p->cap_items; /* as many as the plan's own array: a reset within it allocates nothing */
    const struct arena_part parts[] = {
        {&p->d_block_index_tile_first, (ci + 1) * sizeof(uint64_t)},
        {&p->d_block_index_tile_sums, 2 * n_tiles * sizeof(uint64_t)},
        {&p->d_block_index_summary, sizeof(uint64_t)}};
    if (arena_alloc(&p->d_block_index_arena, ARENA_PARTS(parts))) {
        return 2;
    }
    p->cap_block_index_items = ci;
    p->cap_block_index_tiles = n_tiles;
    return 0;
}

/* what a batch index asks of its arguments */
static bool enc_plan_block_index_args_ok(
    const struct aws_huffman_amd_encode_plan *p, const void *device_input, const struct enc_plan_index_args *ix) {
    return p && ix->directory && !((uintptr_t)ix->directory & 7u) && !((uintptr_t)ix->index & 7u) && !((uintptr_t)ix->status & 3u) &&
           (ix->index == NULL) == (ix->index_capacity == 0) && index_block_symbols_ok(ix->block_symbols) &&
           (!p->n_items || device_input);
}

/* the directory, the hot pass and the scan of a plan's batch index on `stream`: the arguments are good, the engine fitted */
static int enc_plan_block_index_enqueue(
    struct aws_huffman_amd_encode_plan *p, const void *device_input, const struct enc_plan_index_args *ix, void *stream) {

    struct aws_huffman_amd_engine *eng = p->engine;
    ON_DEVICE(eng->device);
    pthread_mutex_lock(&eng->spare_lock);
    if (!eng->d_index_tile_sums) { /* (as aws_huffman_amd_block_index: the engine's first call of either) */
        eng->d_index_tile_sums = hufs_malloc(2 * (size_t)HUFK_INDEX_MAX_TILES * sizeof(uint64_t));
    }
    uint64_t *index_tile_sums = eng->d_index_tile_sums;
    pthread_mutex_unlock(&eng->spare_lock);
    if (!index_tile_sums) {
        return raise_hip(2);
    }
    struct hufk_batch_index job;
    memset(&job, 0, sizeof(job));
    job.pack_tile_items = hufk_pack_tile_items(p->n_items, __atomic_load_n(&s_pack_tile_items, __ATOMIC_RELAXED));
    const int reserved = enc_plan_reserve_block_index(p, p->n_items, p->n_items ? hufk_pack_tiles(p->n_items, job.pack_tile_items) : 1);
    if (reserved) {
        return raise_hip(reserved);
    }
    uint64_t wave_bytes = __atomic_load_n(&s_batch_index_wave_bytes, __ATOMIC_RELAXED);
    wave_bytes = wave_bytes ? wave_bytes : BATCH_INDEX_WAVE_BYTES;
    job.enc_table = eng->d_enc_table;
    job.items = p->d_items;
    job.n_items = p->n_items;
    job.input = device_input;
    job.block_symbols = ix->block_symbols;
    job.wave_bytes = wave_bytes < HUFK_BATCH_WAVE_MAX_BYTES ? wave_bytes : HUFK_BATCH_WAVE_MAX_BYTES;
    job.index_tile_asked = __atomic_load_n(&s_index_tile_blocks, __ATOMIC_RELAXED);
    job.directory = (uint64_t *)ix->directory;
    job.index = ix->index;
    job.capacity = ix->index_capacity;
    job.status = ix->status;
    job.tile_first = p->d_block_index_tile_first;
    job.item_tile_sums = p->d_block_index_tile_sums;
    job.summary = p->d_block_index_summary;
    job.index_tile_sums = index_tile_sums;
    const int err = hufk_batch_block_index(&job, stream ? stream : eng->stream);
    if (err) {
        return raise_hip(err);
    }
    p->block_indexed = true;
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_encode_plan_block_index(
    struct aws_huffman_amd_encode_plan *p,
    const void *device_input,
    uint64_t block_symbols,
    struct aws_huffman_amd_item_blocks *device_directory,
    uint64_t *device_index,
    uint64_t index_capacity,
    uint32_t *device_status,
    void *stream) {

    const struct enc_plan_index_args ix = {block_symbols, device_directory, device_index, index_capacity, device_status};
    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION); /* no GPU: there is no CPU path */
    }
    if (!enc_plan_block_index_args_ok(p, device_input, &ix)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (engine_never_fitted(p->engine)) {
        return aws_raise_error(AWS_ERROR_INVALID_STATE);
    }
    if (enc_plan_block_index_enqueue(p, device_input, &ix, stream)) {
        return AWS_OP_ERR;
    }
    /* (the plan's records and scratch are read on this stream: whoever gets its arrays next waits, as for a launch) */
    ON_DEVICE(p->engine->device);
    const int err = plan_mark_done(&p->done_event, &p->done_on_engine_stream, p->engine, stream);
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

int aws_huffman_amd_encode_plan_block_index_size(struct aws_huffman_amd_encode_plan *p, uint64_t *entries, void *stream) {
    if (!p || !entries || !p->block_indexed) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    uint64_t blocks = 0;
    if (plan_read_words(p->engine->device, p->d_block_index_summary, &blocks, 1, stream ? stream : p->engine->stream)) {
        return AWS_OP_ERR;
    }
    *entries = blocks + 1;
    return AWS_OP_SUCCESS;
}

/* a reset of ranges whose arguments are refused: a plan without items, as a refused range leaves it, and INVALID_ARGUMENT */
static int dec_plan_refuse(struct aws_huffman_amd_decode_plan *p, uint32_t kind, void *stream) {
    struct hufd_item_source src;
    memset(&src, 0, sizeof(src));
    src.kind = kind;
    const int rc = dec_plan_fill_on_device(p, &src, 0, stream);
    return rc ? rc : aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
}

int aws_huffman_amd_decode_plan_reset_block_ranges(
    struct aws_huffman_amd_decode_plan *p,
    const uint64_t *device_index,
    uint64_t length,
    uint64_t block_symbols,
    uint64_t encoded_offset,
    uint64_t encoded_length,
    const struct aws_huffman_amd_block_range *device_ranges,
    size_t range_count,
    void *stream) {

    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    if (!p) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (!device_index || ((uintptr_t)device_index & 7u) || (!device_ranges && range_count) || ((uintptr_t)device_ranges & 7u) ||
        !index_block_symbols_ok(block_symbols)) {
        return dec_plan_refuse(p, HUFD_ITEMS_BLOCK_RANGES, stream);
    }
    struct hufd_item_source src;
    memset(&src, 0, sizeof(src));
    src.kind = HUFD_ITEMS_BLOCK_RANGES;
    /* the planner reads the ranges and the two index entries at each range's ends where it reads any item's record: a
     * refused range is its statistics pass's `invalid`, which comes back with the totals */
    src.block_index = device_index;
    src.block_ranges = (const struct hufd_block_range *)device_ranges;
    src.n_blocks = (length + block_symbols - 1) / block_symbols;
    src.stream_symbols = length;
    src.block_symbols = block_symbols;
    src.encoded_offset = encoded_offset;
    src.encoded_length = encoded_length;
    return dec_plan_fill_on_device(p, &src, range_count, stream);
}

_Static_assert(sizeof(struct aws_huffman_amd_item_block_range) == sizeof(struct hufd_item_block_range), "item block range layout");
_Static_assert(offsetof(struct aws_huffman_amd_item_block_range, first_block) == offsetof(struct hufd_item_block_range, first_block), "item block range layout");
_Static_assert(offsetof(struct aws_huffman_amd_item_block_range, block_count) == offsetof(struct hufd_item_block_range, block_count), "item block range layout");
_Static_assert(offsetof(struct aws_huffman_amd_item_block_range, out_offset) == offsetof(struct hufd_item_block_range, out_offset), "item block range layout");

/* a plan of ranges by item that was reset with the sender's flags: the records and tiles of the ranges in stored items, for
 * the copy behind the emit stage of its plain launches */
static int dec_plan_stored_ranges(struct aws_huffman_amd_decode_plan *p, const uint8_t *device_stored, const void *device_ranges, void *stream) {
    if (!device_stored || p->n_items == 0) {
        return AWS_OP_SUCCESS;
    }
    if (dec_plan_stored_records(p, NULL, NULL, device_stored, device_ranges, NULL, stream)) {
        return AWS_OP_ERR;
    }
    p->stored_ranges = true;
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_decode_plan_reset_item_block_ranges(
    struct aws_huffman_amd_decode_plan *p,
    const struct aws_huffman_amd_item_blocks *device_directory,
    const uint64_t *device_index,
    uint64_t index_entries,
    uint64_t item_count,
    uint64_t block_symbols,
    const uint64_t *device_encoded_offsets,
    const uint64_t *device_encoded_lengths,
    uint64_t encoded_offset,
    uint64_t encoded_length,
    const struct aws_huffman_amd_item_block_range *device_ranges,
    size_t range_count,
    void *stream) {
    return aws_huffman_amd_decode_plan_reset_stored_item_block_ranges(
        p, device_directory, device_index, index_entries, item_count, block_symbols, device_encoded_offsets, device_encoded_lengths, NULL,
        encoded_offset, encoded_length, device_ranges, range_count, stream);
}

int aws_huffman_amd_decode_plan_reset_stored_item_block_ranges(
    struct aws_huffman_amd_decode_plan *p,
    const struct aws_huffman_amd_item_blocks *device_directory,
    const uint64_t *device_index,
    uint64_t index_entries,
    uint64_t item_count,
    uint64_t block_symbols,
    const uint64_t *device_encoded_offsets,
    const uint64_t *device_encoded_lengths,
    const uint8_t *device_stored,
    uint64_t encoded_offset,
    uint64_t encoded_length,
    const struct aws_huffman_amd_item_block_range *device_ranges,
    size_t range_count,
    void *stream) {

    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    if (!p) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (!device_directory || ((uintptr_t)device_directory & 7u) || !device_index || ((uintptr_t)device_index & 7u) || index_entries == 0 ||
        item_count >= 0xFFFFFFFFull || !device_encoded_offsets || ((uintptr_t)device_encoded_offsets & 7u) ||
        ((uintptr_t)device_encoded_lengths & 7u) || (!device_ranges && range_count) || ((uintptr_t)device_ranges & 7u) ||
        !index_block_symbols_ok(block_symbols)) {
        return dec_plan_refuse(p, HUFD_ITEMS_ITEM_BLOCK_RANGES, stream);
    }
    struct hufd_item_source src;
    memset(&src, 0, sizeof(src));
    src.kind = HUFD_ITEMS_ITEM_BLOCK_RANGES;
    /* the planner reads a range, its item's two directory records, place and three index entries where it reads any item's
     * record: a refused range is its statistics pass's `invalid`, which comes back with the totals */
    src.item_block_ranges = (const struct hufd_item_block_range *)device_ranges;
    src.batch_directory = (const uint64_t *)device_directory;
    src.batch_items = item_count;
    src.block_index = device_index;
    src.index_entries = index_entries;
    src.block_symbols = block_symbols;
    src.packed_offsets = device_encoded_offsets;
    src.packed_lengths = device_encoded_lengths;
    src.packed_stored = device_stored;
    src.encoded_offset = encoded_offset;
    src.encoded_length = encoded_length;
    if (dec_plan_fill_on_device(p, &src, range_count, stream)) {
        return AWS_OP_ERR;
    }
    return dec_plan_stored_ranges(p, device_stored, device_ranges, stream);
}

/* ------------------------------------------------------------------ symbols of an indexed stream (huffman_amd_ranges.h) */

_Static_assert(AWS_HUFFMAN_AMD_NO_BIT == HUFD_NO_BIT, "no bit");
_Static_assert(sizeof(struct aws_huffman_amd_symbol_range) == sizeof(struct hufd_symbol_range), "symbol range layout");
_Static_assert(offsetof(struct aws_huffman_amd_symbol_range, symbol_count) == offsetof(struct hufd_symbol_range, symbol_count), "symbol range layout");
_Static_assert(offsetof(struct aws_huffman_amd_symbol_range, out_offset) == offsetof(struct hufd_symbol_range, out_offset), "symbol range layout");

/* A lane alone walks a position that is at most this many codes behind its block's first; a workgroup takes the others.
 * profiles/symbol_ranges_mi355x.json: for 65 536 positions the two roads cross near 2 600 codes; at 512 the lone lane is six
 * times faster ("Symbols of an indexed stream"). */
#define LOCATE_LONE_SYMBOLS 1024u

static uint32_t s_locate_lone_symbols = 0;

void aws_huffman_amd_testing_set_locate_lone_symbols(uint32_t symbols) {
    __atomic_store_n(&s_locate_lone_symbols, symbols, __ATOMIC_RELAXED);
}

/* a job of positions in one indexed stream; the caller adds what is located (symbols or ranges, count, bits, status) */
static void locate_stream_job(
    struct hufd_locate *job, const void *encoded, uint64_t encoded_length, const uint64_t *index, uint64_t length, uint64_t block_symbols) {
    memset(job, 0, sizeof(*job));
    job->encoded = encoded;
    job->encoded_length = encoded_length;
    job->index = index;
    job->length = length;
    job->block_symbols = block_symbols;
    job->n_blocks = (length + block_symbols - 1) / block_symbols;
}

/* the locate launches of a job (and the memset that clears its status in front of them) on `st`: nothing waited for */
static int locate_launch(const struct aws_huffman_amd_engine *eng, struct hufd_locate *job, void *st) {
    const uint32_t asked = __atomic_load_n(&s_locate_lone_symbols, __ATOMIC_RELAXED);
    job->lone_symbols = asked ? asked : LOCATE_LONE_SYMBOLS;
    /* (a coder of one code length needs no walk; blocks no longer than the limit have no position behind it) */
    const uint32_t walks_coop = !eng->tables.fixed_bits && (uint64_t)job->lone_symbols + 1 < job->block_symbols;
    int err = job->status ? hufs_memset(job->status, 0, sizeof(uint32_t), st) : 0;
    if (!err && job->count) {
        err = hufk_locate_symbols(&eng->tables, job, walks_coop, st);
    }
    return err;
}

/* Both ends of every range of a reset of symbol ranges (job->ranges or job->item_ranges), located on the caller's stream into
 * words the plan owns (two a range: grown, never shrunk), in front of the planner's passes, which read a range and its two bits
 * where they read any item's record: a refused range (an end that was not found among them) is the statistics pass's `invalid`,
 * which comes back with the totals. */
static int dec_plan_locate_range_ends(struct aws_huffman_amd_decode_plan *p, struct hufd_locate *job, size_t range_count, void *stream) {
    ON_DEVICE(p->engine->device);
    if (2 * range_count > p->cap_range_bits) {
        hufs_free(p->d_range_bits);
        p->d_range_bits = hufs_malloc(2 * range_count * sizeof(uint64_t));
        p->cap_range_bits = p->d_range_bits ? 2 * range_count : 0;
    }
    if (!p->d_range_bits) {
        return raise_hip(2);
    }
    job->count = 2 * (uint64_t)range_count;
    job->bits = p->d_range_bits;
    const int err = locate_launch(p->engine, job, stream ? stream : p->engine->stream);
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

int aws_huffman_amd_locate_symbols(
    struct aws_huffman_amd_engine *eng,
    const void *device_encoded,
    uint64_t encoded_length,
    const uint64_t *device_index,
    uint64_t length,
    uint64_t block_symbols,
    const uint64_t *device_symbols,
    size_t count,
    uint64_t *device_bits,
    uint32_t *device_status,
    void *stream) {

    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION); /* no GPU: there is no CPU path */
    }
    if (!eng || !device_index || ((uintptr_t)device_index & 7u) || ((uintptr_t)device_status & 3u) ||
        !index_block_symbols_ok(block_symbols) || (length && !device_encoded) ||
        (count && (!device_symbols || !device_bits)) || ((uintptr_t)device_symbols & 7u) || ((uintptr_t)device_bits & 7u)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if ((length + block_symbols - 1) / block_symbols > 0xFFFFFFFFull) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (!eng->can_decode) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    if (engine_never_fitted(eng)) {
        return aws_raise_error(AWS_ERROR_INVALID_STATE);
    }
    struct hufd_locate job;
    locate_stream_job(&job, device_encoded, encoded_length, device_index, length, block_symbols);
    job.symbols = device_symbols;
    job.count = count;
    job.bits = device_bits;
    job.status = device_status;
    ON_DEVICE(eng->device);
    const int err = locate_launch(eng, &job, stream ? stream : eng->stream);
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

int aws_huffman_amd_decode_plan_reset_symbol_ranges(
    struct aws_huffman_amd_decode_plan *p,
    const void *device_input,
    const uint64_t *device_index,
    uint64_t length,
    uint64_t block_symbols,
    uint64_t encoded_offset,
    uint64_t encoded_length,
    const struct aws_huffman_amd_symbol_range *device_ranges,
    size_t range_count,
    void *stream) {

    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    if (!p) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    struct aws_huffman_amd_engine *eng = p->engine;
    if (engine_never_fitted(eng)) {
        return aws_raise_error(AWS_ERROR_INVALID_STATE);
    }
    if (!device_index || ((uintptr_t)device_index & 7u) || (!device_ranges && range_count) || ((uintptr_t)device_ranges & 7u) ||
        (!device_input && range_count) || !index_block_symbols_ok(block_symbols) ||
        (length + block_symbols - 1) / block_symbols > 0xFFFFFFFFull || range_count >= 0xFFFFFFFFull) {
        return dec_plan_refuse(p, HUFD_ITEMS_SYMBOL_RANGES, stream);
    }
    if (!eng->can_decode) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    if (range_count) {
        struct hufd_locate job;
        locate_stream_job(&job, (const uint8_t *)device_input + encoded_offset, encoded_length, device_index, length, block_symbols);
        job.ranges = (const struct hufd_symbol_range *)device_ranges;
        if (dec_plan_locate_range_ends(p, &job, range_count, stream)) {
            return AWS_OP_ERR;
        }
    }
    struct hufd_item_source src;
    memset(&src, 0, sizeof(src));
    src.kind = HUFD_ITEMS_SYMBOL_RANGES;
    src.symbol_ranges = (const struct hufd_symbol_range *)device_ranges;
    src.located_bits = p->d_range_bits;
    src.stream_symbols = length;
    src.block_symbols = block_symbols;
    src.encoded_offset = encoded_offset;
    src.encoded_length = encoded_length;
    return dec_plan_fill_on_device(p, &src, range_count, stream);
}

/* ------------------------------------------------------------------ symbols addressed by item (huffman_amd_batch_index.h) */

_Static_assert(sizeof(struct aws_huffman_amd_item_symbol_range) == sizeof(struct hufd_item_symbol_range), "item symbol range layout");
_Static_assert(offsetof(struct aws_huffman_amd_item_symbol_range, first_symbol) == offsetof(struct hufd_item_symbol_range, first_symbol), "item symbol range layout");
_Static_assert(offsetof(struct aws_huffman_amd_item_symbol_range, symbol_count) == offsetof(struct hufd_item_symbol_range, symbol_count), "item symbol range layout");
_Static_assert(offsetof(struct aws_huffman_amd_item_symbol_range, out_offset) == offsetof(struct hufd_item_symbol_range, out_offset), "item symbol range layout");

/* where the items of an indexed batch lie, as the three calls that address by item are told */
struct batch_place {
    const void *encoded; /* the packed buffer's first byte */
    uint64_t encoded_length;
    const uint64_t *directory, *index, *offsets, *lengths;
    uint64_t index_entries, item_count, block_symbols;
    const uint8_t *stored; /* the sender's flags (huffman_amd_stored_index.h), or NULL */
};

static bool batch_place_ok(const struct batch_place *b) {
    return b->directory && !((uintptr_t)b->directory & 7u) && b->index && !((uintptr_t)b->index & 7u) && b->index_entries &&
           b->item_count < 0xFFFFFFFFull && b->offsets && !((uintptr_t)b->offsets & 7u) && !((uintptr_t)b->lengths & 7u) &&
           index_block_symbols_ok(b->block_symbols);
}

/* as locate_stream_job, for positions addressed by item: items[i] / symbols[i], or the ends of item_ranges */
static void locate_batch_job(struct hufd_locate *job, const struct batch_place *b) {
    memset(job, 0, sizeof(*job));
    job->encoded = b->encoded;
    job->encoded_length = b->encoded_length;
    job->index = b->index;
    job->block_symbols = b->block_symbols;
    job->directory = b->directory;
    job->offsets = b->offsets;
    job->lengths = b->lengths;
    job->stored = b->stored;
    job->item_count = b->item_count;
    job->index_entries = b->index_entries;
}

int aws_huffman_amd_locate_item_symbols(
    struct aws_huffman_amd_engine *eng,
    const void *device_encoded,
    uint64_t encoded_length,
    const struct aws_huffman_amd_item_blocks *device_directory,
    const uint64_t *device_index,
    uint64_t index_entries,
    uint64_t item_count,
    uint64_t block_symbols,
    const uint64_t *device_encoded_offsets,
    const uint64_t *device_encoded_lengths,
    const uint64_t *device_items,
    const uint64_t *device_symbols,
    size_t count,
    uint64_t *device_bits,
    uint32_t *device_status,
    void *stream) {
    return aws_huffman_amd_locate_stored_item_symbols(
        eng, device_encoded, encoded_length, device_directory, device_index, index_entries, item_count, block_symbols,
        device_encoded_offsets, device_encoded_lengths, NULL, device_items, device_symbols, count, device_bits, device_status, stream);
}

int aws_huffman_amd_locate_stored_item_symbols(
    struct aws_huffman_amd_engine *eng,
    const void *device_encoded,
    uint64_t encoded_length,
    const struct aws_huffman_amd_item_blocks *device_directory,
    const uint64_t *device_index,
    uint64_t index_entries,
    uint64_t item_count,
    uint64_t block_symbols,
    const uint64_t *device_encoded_offsets,
    const uint64_t *device_encoded_lengths,
    const uint8_t *device_stored,
    const uint64_t *device_items,
    const uint64_t *device_symbols,
    size_t count,
    uint64_t *device_bits,
    uint32_t *device_status,
    void *stream) {

    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION); /* no GPU: there is no CPU path */
    }
    const struct batch_place place = {device_encoded, encoded_length, (const uint64_t *)device_directory, device_index,
                                      device_encoded_offsets, device_encoded_lengths, index_entries, item_count, block_symbols,
                                      device_stored};
    if (!eng || !batch_place_ok(&place) || ((uintptr_t)device_status & 3u) || (encoded_length && !device_encoded) ||
        (count && (!device_items || !device_symbols || !device_bits)) || ((uintptr_t)device_items & 7u) ||
        ((uintptr_t)device_symbols & 7u) || ((uintptr_t)device_bits & 7u)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (!eng->can_decode) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    if (engine_never_fitted(eng)) {
        return aws_raise_error(AWS_ERROR_INVALID_STATE);
    }
    struct hufd_locate job;
    locate_batch_job(&job, &place);
    job.items = device_items;
    job.symbols = device_symbols;
    job.count = count;
    job.bits = device_bits;
    job.status = device_status;
    ON_DEVICE(eng->device);
    const int err = locate_launch(eng, &job, stream ? stream : eng->stream);
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

int aws_huffman_amd_decode_plan_reset_item_symbol_ranges(
    struct aws_huffman_amd_decode_plan *p,
    const void *device_input,
    const struct aws_huffman_amd_item_blocks *device_directory,
    const uint64_t *device_index,
    uint64_t index_entries,
    uint64_t item_count,
    uint64_t block_symbols,
    const uint64_t *device_encoded_offsets,
    const uint64_t *device_encoded_lengths,
    uint64_t encoded_offset,
    uint64_t encoded_length,
    const struct aws_huffman_amd_item_symbol_range *device_ranges,
    size_t range_count,
    void *stream) {
    return aws_huffman_amd_decode_plan_reset_stored_item_symbol_ranges(
        p, device_input, device_directory, device_index, index_entries, item_count, block_symbols, device_encoded_offsets,
        device_encoded_lengths, NULL, encoded_offset, encoded_length, device_ranges, range_count, stream);
}

int aws_huffman_amd_decode_plan_reset_stored_item_symbol_ranges(
    struct aws_huffman_amd_decode_plan *p,
    const void *device_input,
    const struct aws_huffman_amd_item_blocks *device_directory,
    const uint64_t *device_index,
    uint64_t index_entries,
    uint64_t item_count,
    uint64_t block_symbols,
    const uint64_t *device_encoded_offsets,
    const uint64_t *device_encoded_lengths,
    const uint8_t *device_stored,
    uint64_t encoded_offset,
    uint64_t encoded_length,
    const struct aws_huffman_amd_item_symbol_range *device_ranges,
    size_t range_count,
    void *stream) {

    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    if (!p) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    struct aws_huffman_amd_engine *eng = p->engine;
    if (engine_never_fitted(eng)) {
        return aws_raise_error(AWS_ERROR_INVALID_STATE);
    }
    const struct batch_place place = {(const uint8_t *)device_input + encoded_offset, encoded_length, (const uint64_t *)device_directory,
                                      device_index, device_encoded_offsets, device_encoded_lengths, index_entries, item_count,
                                      block_symbols, device_stored};
    if (!batch_place_ok(&place) || (!device_ranges && range_count) || ((uintptr_t)device_ranges & 7u) || (!device_input && range_count) ||
        range_count >= 0xFFFFFFFFull) {
        return dec_plan_refuse(p, HUFD_ITEMS_ITEM_SYMBOL_RANGES, stream);
    }
    if (!eng->can_decode) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    if (range_count) { /* (as aws_huffman_amd_decode_plan_reset_symbol_ranges) */
        struct hufd_locate job;
        locate_batch_job(&job, &place);
        job.item_ranges = (const struct hufd_item_symbol_range *)device_ranges;
        if (dec_plan_locate_range_ends(p, &job, range_count, stream)) {
            return AWS_OP_ERR;
        }
    }
    struct hufd_item_source src;
    memset(&src, 0, sizeof(src));
    src.kind = HUFD_ITEMS_ITEM_SYMBOL_RANGES;
    src.item_symbol_ranges = (const struct hufd_item_symbol_range *)device_ranges;
    src.located_bits = p->d_range_bits;
    src.batch_directory = (const uint64_t *)device_directory;
    src.batch_items = item_count;
    src.block_symbols = block_symbols;
    src.packed_offsets = device_encoded_offsets;
    src.packed_lengths = device_encoded_lengths;
    src.packed_stored = device_stored;
    src.encoded_offset = encoded_offset;
    src.encoded_length = encoded_length;
    if (dec_plan_fill_on_device(p, &src, range_count, stream)) {
        return AWS_OP_ERR;
    }
    return dec_plan_stored_ranges(p, device_stored, device_ranges, stream);
}

/*
 * Device record -> what aws_huffman_decode would have returned
 * (reference source/huffman.c:240-268; DESIGN.md "Decode outcome").
 */
void aws_huffman_amd_decode_result_from_raw(
    const struct hufd_dec_result *raw,
    const struct aws_huffman_amd_decode_item *item,
    struct aws_huffman_amd_decode_result *out) {

    if (raw->total_symbols > item->out_capacity) {
        /* symbol number out_capacity was recognised with nowhere to go: huffman.c:257-268 */
        out->rc = AWS_OP_ERR;
        out->error = AWS_ERROR_SHORT_BUFFER;
        out->produced = item->out_capacity;
        out->bits_consumed = raw->cap_bit - item->first_bit;
        return;
    }
    out->produced = raw->total_symbols;
    out->bits_consumed = raw->stop_bit - item->first_bit;
    out->rc = AWS_OP_SUCCESS;
    out->error = 0;
    if (raw->stop_kind == HUFD_STOP_INVALID) {
        const uint64_t left = item->in_len * 8 - raw->stop_bit;
        if (left >= 32) { /* huffman.c:240-247 */
            out->rc = AWS_OP_ERR;
            out->error = AWS_ERROR_COMPRESSION_UNKNOWN_SYMBOL;
        }
    } else if (raw->stop_kind == HUFD_STOP_NONE) {
        out->rc = AWS_OP_ERR;
        out->error = AWS_ERROR_INVALID_STATE;
    }
}

bool aws_huffman_amd_decode_plan_is_quiet(const struct aws_huffman_amd_decode_plan *p) {
    return p->quiet;
}

int aws_huffman_amd_decode_plan_road(struct aws_huffman_amd_decode_plan *p, void *stream, uint32_t *road, uint32_t *detail) {
    *road = AWS_HUFFMAN_AMD_ROAD_TWO_PASS;
    if (detail) {
        detail[0] = detail[1] = 0;
    }
    (void)p;
    (void)stream;
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_decode_plan_results(
    struct aws_huffman_amd_decode_plan *p,
    struct aws_huffman_amd_decode_result *results,
    void *stream) {

    void *st = stream ? stream : p->engine->stream;
    uint8_t *fetched = malloc(DEC_SUMMARY_BYTES + (p->n_items ? p->n_items : 1) * sizeof(struct hufd_dec_result));
    if (!fetched) {
        return aws_raise_error(AWS_ERROR_OOM);
    }
    struct hufd_dec_result *raw = (struct hufd_dec_result *)(fetched + DEC_SUMMARY_BYTES);
    ON_DEVICE(p->engine->device);
    /* (the records and, in front of them, what the last launch's lists held: one copy) */
    int err = hufs_copy_d2h(fetched, p->d_summary, DEC_SUMMARY_BYTES + (size_t)p->n_items * sizeof(*raw), st);
    if (!err) {
        err = hufs_stream_sync(st);
    }
    if (err) {
        free(fetched);
        return raise_hip(err);
    }
    if (p->n_chunks && p->launches_with_chunks) {
        /* A launch that listed no chunk for any kernel but the regular ones (an ordinary stream of a coder whose walks fall
         * into step): the plan's next launches go without the kernels that only make listed chunks faster -- four empty
         * launches of ~4 us each.  A launch of a quiet plan that does list chunks sends them the long way (exact for every
         * chunk, a fifth of the speed), says so here, and the kernels are back from the next launch on. */
        const uint32_t *listed = (const uint32_t *)fetched;
        p->quiet = !(listed[HUFK_DEC_COUNT_SLOW] | listed[HUFK_DEC_COUNT_LONG] | listed[HUFK_DEC_COUNT_FEW] |
                     listed[HUFK_DEC_COUNT_EMIT] | listed[HUFK_DEC_COUNT_DENSE]);
    }
    if (p->chained || p->packed) {
        /* the items' lengths were never on the host: the device's records say what each result is a result of (after a
         * packed launch the records that launch wrote: the room it gave each item) */
        const struct hufd_dec_item *records = p->packed ? p->d_packed_items : p->d_items;
        struct hufd_dec_item *dev_items = malloc((p->n_items ? p->n_items : 1) * sizeof(*dev_items));
        err = dev_items ? hufs_copy_d2h(dev_items, records, (size_t)p->n_items * sizeof(*dev_items), st) : 2;
        if (!err) {
            err = hufs_stream_sync(st);
        }
        for (uint32_t i = 0; i < p->n_items && !err; ++i) {
            struct aws_huffman_amd_decode_item it;
            memset(&it, 0, sizeof(it));
            it.in_offset = dev_items[i].in_off;
            it.in_len = dev_items[i].in_len;
            it.first_bit = (uint8_t)dev_items[i].first_bit;
            it.out_offset = dev_items[i].out_off;
            it.out_capacity = dev_items[i].out_cap;
            aws_huffman_amd_decode_result_from_raw(&raw[i], &it, &results[i]);
        }
        free(dev_items);
        free(fetched);
        return err ? raise_hip(err) : AWS_OP_SUCCESS;
    }
    for (uint32_t i = 0; i < p->n_items; ++i) {
        aws_huffman_amd_decode_result_from_raw(&raw[i], &p->h_items[i], &results[i]);
    }
    free(fetched);
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_decode_plan_from_encode(
    struct aws_huffman_amd_decode_plan *p,
    const struct aws_huffman_amd_encode_plan *encoded,
    void *stream) {

    struct aws_huffman_amd_engine *eng = p->engine;
    if (!eng->can_decode) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    if (!encoded || encoded->engine->device != eng->device || !encoded->launched) {
        p->quiet = false; /* (a reset, refused or not: the plan's items stay, what is known of their launches' lists does not) */
        p->launches_with_chunks = 0;
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT); /* (a plan that was never launched has no records to read lengths from) */
    }
    if (encoded->stored) {
        /* (a stored launch left raw bytes among the codes: aws_huffman_amd_decode_plan_reset_packed_stored_input is the way back) */
        p->quiet = false;
        p->launches_with_chunks = 0;
        return aws_raise_error(AWS_ERROR_INVALID_STATE);
    }
    /* Whatever the launch produced, every item must be ONE THREAD's work for the decoder (then the plan has no chunk
     * geometry, which only the host can lay out): the most bytes an item can have left is its output capacity.  The same
     * rule as for a plan from host records (dec_tiny_limit), with the capacities for the lengths. */
    /* (after a packed launch the items' own capacities were not used: the bound is what the longest item can come to --
     * its symbols at the longest code, and the carried bits --, known here without a wait; the records the decode plan is
     * made from are the ones that launch wrote behind) */
    const uint64_t packed_bound =
        (encoded->longest_in_len * (uint64_t)encoded->engine->tables.enc_max_bits + encoded->most_overflow_bits + 7) / 8;
    const struct hufd_enc_item *enc_items = encoded->packed ? encoded->d_packed_items : encoded->d_items;
    const uint64_t n_items = encoded->n_items, longest = encoded->packed ? packed_bound : encoded->largest_out_cap;
    bool thread_each = n_items >= 1 && n_items < 0xFFFFFFFFull && longest <= HUFD_TINY_FEW_BYTES;
    {
        static const uint64_t classes[2] = {HUFD_DEC_COOP_BYTES, HUFD_DEC_TINY_BYTES};
        for (int c = 0; c < 2 && !thread_each && n_items >= 1 && n_items < 0xFFFFFFFFull; ++c) {
            thread_each = longest <= classes[c] && n_items >= tiny_per_byte(true) * longest;
        }
    }
    if (!thread_each) {
        /* items with chunks (or too few short ones for a thread each): the general plan, made on the device from the
         * launch's records -- the lengths stay there; what comes back are the few totals that size the plan */
        struct hufd_item_source src;
        memset(&src, 0, sizeof(src));
        src.kind = HUFD_ITEMS_FROM_ENCODE;
        src.enc_items = enc_items;
        src.enc_results = encoded->d_results;
        return dec_plan_fill_on_device(p, &src, (size_t)n_items, stream);
    }
    p->n_items = p->n_chunks = p->n_large = p->n_runs = p->n_tail = p->n_fixed = p->n_wide = 0;
    p->quiet = false; /* (other items: nothing is known of what their launches list) */
    p->launches_with_chunks = 0; /* (... and no launch of these has left a summary to read it from) */
    p->packed = p->packed_sized = p->stored = p->stored_ranges = false;
    p->longest_in_len = 0;
    p->n_tiny = p->n_deep = 0;
    memset(&p->stats, 0, sizeof(p->stats));
    p->chained = false;
    ON_DEVICE(eng->device);
    int e = dec_plan_reserve(p, n_items, 0, 0, 0);
    if (!e) {
        e = hufk_decode_plan_from_encode(
            enc_items, encoded->d_results, (uint32_t)n_items, p->d_items, p->d_tiny, stream ? stream : eng->stream);
    }
    if (e) {
        return raise_hip(e);
    }
    p->wide_from = wide_min_bytes(0);
    p->tail_stage_bytes = 0;
    p->tail_lanes = 0;
    p->tail_wide_lanes = 0;
    p->n_tail_narrow = 0;
    p->n_items = (uint32_t)n_items;
    p->n_tiny = (uint32_t)n_items;
    p->chained = true;
    p->stats.items = p->stats.by_thread = n_items;
    p->stats.thread_limit = longest;
    e = plan_mark_done(&p->done_event, &p->done_on_engine_stream, eng, stream); /* (hufk_decode_plan_from_encode is in flight) */
    return e ? raise_hip(e) : AWS_OP_SUCCESS;
}

/* ------------------------------------------------------------------ one-item helpers for the host-pointer API */

/* one of the engine's two staging buffers, grown by a quarter more than asked */
static int one_shot_grow(void **buffer, size_t *cap, size_t bytes) {
    if (bytes > *cap) {
        *cap = bytes + bytes / 4 + 4096;
        const struct arena_part whole = {buffer, *cap};
        if (arena_alloc(buffer, &whole, 1)) {
            *cap = 0;
            return aws_raise_error(AWS_ERROR_OOM);
        }
    }
    return AWS_OP_SUCCESS;
}

static int one_shot_reserve(struct aws_huffman_amd_engine *eng, size_t in_bytes, size_t out_bytes) {
    ON_DEVICE(eng->device);
    return one_shot_grow(&eng->one_in, &eng->one_in_cap, in_bytes) || one_shot_grow(&eng->one_out, &eng->one_out_cap, out_bytes)
               ? AWS_OP_ERR
               : AWS_OP_SUCCESS;
}

/*
 * Inputs of up to a few KiB (what the reference's HPACK consumer passes is tens of bytes, one call per header field):
 * the item record and the input go up in ONE copy from a page-locked block, ONE launch does the work -- one thread
 * (enc_tiny / dec_tiny) up to MINI_MAX_IN bytes, beyond that one workgroup (enc_block, dec_block; with long codes one
 * wave of dec_deep) --, the result record and the output come back in ONE copy.  The general road costs a plan upload, four
 * small pageable copies, four or five launches and two synchronisations for the same call.
 */
enum {
    MINI_MAX_IN = 128,     /* symbols to encode / encoded bytes (carried ones included) that are ONE THREAD's work */
    MINI_IN_AT = 64,       /* block layout: [0] item record, [64] input (decode: 16 bytes for the carried ones first), */
    MINI_ZERO_AT = 32896,  /* [32896] zero word, [32960] scratch, */
    MINI_SCRATCH_AT = 32960,
    MINI_RESULT_AT = 33024, /* [33024] result record, [33088] output */
    MINI_OUT_AT = 33088,
    MINI_BLOCK = 131072,
    MINI_MAX_OUT = MINI_BLOCK - MINI_OUT_AT
};

static bool mini_ready(struct aws_huffman_amd_engine *eng) {
    if (eng->mini_host && eng->mini_dev) {
        return true;
    }
    ON_DEVICE(eng->device);
    if (!eng->mini_host) {
        eng->mini_host = hufs_host_alloc(MINI_BLOCK);
    }
    if (!eng->mini_dev) {
        eng->mini_dev = hufs_malloc(MINI_BLOCK);
        if (eng->mini_dev && (hufs_memset(eng->mini_dev, 0, MINI_BLOCK, eng->stream) || hufs_stream_sync(eng->stream))) {
            hufs_free(eng->mini_dev);
            eng->mini_dev = NULL;
        }
    }
    return eng->mini_host && eng->mini_dev;
}

static int mini_encode(
    struct aws_huffman_amd_engine *eng,
    const struct aws_huffman_amd_encode_item *item,
    uint64_t dev_out,
    const uint8_t *host_in,
    uint8_t *host_out,
    bool length_only,
    struct hufd_enc_result *raw) {

    struct hufd_enc_item rec;
    memset(&rec, 0, sizeof(rec));
    rec.in_off = MINI_IN_AT;
    rec.in_len = item->in_len;
    rec.out_off = MINI_OUT_AT;
    rec.out_cap = dev_out;
    rec.ovf_bits = item->overflow_in.num_bits;
    rec.ovf_pattern = rec.ovf_bits >= 32 ? item->overflow_in.pattern
                                         : item->overflow_in.pattern & ((1u << rec.ovf_bits) - 1u);
    rec.eos_padding = item->eos_padding;
    rec.tiny = 1;
    rec.n_segs = 0;
    memcpy(eng->mini_host, &rec, sizeof(rec));
    if (item->in_len) { /* an empty cursor may carry a NULL pointer (source/huffman.c:161-167 never touches it) */
        memcpy(eng->mini_host + MINI_IN_AT, host_in, item->in_len);
    }
    ON_DEVICE(eng->device);
    int err = hufs_copy_h2d(eng->mini_dev, eng->mini_host, MINI_IN_AT + item->in_len, eng->stream);
    if (!err && item->in_len <= MINI_MAX_IN) {
        err = hufk_encode_one_tiny(
            &eng->tables, (const struct hufd_enc_item *)eng->mini_dev, (const uint32_t *)(eng->mini_dev + MINI_ZERO_AT),
            eng->mini_dev, eng->mini_dev, (struct hufd_enc_result *)(eng->mini_dev + MINI_RESULT_AT), length_only,
            eng->stream);
    } else if (!err) {
        err = hufk_encode_one_block(
            &eng->tables, (const struct hufd_enc_item *)eng->mini_dev, (uint32_t)item->in_len, eng->mini_dev, eng->mini_dev,
            (struct hufd_enc_result *)(eng->mini_dev + MINI_RESULT_AT), length_only, eng->stream);
    }
    if (!err) {
        const size_t back = (MINI_OUT_AT - MINI_RESULT_AT) + (length_only ? 0 : dev_out);
        err = hufs_copy_d2h(eng->mini_host + MINI_RESULT_AT, eng->mini_dev + MINI_RESULT_AT, back, eng->stream);
    }
    if (!err) {
        err = hufs_stream_sync(eng->stream);
    }
    if (err) {
        return raise_hip(err);
    }
    memcpy(raw, eng->mini_host + MINI_RESULT_AT, sizeof(*raw));
    if (!length_only && raw->produced) {
        memcpy(host_out, eng->mini_host + MINI_OUT_AT, raw->produced);
    }
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_engine_encode_host(
    struct aws_huffman_amd_engine *eng,
    const struct aws_huffman_amd_encode_item *item_in,
    const uint8_t *host_in,
    uint8_t *host_out,
    bool length_only,
    struct hufd_enc_result *raw) {

    struct aws_huffman_amd_encode_item item = *item_in;
    /*
     * Only the symbols this call can consume are staged.  The reference reads symbol k only while the output has a
     * free byte (source/huffman.c:162-164), i.e. while the bits in front of it -- carried ones + at least min_bits
     * per earlier symbol -- are fewer than 8 * room: at most ceil((8 * room - carried) / min_bits) symbols, one more
     * here so that a call that fills its room exactly still sees input behind it (and says SHORT_BUFFER, as the
     * reference would at the top of its next turn).  A caller that offers its output a few bytes at a time
     * (huffman_test_transitive_chunked, HPACK's SHORT_BUFFER resumption) otherwise pays for the whole rest of its
     * input in every call: O(n^2 / chunk) bytes over the bus and through the count.
     */
    if (!length_only && eng->tables.enc_min_bits && item.out_capacity < (UINT64_MAX >> 4)) {
        const uint64_t room_bits = item.out_capacity * 8;
        const uint64_t carried = item.overflow_in.num_bits;
        const uint64_t fit = room_bits > carried ? (room_bits - carried + eng->tables.enc_min_bits - 1) / eng->tables.enc_min_bits : 0;
        if (fit + 1 < item.in_len) {
            item.in_len = fit + 1;
        }
    }
    /* the device output never needs more than the worst-case encoding */
    const uint64_t worst = (item.in_len * eng->tables.enc_max_bits + item.overflow_in.num_bits + 7) / 8;
    const uint64_t dev_out = item.out_capacity < worst ? item.out_capacity : worst;
    item.in_offset = 0;
    item.out_offset = 0;
    if (hufk_encode_one_block_fits(&eng->tables, item.in_len) && (item.in_len || item.overflow_in.num_bits) && item.overflow_in.num_bits <= 32 &&
        (length_only || dev_out <= MINI_MAX_OUT) && mini_ready(eng)) {
        return mini_encode(eng, &item, dev_out, host_in, host_out, length_only, raw);
    }
    if (one_shot_reserve(eng, item.in_len + 16, length_only ? 0 : dev_out + 16)) {
        return AWS_OP_ERR;
    }
    if (!eng->one_enc) {
        eng->one_enc = calloc(1, sizeof(*eng->one_enc));
        if (!eng->one_enc) {
            return aws_raise_error(AWS_ERROR_OOM);
        }
        eng->one_enc->engine = eng;
    }
    if (enc_plan_fill(eng->one_enc, &item, 1)) {
        return AWS_OP_ERR;
    }
    int err = hufs_copy_h2d(eng->one_in, host_in, item.in_len, eng->stream);
    if (err) {
        return raise_hip(err);
    }
    if (aws_huffman_amd_encode_plan_launch(eng->one_enc, eng->one_in, eng->one_out, length_only, eng->stream)) {
        return AWS_OP_ERR;
    }
    if (aws_huffman_amd_encode_plan_raw_results(eng->one_enc, raw, eng->stream)) {
        return AWS_OP_ERR;
    }
    if (!length_only && raw->produced) {
        err = hufs_copy_d2h(host_out, eng->one_out, raw->produced, eng->stream);
        if (!err) {
            err = hufs_stream_sync(eng->stream);
        }
        if (err) {
            return raise_hip(err);
        }
    }
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_engine_decode_host(
    struct aws_huffman_amd_engine *eng,
    const uint8_t *carry,
    uint32_t carry_bytes,
    uint32_t first_bit,
    const uint8_t *host_in,
    uint64_t in_len,
    uint64_t out_capacity,
    struct aws_huffman_amd_decode_result *result) {

    if (!eng->can_decode) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION);
    }
    /*
     * Only the bytes this call can get through are staged: with room for r symbols the reference stops at the latest
     * when it has recognised symbol r + 1 (source/huffman.c:257-268), which lies within (r + 1) * max_bits bits of
     * the stream's first one; eight bytes more keep a code without a match "at least 32 bits from the end" exactly
     * when it is so in the whole stream (source/huffman.c:240-247).  (The caller's cursor and the decoder's window
     * are worked out from the bits consumed and the real length, in huffman.c.)
     */
    if (out_capacity < (UINT64_MAX >> 8) && eng->tables.max_bits) {
        const uint64_t need_bits = first_bit + (out_capacity + 1) * (eng->tables.max_bits ? eng->tables.max_bits : 32);
        const uint64_t need_bytes = (need_bits + 7) / 8 + 8;
        if (need_bytes < carry_bytes + in_len) {
            in_len = need_bytes > carry_bytes ? need_bytes - carry_bytes : 0;
        }
    }
    /* the carried bytes sit right before the new bytes, which start 16-byte aligned */
    const uint64_t stream_bits = (carry_bytes + in_len) * 8 - first_bit;
    const uint64_t most_symbols = stream_bits / eng->tables.min_bits;
    const uint64_t dev_out = out_capacity < most_symbols ? out_capacity : most_symbols;
    eng->mini_output = false;
    /* (decode: one thread, or one workgroup up to HUFD_DEC_BLOCK_BYTES -- with long codes one wave up to
     * HUFD_DEC_COOP_BYTES; the chunk kernels take what is longer) */
    /* (codes of one length: dec_block's lanes would never settle -- a thread, or the plan's dec_fixed kernels) */
    const uint64_t mini_in =
        eng->tables.deep_entries ? HUFD_DEC_COOP_BYTES : (eng->tables.fixed_bits ? MINI_MAX_IN : HUFD_DEC_BLOCK_MAX_BYTES);
    if (carry_bytes + in_len <= mini_in && carry_bytes + in_len > 0 && dev_out <= MINI_MAX_OUT && mini_ready(eng)) {
        struct hufd_dec_item rec;
        memset(&rec, 0, sizeof(rec));
        rec.in_off = MINI_IN_AT + 16 - carry_bytes;
        rec.in_len = carry_bytes + in_len;
        rec.out_off = MINI_OUT_AT;
        rec.out_cap = dev_out;
        rec.first_bit = first_bit;
        rec.tiny = 1;
        memcpy(eng->mini_host, &rec, sizeof(rec));
        memcpy(eng->mini_host + MINI_IN_AT + 16 - carry_bytes, carry, carry_bytes);
        if (in_len) { /* carried bits and an empty cursor, which may be {0, NULL} (source/huffman.c:196-211) */
            memcpy(eng->mini_host + MINI_IN_AT + 16, host_in, in_len);
        }
        ON_DEVICE(eng->device);
        int e = hufs_copy_h2d(eng->mini_dev, eng->mini_host, MINI_IN_AT + 16 + in_len, eng->stream);
        if (!e) {
            /* a lone thread up to MINI_MAX_IN bytes, a workgroup (a wave with long codes) above */
            if (carry_bytes + in_len <= MINI_MAX_IN) {
                e = hufk_decode_one_tiny(
                    &eng->tables, (const struct hufd_dec_item *)eng->mini_dev, (const uint32_t *)(eng->mini_dev + MINI_ZERO_AT),
                    eng->mini_dev, eng->mini_dev, (struct hufd_dec_item_state *)(eng->mini_dev + MINI_SCRATCH_AT),
                    (struct hufd_dec_result *)(eng->mini_dev + MINI_RESULT_AT), eng->stream);
            } else if (eng->tables.deep_entries) {
                e = hufk_decode_one_coop(
                    &eng->tables, (const struct hufd_dec_item *)eng->mini_dev, (const uint32_t *)(eng->mini_dev + MINI_ZERO_AT),
                    eng->mini_dev, eng->mini_dev, (struct hufd_dec_item_state *)(eng->mini_dev + MINI_SCRATCH_AT),
                    (struct hufd_dec_result *)(eng->mini_dev + MINI_RESULT_AT), eng->stream);
            } else {
                e = hufk_decode_one_block(
                    &eng->tables, &rec, eng->mini_dev, eng->mini_dev,
                    (struct hufd_dec_item_state *)(eng->mini_dev + MINI_SCRATCH_AT),
                    (struct hufd_dec_result *)(eng->mini_dev + MINI_RESULT_AT), eng->stream);
            }
        }
        if (!e) {
            e = hufs_copy_d2h(
                eng->mini_host + MINI_RESULT_AT, eng->mini_dev + MINI_RESULT_AT, (MINI_OUT_AT - MINI_RESULT_AT) + dev_out,
                eng->stream);
        }
        if (!e) {
            e = hufs_stream_sync(eng->stream);
        }
        if (e) {
            return raise_hip(e);
        }
        struct hufd_dec_result raw;
        memcpy(&raw, eng->mini_host + MINI_RESULT_AT, sizeof(raw));
        if (raw.stop_kind == HUFD_STOP_GAVE_UP) {
            goto chunked; /* a stream dec_block's lanes do not settle on: nothing is decoded yet */
        }
        struct aws_huffman_amd_decode_item as_item;
        memset(&as_item, 0, sizeof(as_item));
        as_item.in_len = carry_bytes + in_len;
        as_item.first_bit = first_bit;
        as_item.out_capacity = dev_out;
        aws_huffman_amd_decode_result_from_raw(&raw, &as_item, result);
        eng->mini_output = true;
        if (result->error == AWS_ERROR_SHORT_BUFFER && dev_out < out_capacity) {
            return aws_raise_error(AWS_ERROR_INVALID_STATE);
        }
        return AWS_OP_SUCCESS;
    }
chunked:
    if (one_shot_reserve(eng, 16 + in_len + 16, dev_out + 16)) {
        return AWS_OP_ERR;
    }
    struct aws_huffman_amd_decode_item item;
    memset(&item, 0, sizeof(item));
    item.in_offset = 16 - carry_bytes;
    item.in_len = carry_bytes + in_len;
    item.first_bit = first_bit;
    item.out_offset = 0;
    item.out_capacity = dev_out;
    if (!eng->one_dec) {
        eng->one_dec = calloc(1, sizeof(*eng->one_dec));
        if (!eng->one_dec) {
            return aws_raise_error(AWS_ERROR_OOM);
        }
        eng->one_dec->engine = eng;
    }
    if (dec_plan_fill(eng->one_dec, &item, 1)) {
        return AWS_OP_ERR;
    }
    int err = 0;
    if (carry_bytes) {
        err = hufs_copy_h2d((uint8_t *)eng->one_in + 16 - carry_bytes, carry, carry_bytes, eng->stream);
    }
    if (!err) {
        err = hufs_copy_h2d((uint8_t *)eng->one_in + 16, host_in, in_len, eng->stream);
    }
    if (err) {
        return raise_hip(err);
    }
    if (aws_huffman_amd_decode_plan_launch(eng->one_dec, eng->one_in, eng->one_out, eng->stream)) {
        return AWS_OP_ERR;
    }
    if (aws_huffman_amd_decode_plan_results(eng->one_dec, result, eng->stream)) {
        return AWS_OP_ERR;
    }
    /* the device capacity was clipped to what the stream can hold; undo that in the verdict */
    if (result->error == AWS_ERROR_SHORT_BUFFER && dev_out < out_capacity) {
        return aws_raise_error(AWS_ERROR_INVALID_STATE);
    }
    return AWS_OP_SUCCESS;
}

int aws_huffman_amd_engine_fetch_output(struct aws_huffman_amd_engine *eng, uint8_t *host_out, uint64_t size) {
    if (eng->mini_output) {
        if (size) {
            memcpy(host_out, eng->mini_host + MINI_OUT_AT, size); /* came back with the result record */
        }
        return AWS_OP_SUCCESS;
    }
    int err = hufs_copy_d2h(host_out, eng->one_out, size, eng->stream);
    if (!err) {
        err = hufs_stream_sync(eng->stream);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

/* ------------------------------------------------------------------ device helpers */

int aws_huffman_amd_device_count(void) {
    return hufs_device_count();
}

void *aws_huffman_amd_device_alloc(struct aws_huffman_amd_engine *eng, size_t size) {
    ON_DEVICE(eng->device);
    void *p = hufs_malloc(size);
    if (!p) {
        aws_raise_error(AWS_ERROR_OOM);
    }
    return p;
}

void aws_huffman_amd_device_free(struct aws_huffman_amd_engine *eng, void *ptr) {
    ON_DEVICE(eng->device);
    hufs_free(ptr);
}

int aws_huffman_amd_copy_to_device(struct aws_huffman_amd_engine *eng, void *dst, const void *src, size_t size) {
    ON_DEVICE(eng->device);
    int err = hufs_copy_h2d(dst, src, size, eng->stream);
    if (!err) {
        err = hufs_stream_sync(eng->stream);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

int aws_huffman_amd_copy_to_host(struct aws_huffman_amd_engine *eng, void *dst, const void *src, size_t size) {
    ON_DEVICE(eng->device);
    int err = hufs_copy_d2h(dst, src, size, eng->stream);
    if (!err) {
        err = hufs_stream_sync(eng->stream);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

int aws_huffman_amd_device_fill(struct aws_huffman_amd_engine *eng, void *dst, int byte, size_t size) {
    ON_DEVICE(eng->device);
    int err = hufs_memset(dst, byte, size, eng->stream);
    if (!err) {
        err = hufs_stream_sync(eng->stream);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

int aws_huffman_amd_device_fill_splitmix64(struct aws_huffman_amd_engine *eng, void *dst, size_t size, uint64_t seed) {
    ON_DEVICE(eng->device);
    int err = hufk_fill_splitmix64(dst, size, seed, eng->stream);
    if (!err) {
        err = hufs_stream_sync(eng->stream);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

/* what a workgroup of the counting kernel reads at most between two flushes of its 32-bit LDS counts: the default keeps
 * every counter below 2^32 with room to spare (tests make it small, to run the flushes inside a launch) */
static uint64_t s_count_flush_bytes = 0;

void aws_huffman_amd_testing_set_count_flush_bytes(uint64_t bytes) {
    __atomic_store_n(&s_count_flush_bytes, bytes, __ATOMIC_RELAXED);
}

int aws_huffman_amd_symbol_counts(int device, const void *device_input, uint64_t length, uint64_t *device_counts, void *stream) {
    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION); /* no GPU: there is no CPU path */
    }
    if (length && (!device_input || !device_counts)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (device < 0 && hufs_get_device(&device)) {
        return aws_raise_error(AWS_ERROR_UNKNOWN);
    }
    if (device >= hufs_device_count()) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (length == 0) {
        return AWS_OP_SUCCESS;
    }
    ON_DEVICE(device);
    int err = hufk_init(); /* the grid's size: the device's compute units */
    if (!err) {
        const uint64_t asked = __atomic_load_n(&s_count_flush_bytes, __ATOMIC_RELAXED);
        err = hufk_symbol_counts(device_input, length, device_counts, asked ? asked : (1ull << 30), stream);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

/* the same sums over the current items of an encode plan (huffman_amd_plan_counts.h): the plan's own lists are the work, so
 * nothing is made for the call -- no scratch, no wait -- and nothing of the plan is written */
int aws_huffman_amd_encode_plan_symbol_counts(
    struct aws_huffman_amd_encode_plan *p, const void *device_input, uint64_t *device_counts, void *stream) {
    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION); /* no GPU: there is no CPU path */
    }
    if (!p || !device_counts || ((uintptr_t)device_counts & 7u) || (p->n_items && !device_input)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (p->n_items == 0) {
        return AWS_OP_SUCCESS;
    }
    struct aws_huffman_amd_engine *eng = p->engine;
    ON_DEVICE(eng->device);
    const uint64_t asked = __atomic_load_n(&s_count_flush_bytes, __ATOMIC_RELAXED);
    int err = hufk_plan_symbol_counts(
        p->d_items, p->d_segs, p->n_segs, p->d_solo, p->n_solo, p->d_tiny, p->n_tiny, p->stats.thread_limit, device_input,
        device_counts, asked ? asked : (1ull << 30), stream ? stream : eng->stream);
    if (!err) {
        /* (the plan's records are read on this stream: whoever gets its arrays next waits, as for a launch) */
        err = plan_mark_done(&p->done_event, &p->done_on_engine_stream, eng, stream);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

/* Byte planes (huffman_amd_planes.h): what both calls check on the host, and the enqueue -- one launch, nothing made for it */
static uint32_t s_planes_grid = 0;

void aws_huffman_amd_testing_set_planes_grid(uint32_t workgroups) {
    __atomic_store_n(&s_planes_grid, workgroups, __ATOMIC_RELAXED);
}

/* the checks the two calls share.  1: go on, 0: nothing to do, -1: raised */
static int planes_check(
    int *device, const void *elements, const void *planes, uint64_t element_count, uint32_t element_bytes, uint64_t plane_stride) {
    if (hufs_device_count() <= 0) {
        return aws_raise_error(AWS_ERROR_UNSUPPORTED_OPERATION); /* no GPU: there is no CPU path */
    }
    if (element_bytes != 1 && element_bytes != 2 && element_bytes != 4 && element_bytes != 8) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (element_count && (!elements || !planes)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (plane_stride < element_count) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    /* n * E and (E - 1) * S + n fit 64 bits */
    if (element_count > UINT64_MAX / element_bytes ||
        (element_bytes > 1 && plane_stride > (UINT64_MAX - element_count) / (element_bytes - 1u))) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (*device < 0 && hufs_get_device(device)) {
        return aws_raise_error(AWS_ERROR_UNKNOWN);
    }
    if (*device >= hufs_device_count()) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    if (element_count == 0) {
        return 0;
    }
    /* the two ranges must not meet: [elements, + n * E) and [planes, + (E - 1) * S + n) */
    const uint64_t a = (uint64_t)(uintptr_t)elements, a_len = element_count * element_bytes;
    const uint64_t b = (uint64_t)(uintptr_t)planes, b_len = (uint64_t)(element_bytes - 1u) * plane_stride + element_count;
    if (a_len > UINT64_MAX - a || b_len > UINT64_MAX - b || (a < b + b_len && b < a + a_len)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    return 1;
}

/* the two calls and their twins over differences in runs (huffman_amd_planes_delta.h): run_elements 0 is the plain call */
static int planes_split_any(
    int device, const void *device_input, uint64_t element_count, uint32_t element_bytes, uint32_t run_elements,
    void *device_planes, uint64_t plane_stride, uint64_t *device_counts, void *stream) {
    if (hufs_device_count() > 0 && ((uintptr_t)device_counts & 7u)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    const int go = planes_check(&device, device_input, device_planes, element_count, element_bytes, plane_stride);
    if (go <= 0) {
        return go;
    }
    ON_DEVICE(device);
    int err = hufk_init(); /* the grid's size: the device's compute units */
    if (!err) {
        const uint64_t asked = __atomic_load_n(&s_count_flush_bytes, __ATOMIC_RELAXED);
        err = hufk_planes_split(
            device_input, element_count, element_bytes, run_elements, device_planes, plane_stride, device_counts,
            asked ? asked : (1ull << 30), __atomic_load_n(&s_planes_grid, __ATOMIC_RELAXED), stream);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

static int planes_merge_any(
    int device, const void *device_planes, uint64_t plane_stride, uint64_t element_count, uint32_t element_bytes,
    uint32_t run_elements, void *device_output, void *stream) {
    const int go = planes_check(&device, device_output, device_planes, element_count, element_bytes, plane_stride);
    if (go <= 0) {
        return go;
    }
    ON_DEVICE(device);
    int err = hufk_init();
    if (!err) {
        err = hufk_planes_merge(
            device_planes, plane_stride, element_count, element_bytes, run_elements, device_output,
            __atomic_load_n(&s_planes_grid, __ATOMIC_RELAXED), stream);
    }
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

int aws_huffman_amd_planes_split(
    int device, const void *device_input, uint64_t element_count, uint32_t element_bytes, void *device_planes,
    uint64_t plane_stride, uint64_t *device_counts, void *stream) {
    return planes_split_any(device, device_input, element_count, element_bytes, 0, device_planes, plane_stride, device_counts, stream);
}

int aws_huffman_amd_planes_merge(
    int device, const void *device_planes, uint64_t plane_stride, uint64_t element_count, uint32_t element_bytes,
    void *device_output, void *stream) {
    return planes_merge_any(device, device_planes, plane_stride, element_count, element_bytes, 0, device_output, stream);
}

/* a run: a power of two from 16 to 2048 -- a lane's group is 16 elements (8 of 8 bytes) and the merge's step 2048 elements of
 * 8 bytes, so a run starts on a group and lies in one step.  (Without a GPU the answer is that there is none, whatever else.) */
static bool planes_run_refused(uint32_t run_elements) {
    return hufs_device_count() > 0 && (run_elements < 16 || run_elements > 2048 || (run_elements & (run_elements - 1)));
}

int aws_huffman_amd_plane_delta_split(
    int device, const void *device_input, uint64_t element_count, uint32_t element_bytes, uint32_t run_elements,
    void *device_planes, uint64_t plane_stride, uint64_t *device_counts, void *stream) {
    if (planes_run_refused(run_elements)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    return planes_split_any(
        device, device_input, element_count, element_bytes, run_elements, device_planes, plane_stride, device_counts, stream);
}

int aws_huffman_amd_plane_delta_merge(
    int device, const void *device_planes, uint64_t plane_stride, uint64_t element_count, uint32_t element_bytes,
    uint32_t run_elements, void *device_output, void *stream) {
    if (planes_run_refused(run_elements)) {
        return aws_raise_error(AWS_ERROR_INVALID_ARGUMENT);
    }
    return planes_merge_any(device, device_planes, plane_stride, element_count, element_bytes, run_elements, device_output, stream);
}

int aws_huffman_amd_stream_synchronize(struct aws_huffman_amd_engine *eng, void *stream) {
    ON_DEVICE(eng->device);
    const int err = hufs_stream_sync(stream ? stream : eng->stream);
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

void *aws_huffman_amd_event_new(struct aws_huffman_amd_engine *eng) {
    ON_DEVICE(eng->device);
    return hufs_event_create();
}

void aws_huffman_amd_event_destroy(struct aws_huffman_amd_engine *eng, void *event) {
    ON_DEVICE(eng->device);
    hufs_event_destroy(event);
}

int aws_huffman_amd_event_record(struct aws_huffman_amd_engine *eng, void *event, void *stream) {
    ON_DEVICE(eng->device);
    const int err = hufs_event_record(event, stream ? stream : eng->stream);
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}

int aws_huffman_amd_event_elapsed_ms(struct aws_huffman_amd_engine *eng, void *start, void *stop, float *ms) {
    ON_DEVICE(eng->device);
    const int err = hufs_event_elapsed_ms(start, stop, ms);
    return err ? raise_hip(err) : AWS_OP_SUCCESS;
}
