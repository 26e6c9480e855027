/* TEST INFRASTRUCTURE.  A host-only check of arena_alloc (csrc/host/arena.h), the one place a plan's device arrays
 * are allocated and cut: built with AddressSanitizer + UBSan against the stand-ins for hufs_malloc / hufs_free below, which
 * hand out host memory aligned as device memory is.  Driven by tests/test_host_arena.py; prints "arena ok". */
#include "arena.h"

#include <stdio.h>
#include <stdlib.h>

static size_t s_last_size, s_mallocs, s_frees;
static int s_fail_next;

void *hufs_malloc(size_t size) {
    void *p = NULL;
    ++s_mallocs;
    s_last_size = size;
    if (s_fail_next) {
        s_fail_next = 0;
        return NULL;
    }
    return posix_memalign(&p, 256, size ? size : 1) ? NULL : p; /* (exactly `size` usable bytes as far as ASan goes) */
}

void hufs_free(void *ptr) {
    if (ptr) {
        ++s_frees;
    }
    free(ptr);
}

#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            fprintf(stderr, "arena_check.c:%d: %s\n", __LINE__, #cond);                                                \
            exit(1);                                                                                                   \
        }                                                                                                              \
    } while (0)

#define N_PARTS 8

/* every slot on a multiple of 256 bytes, in the order of the parts, no two parts overlapping, all inside the allocation;
 * every byte of every part is written (the sanitizer watches the bounds) */
static void check_layout(void *arena, uint8_t *const *slots, const size_t *bytes, uint8_t fill) {
    const uint8_t *end = (const uint8_t *)arena;
    CHECK(arena && slots[0] == arena);
    for (int i = 0; i < N_PARTS; ++i) {
        CHECK(((uintptr_t)slots[i] & 255u) == 0);
        CHECK(slots[i] >= end);                 /* behind the part in front of it */
        CHECK(slots[i] - end < 256);            /* ... by no more than the cut */
        memset(slots[i], fill, bytes[i]);
        end = slots[i] + bytes[i];
    }
    CHECK((size_t)(end - (const uint8_t *)arena) == s_last_size); /* the allocation ends with the last part */
}

int main(void) {
    void *arena = NULL;
    uint8_t *slots[N_PARTS] = {0};
    uint32_t *typed = NULL; /* (a slot is a pointer of any object type) */
    size_t bytes[N_PARTS] = {1, 255, 256, 257, 0, 4096, 0, 8}; /* zero-byte parts inside, and side by side with others */
    struct arena_part parts[N_PARTS];
    for (int i = 0; i < N_PARTS; ++i) {
        parts[i].slot = &slots[i];
        parts[i].bytes = bytes[i];
    }

    /* a first allocation */
    CHECK(arena_alloc(&arena, parts, N_PARTS) == 0);
    CHECK(s_mallocs == 1 && s_frees == 0);
    check_layout(arena, slots, bytes, 0x11);
    CHECK(slots[4] == slots[5]); /* a part of no bytes takes no room: the next one starts where it does */

    /* growth: the old block is freed, every slot placed anew */
    for (int i = 0; i < N_PARTS; ++i) {
        bytes[i] = bytes[i] * 3 + 7;
        parts[i].bytes = bytes[i];
    }
    CHECK(arena_alloc(&arena, parts, N_PARTS) == 0);
    CHECK(s_mallocs == 2 && s_frees == 1);
    check_layout(arena, slots, bytes, 0x22);

    /* a zero-byte part at the very end, and a slot of another pointer type */
    bytes[N_PARTS - 1] = 0;
    parts[N_PARTS - 1].bytes = 0;
    parts[N_PARTS - 1].slot = &typed;
    CHECK(arena_alloc(&arena, parts, N_PARTS) == 0);
    slots[N_PARTS - 1] = (uint8_t *)typed;
    check_layout(arena, slots, bytes, 0x33);
    CHECK(s_mallocs == 3 && s_frees == 2);

    /* a failed allocation: 2, the old block freed, the arena NULL, the slots as they were */
    uint8_t *before[N_PARTS];
    memcpy(before, slots, sizeof(before));
    s_fail_next = 1;
    CHECK(arena_alloc(&arena, parts, N_PARTS) == 2);
    CHECK(arena == NULL && s_mallocs == 4 && s_frees == 3);
    slots[N_PARTS - 1] = (uint8_t *)typed;
    CHECK(memcmp(before, slots, sizeof(before)) == 0);

    /* ... and the next call starts from nothing */
    CHECK(arena_alloc(&arena, parts, N_PARTS) == 0);
    slots[N_PARTS - 1] = (uint8_t *)typed;
    check_layout(arena, slots, bytes, 0x44);
    CHECK(s_mallocs == 5 && s_frees == 3);

    /* one part that is its own arena (the engine's staging buffers grow so) */
    void *lone = NULL;
    const struct arena_part whole = {&lone, 1000};
    CHECK(arena_alloc(&lone, &whole, 1) == 0 && lone && ((uintptr_t)lone & 255u) == 0 && s_last_size == 1000);
    memset(lone, 0x55, 1000);

    hufs_free(lone);
    hufs_free(arena);
    CHECK(s_frees == 5);
    puts("arena ok");
    return 0;
}
