#ifndef HUFFMAN_AMD_ARENA_H
#define HUFFMAN_AMD_ARENA_H
/* The one place a plan's device arrays are allocated and cut (engine.c's reservers; on its own here so that a host-only
 * program can check it against stand-ins for the two device calls: tests/emu/arena_check.c). */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../hip/hip_shim.h"

/* A plan's device arrays are cuts of ONE allocation (a new plan paid some twenty-five hipMallocs: 1 .. 15 ms for
 * BASELINE configs[3], where filling it takes 0.5 ms): every array starts at a multiple of 256 bytes. */
static inline size_t arena_cut(size_t *total, size_t bytes) {
    const size_t at = (*total + 255u) & ~(size_t)255u;
    *total = at + bytes;
    return at;
}

/* one array of an arena: where its pointer is kept (the address of a pointer to any object type), and its size */
struct arena_part {
    void *slot;
    size_t bytes;
};
#define ARENA_PARTS(parts) (parts), sizeof(parts) / sizeof((parts)[0])

/* a fresh allocation for the parts, in their order, in place of the one *arena holds (freed first: that waits for what still
 * reads it); every slot then points at its cut.  0, or 2 (hipErrorOutOfMemory) with *arena NULL and the slots as they were */
static inline int arena_alloc(void **arena, const struct arena_part *parts, size_t n) {
    hufs_free(*arena);
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) {
        (void)arena_cut(&total, parts[i].bytes);
    }
    *arena = hufs_malloc(total);
    if (!*arena) {
        return 2;
    }
    total = 0;
    for (size_t i = 0; i < n; ++i) {
        void *at = (uint8_t *)*arena + arena_cut(&total, parts[i].bytes);
        memcpy(parts[i].slot, &at, sizeof(at)); /* (the slots are pointers of many types: written as bytes) */
    }
    return 0;
}

#endif /* HUFFMAN_AMD_ARENA_H */
