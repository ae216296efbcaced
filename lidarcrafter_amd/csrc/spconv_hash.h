// The coordinate hash of the sparse kernels (spconv.hip builds it and reads it for the neighbour tables, spvoxel.hip reads
// it for the point <-> voxel maps): key = batch << 54 | x << 36 | y << 18 | z (18 bits each, 9 for the batch: non-negative
// as an int64) in an open-addressing table of 64-bit keys, linear probing (ordered: between a key's home slot and its
// own there are only smaller keys, which fixes the arrangement; a search does not use the order); value = the row.  A
// query with a component below 0 or above LC_SPCONV_MAX_COORD is absent before any key is formed: nothing wraps into a
// neighbouring field of the key, so no cloud sees another cloud's voxel.
#pragma once
#include "common.h"

namespace {

constexpr unsigned long long SP_EMPTY = ~0ull;

__device__ __forceinline__ unsigned long long sp_key(int b, int x, int y, int z) {
    return ((unsigned long long)b << 54) | ((unsigned long long)x << 36) | ((unsigned long long)y << 18) |
           (unsigned long long)z;
}
__device__ __forceinline__ bool sp_in_range(int b, int x, int y, int z) {
    return (unsigned)b <= (unsigned)LC_SPCONV_MAX_BATCH && (unsigned)x <= (unsigned)LC_SPCONV_MAX_COORD &&
           (unsigned)y <= (unsigned)LC_SPCONV_MAX_COORD && (unsigned)z <= (unsigned)LC_SPCONV_MAX_COORD;
}
__device__ __forceinline__ unsigned sp_slot(unsigned long long k, unsigned mask) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (unsigned)k & mask;
}

__device__ __forceinline__ int sp_find(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ vals,
                                       unsigned cap, int b, int x, int y, int z) {
    if (!sp_in_range(b, x, y, z)) return -1;
    const unsigned long long key = sp_key(b, x, y, z);
    const unsigned mask = cap - 1;
    unsigned h = sp_slot(key, mask);
    for (unsigned probe = 0; probe < cap; ++probe, h = (h + 1) & mask) {
        const unsigned long long k = keys[h];
        if (k == key) return vals[h];
        if (k == SP_EMPTY) return -1;
    }
    return -1;
}

// slots of the table of n rows: a power of two, at least 2 n; keys [cap] then values [cap]
inline unsigned sp_capacity(int64_t n) {
    unsigned cap = 1024;
    while ((int64_t)cap < 2 * n) cap <<= 1;
    return cap;
}

}  // namespace
