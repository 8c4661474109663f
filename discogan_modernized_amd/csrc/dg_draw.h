// The counter-based draw generator (internal): the one text behind every record table the library draws on the device -- dg_augment_draw
// (ingest.hip), dg_pool_draw (pool.hip), dg_diffaug_draw / dg_diffaug_draw_p (diffaug.hip) and dg_swd_draw (swd.hip).
//
// A draw is a pure function of its key and a position -- no generator state, so a resumed run continues the same sequence and the
// grouping of a batch into launches does not matter.  Definition (all arithmetic modulo 2^64; mix = the SplitMix64 output function of
// Steele, Lea & Flood 2014, G = 0x9E3779B97F4A7C15):
//   mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
//   key:     k = mix(seed + G);   k = mix(k ^ (uint64(uint32(rank)) << 32 | uint32(domain)));   k = mix(k ^ uint64(iteration))
//            (dg_draw_key; a feature that must stay apart from the others appends a link k = mix(k ^ LINK), LINK a named constant next
//            to its user; dg_swd_draw's chain is seed -> LINK | level alone)
//   words:   q_i = mix(k + G * (m j + i)), i = 1 .. m, for position j of a table that takes m 64-bit words per record; each gives two
//            32-bit words, high half first
//   range:   lo + ((uint64(w) * count) >> 32)            an integer in [lo, lo + count) from a 32-bit word w
//   unit:    float(w >> 8) * 2^-24                       a float in [0, 1) on the 24-bit grid
// What each feature does with its words is defined in include/discogan_hip.h and restated in numpy by tests/*_ref.py.
#pragma once
#include "dg_common.h"

#define DG_DRAW_G 0x9E3779B97F4A7C15ull

__host__ __device__ __forceinline__ uint64_t dg_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
__device__ __forceinline__ int dg_draw_range(uint32_t w, int lo, uint32_t count) { return lo + (int)(((uint64_t)w * count) >> 32); }
__device__ __forceinline__ float dg_draw_unit(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }

static inline uint64_t dg_draw_key(uint64_t seed, int rank, int64_t iteration, int domain) {
    uint64_t k = dg_mix(seed + DG_DRAW_G);
    k = dg_mix(k ^ (((uint64_t)(uint32_t)rank << 32) | (uint64_t)(uint32_t)domain));
    return dg_mix(k ^ (uint64_t)iteration);
}
