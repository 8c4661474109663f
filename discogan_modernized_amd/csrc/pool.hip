// Image history pool of the discriminators (Shrivastava et al. 2017; CycleGAN's ImagePool.query): a buffer of P generated images per domain,
// from which a D-step's fakes are exchanged at random, so that a discriminator trains on a mix of current and earlier fakes.
// include/discogan_hip.h ("image history pool") defines the sequential semantics, the draw and the record table; tests/pool_ref.py restates
// them in numpy together with an independent sequential pool.
//
// Two kernels.  pool_draw_kernel resolves the IN-ORDER semantics of one batch into a record table (src, slot, st_src, 0) per sample;
// pool_exchange_kernel applies a table in one parallel launch: out[j] = (src == -1 ? pool[slot] : x[src]), and where slot >= 0 the same
// thread then writes pool[slot] = x[st_src] at the same element offset.  In a drawn table only the FIRST toucher of a slot carries its
// store, the stored image is the LAST toucher's, and no slot is read by one record and written by another -- so no element of the pool is
// touched by two threads, and the one thread that both reads and writes an element reads first.
// The draws are dg_draw.h's generator: its key with one more link, one word per sample.
#include "dg_draw.h"

#define POOL_LINK 0x706F6F6Cull                  // "pool": the extra link of the key chain that keeps pool draws apart from augmentation draws
#define DG_POOL_MAX_BATCH 4096

// What sample i does: the slot it touches (insert while the pool fills, else swap when the drawn bit is set), or -1 for a pass.
__device__ __forceinline__ int pool_touch(uint64_t key, int i, uint32_t P, int filled, bool* insert) {
    *insert = (long)filled + i < (long)P;
    if (*insert) return filled + i;
    const uint64_t a = dg_mix(key + DG_DRAW_G * ((uint64_t)i + 1ull));
    return (a >> 63) ? dg_draw_range((uint32_t)a, 0, P) : -1;
}

// One thread per sample; every thread re-evaluates the draws of the other samples to find prev(j) = the last earlier toucher of its slot
// and last(j) = the last toucher of its slot from j on: O(n) draws per thread, n <= 4096, no shared state and no second launch.
__global__ __launch_bounds__(256) void pool_draw_kernel(uint64_t key, int n, uint32_t P, int filled, int* __restrict__ recs) {
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        bool insert, ins_i;
        const int s = pool_touch(key, j, P, filled, &insert);
        int4 r;
        r.x = j; r.y = -1; r.z = j; r.w = 0;                            // pass
        if (s >= 0) {
            int prev = -1, last = j;
            for (int i = 0; i < n; ++i) {
                if (i == j || pool_touch(key, i, P, filled, &ins_i) != s) continue;
                if (i < j) prev = i; else last = i;
            }
            if (prev >= 0) {                                            // the slot holds x[prev] by now, and prev's record stores
                r.x = prev;
            } else {                                                    // first toucher: reads the old slot (swap) and carries the store
                r.x = insert ? j : -1;
                r.y = s;
                r.z = last;
            }
        }
        reinterpret_cast<int4*>(recs)[j] = r;                           // one 16-byte store per record
    }
}

extern "C" int dg_pool_draw(uint64_t seed, int rank, int64_t iteration, int domain, int n, int P, int filled, int32_t* recs, dg_stream_t s) {
    DG_CHECK_ARG(recs != nullptr, "dg_pool_draw: null record table");
    DG_CHECK_ARG(((uintptr_t)recs & 15) == 0, "dg_pool_draw: the record table must be 16-byte aligned");
    DG_CHECK_ARG(P >= 1, "dg_pool_draw: a pool has P >= 1 slots, got %d", P);
    DG_CHECK_ARG(filled >= 0 && filled <= P, "dg_pool_draw: filled = %d outside [0, P = %d]", filled, P);
    DG_CHECK_ARG(n >= 1 && n <= DG_POOL_MAX_BATCH, "dg_pool_draw: 1 <= n <= %d samples per batch, got %d", DG_POOL_MAX_BATCH, n);
    DG_CHECK_ARG(rank >= 0 && iteration >= 0 && (domain == 0 || domain == 1), "dg_pool_draw: rank >= 0, iteration >= 0, domain 0 (A) or 1 (B)");
    const uint64_t k = dg_mix(dg_draw_key(seed, rank, iteration, domain) ^ POOL_LINK);
    hipLaunchKernelGGL(pool_draw_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, k, n, (uint32_t)P, filled, recs);
    DG_CHECK_LAUNCH("pool_draw");
    return DG_OK;
}

// One thread per unit of V 32-bit words (V = 4: 16 bytes per lane; V = 1 where a base or the image length is not a multiple of 16 bytes);
// `units` = units per image.  A unit never crosses an image, so consecutive lanes copy consecutive addresses of one image and every access
// of a wave is coalesced.  Values travel as unsigned integers: a copy, whatever the bits mean.
// The record VALUES need no trust: a record with a field out of range -- src outside [-1, n), slot outside [-1, P), st_src outside [0, n),
// or nothing to read (src == -1 without a slot) -- is taken as the pass record (j, -1, j, 0).  Every address formed below is therefore
// inside x (n images), pool (P images) or out (n images).
template <int V>
__global__ __launch_bounds__(256) void pool_exchange_kernel(const unsigned int* __restrict__ x, unsigned int* pool, unsigned int* __restrict__ out,
                                                            int n, int P, long units, const int* __restrict__ recs) {
    typedef unsigned int word_t __attribute__((ext_vector_type(V)));
    const long total = (long)n * units;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long j = i / units, off = (i - j * units) * V, img = units * V;
        int4 r = reinterpret_cast<const int4*>(recs)[j];
        if (r.x < -1 || r.x >= n || r.y < -1 || r.y >= P || r.z < 0 || r.z >= n || (r.x == -1 && r.y == -1)) {
            r.x = (int)j; r.y = -1; r.z = (int)j;
        }
        const unsigned int* from = r.x == -1 ? pool + (long)r.y * img : x + (long)r.x * img;
        const word_t v = *(const word_t*)(from + off);                  // (the read of a slot this thread overwrites below comes first)
        *(word_t*)(out + j * img + off) = v;
        if (r.y >= 0) {
            const word_t w = r.z == r.x ? v : *(const word_t*)(x + (long)r.z * img + off);
            *(word_t*)(pool + (long)r.y * img + off) = w;
        }
    }
}

static inline bool pool_disjoint(const void* a, size_t na, const void* b, size_t nb) {
    return (const char*)a + na <= (const char*)b || (const char*)b + nb <= (const char*)a;
}

extern "C" int dg_pool_exchange(const float* x, float* pool, float* out, int n, int P, size_t elems, const int32_t* recs, dg_stream_t s) {
    DG_CHECK_ARG(x && pool && out, "dg_pool_exchange: null pointer");
    DG_CHECK_ARG(recs != nullptr, "dg_pool_exchange: null record table");
    DG_CHECK_ARG(((uintptr_t)recs & 15) == 0, "dg_pool_exchange: the record table must be 16-byte aligned");
    DG_CHECK_ARG((((uintptr_t)x | (uintptr_t)pool | (uintptr_t)out) & 3) == 0, "dg_pool_exchange: float pointers must be 4-byte aligned");
    DG_CHECK_ARG(P >= 1 && elems >= 1, "dg_pool_exchange: P >= 1 slots of elems >= 1 floats, got P = %d, elems = %zu", P, elems);
    DG_CHECK_ARG(elems <= ((size_t)1 << 40), "dg_pool_exchange: elems = %zu floats per image is out of range", elems);
    DG_CHECK_ARG(n >= 1 && n <= DG_POOL_MAX_BATCH, "dg_pool_exchange: 1 <= n <= %d samples per batch, got %d", DG_POOL_MAX_BATCH, n);
    const size_t batch = (size_t)n * elems * sizeof(float), slots = (size_t)P * elems * sizeof(float);
    DG_CHECK_ARG(pool_disjoint(x, batch, out, batch) && pool_disjoint(x, batch, pool, slots) && pool_disjoint(out, batch, pool, slots),
                 "dg_pool_exchange: x, out and pool overlap (a slot is read and written in one launch)");
    const bool vec = (elems & 3) == 0 && (((uintptr_t)x | (uintptr_t)pool | (uintptr_t)out) & 15) == 0;
    const long units = (long)(vec ? elems / 4 : elems);
    long g = ((long)n * units + 255) / 256;
    if (g > 4096) g = 4096;
    if (vec)
        hipLaunchKernelGGL(pool_exchange_kernel<4>, dim3((int)g), dim3(256), 0, (hipStream_t)s, (const unsigned int*)x, (unsigned int*)pool,
                           (unsigned int*)out, n, P, units, recs);
    else
        hipLaunchKernelGGL(pool_exchange_kernel<1>, dim3((int)g), dim3(256), 0, (hipStream_t)s, (const unsigned int*)x, (unsigned int*)pool,
                           (unsigned int*)out, n, P, units, recs);
    DG_CHECK_LAUNCH("pool_exchange");
    return DG_OK;
}
