// Differentiable augmentation of the discriminators' inputs (Zhao et al., NeurIPS 2020, policy color,translation,cutout), conjugated to
// images in [0, 1].  include/discogan_hip.h ("differentiable augmentation") defines the transform, its adjoint, the draw and the record
// table; tests/diffaug_ref.py restates them in numpy next to the published function.
//
// Three kernels.  diffaug_draw_kernel fills a record table (eight int32 per sample) from a key of dg_draw.h's generator (four words per
// record); its GATED form (dg_diffaug_draw_p: adaptive augmentation, ada.hip) keeps each stage of a sample with probability (float)*p,
// read from device memory, by three gate words from one more link of the key -- one record builder, so a table drawn with p = 1 is
// dg_diffaug_draw's bit for bit.  diffaug_stats_kernel, with
// DG_DIFFAUG_COLOR only, leaves per sample `parts(S)` fp64 partial sums (forward: of x; backward: of the gathered gradient g, summed where
// it comes from) in the workspace: a fixed partition of the sample, a fixed order inside a block, no atomics.  diffaug_apply_kernel
// is the one pass over the data: every block works on ONE sample (blockIdx.y), adds that sample's partials in a fixed tree, and then
// gathers.  Forward and backward are the same gather with the shift negated: out(p) = in(p + d) where p + d is inside the image and the
// cut test -- on p in the forward, on p + d in the backward -- passes, else the fill (0.5 forward, 0 backward).
#include "dg_draw.h"

#define DA_LINK 0x6469666600000000ull             // "diff" in the high word; the role sits in the low one
#define DA_GATE_LINK 0x6164610000000000ull        // "ada": one more link behind it, for the gate words
#define DG_DIFFAUG_MAX_BATCH 4096
#define DG_DIFFAUG_MAX_SIZE 32768                 // 3 S S stays far below 2^63 and a row index below 2^31
#define DA_MAX_PARTS 64                           // one lane of a wave per partial in the apply kernel's tree
#define DA_PART_ELEMS 8192

static inline int da_T(int S) { return (S + 4) / 8; }                     // floor(S / 8 + 0.5)
__host__ __device__ __forceinline__ int da_cs(int S) { return (S + 1) / 2; }   // floor(S / 2 + 0.5)
// The partition of a sample's E = 3 S S values: `parts` chunks of `chunk` values (a multiple of 4), a function of S alone.
static inline int da_parts(int S) {
    const long E = 3l * S * S;
    const long p = (E + DA_PART_ELEMS - 1) / DA_PART_ELEMS;
    return (int)(p > DA_MAX_PARTS ? DA_MAX_PARTS : p);
}
static inline long da_chunk(int S) {
    const long E = 3l * S * S, p = da_parts(S);
    return ((E + p - 1) / p + 3) / 4 * 4;
}

// GATED: stage kept where its gate word's unit float u < p, p = (float)*p_dev (one rounding): p = 1 keeps every stage, p = 0 (or NaN) none
template <bool GATED>
__global__ __launch_bounds__(256) void diffaug_draw_kernel(uint64_t key, uint64_t key2, int n, int S, int T, int flags,
                                                           const double* __restrict__ p_dev, int* __restrict__ recs) {
    const float p = GATED ? (float)*p_dev : 1.0f;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        const uint64_t q1 = dg_mix(key + DG_DRAW_G * (4ull * (uint64_t)j + 1ull)), q2 = dg_mix(key + DG_DRAW_G * (4ull * (uint64_t)j + 2ull));
        const uint64_t q3 = dg_mix(key + DG_DRAW_G * (4ull * (uint64_t)j + 3ull)), q4 = dg_mix(key + DG_DRAW_G * (4ull * (uint64_t)j + 4ull));
        bool keep_color = true, keep_trans = true, keep_cut = true;
        if (GATED) {
            const uint64_t g1 = dg_mix(key2 + DG_DRAW_G * (2ull * (uint64_t)j + 1ull)), g2 = dg_mix(key2 + DG_DRAW_G * (2ull * (uint64_t)j + 2ull));
            keep_color = dg_draw_unit((uint32_t)(g1 >> 32)) < p;
            keep_trans = dg_draw_unit((uint32_t)g1) < p;
            keep_cut = dg_draw_unit((uint32_t)(g2 >> 32)) < p;
        }
        int4 a, b;
        a.x = a.y = a.z = a.w = 0;
        float fb = 0.0f, fs = 1.0f, fc = 1.0f;
        if ((flags & DG_DIFFAUG_COLOR) && keep_color) {
            fb = (dg_draw_unit((uint32_t)(q1 >> 32)) - 0.5f) * 0.5f;
            fs = 2.0f * dg_draw_unit((uint32_t)q1);
            fc = dg_draw_unit((uint32_t)(q2 >> 32)) + 0.5f;
        }
        if ((flags & DG_DIFFAUG_TRANSLATION) && keep_trans) {
            a.x = dg_draw_range((uint32_t)q2, -T, 2u * (uint32_t)T + 1u);
            a.y = dg_draw_range((uint32_t)(q3 >> 32), -T, 2u * (uint32_t)T + 1u);
        }
        if (flags & DG_DIFFAUG_CUTOUT) {
            if (keep_cut) {
                const int cs = da_cs(S);
                const uint32_t count = (uint32_t)S + 1u - (uint32_t)(cs & 1);
                a.z = dg_draw_range((uint32_t)q3, 0, count) - cs / 2;
                a.w = dg_draw_range((uint32_t)(q4 >> 32), 0, count) - cs / 2;
            } else {
                a.z = a.w = S;                                          // the apply kernels still evaluate the stage: an empty square
            }
        }
        b.x = __float_as_int(fb); b.y = __float_as_int(fs); b.z = __float_as_int(fc); b.w = 0;
        reinterpret_cast<int4*>(recs)[2 * j] = a;
        reinterpret_cast<int4*>(recs)[2 * j + 1] = b;
    }
}

// both draw entry points; p: the device probability of the gated form, else NULL
static int da_draw(const char* who, bool gated, uint64_t seed, int rank, int64_t iteration, int domain, int role, int n, int S,
                   int flags, const double* p, int32_t* recs, dg_stream_t s) {
    DG_CHECK_ARG(recs != nullptr, "%s: null record table", who);
    DG_CHECK_ARG(((uintptr_t)recs & 15) == 0, "%s: the record table must be 16-byte aligned", who);
    DG_CHECK_ARG(!gated || p != nullptr, "%s: null probability pointer", who);
    DG_CHECK_ARG(((uintptr_t)p & 7) == 0, "%s: the probability (a device double) must be 8-byte aligned", who);
    DG_CHECK_ARG(n >= 1 && n <= DG_DIFFAUG_MAX_BATCH, "%s: 1 <= n <= %d samples per batch, got %d", who, DG_DIFFAUG_MAX_BATCH, n);
    DG_CHECK_ARG(S >= 2 && S <= DG_DIFFAUG_MAX_SIZE, "%s: 2 <= S <= %d, got %d", who, DG_DIFFAUG_MAX_SIZE, S);
    DG_CHECK_ARG((flags & ~DG_DIFFAUG_ALL) == 0, "%s: unknown policy flags %d", who, flags);
    DG_CHECK_ARG(rank >= 0 && iteration >= 0 && (domain == 0 || domain == 1) && (role == 0 || role == 1),
                 "%s: rank >= 0, iteration >= 0, domain 0 (A) or 1 (B), role 0 (real) or 1 (fake)", who);
    const uint64_t k = dg_mix(dg_draw_key(seed, rank, iteration, domain) ^ (DA_LINK | (uint64_t)(uint32_t)role));
    const dim3 grid((n + 255) / 256);
    if (gated)
        hipLaunchKernelGGL(diffaug_draw_kernel<true>, grid, dim3(256), 0, (hipStream_t)s, k, dg_mix(k ^ DA_GATE_LINK), n, S, da_T(S), flags, p, recs);
    else
        hipLaunchKernelGGL(diffaug_draw_kernel<false>, grid, dim3(256), 0, (hipStream_t)s, k, (uint64_t)0, n, S, da_T(S), flags, p, recs);
    DG_CHECK_LAUNCH(who + 3);                                           // the kernel's name: who without "dg_"
    return DG_OK;
}

extern "C" int dg_diffaug_draw(uint64_t seed, int rank, int64_t iteration, int domain, int role, int n, int S, int flags, int32_t* recs,
                               dg_stream_t s) {
    return da_draw("dg_diffaug_draw", false, seed, rank, iteration, domain, role, n, S, flags, nullptr, recs, s);
}
extern "C" int dg_diffaug_draw_p(uint64_t seed, int rank, int64_t iteration, int domain, int role, int n, int S, int flags, const double* p,
                                 int32_t* recs, dg_stream_t s) {
    return da_draw("dg_diffaug_draw_p", true, seed, rank, iteration, domain, role, n, S, flags, p, recs, s);
}

// What the kernels keep of one record: the shift of the gather (64-bit: any int32 is safe), the cut square, the factors.
struct DaRec {
    long dx, dy;                // in(p + d): (tx, ty) forward, (-tx, -ty) backward
    long cx0, cy0, cx1, cy1;    // the cut square [cy0, cy1) x [cx0, cx1); empty without DG_DIFFAUG_CUTOUT
    float b, s, c;
};
template <bool BWD>
__device__ __forceinline__ DaRec da_load(const int* __restrict__ recs, long j, int S, int flags) {
    const int4 a = reinterpret_cast<const int4*>(recs)[2 * j], f = reinterpret_cast<const int4*>(recs)[2 * j + 1];
    DaRec r;
    r.dx = r.dy = 0;
    if (flags & DG_DIFFAUG_TRANSLATION) {
        r.dx = BWD ? -(long)a.x : (long)a.x;
        r.dy = BWD ? -(long)a.y : (long)a.y;
    }
    r.cx0 = r.cy0 = r.cx1 = r.cy1 = 0;
    if (flags & DG_DIFFAUG_CUTOUT) {
        r.cx0 = a.z; r.cy0 = a.w;
        r.cx1 = (long)a.z + da_cs(S); r.cy1 = (long)a.w + da_cs(S);
    }
    r.b = __int_as_float(f.x); r.s = __int_as_float(f.y); r.c = __int_as_float(f.z);
    return r;
}

struct DaStatArgs {
    DgPtrs in, ws, recs;
    int n, S, flags, parts;
    long chunk;
};

// grid (parts, groups * n), 256 threads.  A thread takes the 4-value units t, t + 256, ... of its chunk, adds each as (e0 + e1) + (e2 + e3)
// in fp64 (V = 4: one 16-byte load; V = 1: four 4-byte loads, values past the sample count as 0), so the sum does not depend on V.
// BWD: the value at p counts where the forward wrote it from the image (p not cut, p + t inside) -- the sum of g over its sources.
template <int V, bool BWD>
__global__ __launch_bounds__(256) void diffaug_stats_kernel(const DaStatArgs A) {
    __shared__ double red[4];
    const int grp = blockIdx.y / A.n;
    const long j = blockIdx.y - grp * A.n;
    const int S = A.S;
    const long E = 3l * S * S, plane = (long)S * S;
    const float* __restrict__ in = dg_pick<const float>(A.in, grp) + j * E;
    DaRec r;
    if (BWD) r = da_load<false>(dg_pick<const int>(A.recs, grp), j, S, A.flags);
    const long e_begin = blockIdx.x * A.chunk, e_stop = min(E, e_begin + A.chunk);
    double acc = 0.0;
    for (long e = e_begin + 4l * threadIdx.x; e < e_stop; e += 1024) {
        float v[4];
        if (V == 4) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(in + e);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = e + i < E ? in[e + i] : 0.0f;
        }
        if (BWD) {                                                      // (E <= 3 * 2^30: 32-bit index arithmetic)
            uint32_t rem = (uint32_t)e % (uint32_t)plane, y = rem / (uint32_t)S, x = rem - y * (uint32_t)S;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (V == 1 && i > 0) {                                  // (V = 4: S % 4 == 0, a unit stays inside one row)
                    rem = (uint32_t)(e + i) % (uint32_t)plane; y = rem / (uint32_t)S; x = rem - y * (uint32_t)S;
                } else if (i > 0) {
                    ++x;
                }
                const bool cut = (long)y >= r.cy0 && (long)y < r.cy1 && (long)x >= r.cx0 && (long)x < r.cx1;
                const long sy = (long)y + r.dy, sx = (long)x + r.dx;
                if (cut || sy < 0 || sy >= S || sx < 0 || sx >= S) v[i] = 0.0f;
            }
        }
        acc += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
    }
    dg_block_stage_d(acc, red);
    if (threadIdx.x == 0) dg_pick<double>(A.ws, grp)[j * A.parts + blockIdx.x] = dg_sum4_pair(red);
}

struct DaApplyArgs {
    DgPtrs in, out, ws, recs;
    int n, S, flags, parts;
    long units;                 // V-pixel units per channel plane: S * ceil(S / V) (V = 4 only where S % 4 == 0)
};

// grid (blocks per sample, groups * n), 256 threads; a thread produces V pixels of one row in all three channels (colour mixes them).
// Without COLOR the values travel as unsigned integers: a copy, whatever the bits mean.
template <int V, bool BWD, bool COLOR>
__global__ __launch_bounds__(256) void diffaug_apply_kernel(const DaApplyArgs A) {
    typedef unsigned int word_t __attribute__((ext_vector_type(V)));
    __shared__ double mean_sh;
    const int grp = blockIdx.y / A.n;
    const long j = blockIdx.y - grp * A.n;
    const int S = A.S;
    const long plane = (long)S * S, E = 3 * plane;
    const unsigned int* __restrict__ in = dg_pick<const unsigned int>(A.in, grp) + j * E;
    unsigned int* __restrict__ out = dg_pick<unsigned int>(A.out, grp) + j * E;
    const DaRec r = da_load<BWD>(dg_pick<const int>(A.recs, grp), j, S, A.flags);
    const unsigned int fill = BWD ? 0u : 0x3F000000u;                   // 0.0f | 0.5f
    float m2 = 0.0f, k_g = 0.0f, k_m = 0.0f;
    if (COLOR) {
        // the sample's partial sums, one per lane of the first wave, added in the fixed tree of dg_wave_sum_d
        if (threadIdx.x < 64) {
            const double* p = dg_pick<const double>(A.ws, grp) + j * A.parts;
            double v = (int)threadIdx.x < A.parts ? p[threadIdx.x] : 0.0;
            v = dg_wave_sum_d(v);
            if (threadIdx.x == 0) mean_sh = v / (double)E;
        }
        __syncthreads();
        if (BWD) {
            m2 = (1.0f - r.c) * (float)mean_sh;                         // (1 - c) G
            k_g = r.s * r.c;
            k_m = (1.0f - r.s) * r.c;
        } else {
            m2 = (float)(mean_sh + (double)r.b);                        // mean of x + b = mean of the saturated image
        }
    }
    const int row_units = (S + V - 1) / V;
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < A.units; u += (long)gridDim.x * 256) {
        const long y = (uint32_t)u / (uint32_t)row_units, x0 = (u - y * row_units) * V;    // (units <= 2^30)
        const long sy = y + r.dy, sx0 = x0 + r.dx;
        const long cy = BWD ? sy : y, cxb = BWD ? sx0 : x0;             // where the cut test looks
        const bool row_ok = sy >= 0 && sy < S && !(cy >= r.cy0 && cy < r.cy1 && cxb >= r.cx0 && cxb + V <= r.cx1);
        unsigned int w[3][V];
        bool ok[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const long sx = sx0 + i, cx = cxb + i;
            ok[i] = row_ok && sx >= 0 && sx < S && !(cy >= r.cy0 && cy < r.cy1 && cx >= r.cx0 && cx < r.cx1);
        }
        if (V == 4 && row_ok && (r.dx & 3) == 0 && sx0 >= 0 && sx0 < S) {   // the shifted unit is a whole aligned unit of the source row
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const word_t q = *reinterpret_cast<const word_t*>(in + ch * plane + sy * S + sx0);
#pragma unroll
                for (int i = 0; i < V; ++i) w[ch][i] = q[i];
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int i = 0; i < V; ++i) w[ch][i] = ok[i] ? in[ch * plane + sy * S + sx0 + i] : fill;
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
            if (!ok[i]) w[0][i] = w[1][i] = w[2][i] = fill;
            if (COLOR && (BWD || ok[i])) {                              // (backward: g = 0 there, and dx = (1 - c) G, or NaN by a NaN factor)
                float v0 = __uint_as_float(w[0][i]), v1 = __uint_as_float(w[1][i]), v2 = __uint_as_float(w[2][i]);
                if (BWD) {                                              // s c g + (1 - s) c chanmean(g) + (1 - c) G
                    const float t = fmaf(k_m, (v0 + v1 + v2) / 3.0f, m2);
                    v0 = fmaf(k_g, v0, t); v1 = fmaf(k_g, v1, t); v2 = fmaf(k_g, v2, t);
                } else {
                    v0 += r.b; v1 += r.b; v2 += r.b;
                    const float m1 = (v0 + v1 + v2) / 3.0f;
                    v0 = fmaf(v0 - m1, r.s, m1); v1 = fmaf(v1 - m1, r.s, m1); v2 = fmaf(v2 - m1, r.s, m1);
                    v0 = fmaf(v0 - m2, r.c, m2); v1 = fmaf(v1 - m2, r.c, m2); v2 = fmaf(v2 - m2, r.c, m2);
                }
                w[0][i] = __float_as_uint(v0); w[1][i] = __float_as_uint(v1); w[2][i] = __float_as_uint(v2);
            }
        }
        if (V == 4) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                word_t q;
#pragma unroll
                for (int i = 0; i < V; ++i) q[i] = w[ch][i];
                *reinterpret_cast<word_t*>(out + ch * plane + y * S + x0) = q;
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out[ch * plane + y * S + x0] = w[ch][0];
        }
    }
}

extern "C" size_t dg_diffaug_workspace_bytes(int n, int S, int flags) {
    if (!(flags & DG_DIFFAUG_COLOR) || n < 1 || S < 2 || S > DG_DIFFAUG_MAX_SIZE) return 0;
    return (size_t)n * da_parts(S) * sizeof(double);
}

static inline bool da_disjoint(const void* a, const void* b, size_t nb) {
    return (const char*)a + nb <= (const char*)b || (const char*)b + nb <= (const char*)a;
}

template <bool BWD>
static int da_run(const char* who, int groups, const float* const* in, float* const* out, int n, int S, int flags, const int32_t* const* recs,
                  void* const* ws, size_t ws_bytes, hipStream_t st) {
    DG_CHECK_ARG(groups >= 1 && groups <= DG_MAX_GROUPS, "%s: 1 <= groups <= %d, got %d", who, DG_MAX_GROUPS, groups);
    DG_CHECK_ARG(in && out && recs, "%s: null pointer table", who);
    DG_CHECK_ARG(n >= 1 && n <= DG_DIFFAUG_MAX_BATCH, "%s: 1 <= n <= %d samples per batch, got %d", who, DG_DIFFAUG_MAX_BATCH, n);
    DG_CHECK_ARG(S >= 2 && S <= DG_DIFFAUG_MAX_SIZE, "%s: 2 <= S <= %d, got %d", who, DG_DIFFAUG_MAX_SIZE, S);
    DG_CHECK_ARG((flags & ~DG_DIFFAUG_ALL) == 0, "%s: unknown policy flags %d", who, flags);
    const bool color = (flags & DG_DIFFAUG_COLOR) != 0;
    const size_t bytes = (size_t)n * 3 * S * S * sizeof(float), need = dg_diffaug_workspace_bytes(n, S, flags);
    DG_CHECK_ARG(!color || (ws != nullptr && ws_bytes >= need), "%s: DG_DIFFAUG_COLOR needs a workspace of %zu bytes per problem, got %zu", who, need,
                 ws_bytes);
    uintptr_t low = 0;
    for (int g = 0; g < groups; ++g) {
        DG_CHECK_ARG(in[g] && out[g] && recs[g], "%s: null pointer (problem %d)", who, g);
        DG_CHECK_ARG(((uintptr_t)recs[g] & 15) == 0, "%s: the record table must be 16-byte aligned (problem %d)", who, g);
        DG_CHECK_ARG((((uintptr_t)in[g] | (uintptr_t)out[g]) & 3) == 0, "%s: float pointers must be 4-byte aligned (problem %d)", who, g);
        DG_CHECK_ARG(!color || (ws[g] != nullptr && ((uintptr_t)ws[g] & 7) == 0), "%s: the workspace must be 8-byte aligned (problem %d)", who, g);
        for (int h = 0; h < groups; ++h)        // no output may overlap any input of the launch (or, but for itself, any output)
            DG_CHECK_ARG(da_disjoint(out[g], in[h], bytes) && (h == g || da_disjoint(out[g], out[h], bytes)),
                         "%s: input and output overlap (problems %d and %d)", who, g, h);
        low |= (uintptr_t)in[g] | (uintptr_t)out[g];
    }
    const bool vec = (S & 3) == 0 && (low & 15) == 0;
    if (color) {
        DaStatArgs a;
        a.in = dg_ptrs((const void* const*)in, groups); a.ws = dg_ptrs((const void* const*)ws, groups);
        a.recs = dg_ptrs((const void* const*)recs, groups);
        a.n = n; a.S = S; a.flags = flags; a.parts = da_parts(S); a.chunk = da_chunk(S);
        const dim3 grid(a.parts, groups * n);
        if (vec) hipLaunchKernelGGL((diffaug_stats_kernel<4, BWD>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((diffaug_stats_kernel<1, BWD>), grid, dim3(256), 0, st, a);
        DG_CHECK_LAUNCH(who);
    }
    DaApplyArgs a;
    a.in = dg_ptrs((const void* const*)in, groups); a.out = dg_ptrs((const void* const*)out, groups);
    a.ws = dg_ptrs((const void* const*)ws, color ? groups : 0); a.recs = dg_ptrs((const void* const*)recs, groups);
    a.n = n; a.S = S; a.flags = flags; a.parts = da_parts(S);
    a.units = vec ? (long)S * (S / 4) : (long)S * S;
    long gx = (a.units + 255) / 256, cap = 4096 / ((long)groups * n);
    if (cap < 1) cap = 1;
    if (gx > cap) gx = cap;
    const dim3 grid((unsigned)gx, groups * n);
    if (vec && color) hipLaunchKernelGGL((diffaug_apply_kernel<4, BWD, true>), grid, dim3(256), 0, st, a);
    else if (vec) hipLaunchKernelGGL((diffaug_apply_kernel<4, BWD, false>), grid, dim3(256), 0, st, a);
    else if (color) hipLaunchKernelGGL((diffaug_apply_kernel<1, BWD, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((diffaug_apply_kernel<1, BWD, false>), grid, dim3(256), 0, st, a);
    DG_CHECK_LAUNCH(who);
    return DG_OK;
}

extern "C" int dg_diffaug_fwd(const float* x, float* z, int n, int S, int flags, const int32_t* recs, void* ws, size_t ws_bytes, dg_stream_t s) {
    return da_run<false>("dg_diffaug_fwd", 1, &x, &z, n, S, flags, &recs, &ws, ws_bytes, (hipStream_t)s);
}
extern "C" int dg_diffaug_bwd(const float* dz, float* dx, int n, int S, int flags, const int32_t* recs, void* ws, size_t ws_bytes, dg_stream_t s) {
    return da_run<true>("dg_diffaug_bwd", 1, &dz, &dx, n, S, flags, &recs, &ws, ws_bytes, (hipStream_t)s);
}
extern "C" int dg_diffaug_fwd_g(int groups, const float* const* x, float* const* z, int n, int S, int flags, const int32_t* const* recs,
                                void* const* ws, size_t ws_bytes, dg_stream_t s) {
    return da_run<false>("dg_diffaug_fwd_g", groups, x, z, n, S, flags, recs, ws, ws_bytes, (hipStream_t)s);
}
extern "C" int dg_diffaug_bwd_g(int groups, const float* const* dz, float* const* dx, int n, int S, int flags, const int32_t* const* recs,
                                void* const* ws, size_t ws_bytes, dg_stream_t s) {
    return da_run<true>("dg_diffaug_bwd_g", groups, dz, dx, n, S, flags, recs, ws, ws_bytes, (hipStream_t)s);
}
