// Sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al., ICLR 2018, section 5): the unpaired score of evaluate.py.
// include/discogan_hip.h ("sliced Wasserstein distance") defines levels, pyramid, draw, descriptors, normalisation and distance; this
// file is the six stages, each a C-ABI entry of its own so that each can be tested against float64 at its boundary.
//
//   dg_lap_pyramid       2 (L - 1) launches and no workspace.  G_{l+1} = down(G_l) is written straight into level l + 1's slot of `out`;
//                        then level l's slot becomes G_l - up(G_{l+1}) (level 0 reads x, the others rewrite their own slot element by
//                        element: a thread reads only the element it writes there).  With L = 1 the one level is a bit copy of x.
//                        A thread produces four neighbouring outputs of a row and moves them as 16 bytes when the output row length is a
//                        multiple of 4 and the bases are 16-byte aligned, else one output; both forms evaluate the same chain of explicit
//                        fmaf per element (nothing is left to the compiler's contraction, which differed between the two forms), so the
//                        bits do not depend on alignment.  Filter taps are read as scalars (they hit L2).
//   dg_swd_draw          one thread per record, one word of dg_draw.h's generator each.
//   dg_swd_descriptors   block b owns descriptors [32 b, 32 b + 32): NB = ceil(M / 32) blocks, a function of M alone.  Pass 1 gathers
//                        (a bit copy) and leaves three fp64 sums per block; pass 2 re-reads the block's descriptors and leaves the sums
//                        of (v - mean)^2 (two passes: no cancellation, a flat channel gives a variance of exactly 0); a one-block kernel
//                        writes mean and population standard deviation.  Every block adds the NB partials in the same fixed order
//                        (thread t: t, t + 256, ...; wave; four waves), fp64 throughout, no atomics.
//   dg_swd_project       64 descriptors x 64 directions per 256-thread block, 4 x 4 per thread, K = 147 in three chunks of 49 = one
//                        channel each.  xhat = fp32(((double)v - mean) / std), 0 for a flat channel, is formed while the tile is staged;
//                        the products are one fp32 fma chain in ascending k.  No bf16, no MFMA: 5 GFLOP per level and set.
//   dg_swd_sort_rows / dg_swd_row_distance
//                        one 1024-thread workgroup per row; the row lives in dynamic LDS as N = 2^ceil(log2 M) 32-bit keys, up to
//                        DG_SWD_MAX_ROW * 4 bytes = 128 KiB of the CU's 160 KiB (the limit is raised per kernel with
//                        hipFuncSetAttribute, as edge.hip does for its 96 KiB kernel; a launch asks for N * 4 bytes only).  A key is the
//                        float's bits made monotone (negative: all bits flipped, else the sign bit set), so the order is total:
//                        -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN.  Padding keys are 0xFFFFFFFF, which sort behind everything, so the
//                        first M keys are always the row itself.  Plain bitonic network, one barrier per pass; bank conflicts of the wide
//                        strides are left alone.  The distance kernel then sums |a_(i) - ref_(i)|: thread t takes i = t, t + 1024, ... in
//                        fp32, fp64 from the wave sum on, the 16 wave sums in index order, divided by M.  A NaN (or inf - inf) stays in
//                        its row's sum.  |a - b| = |b - a| and the partition depends on M only: exchanging the sets gives the same bits.
//
// fp32 rounding chains (the k of the tests' gamma(k) bounds):
//   SWD_K_DOWN = 10   one down(): per axis five fma, at most one rounding each; two axes
//   SWD_K_UP   = 10   one up(): at most three non-zero taps per axis; counted like down()
//   level l < L - 1:  G_l carries l SWD_K_DOWN, up(G_{l+1}) carries (l + 1) SWD_K_DOWN + SWD_K_UP, the subtraction one more:
//                     |err| <= gamma((l + 1) SWD_K_DOWN + SWD_K_UP + 1) (mag(G_l) + up(mag(G_{l+1}))), mag = the same chain on |x|
//   projection:       147 fma + the rounding of xhat + the fp64 statistics: gamma(147 + 3) sum_k |xhat_k| |dir_k|
//   distance:         ceil(M / 1024) terms per thread, one rounding for the difference, fp64 after that: gamma(ceil(M / 1024) + 2)
#include "dg_draw.h"

#define SWD_PATCH 7
#define SWD_DESC 147               // 3 x 7 x 7, [channel][dy][dx]
#define SWD_CH 49                  // values of one channel in a descriptor
#define SWD_PYR_MAX_BLOCKS 16384
#define SWD_DESC_PER_BLOCK 32
#define SWD_SORT_THREADS 1024
#define SWD_LINK 0x7377640000000000ull             // "swd" in the high word; the level sits in the low one

static int swd_levels(int S) {
    if (S < 16) return 0;
    int L = 1;
    while (S % 2 == 0 && S / 2 >= 16) {
        S /= 2;
        ++L;
    }
    return L;
}

extern "C" int dg_swd_max_row(void) { return DG_SWD_MAX_ROW; }
extern "C" int dg_swd_levels(int S) { return swd_levels(S); }

extern "C" size_t dg_lap_pyramid_elems(int n, int S) {
    const int L = swd_levels(S);
    if (n < 1 || L < 1) return 0;
    size_t e = 0;
    for (int l = 0, R = S; l < L; ++l, R /= 2) e += (size_t)n * 3 * (size_t)R * (size_t)R;
    return e;
}

// ---- pyramid -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int swd_mirror(int i, int R) {        // -1 -> 1, R -> R - 2 (no edge repeat); R >= 3 and -2 <= i <= R + 1
    i = i < 0 ? -i : i;
    return i >= R ? 2 * R - 2 - i : i;
}

// one pixel of down(a): the 5 x 5 filter centred on (2 yo, 2 xo) of the R x R plane `a`
__device__ __forceinline__ float swd_down_at(const float* __restrict__ a, int R, int yo, int xo) {
    const float w[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    int xs[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) xs[j] = swd_mirror(2 * xo + j - 2, R);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const float* row = a + (long)swd_mirror(2 * yo + i - 2, R) * R;
        float r = 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j) r = fmaf(w[j], row[xs[j]], r);
        acc = fmaf(w[i], r, acc);
    }
    return acc;
}

// one pixel of up(c): c (Rc x Rc) at the even positions of a zero image of side R = 2 Rc, filtered with 4 w (x) w under the mirror rule
__device__ __forceinline__ float swd_up_at(const float* __restrict__ c, int Rc, int y, int x) {
    const float w[5] = {0.125f, 0.5f, 0.75f, 0.5f, 0.125f};
    const int R = 2 * Rc;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int yy = swd_mirror(y + i - 2, R);
        if (yy & 1) continue;
        const float* row = c + (long)(yy >> 1) * Rc;
        float r = 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int xx = swd_mirror(x + j - 2, R);
            if (xx & 1) continue;
            r = fmaf(w[j], row[xx >> 1], r);
        }
        acc = fmaf(w[i], r, acc);
    }
    return acc;
}

// dst [planes][Ro][Ro] = down(src [planes][R][R]), Ro = R / 2; V outputs of one row per thread (V = 4: Ro % 4 == 0, dst 16-byte aligned)
template <int V>
__global__ __launch_bounds__(256) void swd_down_kernel(const float* __restrict__ src, float* __restrict__ dst, long planes, int R) {
    const int Ro = R / 2, Q = Ro / V;
    const long items = planes * Ro * Q;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
        const int q = (int)(it % Q);
        const long t = it / Q;
        const int yo = (int)(t % Ro);
        const long pl = t / Ro;
        const float* a = src + pl * R * R;
        float v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = swd_down_at(a, R, yo, q * V + j);
        float* o = dst + (pl * Ro + yo) * Ro + q * V;
        if (V == 4) {
            const f32x4 p = {v[0], v[1], v[2], v[3]};
            *(f32x4*)o = p;
        } else {
            o[0] = v[0];
        }
    }
}

// out [planes][R][R] = g - up(c [planes][R / 2][R / 2]); out may be g itself (a thread reads of g only what it writes)
template <int V>
__global__ __launch_bounds__(256) void swd_lap_kernel(const float* g, const float* __restrict__ c, float* out, long planes, int R) {
    const int Rc = R / 2, Q = R / V;
    const long items = planes * R * Q;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < items; it += (long)gridDim.x * 256) {
        const int q = (int)(it % Q);
        const long t = it / Q;
        const int y = (int)(t % R);
        const long pl = t / R;
        const float* cp = c + pl * Rc * Rc;
        const long o = (pl * R + y) * R + q * V;
        if (V == 4) {
            const f32x4 a = *(const f32x4*)(g + o);
            f32x4 p;
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = a[j] - swd_up_at(cp, Rc, y, q * 4 + j);
            *(f32x4*)(out + o) = p;
        } else {
            out[o] = g[o] - swd_up_at(cp, Rc, y, q);
        }
    }
}

static unsigned swd_grid(long items) {
    const long b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b < SWD_PYR_MAX_BLOCKS ? b : SWD_PYR_MAX_BLOCKS));
}

extern "C" int dg_lap_pyramid(const float* x, int n, int S, float* out, dg_stream_t s) {
    DG_CHECK_ARG(x != nullptr && out != nullptr, "dg_lap_pyramid: null pointer");
    DG_CHECK_ARG(n >= 1, "dg_lap_pyramid: n %d < 1", n);
    DG_CHECK_ARG(S >= 16 && S <= 16384, "dg_lap_pyramid: 16 <= S <= 16384, got %d", S);
    DG_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)out & 3) == 0, "dg_lap_pyramid: batches must be 4-byte aligned");
    const int L = swd_levels(S);
    const long planes = (long)n * 3;
    hipStream_t st = (hipStream_t)s;
    if (L == 1) {
        if (hipMemcpyAsync(out, x, (size_t)planes * S * S * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
            return dg_fail(DG_ERR_HIP, "dg_lap_pyramid: copy failed");
        return DG_OK;
    }
    // G_{l+1} into slot l + 1, then slot l = G_l - up(G_{l+1})
    const float* g = x;             // G_l
    float* slot = out;              // level l's slot
    int R = S;
    for (int l = 0; l + 1 < L; ++l) {
        float* next = slot + planes * R * R;
        const int Ro = R / 2;
        if (Ro % 4 == 0 && ((uintptr_t)next & 15) == 0)
            hipLaunchKernelGGL(swd_down_kernel<4>, dim3(swd_grid(planes * Ro * (Ro / 4))), dim3(256), 0, st, g, next, planes, R);
        else
            hipLaunchKernelGGL(swd_down_kernel<1>, dim3(swd_grid(planes * Ro * Ro)), dim3(256), 0, st, g, next, planes, R);
        DG_CHECK_LAUNCH("swd_down");
        if (R % 4 == 0 && (((uintptr_t)g | (uintptr_t)slot) & 15) == 0)
            hipLaunchKernelGGL(swd_lap_kernel<4>, dim3(swd_grid(planes * R * (R / 4))), dim3(256), 0, st, g, (const float*)next, slot, planes, R);
        else
            hipLaunchKernelGGL(swd_lap_kernel<1>, dim3(swd_grid(planes * R * R)), dim3(256), 0, st, g, (const float*)next, slot, planes, R);
        DG_CHECK_LAUNCH("swd_lap");
        g = next;
        slot = next;
        R = Ro;
    }
    return DG_OK;
}

// ---- draw --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swd_draw_kernel(uint64_t key, long count, int span, int* __restrict__ recs) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) {
        const uint64_t q = dg_mix(key + DG_DRAW_G * ((uint64_t)i + 1ull));
        recs[2 * i] = dg_draw_range((uint32_t)(q >> 32), 0, (uint32_t)span);
        recs[2 * i + 1] = dg_draw_range((uint32_t)q, 0, (uint32_t)span);
    }
}

extern "C" int dg_swd_draw(uint64_t seed, int level, int n, int R, int P, int32_t* recs, dg_stream_t s) {
    DG_CHECK_ARG(recs != nullptr, "dg_swd_draw: null record table");
    DG_CHECK_ARG(((uintptr_t)recs & 7) == 0, "dg_swd_draw: the record table must be 8-byte aligned");
    DG_CHECK_ARG(level >= 0 && level < 64, "dg_swd_draw: 0 <= level < 64, got %d", level);
    DG_CHECK_ARG(n >= 1 && P >= 1 && (long)n * P <= DG_SWD_MAX_ROW, "dg_swd_draw: n, P >= 1 and n P <= %d, got n=%d P=%d", DG_SWD_MAX_ROW, n, P);
    DG_CHECK_ARG(R >= SWD_PATCH && R <= 16384, "dg_swd_draw: %d <= R <= 16384, got %d", SWD_PATCH, R);
    const uint64_t k = dg_mix(dg_mix(seed + DG_DRAW_G) ^ (SWD_LINK | (uint64_t)(uint32_t)level));
    const long count = (long)n * P;
    hipLaunchKernelGGL(swd_draw_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)s, k, count, R - (SWD_PATCH - 1), recs);
    DG_CHECK_LAUNCH("swd_draw");
    return DG_OK;
}

// ---- descriptors and their statistics -----------------------------------------------------------------------------------------------------
static int swd_stat_blocks(long M) { return (int)((M + SWD_DESC_PER_BLOCK - 1) / SWD_DESC_PER_BLOCK); }

extern "C" size_t dg_swd_descriptors_workspace_bytes(int M) {
    if (M < 1 || M > DG_SWD_MAX_ROW) return 0;
    return (size_t)6 * (size_t)swd_stat_blocks(M) * sizeof(double);
}

// three block sums (one per channel) in fixed order; the results are valid in every thread.  red: 3 x 4 doubles of LDS
__device__ __forceinline__ void swd_block_sum3(double (&a)[3], double (*red)[4]) {
    dg_block_stage_d(a, red);
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = dg_sum4_pair(red[c]);
}

// the sum of the nb block partials part[c][0..nb) of every channel, the same bits in every block
__device__ __forceinline__ void swd_sum_parts(const double* __restrict__ part, int nb, double (&a)[3], double (*red)[4]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double v = 0.0;
        for (int i = threadIdx.x; i < nb; i += 256) v += part[(long)c * nb + i];
        a[c] = v;
    }
    swd_block_sum3(a, red);
}

__global__ __launch_bounds__(256) void swd_gather_kernel(const float* __restrict__ lev, int R, int P, long M, const int* __restrict__ recs,
                                                         float* __restrict__ desc, double* __restrict__ part) {
    __shared__ double red[3][4];
    const long e0 = (long)blockIdx.x * SWD_DESC_PER_BLOCK * SWD_DESC;
    const long e1 = min(M * SWD_DESC, e0 + (long)SWD_DESC_PER_BLOCK * SWD_DESC);
    const long plane = (long)R * R;
    double a[3] = {0.0, 0.0, 0.0};
    for (long e = e0 + threadIdx.x; e < e1; e += 256) {
        const long i = e / SWD_DESC;
        const int r = (int)(e - i * SWD_DESC);
        const int c = r / SWD_CH, rr = r - c * SWD_CH, dy = rr / SWD_PATCH, dx = rr - dy * SWD_PATCH;
        const int oy = min(max(recs[2 * i], 0), R - SWD_PATCH), ox = min(max(recs[2 * i + 1], 0), R - SWD_PATCH);
        const float v = lev[((i / P) * 3 + c) * plane + (long)(oy + dy) * R + (ox + dx)];
        desc[e] = v;
        a[0] += c == 0 ? (double)v : 0.0;           // c is a runtime value: selects, not an indexed register array
        a[1] += c == 1 ? (double)v : 0.0;
        a[2] += c == 2 ? (double)v : 0.0;
    }
    swd_block_sum3(a, red);
    if (threadIdx.x < 3) part[(long)threadIdx.x * gridDim.x + blockIdx.x] = a[threadIdx.x];
}

__global__ __launch_bounds__(256) void swd_var_kernel(const float* __restrict__ desc, long M, const double* __restrict__ part1,
                                                      double* __restrict__ part2) {
    __shared__ double red[3][4];
    double mean[3];
    swd_sum_parts(part1, (int)gridDim.x, mean, red);
    const double count = (double)M * SWD_CH;       // a division, not a reciprocal: N copies of one fp32 value sum exactly and give it back
#pragma unroll
    for (int c = 0; c < 3; ++c) mean[c] /= count;
    const long e0 = (long)blockIdx.x * SWD_DESC_PER_BLOCK * SWD_DESC;
    const long e1 = min(M * SWD_DESC, e0 + (long)SWD_DESC_PER_BLOCK * SWD_DESC);
    double a[3] = {0.0, 0.0, 0.0};
    for (long e = e0 + threadIdx.x; e < e1; e += 256) {
        const int c = (int)(e % SWD_DESC) / SWD_CH;
        const double d = (double)desc[e] - (c == 0 ? mean[0] : c == 1 ? mean[1] : mean[2]);
        a[0] += c == 0 ? d * d : 0.0;
        a[1] += c == 1 ? d * d : 0.0;
        a[2] += c == 2 ? d * d : 0.0;
    }
    swd_block_sum3(a, red);
    if (threadIdx.x < 3) part2[(long)threadIdx.x * gridDim.x + blockIdx.x] = a[threadIdx.x];
}

__global__ __launch_bounds__(256) void swd_stats_kernel(long M, int nb, const double* __restrict__ part1, const double* __restrict__ part2,
                                                        double* __restrict__ stats) {
    __shared__ double red[3][4];
    double mean[3], var[3];
    swd_sum_parts(part1, nb, mean, red);
    swd_sum_parts(part2, nb, var, red);
    const double count = (double)M * SWD_CH;
    if (threadIdx.x < 3) {
        stats[2 * threadIdx.x] = mean[threadIdx.x] / count;
        stats[2 * threadIdx.x + 1] = sqrt(var[threadIdx.x] / count);
    }
}

extern "C" int dg_swd_descriptors(const float* level, int n, int R, int P, const int32_t* recs, float* desc, double* stats, void* ws,
                                  size_t ws_bytes, dg_stream_t s) {
    DG_CHECK_ARG(level != nullptr && recs != nullptr && desc != nullptr && stats != nullptr, "dg_swd_descriptors: null pointer");
    DG_CHECK_ARG(n >= 1 && P >= 1 && (long)n * P <= DG_SWD_MAX_ROW, "dg_swd_descriptors: n, P >= 1 and n P <= %d, got n=%d P=%d", DG_SWD_MAX_ROW,
                 n, P);
    DG_CHECK_ARG(R >= SWD_PATCH && R <= 16384, "dg_swd_descriptors: %d <= R <= 16384, got %d", SWD_PATCH, R);
    DG_CHECK_ARG(((uintptr_t)level & 3) == 0 && ((uintptr_t)desc & 3) == 0 && ((uintptr_t)recs & 3) == 0,
                 "dg_swd_descriptors: level, records and descriptors must be 4-byte aligned");
    DG_CHECK_ARG(((uintptr_t)stats & 7) == 0, "dg_swd_descriptors: stats must be 8-byte aligned");
    const int M = n * P;
    if (ws == nullptr || ws_bytes < dg_swd_descriptors_workspace_bytes(M))
        return dg_fail(DG_ERR_WORKSPACE, "dg_swd_descriptors: workspace too small (%zu bytes, %zu needed)", ws_bytes,
                       dg_swd_descriptors_workspace_bytes(M));
    DG_CHECK_ARG(((uintptr_t)ws & 7) == 0, "dg_swd_descriptors: the workspace must be 8-byte aligned");
    const int nb = swd_stat_blocks(M);
    double* part1 = (double*)ws;
    double* part2 = part1 + 3 * (size_t)nb;
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(swd_gather_kernel, dim3(nb), dim3(256), 0, st, level, R, P, (long)M, recs, desc, part1);
    DG_CHECK_LAUNCH("swd_gather");
    hipLaunchKernelGGL(swd_var_kernel, dim3(nb), dim3(256), 0, st, (const float*)desc, (long)M, (const double*)part1, part2);
    DG_CHECK_LAUNCH("swd_var");
    hipLaunchKernelGGL(swd_stats_kernel, dim3(1), dim3(256), 0, st, (long)M, nb, (const double*)part1, (const double*)part2, stats);
    DG_CHECK_LAUNCH("swd_stats");
    return DG_OK;
}

// ---- projection ---------------------------------------------------------------------------------------------------------------------------
#define PJ_T 64                    // tile side, descriptors and directions

__global__ __launch_bounds__(256) void swd_project_kernel(const float* __restrict__ desc, const double* __restrict__ stats, int M,
                                                          const float* __restrict__ dirs, int D, float* __restrict__ proj) {
    __shared__ __attribute__((aligned(16))) float As[SWD_CH][PJ_T];
    __shared__ __attribute__((aligned(16))) float Bs[SWD_CH][PJ_T];
    const int t = threadIdx.x, ti = t & 15, td = t >> 4;
    const int i0 = blockIdx.x * PJ_T, d0 = blockIdx.y * PJ_T;
    float acc[4][4] = {};
    for (int c = 0; c < 3; ++c) {
        const double mean = stats[2 * c], sd = stats[2 * c + 1];
        const double inv = 1.0 / sd;
        __syncthreads();                           // the previous chunk is consumed
        for (int e = t; e < PJ_T * SWD_CH; e += 256) {
            const int r = e / SWD_CH, k = e - r * SWD_CH;
            float a = 0.f, b = 0.f;
            if (i0 + r < M) {
                const float v = desc[(long)(i0 + r) * SWD_DESC + c * SWD_CH + k];
                a = sd == 0.0 ? 0.f : (float)(((double)v - mean) * inv);
            }
            if (d0 + r < D) b = dirs[(long)(d0 + r) * SWD_DESC + c * SWD_CH + k];
            As[k][r] = a;
            Bs[k][r] = b;
        }
        __syncthreads();
#pragma unroll 7
        for (int k = 0; k < SWD_CH; ++k) {
            const f32x4 a = *(const f32x4*)&As[k][ti * 4];
            const f32x4 b = *(const f32x4*)&Bs[k][td * 4];
#pragma unroll
            for (int y = 0; y < 4; ++y)
#pragma unroll
                for (int x = 0; x < 4; ++x) acc[y][x] = fmaf(a[x], b[y], acc[y][x]);
        }
    }
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        const int d = d0 + td * 4 + y;
        if (d >= D) continue;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int i = i0 + ti * 4 + x;
            if (i < M) proj[(long)d * M + i] = acc[y][x];
        }
    }
}

#define SWD_CHECK_ROWS(who, D, M)                                                                                  \
    DG_CHECK_ARG((M) >= 1 && (M) <= DG_SWD_MAX_ROW, who ": 1 <= M <= %d (one workgroup's LDS), got %d", DG_SWD_MAX_ROW, (M)); \
    DG_CHECK_ARG((D) >= 1 && (D) <= 65535, who ": 1 <= D <= 65535, got %d", (D))

extern "C" int dg_swd_project(const float* desc, const double* stats, int M, const float* dirs, int D, float* proj, dg_stream_t s) {
    DG_CHECK_ARG(desc != nullptr && stats != nullptr && dirs != nullptr && proj != nullptr, "dg_swd_project: null pointer");
    SWD_CHECK_ROWS("dg_swd_project", D, M);
    DG_CHECK_ARG(((uintptr_t)desc & 3) == 0 && ((uintptr_t)dirs & 3) == 0 && ((uintptr_t)proj & 3) == 0 && ((uintptr_t)stats & 7) == 0,
                 "dg_swd_project: misaligned pointer");
    hipLaunchKernelGGL(swd_project_kernel, dim3((M + PJ_T - 1) / PJ_T, (D + PJ_T - 1) / PJ_T), dim3(256), 0, (hipStream_t)s, desc, stats, M, dirs,
                       D, proj);
    DG_CHECK_LAUNCH("swd_project");
    return DG_OK;
}

// ---- sort and distance --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t swd_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float swd_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// DIST 0: row d of `rows` is sorted in place.  DIST 1: `rows` is only read; out[d] = mean_i |sorted(row)_i - ref[d][i]|, and the sorted
// row goes to sorted_out[d] when that is not NULL.
template <int DIST>
__global__ __launch_bounds__(SWD_SORT_THREADS) void swd_sort_kernel(float* rows, const float* __restrict__ ref, int M, int N,
                                                                    double* __restrict__ out, float* __restrict__ sorted_out) {
    extern __shared__ uint32_t keys[];             // N keys
    __shared__ double red[SWD_SORT_THREADS / 64];
    const int t = threadIdx.x;
    const long base = (long)blockIdx.x * M;
    for (int i = t; i < N; i += SWD_SORT_THREADS) keys[i] = i < M ? swd_key(rows[base + i]) : 0xFFFFFFFFu;
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = t; p < (N >> 1); p += SWD_SORT_THREADS) {
                const int lo = p & (j - 1);
                const int i = ((p - lo) << 1) | lo;
                const uint32_t a = keys[i], b = keys[i + j];
                const bool up = (i & k) == 0;
                if ((a > b) == up) {
                    keys[i] = b;
                    keys[i + j] = a;
                }
            }
            __syncthreads();
        }
    }
    if (DIST == 0) {
        for (int i = t; i < M; i += SWD_SORT_THREADS) rows[base + i] = swd_unkey(keys[i]);
    } else {
        float acc = 0.f;
        for (int i = t; i < M; i += SWD_SORT_THREADS) {
            const float v = swd_unkey(keys[i]);
            acc += fabsf(v - ref[base + i]);
            if (sorted_out != nullptr) sorted_out[base + i] = v;
        }
        const double w = dg_wave_sum_d((double)acc);
        if ((t & 63) == 0) red[t >> 6] = w;
        __syncthreads();
        if (t == 0) {
            double sum = 0.0;
#pragma unroll
            for (int i = 0; i < SWD_SORT_THREADS / 64; ++i) sum += red[i];
            out[blockIdx.x] = sum / (double)M;
        }
    }
}

static int swd_pow2(int M) {
    int N = 1;
    while (N < M) N <<= 1;
    return N;
}

template <int DIST>
static int swd_sort_launch(const char* who, float* rows, const float* ref, int D, int M, double* out, float* sorted_out, hipStream_t st) {
    static const hipError_t once = hipFuncSetAttribute((const void*)swd_sort_kernel<DIST>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       DG_SWD_MAX_ROW * (int)sizeof(uint32_t));
    if (once != hipSuccess) return dg_fail(DG_ERR_HIP, "%s: cannot raise the dynamic LDS limit to %d bytes: %s", who,
                                           DG_SWD_MAX_ROW * (int)sizeof(uint32_t), hipGetErrorString(once));
    const int N = swd_pow2(M);
    hipLaunchKernelGGL(swd_sort_kernel<DIST>, dim3(D), dim3(SWD_SORT_THREADS), (size_t)N * sizeof(uint32_t), st, rows, ref, M, N, out, sorted_out);
    DG_CHECK_LAUNCH(who);
    return DG_OK;
}

extern "C" int dg_swd_sort_rows(float* proj, int D, int M, dg_stream_t s) {
    DG_CHECK_ARG(proj != nullptr, "dg_swd_sort_rows: null pointer");
    SWD_CHECK_ROWS("dg_swd_sort_rows", D, M);
    DG_CHECK_ARG(((uintptr_t)proj & 3) == 0, "dg_swd_sort_rows: misaligned pointer");
    return swd_sort_launch<0>("dg_swd_sort_rows", proj, nullptr, D, M, nullptr, nullptr, (hipStream_t)s);
}

extern "C" int dg_swd_row_distance(const float* proj, const float* ref_sorted, int D, int M, double* out, float* sorted_out, dg_stream_t s) {
    DG_CHECK_ARG(proj != nullptr && ref_sorted != nullptr && out != nullptr, "dg_swd_row_distance: null pointer");
    SWD_CHECK_ROWS("dg_swd_row_distance", D, M);
    DG_CHECK_ARG(((uintptr_t)proj & 3) == 0 && ((uintptr_t)ref_sorted & 3) == 0 && ((uintptr_t)sorted_out & 3) == 0 && ((uintptr_t)out & 7) == 0,
                 "dg_swd_row_distance: misaligned pointer");
    DG_CHECK_ARG(sorted_out == nullptr || (sorted_out != proj && sorted_out != ref_sorted), "dg_swd_row_distance: sorted_out overlaps an input");
    return swd_sort_launch<1>("dg_swd_row_distance", (float*)proj, ref_sorted, D, M, out, sorted_out, (hipStream_t)s);
}
