// Multi-scale SSIM (Wang, Simoncelli, Bovik 2003) as a trainable criterion and as a per-image metric (include/discogan_hip.h,
// "multi-scale SSIM").  x (the reconstruction) and t (the real image): float [n][3][S][S]; M scales; level 0 is the image, level j + 1
// the 2 x 2 fp32 average 0.25f ((a + b) + (c + d)) of level j (side floor(S_j / 2): a last odd row / column is dropped).  Per scale,
// image and channel V_j = mean over the (S_j - 10)^2 valid windows of A2 / B2 (j < M - 1) or of A1 A2 / (B1 B2) (j = M - 1) -- window,
// constants and the four factors are ssim_tile.h's --, ms(i, c) = prod_j V_j^beta_j (0 with gradient 0 when some V_j <= 0), and
//   loss = w_mse mean (x - t)^2 + w_l1 mean |x - t| + w_ms (1 - mean over i, c of ms(i, c)).
//
// Kernels.
//   ms_pyramid_kernel   one launch builds levels 1 .. M-1 of x and of t.  Item = one 32 x 32 level-0 tile of one plane of one of the two
//                       tensors (tiles nest: 32 = 2^5, and a level-j pixel that exists has its four children): a 256-thread block loads
//                       the tile as one quad per thread (16-byte loads under recon.hip's `vec` rule), and reduces 16 x 16, 8 x 8, 4 x 4,
//                       2 x 2 through 5.4 KB of LDS.  Reads 4 B, writes <= 1.33 B per pixel and tensor.
//   ms_fwd_tile_kernel  ONE launch over the items of all scales, item -> (scale, image, channel, tile) by the prefix table of MsGeom;
//                       ssim_tile.h's halo, horizontal and vertical pass (41664 B of LDS + 96 B: three 256-thread blocks per CU), one
//                       quotient per corner (A2 / B2, or the full SSIM at the last scale), at scale 0 also (x - t)^2 and |x - t| when
//                       their weights are on.  fp32 in a thread, fp64 from the wave sum on; partials [items] + 2 x [items of scale 0].
//   ms_final_kernel     one block per problem: thread (i, c) adds the T_j^2 partials of each scale in index order (so ms(i, c) does not
//                       depend on n or on other images), forms V_j, ms and k_j = beta_j ms / V_j in double, writes the k table; the
//                       block sums ms, sse, sae in a fixed order, combines the loss in double and rounds once; the metric entry gets
//                       the per-image means.  No atomics anywhere.
//   ms_bwd_coarse_kernel  scales 1 .. M-1 in one tile launch: the gather form of recon.hip's backward (88144 B of LDS, one 512-thread
//                       block per CU) with, for j < M - 1, the derivatives of A2 / B2 alone (dmu = 0, dsig = -A2 / B2^2, dc = 2 / B2);
//                       writes G_j = k_j g_j / (3 n (S_j - 10)^2 4^j) per level-j pixel into the workspace.
//   ms_bwd_fine_kernel  the level-0 tile kernel: g_0, the gather of G_j(q >> j) for q inside the 2^j S_j square, the MSE and L1 parts;
//                       the combination in double, rounded once, overwriting dx.  Gather only: two calls give the same bits; a tile
//                       and its k row belong to one image: a NaN / inf stays in that image's rows of dx.
// All tile kernels launch at most MS_MAX_BLOCKS blocks per problem and stride; blockIdx.y = the problem (DgPtrs).  The scale tables of
// MsGeom are indexed with a run-time scale in the kernel arguments (scalar loads; no kernel here uses scratch).
// w_ms == 0: the term is not evaluated -- no pyramid, the level-0 tiles alone with no stencil pass in either direction (the tile kernels
// then only sum, or combine, the differences), and the save buffer is neither written nor read.
//
// Saved state.  recon.hip's backward recomputes everything from x and t; this one cannot.  k_j(i, c) needs ms(i, c), the product over ALL
// scales of means over whole planes: the entire forward's sums.  So the forward fills a caller-owned buffer with the k table
// (24 n M B) and, since it is there, the pyramid levels of x and t: (1/4 + 1/16 + ...) < 1/3 of an image per tensor -- at 512 px, batch
// 32 and M = 5 2 x 33.4 MB against 2 x 100.7 MB for reading both images again to rebuild them (and the rebuild's 2 x 33.4 MB of writes).
#include "ssim_tile.h"

#define MS_MAX_BLOCKS 8192
#define MS_MAX_SCALES 5
#define MT 32                 // tile side
#define MK SSIM_K             // window taps
#define MBC SSIM_C            // backward: window corners per axis around a tile: 42
#define MBH (MBC + MK - 1)    // backward halo rows: 52
#define MBY0 (MK - 1)         // the halo starts 10 rows above the tile
#define MBX0 12               // and 12 columns left of it (a whole number of quads)
#define MBP 56                // backward halo pitch
#define MBT 512               // backward block size
static_assert(MT == SSIM_T, "one tile side");

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct MsW {
    float mse, l1, ms;
};

struct MsBeta {
    float b[MS_MAX_SCALES];
};

// scale j: side S[j], T[j] tiles per axis, items start[j] .. start[j + 1] of the forward tile launch (n 3 T[j]^2 of them), 16-byte
// loads when vec[j]; level j >= 1 of x at float offset off[j] of the pyramid buffer, of t at toff + off[j]; the G maps of the backward
// lie at off[j] of the workspace.  Every off[] is a multiple of 4 floats.
struct MsGeom {
    int M, n;
    int S[MS_MAX_SCALES], T[MS_MAX_SCALES], vec[MS_MAX_SCALES];
    long start[MS_MAX_SCALES + 1];
    long off[MS_MAX_SCALES];
    long toff;
};

static long ms_round4(long v) { return (v + 3) / 4 * 4; }

static MsGeom ms_geom(int n, int S, int M) {
    MsGeom g = {};
    g.M = M;
    g.n = n;
    long start = 0, off = 0;
    for (int j = 0; j < M; ++j) {
        const int Sj = S >> j;
        g.S[j] = Sj;
        g.T[j] = (Sj + MT - 1) / MT;
        g.vec[j] = Sj % 4 == 0;
        g.start[j] = start;
        start += (long)n * 3 * g.T[j] * g.T[j];
        g.off[j] = j >= 1 ? off : 0;
        if (j >= 1) off += ms_round4((long)n * 3 * Sj * Sj);
    }
    for (int j = M; j <= MS_MAX_SCALES; ++j) g.start[j] = start;
    g.toff = off;
    return g;
}

static MsBeta ms_beta(int M) {
    static const double e[MS_MAX_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    double sum = 0.0;
    for (int j = 0; j < M; ++j) sum += e[j];
    MsBeta b = {};
    for (int j = 0; j < M; ++j) b.b[j] = (float)(e[j] / sum);
    return b;
}

extern "C" int dg_ms_ssim_max_scales(int S) {
    int m = 0;
    while (m < MS_MAX_SCALES && (S >> m) >= MK) ++m;
    return S < MK ? 0 : m;
}

static bool ms_shape_ok(int n, int S, int M) { return n >= 1 && S >= MK && M >= 1 && M <= dg_ms_ssim_max_scales(S) && S <= 32768; }

// doubles of the partials: [items] quotient sums, 2 x [items of scale 0] sse and sae, [3 n] ms
static size_t ms_part_bytes(const MsGeom& g) {
    return dg_align_up((size_t)(g.start[g.M] + 2 * g.start[1] + 3 * (long)g.n) * sizeof(double), 16);
}

extern "C" size_t dg_ms_ssim_save_bytes(int n, int S, int M) {
    if (!ms_shape_ok(n, S, M)) return 0;
    const MsGeom g = ms_geom(n, S, M);
    return (size_t)(2 * g.toff) * sizeof(float) + (size_t)n * 3 * M * sizeof(double);
}

// the forward's partials followed by room for both pyramids (the metric entry keeps them here)
extern "C" size_t dg_ms_ssim_workspace_bytes(int n, int S, int M) {
    if (!ms_shape_ok(n, S, M)) return 0;
    const MsGeom g = ms_geom(n, S, M);
    return ms_part_bytes(g) + (size_t)(2 * g.toff) * sizeof(float);
}

// the backward's G maps: one float per pixel of levels 1 .. M-1 (16 bytes at M = 1, where nothing is stored)
extern "C" size_t dg_ms_ssim_bwd_workspace_bytes(int n, int S, int M) {
    if (!ms_shape_ok(n, S, M)) return 0;
    const MsGeom g = ms_geom(n, S, M);
    return (size_t)(g.toff > 0 ? g.toff : 4) * sizeof(float);
}

// ---- pyramid ---------------------------------------------------------------------------------------------------------------------------
// item = (plane, tile, tensor): tensor = item & 1; pyr: levels of x at off[j], of t at toff + off[j]
__global__ __launch_bounds__(256) void ms_pyramid_kernel(const DgPtrs xs, const DgPtrs ts, const DgPtrs pyrs, const MsGeom g, long items) {
    __shared__ __attribute__((aligned(16))) float l0[MT * MT];
    __shared__ float l1[16 * 16], l2[8 * 8], l3[4 * 4];
    const int t = threadIdx.x;
    const int S = g.S[0], T = g.T[0], TT = T * T, M = g.M;
    float* __restrict__ pyr = dg_pick<float>(pyrs, blockIdx.y);
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const int which = (int)(item & 1);
        const long pt = item >> 1;
        const long pl = pt / TT;                    // plane = img * 3 + ch
        const int tt = (int)(pt - pl * TT);
        const int ty = tt / T, tx = tt - ty * T;
        const float* __restrict__ src = (which ? dg_pick<const float>(ts, blockIdx.y) : dg_pick<const float>(xs, blockIdx.y)) + pl * (long)S * S;
        float* __restrict__ dst = pyr + (which ? g.toff : 0);
        __syncthreads();                            // the previous item's LDS reads are done
        {
            const int r = t >> 3, q = t & 7;
            const int gy = ty * MT + r, gx = tx * MT + 4 * q;
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if (gy < S) {
                const long o = (long)gy * S + gx;
                if (g.vec[0]) {
                    if (gx + 3 < S) a = *(const f32x4*)(src + o);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (gx + e < S) a[e] = src[o + e];
                }
            }
            *(f32x4*)(l0 + r * MT + 4 * q) = a;
        }
        __syncthreads();
        // level 1: 16 x 16 per tile, one per thread
        {
            const int y = t >> 4, x = t & 15;
            const float* p = l0 + (2 * y) * MT + 2 * x;
            const float v = 0.25f * ((p[0] + p[1]) + (p[MT] + p[MT + 1]));
            l1[t] = v;
            const int Sj = g.S[1], gy = ty * 16 + y, gx = tx * 16 + x;
            if (gy < Sj && gx < Sj) dst[g.off[1] + pl * (long)Sj * Sj + (long)gy * Sj + gx] = v;
        }
        if (M > 2) {
            __syncthreads();
            if (t < 64) {
                const int y = t >> 3, x = t & 7;
                const float* p = l1 + (2 * y) * 16 + 2 * x;
                const float v = 0.25f * ((p[0] + p[1]) + (p[16] + p[17]));
                l2[t] = v;
                const int Sj = g.S[2], gy = ty * 8 + y, gx = tx * 8 + x;
                if (gy < Sj && gx < Sj) dst[g.off[2] + pl * (long)Sj * Sj + (long)gy * Sj + gx] = v;
            }
        }
        if (M > 3) {
            __syncthreads();
            if (t < 16) {
                const int y = t >> 2, x = t & 3;
                const float* p = l2 + (2 * y) * 8 + 2 * x;
                const float v = 0.25f * ((p[0] + p[1]) + (p[8] + p[9]));
                l3[t] = v;
                const int Sj = g.S[3], gy = ty * 4 + y, gx = tx * 4 + x;
                if (gy < Sj && gx < Sj) dst[g.off[3] + pl * (long)Sj * Sj + (long)gy * Sj + gx] = v;
            }
        }
        if (M > 4) {
            __syncthreads();
            if (t < 4) {
                const int y = t >> 1, x = t & 1;
                const float* p = l3 + (2 * y) * 4 + 2 * x;
                const float v = 0.25f * ((p[0] + p[1]) + (p[4] + p[5]));
                const int Sj = g.S[4], gy = ty * 2 + y, gx = tx * 2 + x;
                if (gy < Sj && gx < Sj) dst[g.off[4] + pl * (long)Sj * Sj + (long)gy * Sj + gx] = v;
            }
        }
    }
}

// the scale of a forward item (block-uniform)
__device__ __forceinline__ int ms_scale_of(const MsGeom& g, long item) {
    int j = 0;
    while (j + 1 < g.M && item >= g.start[j + 1]) ++j;
    return j;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
// part: [items] quotient sums (written when do_ms), then [items0] sse, [items0] sae (written when do_px).  do_ms == 0 (w_ms == 0): the
// host passes the one-scale geometry and no stencil pass runs.
__global__ __launch_bounds__(256) void ms_fwd_tile_kernel(const DgPtrs xs, const DgPtrs ts, const DgPtrs pyrs, const MsGeom g, int do_px, int do_ms,
                                                          const SsimTaps taps, const DgPtrs parts) {
    constexpr int PITCH = 44;           // halo pitch (whole quads)
    __shared__ __attribute__((aligned(16))) float sx[SSIM_C * PITCH];
    __shared__ __attribute__((aligned(16))) float sy[SSIM_C * PITCH];
    __shared__ float hp[5][SSIM_C * SSIM_T];
    __shared__ double red[3][4];
    const int t = threadIdx.x;
    const float* __restrict__ x0 = dg_pick<const float>(xs, blockIdx.y);
    const float* __restrict__ t0 = dg_pick<const float>(ts, blockIdx.y);
    const float* __restrict__ pyr = dg_pick<const float>(pyrs, blockIdx.y);
    double* __restrict__ part = dg_pick<double>(parts, blockIdx.y);
    const long items = g.start[g.M], items0 = g.start[1];
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const int j = ms_scale_of(g, item);
        const int S = g.S[j], T = g.T[j], TT = T * T, vec = g.vec[j];
        const bool last = j == g.M - 1;
        const long local = item - g.start[j];
        const long pl = local / TT;                // plane = img * 3 + ch
        const int tt = (int)(local - pl * TT);
        const int gy0 = (tt / T) * SSIM_T, gx0 = (tt % T) * SSIM_T;
        const long base = pl * (long)S * S;
        const float* __restrict__ bx = (j == 0 ? x0 : pyr + g.off[j]) + base;
        const float* __restrict__ by = (j == 0 ? t0 : pyr + g.toff + g.off[j]) + base;
        const int nvalid = S - (SSIM_K - 1);
        __syncthreads();                           // the previous item's LDS reads are done
        ssim_stage_halo<256, SSIM_C, PITCH, 0, 0>(bx, by, S, gy0, gx0, vec, sx, sy);
        __syncthreads();
        float sse = 0.f, sae = 0.f;
        if (j == 0 && do_px) {
            float e2[4], e1[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = t + 256 * e, r = i >> 5, c = i & 31;
                const bool in = gy0 + r < S && gx0 + c < S;
                const float d = sx[r * PITCH + c] - sy[r * PITCH + c];
                e2[e] = in ? d * d : 0.f;
                e1[e] = in ? fabsf(d) : 0.f;
            }
            sse = (e2[0] + e2[1]) + (e2[2] + e2[3]);
            sae = (e1[0] + e1[1]) + (e1[2] + e1[3]);
        }
        float ss = 0.f;
        if (do_ms) {
            const int cr = min(SSIM_C / 2, S - 1 - gy0), cc = min(SSIM_C / 2, S - 1 - gx0);
            const float cx = sx[cr * PITCH + cc], cy = sy[cr * PITCH + cc];
            ssim_hpass<256, SSIM_C, SSIM_T, PITCH, 0>(sx, sy, cx, cy, taps, hp);
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = t + 256 * e, r = i >> 5, c = i & 31;
                if (gy0 + r < nvalid && gx0 + c < nvalid) {
                    const SsimTerms s = ssim_terms(ssim_vpass<SSIM_C, SSIM_T>(hp, r, c, taps), cx, cy);
                    ss += last ? (s.A1 * s.A2) / (s.B1 * s.B2) : s.A2 / s.B2;
                }
            }
        }
        double sums[3] = {(double)ss, (double)sse, (double)sae};
        dg_block_stage_d(sums, red);
        if (t == 0 && do_ms) part[item] = dg_sum4_pair(red[0]);
        if (j == 0 && do_px && (t == 1 || t == 2)) part[items + (t - 1) * items0 + item] = dg_sum4_pair(red[t]);
    }
}

// one block per problem (blockIdx.x).  ktab: [n][3][M] doubles per problem (null table entry: not wanted); msb: [3 n] doubles of scratch
// behind the partials; metric: [n] floats (problem 0 only) or null
__global__ __launch_bounds__(256) void ms_final_kernel(const DgPtrs parts, const DgPtrs ktabs, const MsGeom g, const MsBeta beta, const MsW w,
                                                       int do_px, double inv_px, const DgPtrs losses, float* __restrict__ metric) {
    __shared__ double red[3][4];
    const double* __restrict__ part = dg_pick<const double>(parts, blockIdx.x);
    double* __restrict__ ktab = dg_pick<double>(ktabs, blockIdx.x);
    float* __restrict__ loss = dg_pick<float>(losses, blockIdx.x);
    const int t = threadIdx.x, M = g.M;
    const long items = g.start[M], items0 = g.start[1], pairs = 3 * (long)g.n;
    double* __restrict__ msb = (double*)part + items + 2 * items0;
    double s[3] = {0.0, 0.0, 0.0};                 // sums of ms, (x - t)^2, |x - t|
    for (long pair = t; pair < (w.ms > 0.f ? pairs : 0); pair += 256) {      // (w_ms == 0: no quotient partials exist)
        double V[MS_MAX_SCALES];
        bool nan = false, dead = false;
#pragma unroll
        for (int j = 0; j < MS_MAX_SCALES; ++j) {
            if (j < M) {
                const int TT = g.T[j] * g.T[j];
                const double win = (double)(g.S[j] - (MK - 1));
                const double* p = part + g.start[j] + pair * TT;
                double a = 0.0;
                for (int i = 0; i < TT; ++i) a += p[i];
                V[j] = a / (win * win);
                nan = nan || V[j] != V[j];
                dead = dead || V[j] <= 0.0;
            }
        }
        double ms = 1.0;
        if (nan) {
            ms = __builtin_nan("");
        } else if (dead) {
            ms = 0.0;
        } else {
#pragma unroll
            for (int j = 0; j < MS_MAX_SCALES; ++j)
                if (j < M) ms *= pow(V[j], (double)beta.b[j]);
        }
        if (ktab != nullptr) {
#pragma unroll
            for (int j = 0; j < MS_MAX_SCALES; ++j)
                if (j < M) ktab[pair * M + j] = nan ? ms : (dead ? 0.0 : (double)beta.b[j] * ms / V[j]);
        }
        msb[pair] = ms;
        s[0] += ms;
    }
    if (do_px)
        for (long i = t; i < items0; i += 256) {
            s[1] += part[items + i];
            s[2] += part[items + items0 + i];
        }
    dg_block_stage_d(s, red);                      // (its barriers also publish msb to the block)
    if (t == 0 && loss != nullptr) {
        double v = 0.0;
        if (w.mse > 0.f) v += (double)w.mse * (dg_sum4_pair(red[1]) * inv_px);
        if (w.l1 > 0.f) v += (double)w.l1 * (dg_sum4_pair(red[2]) * inv_px);
        if (w.ms > 0.f) v += (double)w.ms * (1.0 - dg_sum4_pair(red[0]) / (double)pairs);
        loss[0] = (float)v;
    }
    if (metric != nullptr)
        for (long img = t; img < g.n; img += 256) metric[img] = (float)(((msb[3 * img] + msb[3 * img + 1]) + msb[3 * img + 2]) / 3.0);
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// The gather form on one tile of one plane (bx, by: the plane of level j, side S): per thread the bracket sums g(q) of its two
// neighbouring pixels (row r = t >> 4, columns 2 (t & 15), + 1 of the tile) and the pixels' values.  full: the derivatives of the whole
// SSIM quotient (the last scale); else those of A2 / B2.  Steps 1 - 5 are those of recon_bwd_tile_kernel (recon.hip), which keeps its own
// text so that the single-scale kinds keep their kernels and bits; likewise ms_fwd_tile_kernel and ssim_fwd_tiles (ssim_tile.h).  A fix
// to the adjoint stencil belongs in both.
__device__ __forceinline__ void ms_bwd_tile(const float* __restrict__ bx, const float* __restrict__ by, int S, int gy0, int gx0, int vec, bool full,
                                            const SsimTaps& taps, float (&gq)[2], float (&xv)[2], float (&tv)[2]) {
    __shared__ __attribute__((aligned(16))) float sx[MBH * MBP];
    __shared__ __attribute__((aligned(16))) float sy[MBH * MBP];
    __shared__ __attribute__((aligned(16))) float hp[5][MBH * MBC];     // horizontal moment planes: 52 rows x 42 corner columns
    __shared__ float cm[3][MBC * MBC];                                 // coefficient maps a, b, c over the 42 x 42 corners
    float* const hq = &hp[0][0];                                       // adjoint horizontal planes [3][42 x 32], once hp has been read
    const int t = threadIdx.x;
    const int nvalid = S - (MK - 1);
    __syncthreads();                               // the previous item's LDS reads are done
    ssim_stage_halo<MBT, MBH, MBP, MBY0, MBX0>(bx, by, S, gy0, gx0, vec, sx, sy);
    __syncthreads();
    const int cr = min(gy0 + MT / 2, S - 1) - gy0 + MBY0, cc = min(gx0 + MT / 2, S - 1) - gx0 + MBX0;
    const float cx = sx[cr * MBP + cc], cy = sy[cr * MBP + cc];
    ssim_hpass<MBT, MBH, MBC, MBP, MBX0 - MBY0>(sx, sy, cx, cy, taps, hp);
    __syncthreads();
    for (int i = t; i < MBC * MBC; i += MBT) {
        const int ci = i / MBC, cj = i - ci * MBC;
        const int gr = gy0 - MBY0 + ci, gc = gx0 - MBY0 + cj;
        float ca = 0.f, cb = 0.f, cq = 0.f;
        if (gr >= 0 && gr < nvalid && gc >= 0 && gc < nvalid) {
            const SsimMoments m = ssim_vpass<MBH, MBC>(hp, ci, cj, taps);
            const SsimTerms s = ssim_terms(m, cx, cy);
            float dmu, dsig, dc;
            if (full) {
                const float r12 = 1.f / (s.B1 * s.B2);
                const float sv = s.A1 * s.A2 * r12;
                dmu = 2.f * s.my * s.A2 * r12 - 2.f * s.mx * sv / s.B1;
                dsig = -sv / s.B2;
                dc = 2.f * s.A1 * r12;
            } else {
                const float r2 = 1.f / s.B2;
                dmu = 0.f;
                dsig = -(s.A2 * r2) * r2;
                dc = 2.f * r2;
            }
            ca = dmu - 2.f * m.m0 * dsig - m.m1 * dc;
            cb = 2.f * dsig;
            cq = dc;
        }
        cm[0][i] = ca; cm[1][i] = cb; cm[2][i] = cq;
    }
    __syncthreads();                               // hp is read; hq takes its place
    for (int i = t; i < MBC * MT; i += MBT) {
        const int ci = i >> 5, c = i & 31;
        const int o = ci * MBC + c;
        float q0 = 0.f, q1 = 0.f, q2 = 0.f;
#pragma unroll
        for (int e = 0; e < MK; ++e) {
            const float gw = taps.g[MK - 1 - e];
            q0 += gw * cm[0][o + e];
            q1 += gw * cm[1][o + e];
            q2 += gw * cm[2][o + e];
        }
        hq[i] = q0; hq[MBC * MT + i] = q1; hq[2 * MBC * MT + i] = q2;
    }
    __syncthreads();
    const int r = t >> 4, c = (t & 15) * 2;
    f32x2 q0 = {0.f, 0.f}, q1 = {0.f, 0.f}, q2 = {0.f, 0.f};
#pragma unroll
    for (int e = 0; e < MK; ++e) {
        const float gw = taps.g[MK - 1 - e];
        const int o = (r + e) * MT + c;
        q0 += gw * *(const f32x2*)(hq + o);
        q1 += gw * *(const f32x2*)(hq + MBC * MT + o);
        q2 += gw * *(const f32x2*)(hq + 2 * MBC * MT + o);
    }
    const int ho = (r + MBY0) * MBP + c + MBX0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        xv[e] = sx[ho + e];
        tv[e] = sy[ho + e];
        gq[e] = q0[e] + (xv[e] - cx) * q1[e] + (tv[e] - cy) * q2[e];
    }
}

// scales 1 .. M-1: G_j = k_j g_j / (3 n (S_j - 10)^2 4^j) into gm + off[j]; items: start[1] .. start[M] of the forward's table
__global__ __launch_bounds__(MBT) void ms_bwd_coarse_kernel(const DgPtrs saves, const DgPtrs gms, const MsGeom g, const SsimTaps taps) {
    const float* __restrict__ pyr = dg_pick<const float>(saves, blockIdx.y);
    const double* __restrict__ ktab = (const double*)(pyr + 2 * g.toff);
    float* __restrict__ gm = dg_pick<float>(gms, blockIdx.y);
    const int t = threadIdx.x, M = g.M;
    const long items = g.start[M];
    for (long item = g.start[1] + blockIdx.x; item < items; item += gridDim.x) {
        const int j = ms_scale_of(g, item);
        const int S = g.S[j], T = g.T[j], TT = T * T;
        const long local = item - g.start[j];
        const long pl = local / TT;
        const int tt = (int)(local - pl * TT);
        const int gy0 = (tt / T) * MT, gx0 = (tt % T) * MT;
        const long base = pl * (long)S * S;
        const double k = ktab[pl * M + j];
        const double win = (double)(S - (MK - 1));
        const double f = k / (3.0 * (double)g.n * win * win * (double)(1 << (2 * j)));
        float gq[2] = {0.f, 0.f}, xv[2], tv[2];
        if (k != 0.0) ms_bwd_tile(pyr + g.off[j] + base, pyr + g.toff + g.off[j] + base, S, gy0, gx0, g.vec[j], j == M - 1, taps, gq, xv, tv);
        const int gy = gy0 + (t >> 4), gx = gx0 + (t & 15) * 2;
        if (gy < S) {
            float* o = gm + g.off[j] + base + (long)gy * S + gx;
            if (gx < S) o[0] = k != 0.0 ? (float)(f * (double)gq[0]) : 0.f;
            if (gx + 1 < S) o[1] = k != 0.0 ? (float)(f * (double)gq[1]) : 0.f;
        }
    }
}

// level 0: dx = gout ( w_mse 2 (x - t) / N + w_l1 sign(x - t) / N - w_ms [ k_0 g_0 / (3 n (S - 10)^2) + sum_j G_j(q >> j) ] )
__global__ __launch_bounds__(MBT) void ms_bwd_fine_kernel(const DgPtrs xs, const DgPtrs ts, const DgPtrs gouts, const DgPtrs dxs, const DgPtrs saves,
                                                          const DgPtrs gms, const MsGeom g, int vec, const SsimTaps taps, const MsW w, double inv_px) {
    const float* __restrict__ x = dg_pick<const float>(xs, blockIdx.y);
    const float* __restrict__ y = dg_pick<const float>(ts, blockIdx.y);
    const float* __restrict__ gout = dg_pick<const float>(gouts, blockIdx.y);
    float* __restrict__ dx = dg_pick<float>(dxs, blockIdx.y);
    const float* __restrict__ pyr = dg_pick<const float>(saves, blockIdx.y);
    const double* __restrict__ ktab = (const double*)(pyr + 2 * g.toff);
    const float* __restrict__ gm = dg_pick<const float>(gms, blockIdx.y);
    const int t = threadIdx.x, M = g.M;
    const int S = g.S[0], T = g.T[0], TT = T * T;
    const long items = g.start[1];
    const double go = (double)gout[0];
    const double kmse = go * (double)w.mse * 2.0 * inv_px, kl1 = go * (double)w.l1 * inv_px, kms = go * (double)w.ms;
    const double win = (double)(S - (MK - 1));
    const double inv_win = 1.0 / (3.0 * (double)g.n * win * win);
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long pl = item / TT;
        const int tt = (int)(item - pl * TT);
        const int gy0 = (tt / T) * MT, gx0 = (tt % T) * MT;
        const long base = pl * (long)S * S;
        const bool on = w.ms > 0.f;                // w_ms == 0: the term is not evaluated -- no stencil, no read of save or of the G maps
        const double k0 = on ? ktab[pl * M] : 0.0;
        const bool dead = k0 == 0.0;               // ms = 0: every k_j is 0 and the MS-SSIM term has no gradient
        const int gy = gy0 + (t >> 4), gx = gx0 + (t & 15) * 2;
        float gq[2] = {0.f, 0.f}, xv[2] = {0.f, 0.f}, tv[2] = {0.f, 0.f};
        if (on) {
            ms_bwd_tile(x + base, y + base, S, gy0, gx0, vec, M == 1, taps, gq, xv, tv);
        } else if (gy < S) {
#pragma unroll
            for (int e = 0; e < 2; ++e)
                if (gx + e < S) {
                    xv[e] = x[base + (long)gy * S + gx + e];
                    tv[e] = y[base + (long)gy * S + gx + e];
                }
        }
        double coarse = 0.0;
        if (!dead) {
#pragma unroll
            for (int j = 1; j < MS_MAX_SCALES; ++j)
                if (j < M) {
                    const int Sj = g.S[j], cy_ = gy >> j, cx_ = gx >> j;
                    if (cy_ < Sj && cx_ < Sj) coarse += (double)gm[g.off[j] + pl * (long)Sj * Sj + (long)cy_ * Sj + cx_];
                }
        }
        f32x2 res;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double d = (double)xv[e] - (double)tv[e];
            double v = 0.0;
            if (w.mse > 0.f) v += d * kmse;
            if (w.l1 > 0.f) v += (d != d ? d : (d > 0.0 ? kl1 : (d < 0.0 ? -kl1 : 0.0)));
            if (w.ms > 0.f && !dead) v -= kms * (k0 * inv_win * (double)gq[e] + coarse);
            res[e] = (float)v;
        }
        if (gy < S) {
            float* o = dx + base + (long)gy * S + gx;
            if (vec) {
                if (gx + 1 < S) *(f32x2*)o = res;
            } else {
                if (gx < S) o[0] = res[0];
                if (gx + 1 < S) o[1] = res[1];
            }
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// the checks all entry points share; tabs: the pointer tables, each with `groups` non-null entries aligned to `align[i]` bytes
static int ms_check(const char* who, int groups, int n, int S, int M, const float* w, const void* const* const* tabs, const int* align, int ntabs) {
    DG_CHECK_ARG(groups >= 1 && groups <= DG_MAX_GROUPS, "%s: groups=%d (1..%d)", who, groups, DG_MAX_GROUPS);
    DG_CHECK_ARG(w != nullptr, "%s: null weights", who);
    for (int i = 0; i < 3; ++i) DG_CHECK_ARG(isfinite(w[i]) && w[i] >= 0.f, "%s: weight %d = %g must be finite and >= 0", who, i, (double)w[i]);
    DG_CHECK_ARG(w[0] > 0.f || w[1] > 0.f || w[2] > 0.f, "%s: all three weights are 0", who);
    DG_CHECK_ARG(n >= 1, "%s: n %d < 1", who, n);
    DG_CHECK_ARG(S >= MK, "%s: S %d < %d (the window does not fit)", who, S, MK);
    DG_CHECK_ARG(S <= 32768, "%s: S %d is too large", who, S);
    DG_CHECK_ARG(M >= 1 && M <= dg_ms_ssim_max_scales(S), "%s: M %d scales (1..%d at S %d: every scale needs a side >= %d)", who, M,
                 dg_ms_ssim_max_scales(S), S, MK);
    for (int k = 0; k < ntabs; ++k) {
        DG_CHECK_ARG(tabs[k] != nullptr, "%s: null pointer table", who);
        for (int i = 0; i < groups; ++i) {
            DG_CHECK_ARG(tabs[k][i] != nullptr, "%s: null pointer (problem %d)", who, i);
            DG_CHECK_ARG(((uintptr_t)tabs[k][i] & (uintptr_t)(align[k] - 1)) == 0, "%s: pointer of problem %d is not %d-byte aligned", who, i, align[k]);
        }
    }
    return DG_OK;
}

static int ms_vec(int groups, int S, const void* const* a, const void* const* b, const void* const* c) {
    uintptr_t bits = 0;
    for (int i = 0; i < groups; ++i) bits |= (uintptr_t)a[i] | (uintptr_t)b[i] | (c ? (uintptr_t)c[i] : 0);
    return S % 4 == 0 && (bits & 15) == 0;
}

static unsigned ms_grid(long items) { return (unsigned)(items < MS_MAX_BLOCKS ? items : MS_MAX_BLOCKS); }

// pyramid, tile pass and final block of `groups` problems; pyr: where the levels go; ktab: the k tables (or null); loss: the slots (or
// null); metric: [n] floats of problem 0 (or null)
static int ms_forward(const char* who, int groups, const void* const* x, const void* const* t, int n, int S, int M, const MsW w, void* const* pyr,
                      void* const* ktab, const void* const* loss, void* const* ws, float* metric, hipStream_t st) {
    const int do_ms = w.ms > 0.f;
    if (!do_ms) M = 1;                             // a term of weight 0 is not evaluated: no pyramid, the tiles of level 0 alone, no stencil pass
    MsGeom g = ms_geom(n, S, M);
    g.vec[0] = ms_vec(groups, S, x, t, nullptr);
    const DgPtrs px = dg_ptrs(x, groups), pt = dg_ptrs(t, groups), pp = dg_ptrs((const void* const*)pyr, groups),
                 pw = dg_ptrs((const void* const*)ws, groups);
    const int do_px = w.mse > 0.f || w.l1 > 0.f;
    if (M > 1) {
        const long pitems = 2 * g.start[1];
        hipLaunchKernelGGL(ms_pyramid_kernel, dim3(ms_grid(pitems), groups), dim3(256), 0, st, px, pt, pp, g, pitems);
        DG_CHECK_LAUNCH("ms_pyramid");
    }
    hipLaunchKernelGGL(ms_fwd_tile_kernel, dim3(ms_grid(g.start[M]), groups), dim3(256), 0, st, px, pt, pp, g, do_px, do_ms, ssim_taps(), pw);
    DG_CHECK_LAUNCH("ms_fwd_tile");
    hipLaunchKernelGGL(ms_final_kernel, dim3(groups), dim3(256), 0, st, pw, dg_ptrs((const void* const*)ktab, groups), g, ms_beta(M), w, do_px,
                       1.0 / ((double)n * 3.0 * (double)S * (double)S), dg_ptrs(loss, groups), metric);
    DG_CHECK_LAUNCH("ms_final");
    return DG_OK;
}

extern "C" int dg_ms_ssim_loss_fwd_g(int groups, const float* const* x, const float* const* t, int n, int S, int M, const float* w,
                                     float* const* loss, void* const* save, size_t save_bytes, void* const* ws, size_t ws_bytes, dg_stream_t stream) {
    const void* const* tabs[] = {(const void* const*)x, (const void* const*)t, (const void* const*)loss, (const void* const*)save,
                                 (const void* const*)ws};
    const int align[] = {4, 4, 4, 16, 16};
    const int rc = ms_check("dg_ms_ssim_loss_fwd", groups, n, S, M, w, tabs, align, 5);
    if (rc != DG_OK) return rc;
    if (ws_bytes < dg_ms_ssim_workspace_bytes(n, S, M))
        return dg_fail(DG_ERR_WORKSPACE, "dg_ms_ssim_loss_fwd: workspace too small (%zu bytes, %zu needed)", ws_bytes,
                       dg_ms_ssim_workspace_bytes(n, S, M));
    if (save_bytes < dg_ms_ssim_save_bytes(n, S, M))
        return dg_fail(DG_ERR_WORKSPACE, "dg_ms_ssim_loss_fwd: save buffer too small (%zu bytes, %zu needed)", save_bytes,
                       dg_ms_ssim_save_bytes(n, S, M));
    const MsGeom g = ms_geom(n, S, M);
    void* ktab[DG_MAX_GROUPS];
    for (int i = 0; i < groups; ++i) ktab[i] = (float*)save[i] + 2 * g.toff;
    const MsW mw = {w[0], w[1], w[2]};
    return ms_forward("dg_ms_ssim_loss_fwd", groups, tabs[0], tabs[1], n, S, M, mw, save, ktab, tabs[2], ws, nullptr, (hipStream_t)stream);
}

extern "C" int dg_ms_ssim_loss_fwd(const float* x, const float* t, int n, int S, int M, const float* w, float* loss, void* save, size_t save_bytes,
                                   void* ws, size_t ws_bytes, dg_stream_t stream) {
    return dg_ms_ssim_loss_fwd_g(1, &x, &t, n, S, M, w, &loss, &save, save_bytes, &ws, ws_bytes, stream);
}

extern "C" int dg_ms_ssim_loss_bwd_g(int groups, const float* const* x, const float* const* t, int n, int S, int M, const float* w,
                                     const float* const* gout, const void* const* save, size_t save_bytes, float* const* dx, void* const* ws,
                                     size_t ws_bytes, dg_stream_t stream) {
    const void* const* tabs[] = {(const void* const*)x, (const void* const*)t, (const void* const*)gout, (const void* const*)save,
                                 (const void* const*)dx, (const void* const*)ws};
    const int align[] = {4, 4, 4, 16, 4, 16};
    const int rc = ms_check("dg_ms_ssim_loss_bwd", groups, n, S, M, w, tabs, align, 6);
    if (rc != DG_OK) return rc;
    if (ws_bytes < dg_ms_ssim_bwd_workspace_bytes(n, S, M))
        return dg_fail(DG_ERR_WORKSPACE, "dg_ms_ssim_loss_bwd: workspace too small (%zu bytes, %zu needed)", ws_bytes,
                       dg_ms_ssim_bwd_workspace_bytes(n, S, M));
    if (save_bytes < dg_ms_ssim_save_bytes(n, S, M))
        return dg_fail(DG_ERR_WORKSPACE, "dg_ms_ssim_loss_bwd: save buffer too small (%zu bytes, %zu needed)", save_bytes,
                       dg_ms_ssim_save_bytes(n, S, M));
    const MsGeom g = ms_geom(n, S, M);
    const MsW mw = {w[0], w[1], w[2]};
    const int vec = ms_vec(groups, S, tabs[0], tabs[1], tabs[4]);
    const DgPtrs px = dg_ptrs(tabs[0], groups), pt = dg_ptrs(tabs[1], groups), pg = dg_ptrs(tabs[2], groups), ps = dg_ptrs(tabs[3], groups),
                 pd = dg_ptrs(tabs[4], groups), pw = dg_ptrs(tabs[5], groups);
    hipStream_t st = (hipStream_t)stream;
    if (M > 1 && mw.ms > 0.f) {
        hipLaunchKernelGGL(ms_bwd_coarse_kernel, dim3(ms_grid(g.start[M] - g.start[1]), groups), dim3(MBT), 0, st, ps, pw, g, ssim_taps());
        DG_CHECK_LAUNCH("ms_bwd_coarse");
    }
    hipLaunchKernelGGL(ms_bwd_fine_kernel, dim3(ms_grid(g.start[1]), groups), dim3(MBT), 0, st, px, pt, pg, pd, ps, pw, g, vec, ssim_taps(), mw,
                       1.0 / ((double)n * 3.0 * (double)S * (double)S));
    DG_CHECK_LAUNCH("ms_bwd_fine");
    return DG_OK;
}

extern "C" int dg_ms_ssim_loss_bwd(const float* x, const float* t, int n, int S, int M, const float* w, const float* gout, const void* save,
                                   size_t save_bytes, float* dx, void* ws, size_t ws_bytes, dg_stream_t stream) {
    return dg_ms_ssim_loss_bwd_g(1, &x, &t, n, S, M, w, &gout, &save, save_bytes, &dx, &ws, ws_bytes, stream);
}

extern "C" int dg_image_ms_ssim(const float* x, const float* y, int n, int S, int M, float* out, void* ws, size_t ws_bytes, dg_stream_t stream) {
    const float w[3] = {0.f, 0.f, 1.f};
    const void* const* tabs[] = {(const void* const*)&x, (const void* const*)&y, (const void* const*)&out, (const void* const*)&ws};
    const int align[] = {4, 4, 4, 16};
    const int rc = ms_check("dg_image_ms_ssim", 1, n, S, M, w, tabs, align, 4);
    if (rc != DG_OK) return rc;
    if (ws_bytes < dg_ms_ssim_workspace_bytes(n, S, M))
        return dg_fail(DG_ERR_WORKSPACE, "dg_image_ms_ssim: workspace too small (%zu bytes, %zu needed)", ws_bytes,
                       dg_ms_ssim_workspace_bytes(n, S, M));
    const MsGeom g = ms_geom(n, S, M);
    void* pyr = (char*)ws + ms_part_bytes(g);
    const MsW mw = {0.f, 0.f, 1.f};
    return ms_forward("dg_image_ms_ssim", 1, tabs[0], tabs[1], n, S, M, mw, &pyr, nullptr, nullptr, &ws, out, (hipStream_t)stream);
}
