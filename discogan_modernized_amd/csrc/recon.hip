// Trainable reconstruction criterion (include/discogan_hip.h, "reconstruction loss"): for float NCHW batches x (the reconstruction) and
// t (the real image) of [n][3][S][S] and weights (w_mse, w_l1, w_ssim) >= 0
//   loss = w_mse mean (x - t)^2 + w_l1 mean |x - t| + w_ssim (1 - mean over n 3 (S - 10)^2 valid windows of SSIM)
// with SSIM exactly the quantity of dg_image_metrics: both run the one stencil of ssim_tile.h (window, constants, tile geometry and the
// moments about a per-tile constant are written there), and its gradient with respect to x.  The reference trains on nn.MSELoss only
// (image_translation.py:267,349-350); this is the CycleGAN (L1) and the restoration (SSIM + L1, Zhao et al. 2017) choice of the same term.
//
// Forward.  w_ssim > 0: ssim_tile.h's forward tile body with problems picked by blockIdx.y, three fp64 block sums per item to the
// workspace: [3][n P] doubles per problem, P = 3 ceil(S / 32)^2.  w_ssim == 0: no stencil, a plain streaming pass (quads summed pairwise in fp32, fp64 from there on) into
// [2][blocks] partials.  One final block per problem sums the partials in a fixed order (thread t: t, t + 256, ...; wave; four waves),
// forms w_mse sse / N + w_l1 sae / N + w_ssim (1 - ss / windows) in double and rounds once into loss[g], a slot of the trainer's loss
// vector.  A term whose weight is 0 is left out of the sum (0 x inf would poison it).
//
// Backward: dx = gout ( w_mse 2 (x - t) / N + w_l1 sign(x - t) / N - w_ssim d(mean SSIM) / dx ), one pass, overwriting, sign(0) = 0.
// Per window p with A1 = 2 mx my + C1, A2 = 2 sxy + C2, B1 = mx^2 + my^2 + C1, B2 = sx2 + sy2 + C2:
//   dmu = 2 my A2 / (B1 B2) - 2 mx A1 A2 / (B1^2 B2),  dsig = -A1 A2 / (B1 B2^2),  dc = 2 A1 / (B1 B2)
//   d(mean SSIM) / dx(q) = sum over the valid windows p that contain q of w(q - p) [ dmu + 2 dsig (x(q) - mx) + dc (t(q) - my) ] / windows
// and with the moments about the tile's constants (m0 = mx - cx, m1 = my - cy, x' = x - cx, t' = t - cy) the bracket is
//   a + x'(q) b + t'(q) c,   a = dmu - 2 m0 dsig - m1 dc,  b = 2 dsig,  c = dc:
// three coefficient maps over the window corners and the adjoint ("full") separable pass over them, written as a GATHER per output
// pixel: no atomics, two calls give the same bits.
//
// The coefficient maps are RECOMPUTED in the backward, not saved by the forward.  Saved maps are 3 floats per window: the forward would
// write 12 B and the backward read 12 x (42 / 32)^2 = 20.7 B per pixel on top of the 8 + 4 B of x, t and dx, against 8 x (52 / 32)^2 =
// 21.1 B of halo reads here, most of which are the neighbouring tiles' lines in L2 -- recomputing moves FEWER bytes through HBM (forward
// + backward 8 + 12 B/pixel of compulsory traffic instead of 20 + 24), keeps 2 x 290 MB (512 px, batch 32, two domains) out of the
// allocator, and a forward called for the log line alone (no_grad) pays nothing for a backward that never comes.  The price is LDS work:
// a 32 x 32 output tile needs the 42 x 42 corners around it, hence a 52 x 52 halo (stored 52 x 56 from column -12, so that quads stay on
// 16-byte lines), a horizontal pass over 52 x 42 and a vertical over 42 x 42 for five planes, then the adjoint passes over 42 x 32 and
// 32 x 32 for three: about 2.3 x the forward's multiply-adds.  LDS: 2 x 11648 B halo + 43680 B moment planes (re-used by the adjoint's
// horizontal planes) + 21168 B coefficient maps = 88144 B, one 512-thread block (8 waves) per CU of 160 KiB.
// One work item = one tile; both tile kernels launch at most RC_MAX_BLOCKS blocks per problem and stride; blockIdx.y = the problem
// (DgPtrs).  A tile belongs to one image: a NaN / inf stays in that image's rows of dx.
// fp32 inside the stencils; the per-pixel combination gout (...) is formed in double and rounded once, so the MSE and L1 parts alone are
// one rounding away from gout 2 (x - t) / N and gout sign(x - t) / N.
#include "ssim_tile.h"

#define RC_MAX_BLOCKS 8192
#define RC_STREAM_BLOCKS 1024
#define RT 32                 // tile side
#define RK SSIM_K             // window taps
#define BC SSIM_C             // backward: window corners per axis around a tile: 42
#define BH (BC + RK - 1)      // backward halo rows: 52
#define BY0 (RK - 1)          // the halo starts 10 rows above the tile
#define BX0 12                // and 12 columns left of it (a whole number of quads)
#define BP 56                 // backward halo pitch: 12 + 32 + 10 = 54 columns, rounded up to quads
#define BT 512                // backward block size
static_assert(RT == SSIM_T, "one tile side");

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct RcW {
    float mse, l1, ssim;
};

__global__ __launch_bounds__(256) void recon_fwd_tile_kernel(const DgPtrs xs, const DgPtrs ts, long items, int S, int T, int vec, const SsimTaps taps,
                                                             const DgPtrs parts) {
    ssim_fwd_tiles(dg_pick<const float>(xs, blockIdx.y), dg_pick<const float>(ts, blockIdx.y), items, S, T, vec, taps,
                   dg_pick<double>(parts, blockIdx.y), [items](int t, long img, int p, long item) { return t * items + item; });
}

// w_ssim == 0: sums of (x - t)^2 and |x - t| over all `count` values; part: [2][gridDim.x]
__global__ __launch_bounds__(256) void recon_fwd_stream_kernel(const DgPtrs xs, const DgPtrs ts, long count, int vec, const DgPtrs parts) {
    __shared__ double red[2][4];
    const float* __restrict__ x = dg_pick<const float>(xs, blockIdx.y);
    const float* __restrict__ y = dg_pick<const float>(ts, blockIdx.y);
    double* __restrict__ part = dg_pick<double>(parts, blockIdx.y);
    const int t = threadIdx.x;
    double s[2] = {0.0, 0.0};                      // sums of (x - t)^2 and of |x - t|
    const long n4 = count >> 2;
    for (long i = (long)blockIdx.x * 256 + t; i < n4; i += (long)gridDim.x * 256) {
        f32x4 a, b;
        if (vec) {
            a = *(const f32x4*)(x + i * 4);
            b = *(const f32x4*)(y + i * 4);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] = x[i * 4 + j];
                b[j] = y[i * 4 + j];
            }
        }
        const f32x4 d = a - b;
        s[0] += (double)((d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]));
        s[1] += (double)((fabsf(d[0]) + fabsf(d[1])) + (fabsf(d[2]) + fabsf(d[3])));
    }
    if (blockIdx.x == 0 && t == 0)
        for (long e = n4 * 4; e < count; ++e) {
            const float d = x[e] - y[e];
            s[0] += (double)(d * d);
            s[1] += (double)fabsf(d);
        }
    dg_block_stage_d(s, red);
    if (t < 2) part[(long)t * gridDim.x + blockIdx.x] = dg_sum4_pair(red[t]);
}

// part: [nsum][nparts] doubles per problem (nsum = 3 with the SSIM plane, else 2); one block per problem
__global__ __launch_bounds__(256) void recon_final_kernel(const DgPtrs parts, long nparts, int nsum, double inv_px, double inv_win, const RcW w,
                                                          const DgPtrs outs) {
    __shared__ double red[3][4];
    const double* __restrict__ p = dg_pick<const double>(parts, blockIdx.x);
    float* __restrict__ out = dg_pick<float>(outs, blockIdx.x);
    const int t = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (long i = t; i < nparts; i += 256) {
        s[0] += p[i];
        s[1] += p[nparts + i];
        if (nsum == 3) s[2] += p[2 * nparts + i];
    }
    dg_block_stage_d(s, red);
    if (t == 0) {
        double v = 0.0;
        if (w.mse > 0.f) v += (double)w.mse * (dg_sum4_pair(red[0]) * inv_px);
        if (w.l1 > 0.f) v += (double)w.l1 * (dg_sum4_pair(red[1]) * inv_px);
        if (w.ssim > 0.f) v += (double)w.ssim * (1.0 - dg_sum4_pair(red[2]) * inv_win);
        out[0] = (float)v;
    }
}

// gout ( w_mse 2 (x - t) / N + w_l1 sign(x - t) / N - w_ssim g ), in double, rounded once; k*: the three factors with gout folded in
__device__ __forceinline__ float recon_combine(float xv, float tv, float g, const RcW& w, double kmse, double kl1, double kss) {
    const double d = (double)xv - (double)tv;
    double v = 0.0;
    if (w.mse > 0.f) v += d * kmse;
    if (w.l1 > 0.f) v += (d != d ? d : (d > 0.0 ? kl1 : (d < 0.0 ? -kl1 : 0.0)));
    if (w.ssim > 0.f) v -= kss * (double)g;
    return (float)v;
}

__global__ __launch_bounds__(256) void recon_bwd_stream_kernel(const DgPtrs xs, const DgPtrs ts, const DgPtrs gouts, const DgPtrs dxs, long count,
                                                               int vec, const RcW w, double inv_px) {
    const float* __restrict__ x = dg_pick<const float>(xs, blockIdx.y);
    const float* __restrict__ y = dg_pick<const float>(ts, blockIdx.y);
    const float* __restrict__ gout = dg_pick<const float>(gouts, blockIdx.y);
    float* __restrict__ dx = dg_pick<float>(dxs, blockIdx.y);
    const double go = (double)gout[0];
    const double kmse = go * (double)w.mse * 2.0 * inv_px, kl1 = go * (double)w.l1 * inv_px;
    const long n4 = count >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        f32x4 a, b, r;
        if (vec) {
            a = *(const f32x4*)(x + i * 4);
            b = *(const f32x4*)(y + i * 4);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a[j] = x[i * 4 + j];
                b[j] = y[i * 4 + j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = recon_combine(a[j], b[j], 0.f, w, kmse, kl1, 0.0);
        if (vec) {
            *(f32x4*)(dx + i * 4) = r;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) dx[i * 4 + j] = r[j];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long e = n4 * 4; e < count; ++e) dx[e] = recon_combine(x[e], y[e], 0.f, w, kmse, kl1, 0.0);
}

__global__ __launch_bounds__(BT) void recon_bwd_tile_kernel(const DgPtrs xs, const DgPtrs ts, const DgPtrs gouts, const DgPtrs dxs, long items, int S,
                                                            int T, int vec, const SsimTaps taps, const RcW w, double inv_px, double inv_win) {
    __shared__ __attribute__((aligned(16))) float sx[BH * BP];
    __shared__ __attribute__((aligned(16))) float sy[BH * BP];
    __shared__ __attribute__((aligned(16))) float hp[5][BH * BC];      // horizontal moment planes: 52 rows x 42 corner columns
    __shared__ float cm[3][BC * BC];                                  // coefficient maps a, b, c over the 42 x 42 corners
    float* const hq = &hp[0][0];                                      // adjoint horizontal planes [3][42 x 32], once hp has been read
    const float* __restrict__ x = dg_pick<const float>(xs, blockIdx.y);
    const float* __restrict__ y = dg_pick<const float>(ts, blockIdx.y);
    const float* __restrict__ gout = dg_pick<const float>(gouts, blockIdx.y);
    float* __restrict__ dx = dg_pick<float>(dxs, blockIdx.y);
    const int t = threadIdx.x;
    const long plane = (long)S * S;
    const int P = 3 * T * T;
    const int nvalid = S - (RK - 1);
    const double go = (double)gout[0];
    const double kmse = go * (double)w.mse * 2.0 * inv_px, kl1 = go * (double)w.l1 * inv_px, kss = go * (double)w.ssim * inv_win;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long img = item / P;
        const int p = (int)(item - img * P);
        const int ch = p / (T * T), tt = p - ch * T * T;
        const int gy0 = (tt / T) * RT, gx0 = (tt % T) * RT;
        const long base = (img * 3 + ch) * plane;
        __syncthreads();                           // the previous item's LDS reads are done
        // 1. halo: rows [gy0 - 10, gy0 + 42), columns [gx0 - 12, gx0 + 44)
        ssim_stage_halo<BT, BH, BP, BY0, BX0>(x + base, y + base, S, gy0, gx0, vec, sx, sy);
        __syncthreads();
        // the tile's constants: the pixel at the tile's centre, clamped into the image
        const int cr = min(gy0 + RT / 2, S - 1) - gy0 + BY0, cc = min(gx0 + RT / 2, S - 1) - gx0 + BX0;
        const float cx = sx[cr * BP + cc], cy = sy[cr * BP + cc];
        // 2. horizontal pass: corner column cj (global gx0 - 10 + cj) starts at halo column cj + 2
        ssim_hpass<BT, BH, BC, BP, BX0 - BY0>(sx, sy, cx, cy, taps, hp);
        __syncthreads();
        // 3. vertical pass and the coefficient maps; a corner outside the valid range contributes nothing
        for (int i = t; i < BC * BC; i += BT) {
            const int ci = i / BC, cj = i - ci * BC;
            const int gr = gy0 - BY0 + ci, gc = gx0 - BY0 + cj;
            float ca = 0.f, cb = 0.f, cq = 0.f;
            if (gr >= 0 && gr < nvalid && gc >= 0 && gc < nvalid) {
                const SsimMoments m = ssim_vpass<BH, BC>(hp, ci, cj, taps);
                const SsimTerms s = ssim_terms(m, cx, cy);
                const float r12 = 1.f / (s.B1 * s.B2);
                const float sv = s.A1 * s.A2 * r12;                   // the window's SSIM
                const float dmu = 2.f * s.my * s.A2 * r12 - 2.f * s.mx * sv / s.B1;
                const float dsig = -sv / s.B2;
                const float dc = 2.f * s.A1 * r12;
                ca = dmu - 2.f * m.m0 * dsig - m.m1 * dc;
                cb = 2.f * dsig;
                cq = dc;
            }
            cm[0][i] = ca; cm[1][i] = cb; cm[2][i] = cq;
        }
        __syncthreads();                           // hp is read; hq takes its place
        // 4. adjoint horizontal pass: output column c (global gx0 + c) lies in the corners cj = c .. c + 10 with weight g[c + 10 - cj]
        for (int i = t; i < BC * RT; i += BT) {
            const int ci = i >> 5, c = i & 31;
            const int o = ci * BC + c;
            float q0 = 0.f, q1 = 0.f, q2 = 0.f;
#pragma unroll
            for (int j = 0; j < RK; ++j) {
                const float g = taps.g[RK - 1 - j];
                q0 += g * cm[0][o + j];
                q1 += g * cm[1][o + j];
                q2 += g * cm[2][o + j];
            }
            hq[i] = q0; hq[BC * RT + i] = q1; hq[2 * BC * RT + i] = q2;
        }
        __syncthreads();
        // 5. adjoint vertical pass and the output: two neighbouring pixels per thread
        {
            const int r = t >> 4, c = (t & 15) * 2;
            f32x2 q0 = {0.f, 0.f}, q1 = {0.f, 0.f}, q2 = {0.f, 0.f};
#pragma unroll
            for (int j = 0; j < RK; ++j) {
                const float g = taps.g[RK - 1 - j];
                const int o = (r + j) * RT + c;
                q0 += g * *(const f32x2*)(hq + o);
                q1 += g * *(const f32x2*)(hq + BC * RT + o);
                q2 += g * *(const f32x2*)(hq + 2 * BC * RT + o);
            }
            const int gy = gy0 + r, gx = gx0 + c;
            const int ho = (r + BY0) * BP + c + BX0;
            f32x2 res;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float xv = sx[ho + e], tv = sy[ho + e];
                const float g = q0[e] + (xv - cx) * q1[e] + (tv - cy) * q2[e];
                res[e] = recon_combine(xv, tv, g, w, kmse, kl1, kss);
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
}

extern "C" size_t dg_recon_loss_workspace_bytes(int n, int S) {
    if (n < 1 || S < 1) return 0;
    const size_t tile = (size_t)3 * (size_t)n * (size_t)ssim_tiles(S), stream = (size_t)2 * RC_STREAM_BLOCKS;
    return (tile > stream ? tile : stream) * sizeof(double);
}

// the checks both entry points share; tabs: the pointer tables, each with `groups` non-null entries aligned to `align[i]` bytes
static int recon_check(const char* who, int groups, int n, int S, const float* w, const void* const* const* tabs, const int* align, int ntabs) {
    DG_CHECK_ARG(groups >= 1 && groups <= DG_MAX_GROUPS, "%s: groups=%d (1..%d)", who, groups, DG_MAX_GROUPS);
    DG_CHECK_ARG(w != nullptr, "%s: null weights", who);
    for (int i = 0; i < 3; ++i) DG_CHECK_ARG(isfinite(w[i]) && w[i] >= 0.f, "%s: weight %d = %g must be finite and >= 0", who, i, (double)w[i]);
    DG_CHECK_ARG(w[0] > 0.f || w[1] > 0.f || w[2] > 0.f, "%s: all three weights are 0", who);
    DG_CHECK_ARG(n >= 1 && S >= 1, "%s: n=%d, S=%d", who, n, S);
    DG_CHECK_ARG(w[2] == 0.f || S >= RK, "%s: S %d < %d with the SSIM term on (the window does not fit)", who, S, RK);
    DG_CHECK_ARG(ssim_tiles(S) <= 0x7fffffffL / 3, "%s: S %d is too large", who, S);
    for (int k = 0; k < ntabs; ++k) {
        DG_CHECK_ARG(tabs[k] != nullptr, "%s: null pointer table", who);
        for (int i = 0; i < groups; ++i) {
            DG_CHECK_ARG(tabs[k][i] != nullptr, "%s: null pointer (problem %d)", who, i);
            DG_CHECK_ARG(((uintptr_t)tabs[k][i] & (uintptr_t)(align[k] - 1)) == 0, "%s: pointer of problem %d is not %d-byte aligned", who, i, align[k]);
        }
    }
    return DG_OK;
}

static int recon_vec(int groups, int S, const void* const* a, const void* const* b, const void* const* c) {
    uintptr_t bits = 0;
    for (int i = 0; i < groups; ++i) bits |= (uintptr_t)a[i] | (uintptr_t)b[i] | (c ? (uintptr_t)c[i] : 0);
    return S % 4 == 0 && (bits & 15) == 0;
}

extern "C" int dg_recon_loss_fwd_g(int groups, const float* const* x, const float* const* t, int n, int S, const float* w, float* const* loss,
                                   void* const* ws, size_t ws_bytes, dg_stream_t stream) {
    const void* const* tabs[] = {(const void* const*)x, (const void* const*)t, (const void* const*)loss, (const void* const*)ws};
    const int align[] = {4, 4, 4, 8};
    const int rc = recon_check("dg_recon_loss_fwd", groups, n, S, w, tabs, align, 4);
    if (rc != DG_OK) return rc;
    if (ws_bytes < dg_recon_loss_workspace_bytes(n, S))
        return dg_fail(DG_ERR_WORKSPACE, "dg_recon_loss_fwd: workspace too small (%zu bytes, %zu needed)", ws_bytes, dg_recon_loss_workspace_bytes(n, S));
    const RcW rw = {w[0], w[1], w[2]};
    const long count = (long)n * 3 * S * S;
    const int vec = recon_vec(groups, S, tabs[0], tabs[1], nullptr);
    const DgPtrs px = dg_ptrs(tabs[0], groups), pt = dg_ptrs(tabs[1], groups), pw = dg_ptrs(tabs[3], groups), pl = dg_ptrs(tabs[2], groups);
    hipStream_t st = (hipStream_t)stream;
    if (rw.ssim > 0.f) {
        const int P = (int)ssim_tiles(S), T = (S + RT - 1) / RT;
        const long items = (long)n * P;
        const int win = S - (RK - 1);
        hipLaunchKernelGGL(recon_fwd_tile_kernel, dim3((unsigned)(items < RC_MAX_BLOCKS ? items : RC_MAX_BLOCKS), groups), dim3(256), 0, st, px, pt, items,
                           S, T, vec, ssim_taps(), pw);
        DG_CHECK_LAUNCH("recon_fwd_tile");
        hipLaunchKernelGGL(recon_final_kernel, dim3(groups), dim3(256), 0, st, pw, items, 3, 1.0 / (double)count,
                           1.0 / ((double)n * 3.0 * (double)win * (double)win), rw, pl);
    } else {
        long g = (count / 4 + 255) / 256;
        g = g < 1 ? 1 : (g > RC_STREAM_BLOCKS ? RC_STREAM_BLOCKS : g);
        hipLaunchKernelGGL(recon_fwd_stream_kernel, dim3((unsigned)g, groups), dim3(256), 0, st, px, pt, count, vec, pw);
        DG_CHECK_LAUNCH("recon_fwd_stream");
        hipLaunchKernelGGL(recon_final_kernel, dim3(groups), dim3(256), 0, st, pw, g, 2, 1.0 / (double)count, 0.0, rw, pl);
    }
    DG_CHECK_LAUNCH("recon_final");
    return DG_OK;
}

extern "C" int dg_recon_loss_fwd(const float* x, const float* t, int n, int S, const float* w, float* loss, void* ws, size_t ws_bytes,
                                 dg_stream_t stream) {
    return dg_recon_loss_fwd_g(1, &x, &t, n, S, w, &loss, &ws, ws_bytes, stream);
}

extern "C" int dg_recon_loss_bwd_g(int groups, const float* const* x, const float* const* t, int n, int S, const float* w, const float* const* gout,
                                   float* const* dx, dg_stream_t stream) {
    const void* const* tabs[] = {(const void* const*)x, (const void* const*)t, (const void* const*)gout, (const void* const*)dx};
    const int align[] = {4, 4, 4, 4};
    const int rc = recon_check("dg_recon_loss_bwd", groups, n, S, w, tabs, align, 4);
    if (rc != DG_OK) return rc;
    const RcW rw = {w[0], w[1], w[2]};
    const long count = (long)n * 3 * S * S;
    const int vec = recon_vec(groups, S, tabs[0], tabs[1], tabs[3]);
    const DgPtrs px = dg_ptrs(tabs[0], groups), pt = dg_ptrs(tabs[1], groups), pg = dg_ptrs(tabs[2], groups), pd = dg_ptrs(tabs[3], groups);
    hipStream_t st = (hipStream_t)stream;
    if (rw.ssim > 0.f) {
        const int P = (int)ssim_tiles(S), T = (S + RT - 1) / RT;
        const long items = (long)n * P;
        const int win = S - (RK - 1);
        hipLaunchKernelGGL(recon_bwd_tile_kernel, dim3((unsigned)(items < RC_MAX_BLOCKS ? items : RC_MAX_BLOCKS), groups), dim3(BT), 0, st, px, pt, pg, pd,
                           items, S, T, vec, ssim_taps(), rw, 1.0 / (double)count, 1.0 / ((double)n * 3.0 * (double)win * (double)win));
        DG_CHECK_LAUNCH("recon_bwd_tile");
    } else {
        long g = (count / 4 + 255) / 256;
        g = g < 1 ? 1 : (g > 2 * RC_STREAM_BLOCKS ? 2 * RC_STREAM_BLOCKS : g);
        hipLaunchKernelGGL(recon_bwd_stream_kernel, dim3((unsigned)g, groups), dim3(256), 0, st, px, pt, pg, pd, count, vec, rw, 1.0 / (double)count);
        DG_CHECK_LAUNCH("recon_bwd_stream");
    }
    return DG_OK;
}

extern "C" int dg_recon_loss_bwd(const float* x, const float* t, int n, int S, const float* w, const float* gout, float* dx, dg_stream_t stream) {
    return dg_recon_loss_bwd_g(1, &x, &t, n, S, w, &gout, &dx, stream);
}
