// The SSIM tile stencil (internal): the one text behind dg_image_metrics (metrics.hip) and both directions of dg_recon_loss (recon.hip),
// so that "the SSIM of the reconstruction loss is the SSIM of the metrics" holds by construction (tests/test_recon_gpu.py pins it).
//
// Window: 11 taps, the sigma 1.5 Gaussian normalised in double on the host and rounded once to fp32; C1 = 0.01^2, C2 = 0.03^2 (data
// range 1); "valid" corners only (row, column <= S - 11).  One work item = one 32 x 32 tile of one channel of one image, P = 3 T^2
// items per image, T = ceil(S / 32).  The steps, each a function of its geometry:
//   ssim_stage_halo   rows [gy0 - Y0, +ROWS) x columns [gx0 - X0, +PITCH) of x and y into LDS, in quads: 16-byte loads when `vec` (S % 4
//                     == 0 and 16-byte aligned batches: a quad is then inside or outside the image as a whole), scalar loads otherwise;
//                     0 outside the image (such pixels feed skipped corners only).
//   ssim_hpass        horizontal 11-tap pass -> five moment planes (x', y', x'^2, y'^2, x'y') of ROWS x COLS in LDS.
//   ssim_vpass        vertical 11-tap pass: the five moments of one window corner.
//   ssim_terms        the four factors A1 = 2 mx my + C1, A2 = 2 sxy + C2, B1 = mx^2 + my^2 + C1, B2 = sx2 + sy2 + C2 of a corner.
// The moments are taken about per-tile constants: x' = x - cx, cx = one pixel of the tile (which one is the calling kernel's choice, and
// its bits depend on it), likewise y.  Variances and the covariance do not depend on the constant, mx = cx + sum w x'; on a nearly flat
// region x'^2 is tiny, where the plain sum w x^2 - mx^2 cancels to the rounding error of a value near x^2.  |x'| <= 1 for data in [0, 1]:
// never worse than the plain form.  Every 32-lane group reads one consecutive run of an LDS row in both passes (no bank conflict at any
// pitch).  fp32 throughout; the callers go to fp64 from the wave sum on.
//
// ssim_fwd_tiles is the forward tile body both forward kernels run: a 256-thread block
//   1. stages the 42 x 42 halo of x and y (pitch 44: 2 x 7392 B);
//   2. sums its own pixels' (x - y)^2 and |x - y|: 4 per thread, pairwise in fp32;
//   3. horizontal pass about the pixel at the halo's centre (clamped into the image) -> 42 x 32 planes (26880 B);
//   4. vertical pass + the quotient A1 A2 / (B1 B2): 4 corners per thread, summed in fp32;
//   5. block sums in fp64 -> the three partials of the item, stored where the caller's index says.
// 41664 B of LDS + 96 B of reduction scratch: three blocks per CU.
#pragma once
#include "dg_common.h"
#include <math.h>

#define SSIM_T 32                       // tile side
#define SSIM_K 11                       // window taps
#define SSIM_C (SSIM_T + SSIM_K - 1)    // window corners (and forward halo side) per axis of a tile: 42

struct SsimTaps {
    float g[SSIM_K];
};

static SsimTaps ssim_taps(void) {
    SsimTaps taps;
    double g[SSIM_K], sum = 0.0;
    for (int k = 0; k < SSIM_K; ++k) {
        const double d = k - SSIM_K / 2;
        g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += g[k];
    }
    for (int k = 0; k < SSIM_K; ++k) taps.g[k] = (float)(g[k] / sum);
    return taps;
}

// work items per image
static long ssim_tiles(int S) {
    const long T = ((long)S + SSIM_T - 1) / SSIM_T;
    return 3 * T * T;
}

template <int THREADS, int ROWS, int PITCH, int Y0, int X0>
__device__ __forceinline__ void ssim_stage_halo(const float* __restrict__ bx, const float* __restrict__ by, int S, int gy0, int gx0, int vec,
                                                float* sx, float* sy) {
    constexpr int Q = PITCH / 4;
    for (int i = threadIdx.x; i < ROWS * Q; i += THREADS) {
        const int r = i / Q, q = i - r * Q;
        const int gy = gy0 - Y0 + r, gx = gx0 - X0 + 4 * q;
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if ((Y0 == 0 || gy >= 0) && gy < S) {
            const long o = (long)gy * S + gx;
            if (vec) {
                if ((X0 == 0 || gx >= 0) && gx + 3 < S) {
                    a = *(const f32x4*)(bx + o);
                    b = *(const f32x4*)(by + o);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((X0 == 0 || gx + j >= 0) && gx + j < S) {
                        a[j] = bx[o + j];
                        b[j] = by[o + j];
                    }
            }
        }
        *(f32x4*)(sx + r * PITCH + 4 * q) = a;
        *(f32x4*)(sy + r * PITCH + 4 * q) = b;
    }
}

// plane column c starts at halo column c + XOFF
template <int THREADS, int ROWS, int COLS, int PITCH, int XOFF>
__device__ __forceinline__ void ssim_hpass(const float* sx, const float* sy, float cx, float cy, const SsimTaps& taps, float (*hp)[ROWS * COLS]) {
    for (int i = threadIdx.x; i < ROWS * COLS; i += THREADS) {
        const int r = i / COLS, c = i - r * COLS;
        const int o = r * PITCH + c + XOFF;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_K; ++k) {
            const float w = taps.g[k];
            const float a = sx[o + k] - cx, b = sy[o + k] - cy;
            m0 += w * a;
            m1 += w * b;
            m2 += w * (a * a);
            m3 += w * (b * b);
            m4 += w * (a * b);
        }
        hp[0][i] = m0; hp[1][i] = m1; hp[2][i] = m2; hp[3][i] = m3; hp[4][i] = m4;
    }
}

struct SsimMoments {
    float m0, m1, m2, m3, m4;           // sum w x', sum w y', sum w x'^2, sum w y'^2, sum w x'y'
};

// the window whose corner is row r, column c of the planes
template <int ROWS, int COLS>
__device__ __forceinline__ SsimMoments ssim_vpass(const float (*hp)[ROWS * COLS], int r, int c, const SsimTaps& taps) {
    SsimMoments m = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < SSIM_K; ++k) {
        const float w = taps.g[k];
        const int o = (r + k) * COLS + c;
        m.m0 += w * hp[0][o];
        m.m1 += w * hp[1][o];
        m.m2 += w * hp[2][o];
        m.m3 += w * hp[3][o];
        m.m4 += w * hp[4][o];
    }
    return m;
}

struct SsimTerms {
    float mx, my, A1, A2, B1, B2;
};

__device__ __forceinline__ SsimTerms ssim_terms(const SsimMoments& m, float cx, float cy) {
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    SsimTerms s;
    s.mx = cx + m.m0;
    s.my = cy + m.m1;
    const float vx = m.m2 - m.m0 * m.m0, vy = m.m3 - m.m1 * m.m1, cxy = m.m4 - m.m0 * m.m1;
    s.A1 = 2.f * s.mx * s.my + C1;
    s.A2 = 2.f * cxy + C2;
    s.B1 = s.mx * s.mx + s.my * s.my + C1;
    s.B2 = vx + vy + C2;
    return s;
}

// x, y: one problem's batches; the block strides over the `items` tiles; part[at(t, img, p, item)], t = 0, 1, 2, takes the item's sums of
// (x - y)^2, |x - y| and the SSIM quotient (img = item / P, p = item % P)
template <typename PartAt>
__device__ __forceinline__ void ssim_fwd_tiles(const float* __restrict__ x, const float* __restrict__ y, long items, int S, int T, int vec,
                                               const SsimTaps& taps, double* __restrict__ part, PartAt at) {
    constexpr int PITCH = 44;           // halo pitch (whole quads)
    __shared__ __attribute__((aligned(16))) float sx[SSIM_C * PITCH];
    __shared__ __attribute__((aligned(16))) float sy[SSIM_C * PITCH];
    __shared__ float hp[5][SSIM_C * SSIM_T];
    __shared__ double red[3][4];
    const int t = threadIdx.x;
    const long plane = (long)S * S;
    const int P = 3 * T * T;
    const int nvalid = S - (SSIM_K - 1);           // valid corners per axis
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long img = item / P;
        const int p = (int)(item - img * P);
        const int ch = p / (T * T), tt = p - ch * T * T;
        const int gy0 = (tt / T) * SSIM_T, gx0 = (tt % T) * SSIM_T;
        __syncthreads();                           // the previous item's LDS reads are done
        ssim_stage_halo<256, SSIM_C, PITCH, 0, 0>(x + (img * 3 + ch) * plane, y + (img * 3 + ch) * plane, S, gy0, gx0, vec, sx, sy);
        __syncthreads();
        float e2[4], e1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = t + 256 * j, r = i >> 5, c = i & 31;
            const bool in = gy0 + r < S && gx0 + c < S;
            const float d = sx[r * PITCH + c] - sy[r * PITCH + c];
            e2[j] = in ? d * d : 0.f;
            e1[j] = in ? fabsf(d) : 0.f;
        }
        const float sse = (e2[0] + e2[1]) + (e2[2] + e2[3]);
        const float sae = (e1[0] + e1[1]) + (e1[2] + e1[3]);
        const int cr = min(SSIM_C / 2, S - 1 - gy0), cc = min(SSIM_C / 2, S - 1 - gx0);
        const float cx = sx[cr * PITCH + cc], cy = sy[cr * PITCH + cc];
        ssim_hpass<256, SSIM_C, SSIM_T, PITCH, 0>(sx, sy, cx, cy, taps, hp);
        __syncthreads();
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = t + 256 * j, r = i >> 5, c = i & 31;
            if (gy0 + r < nvalid && gx0 + c < nvalid) {
                const SsimTerms s = ssim_terms(ssim_vpass<SSIM_C, SSIM_T>(hp, r, c, taps), cx, cy);
                ss += (s.A1 * s.A2) / (s.B1 * s.B2);
            }
        }
        double sums[3] = {(double)sse, (double)sae, (double)ss};
        dg_block_stage_d(sums, red);
        if (t < 3) part[at(t, img, p, item)] = dg_sum4_pair(red[t]);
    }
}
