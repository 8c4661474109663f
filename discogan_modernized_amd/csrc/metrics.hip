// Held-out image metrics on the device: per image pair MSE, MAE and SSIM (Wang et al. 2004) of two float NCHW batches [n][3][S][S].
// The reference has no counterpart (its quality signal is the RECON: field of the log line); evaluate.py turns the rows into PSNR etc.
//
//   out[i][0] = mean (x - y)^2, out[i][1] = mean |x - y| over the 3 S^2 values of pair i (no clamp, no quantisation: data range L = 1)
//   out[i][2] = mean over 3 channels x (S - 10)^2 "valid" window corners of
//               (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sx2 + sy2 + C2)),  C1 = 0.01^2, C2 = 0.03^2,
//               mx = sum w x, sx2 = sum w x^2 - mx^2, sxy = sum w x y - mx my, w = g[i] g[j], g = the 11-tap sigma 1.5 Gaussian
//               (normalised in double on the host, rounded once to fp32)
//
// Geometry.  One work item = one 32 x 32 tile of one channel of one pair: P = 3 T^2 items per pair, T = ceil(S / 32).  Tiles cover the
// INPUT domain: item (ch, ty, tx) owns the pixels [32 ty, +32) x [32 tx, +32) (their (x - y)^2 and |x - y| sums) and the window corners
// in the same square that are valid (row, column <= S - 11).  A 256-thread block
//   1. stages the 42 x 42 halo of x and y in LDS (pitch 44: 2 x 7392 B; pixels outside the image are 0 and feed skipped corners only):
//      16-byte loads when S % 4 == 0 and both batches are 16-byte aligned (a tile row then starts on a 16-byte line), else scalar loads;
//   2. sums its own pixels: 4 per thread, pairwise in fp32;
//   3. horizontal 11-tap pass -> five moment planes (x', y', x'^2, y'^2, x'y') of 42 x 32 in LDS (26880 B);
//   4. vertical 11-tap pass + the map: 4 corners per thread, summed in fp32;
//   5. block sum in fp64 from the wave sum on (the convention of loss.hip) -> three fp64 partials of this item in the workspace.
// 41664 B of LDS + 96 B of reduction scratch: three blocks per CU.  Every 32-lane group reads one consecutive run of an LDS row in
// both passes (no bank conflict at any pitch).
// The moments are taken about a per-tile constant: x' = x - cx, cx = the pixel at the halo's centre (clamped into the image), likewise
// y.  Variances and the covariance do not depend on the constant, mx = cx + sum w x'; on a nearly flat region x'^2 is tiny, where the
// plain sum w x^2 - mx^2 cancels to the rounding error of a value near x^2.  |x'| <= 1 for data in [0, 1]: never worse than the plain form.
// A second kernel sums the P partials of each pair in a fixed order (thread t: t, t + 256, ...; wave; four waves), divides, rounds to fp32.
// No atomics; two calls give the same bits; the partial layout [n][3][P] depends on S only, so row i is the same bits at any n and
// next to any other images; a NaN / inf stays in its own pair's partials.
//
// Grid cap: both kernels launch at most METRICS_MAX_BLOCKS = 8192 blocks and stride over the n P items (the n pairs).
// fp32 chain before the fp64 hand-over: 4 terms per thread and item, summed pairwise.  MSE: two roundings from the subtraction (it is
// squared), one from the square, two additions, the result's rounding to fp32: k = 4 + 2 = 6, error <= gamma(6) * MSE; MAE fewer.
#include "dg_common.h"

#define METRICS_MAX_BLOCKS 8192
#define MT 32                 // tile side
#define MK 11                 // window taps
#define MH (MT + MK - 1)      // halo side: 42
#define MP 44                 // halo pitch (whole quads)
#define MQ (MP / 4)           // quads per halo row: 11

struct MetricsTaps {
    float g[MK];
};

__global__ __launch_bounds__(256) void image_metrics_tile_kernel(const float* __restrict__ x, const float* __restrict__ y, long items, int S,
                                                                 int T, int vec, const MetricsTaps taps, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sx[MH * MP];
    __shared__ __attribute__((aligned(16))) float sy[MH * MP];
    __shared__ float hp[5][MH * MT];
    __shared__ double red[3][4];
    const int t = threadIdx.x;
    const long plane = (long)S * S;
    const int P = 3 * T * T;
    const int nvalid = S - (MK - 1);               // valid corners per axis
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const long img = item / P;
        const int p = (int)(item - img * P);
        const int ch = p / (T * T), tt = p - ch * T * T;
        const int gy0 = (tt / T) * MT, gx0 = (tt % T) * MT;
        const float* bx = x + (img * 3 + ch) * plane;
        const float* by = y + (img * 3 + ch) * plane;
        __syncthreads();                           // the previous item's LDS reads are done
        // 1. halo
        for (int i = t; i < MH * MQ; i += 256) {
            const int r = i / MQ, q = i - r * MQ;
            const int gy = gy0 + r, gx = gx0 + 4 * q;
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (gy < S) {
                const long o = (long)gy * S + gx;
                if (vec) {
                    if (gx + 3 < S) {              // S % 4 == 0: a quad is inside or outside as a whole
                        a = *(const f32x4*)(bx + o);
                        b = *(const f32x4*)(by + o);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (gx + j < S) {
                            a[j] = bx[o + j];
                            b[j] = by[o + j];
                        }
                }
            }
            *(f32x4*)(sx + r * MP + 4 * q) = a;
            *(f32x4*)(sy + r * MP + 4 * q) = b;
        }
        __syncthreads();
        // 2. this tile's own pixels
        float e2[4], e1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = t + 256 * j, r = i >> 5, c = i & 31;
            const bool in = gy0 + r < S && gx0 + c < S;
            const float d = sx[r * MP + c] - sy[r * MP + c];
            e2[j] = in ? d * d : 0.f;
            e1[j] = in ? fabsf(d) : 0.f;
        }
        const float sse = (e2[0] + e2[1]) + (e2[2] + e2[3]);
        const float sae = (e1[0] + e1[1]) + (e1[2] + e1[3]);
        // 3. horizontal pass about the tile's constants
        const int cr = min(MH / 2, S - 1 - gy0), cc = min(MH / 2, S - 1 - gx0);
        const float cx = sx[cr * MP + cc], cy = sy[cr * MP + cc];
        for (int i = t; i < MH * MT; i += 256) {
            const int r = i >> 5, c = i & 31;
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int k = 0; k < MK; ++k) {
                const float w = taps.g[k];
                const float a = sx[r * MP + c + k] - cx, b = sy[r * MP + c + k] - cy;
                m0 += w * a;
                m1 += w * b;
                m2 += w * (a * a);
                m3 += w * (b * b);
                m4 += w * (a * b);
            }
            hp[0][i] = m0; hp[1][i] = m1; hp[2][i] = m2; hp[3][i] = m3; hp[4][i] = m4;
        }
        __syncthreads();
        // 4. vertical pass and the map
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = t + 256 * j, r = i >> 5, c = i & 31;
            if (gy0 + r < nvalid && gx0 + c < nvalid) {
                float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
                for (int k = 0; k < MK; ++k) {
                    const float w = taps.g[k];
                    const int o = (r + k) * MT + c;
                    m0 += w * hp[0][o];
                    m1 += w * hp[1][o];
                    m2 += w * hp[2][o];
                    m3 += w * hp[3][o];
                    m4 += w * hp[4][o];
                }
                const float mx = cx + m0, my = cy + m1;
                const float vx = m2 - m0 * m0, vy = m3 - m1 * m1, cxy = m4 - m0 * m1;
                ss += ((2.f * mx * my + C1) * (2.f * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2));
            }
        }
        // 5. block sums, fp64 from here on
        const double d0 = dg_wave_sum_d((double)sse), d1 = dg_wave_sum_d((double)sae), d2 = dg_wave_sum_d((double)ss);
        if ((t & 63) == 0) {
            red[0][t >> 6] = d0;
            red[1][t >> 6] = d1;
            red[2][t >> 6] = d2;
        }
        __syncthreads();
        if (t < 3) part[(img * 3 + t) * P + p] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
    }
}

__global__ __launch_bounds__(256) void image_metrics_final_kernel(const double* __restrict__ part, long n, int P, double inv_px, double inv_win,
                                                                  float* __restrict__ out) {
    __shared__ double red[3][4];
    const int t = threadIdx.x;
    for (long img = blockIdx.x; img < n; img += gridDim.x) {
        const double* p = part + img * 3 * P;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int i = t; i < P; i += 256) {
            s0 += p[i];
            s1 += p[P + i];
            s2 += p[2 * P + i];
        }
        s0 = dg_wave_sum_d(s0);
        s1 = dg_wave_sum_d(s1);
        s2 = dg_wave_sum_d(s2);
        __syncthreads();                           // the previous image's sums are read
        if ((t & 63) == 0) {
            red[0][t >> 6] = s0;
            red[1][t >> 6] = s1;
            red[2][t >> 6] = s2;
        }
        __syncthreads();
        if (t < 3) out[img * 3 + t] = (float)(((red[t][0] + red[t][1]) + (red[t][2] + red[t][3])) * (t < 2 ? inv_px : inv_win));
    }
}

static long metrics_tiles(int S) {
    const long T = ((long)S + MT - 1) / MT;
    return 3 * T * T;
}

extern "C" size_t dg_image_metrics_workspace_bytes(int n, int S) {
    if (n < 1 || S < MK) return 0;
    return (size_t)n * 3 * (size_t)metrics_tiles(S) * sizeof(double);
}

extern "C" int dg_image_metrics(const float* x, const float* y, int n, int S, float* out, void* ws, size_t ws_bytes, dg_stream_t s) {
    DG_CHECK_ARG(x != nullptr && y != nullptr, "dg_image_metrics: null batch pointer");
    DG_CHECK_ARG(out != nullptr, "dg_image_metrics: null out");
    DG_CHECK_ARG(n >= 1, "dg_image_metrics: n %d < 1", n);
    DG_CHECK_ARG(S >= MK, "dg_image_metrics: S %d < %d (the window does not fit)", S, MK);
    DG_CHECK_ARG(metrics_tiles(S) <= 0x7fffffffL / 3, "dg_image_metrics: S %d is too large", S);
    DG_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0, "dg_image_metrics: batches must be 4-byte aligned");
    if (ws == nullptr || ws_bytes < dg_image_metrics_workspace_bytes(n, S))
        return dg_fail(DG_ERR_WORKSPACE, "dg_image_metrics: workspace too small (%zu bytes, %zu needed)", ws_bytes,
                       dg_image_metrics_workspace_bytes(n, S));
    DG_CHECK_ARG(((uintptr_t)ws & 7) == 0, "dg_image_metrics: the workspace must be 8-byte aligned");
    MetricsTaps taps;
    double g[MK], sum = 0.0;
    for (int k = 0; k < MK; ++k) {
        const double d = k - MK / 2;
        g[k] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += g[k];
    }
    for (int k = 0; k < MK; ++k) taps.g[k] = (float)(g[k] / sum);
    const int P = (int)metrics_tiles(S), T = (S + MT - 1) / MT;
    const long items = (long)n * P;
    const int vec = (S % 4 == 0) && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    const int win = S - (MK - 1);
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(image_metrics_tile_kernel, dim3((unsigned)(items < METRICS_MAX_BLOCKS ? items : METRICS_MAX_BLOCKS)), dim3(256), 0, st, x, y,
                       items, S, T, vec, taps, (double*)ws);
    DG_CHECK_LAUNCH("image_metrics_tile");
    hipLaunchKernelGGL(image_metrics_final_kernel, dim3((unsigned)(n < METRICS_MAX_BLOCKS ? n : METRICS_MAX_BLOCKS)), dim3(256), 0, st,
                       (const double*)ws, (long)n, P, 1.0 / (3.0 * (double)S * (double)S), 1.0 / (3.0 * (double)win * (double)win), out);
    DG_CHECK_LAUNCH("image_metrics_final");
    return DG_OK;
}
