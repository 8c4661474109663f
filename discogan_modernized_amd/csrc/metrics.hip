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
// in the same square that are valid (row, column <= S - 11).  The tile kernel is ssim_tile.h's forward body (halo, own pixels, the two
// 11-tap passes about a per-tile constant, fp64 block sums; its LDS budget and the reasons are written there) with the three fp64
// partials of an item stored at [pair][3][P].
// A second kernel sums the P partials of each pair in a fixed order (thread t: t, t + 256, ...; wave; four waves), divides, rounds to fp32.
// No atomics; two calls give the same bits; the partial layout [n][3][P] depends on S only, so row i is the same bits at any n and
// next to any other images; a NaN / inf stays in its own pair's partials.
//
// Grid cap: both kernels launch at most METRICS_MAX_BLOCKS = 8192 blocks and stride over the n P items (the n pairs).
// fp32 chain before the fp64 hand-over: 4 terms per thread and item, summed pairwise.  MSE: two roundings from the subtraction (it is
// squared), one from the square, two additions, the result's rounding to fp32: k = 4 + 2 = 6, error <= gamma(6) * MSE; MAE fewer.
#include "ssim_tile.h"

#define METRICS_MAX_BLOCKS 8192

__global__ __launch_bounds__(256) void image_metrics_tile_kernel(const float* __restrict__ x, const float* __restrict__ y, long items, int S,
                                                                 int T, int vec, const SsimTaps taps, double* __restrict__ part) {
    const int P = 3 * T * T;
    ssim_fwd_tiles(x, y, items, S, T, vec, taps, part, [P](int t, long img, int p, long item) { return (img * 3 + t) * P + p; });
}

__global__ __launch_bounds__(256) void image_metrics_final_kernel(const double* __restrict__ part, long n, int P, double inv_px, double inv_win,
                                                                  float* __restrict__ out) {
    __shared__ double red[3][4];
    const int t = threadIdx.x;
    for (long img = blockIdx.x; img < n; img += gridDim.x) {
        const double* p = part + img * 3 * P;
        double s[3] = {0.0, 0.0, 0.0};
        for (int i = t; i < P; i += 256) {
            s[0] += p[i];
            s[1] += p[P + i];
            s[2] += p[2 * P + i];
        }
        dg_block_stage_d(s, red);
        if (t < 3) out[img * 3 + t] = (float)(dg_sum4_pair(red[t]) * (t < 2 ? inv_px : inv_win));
    }
}

extern "C" size_t dg_image_metrics_workspace_bytes(int n, int S) {
    if (n < 1 || S < SSIM_K) return 0;
    return (size_t)n * 3 * (size_t)ssim_tiles(S) * sizeof(double);
}

extern "C" int dg_image_metrics(const float* x, const float* y, int n, int S, float* out, void* ws, size_t ws_bytes, dg_stream_t s) {
    DG_CHECK_ARG(x != nullptr && y != nullptr, "dg_image_metrics: null batch pointer");
    DG_CHECK_ARG(out != nullptr, "dg_image_metrics: null out");
    DG_CHECK_ARG(n >= 1, "dg_image_metrics: n %d < 1", n);
    DG_CHECK_ARG(S >= SSIM_K, "dg_image_metrics: S %d < %d (the window does not fit)", S, SSIM_K);
    DG_CHECK_ARG(ssim_tiles(S) <= 0x7fffffffL / 3, "dg_image_metrics: S %d is too large", S);
    DG_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0, "dg_image_metrics: batches must be 4-byte aligned");
    if (ws == nullptr || ws_bytes < dg_image_metrics_workspace_bytes(n, S))
        return dg_fail(DG_ERR_WORKSPACE, "dg_image_metrics: workspace too small (%zu bytes, %zu needed)", ws_bytes,
                       dg_image_metrics_workspace_bytes(n, S));
    DG_CHECK_ARG(((uintptr_t)ws & 7) == 0, "dg_image_metrics: the workspace must be 8-byte aligned");
    const int P = (int)ssim_tiles(S), T = (S + SSIM_T - 1) / SSIM_T;
    const long items = (long)n * P;
    const int vec = (S % 4 == 0) && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    const int win = S - (SSIM_K - 1);
    hipStream_t st = (hipStream_t)s;
    hipLaunchKernelGGL(image_metrics_tile_kernel, dim3((unsigned)(items < METRICS_MAX_BLOCKS ? items : METRICS_MAX_BLOCKS)), dim3(256), 0, st, x, y,
                       items, S, T, vec, ssim_taps(), (double*)ws);
    DG_CHECK_LAUNCH("image_metrics_tile");
    hipLaunchKernelGGL(image_metrics_final_kernel, dim3((unsigned)(n < METRICS_MAX_BLOCKS ? n : METRICS_MAX_BLOCKS)), dim3(256), 0, st,
                       (const double*)ws, (long)n, P, 1.0 / (3.0 * (double)S * (double)S), 1.0 / (3.0 * (double)win * (double)win), out);
    DG_CHECK_LAUNCH("image_metrics_final");
    return DG_OK;
}
