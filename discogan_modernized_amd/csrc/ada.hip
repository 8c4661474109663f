// Adaptive discriminator augmentation (Karras et al., NeurIPS 2020, "Training Generative Adversarial Networks with Limited Data"): the
// probability p of every stage of the differentiable augmentation, the overfitting measure r_t = E[sign(D(real) - threshold)] and the
// controller that moves p towards a target r_t, all in device memory.  include/discogan_hip.h ("adaptive discriminator augmentation")
// defines the state, the gate words and the order of the controller's operations; tests/ada_ref.py restates them in numpy.
//
// Three kernels, none of them a hot path.  diffaug_draw_p_kernel is diffaug.hip's draw with each stage of a sample kept with probability
// (float)*p, read from device memory by the kernel.  ada_accumulate_kernel adds the signs of one batch of discriminator outputs to a
// window: ONE block, integer partials, a fixed tree, no atomics.  ada_update_kernel closes a window: one lane.
#include "dg_common.h"

// ---- the draw's generator, as in diffaug.hip (one text each: a table drawn here with p = 1 is dg_diffaug_draw's bit for bit) ---------
__host__ __device__ __forceinline__ uint64_t ada_mix(uint64_t z) {       // the SplitMix64 output function
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
#define ADA_G 0x9E3779B97F4A7C15ull
#define ADA_DIFF_LINK 0x6469666600000000ull       // "diff": the link of dg_diffaug_draw's key
#define ADA_GATE_LINK 0x6164610000000000ull       // "ada": one more link behind it, for the gate words
#define ADA_MAX_BATCH 4096                        // DG_DIFFAUG_MAX_BATCH
#define ADA_MAX_SIZE 32768                        // DG_DIFFAUG_MAX_SIZE
#define ADA_MAX_OUTPUTS 65536                     // values of one dg_ada_accumulate call

static inline int ada_T(int S) { return (S + 4) / 8; }                    // floor(S / 8 + 0.5)
__device__ __forceinline__ int ada_cs(int S) { return (S + 1) / 2; }      // floor(S / 2 + 0.5)
__device__ __forceinline__ int ada_range(uint32_t w, int lo, uint32_t count) { return lo + (int)(((uint64_t)w * count) >> 32); }
__device__ __forceinline__ float ada_unit(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }

__global__ __launch_bounds__(256) void diffaug_draw_p_kernel(uint64_t key, uint64_t key2, int n, int S, int T, int flags,
                                                             const double* __restrict__ p_dev, int* __restrict__ recs) {
    const float p = (float)*p_dev;                                      // one rounding; u < p: p = 1 keeps every stage, p = 0 (or NaN) none
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        const uint64_t q1 = ada_mix(key + ADA_G * (4ull * (uint64_t)j + 1ull)), q2 = ada_mix(key + ADA_G * (4ull * (uint64_t)j + 2ull));
        const uint64_t q3 = ada_mix(key + ADA_G * (4ull * (uint64_t)j + 3ull)), q4 = ada_mix(key + ADA_G * (4ull * (uint64_t)j + 4ull));
        const uint64_t g1 = ada_mix(key2 + ADA_G * (2ull * (uint64_t)j + 1ull)), g2 = ada_mix(key2 + ADA_G * (2ull * (uint64_t)j + 2ull));
        const bool keep_color = ada_unit((uint32_t)(g1 >> 32)) < p, keep_trans = ada_unit((uint32_t)g1) < p;
        const bool keep_cut = ada_unit((uint32_t)(g2 >> 32)) < p;
        int4 a, b;
        a.x = a.y = a.z = a.w = 0;
        float fb = 0.0f, fs = 1.0f, fc = 1.0f;
        if ((flags & DG_DIFFAUG_COLOR) && keep_color) {
            fb = (ada_unit((uint32_t)(q1 >> 32)) - 0.5f) * 0.5f;
            fs = 2.0f * ada_unit((uint32_t)q1);
            fc = ada_unit((uint32_t)(q2 >> 32)) + 0.5f;
        }
        if ((flags & DG_DIFFAUG_TRANSLATION) && keep_trans) {
            a.x = ada_range((uint32_t)q2, -T, 2u * (uint32_t)T + 1u);
            a.y = ada_range((uint32_t)(q3 >> 32), -T, 2u * (uint32_t)T + 1u);
        }
        if (flags & DG_DIFFAUG_CUTOUT) {
            if (keep_cut) {
                const int cs = ada_cs(S);
                const uint32_t count = (uint32_t)S + 1u - (uint32_t)(cs & 1);
                a.z = ada_range((uint32_t)q3, 0, count) - cs / 2;
                a.w = ada_range((uint32_t)(q4 >> 32), 0, count) - cs / 2;
            } else {
                a.z = a.w = S;                                          // the apply kernels still evaluate the stage: an empty square
            }
        }
        b.x = __float_as_int(fb); b.y = __float_as_int(fs); b.z = __float_as_int(fc); b.w = 0;
        reinterpret_cast<int4*>(recs)[2 * j] = a;
        reinterpret_cast<int4*>(recs)[2 * j + 1] = b;
    }
}

extern "C" int dg_diffaug_draw_p(uint64_t seed, int rank, int64_t iteration, int domain, int role, int n, int S, int flags, const double* p,
                                 int32_t* recs, dg_stream_t s) {
    DG_CHECK_ARG(recs != nullptr, "dg_diffaug_draw_p: null record table");
    DG_CHECK_ARG(((uintptr_t)recs & 15) == 0, "dg_diffaug_draw_p: the record table must be 16-byte aligned");
    DG_CHECK_ARG(p != nullptr, "dg_diffaug_draw_p: null probability pointer");
    DG_CHECK_ARG(((uintptr_t)p & 7) == 0, "dg_diffaug_draw_p: the probability (a device double) must be 8-byte aligned");
    DG_CHECK_ARG(n >= 1 && n <= ADA_MAX_BATCH, "dg_diffaug_draw_p: 1 <= n <= %d samples per batch, got %d", ADA_MAX_BATCH, n);
    DG_CHECK_ARG(S >= 2 && S <= ADA_MAX_SIZE, "dg_diffaug_draw_p: 2 <= S <= %d, got %d", ADA_MAX_SIZE, S);
    DG_CHECK_ARG((flags & ~DG_DIFFAUG_ALL) == 0, "dg_diffaug_draw_p: unknown policy flags %d", flags);
    DG_CHECK_ARG(rank >= 0 && iteration >= 0 && (domain == 0 || domain == 1) && (role == 0 || role == 1),
                 "dg_diffaug_draw_p: rank >= 0, iteration >= 0, domain 0 (A) or 1 (B), role 0 (real) or 1 (fake)");
    uint64_t k = ada_mix(seed + ADA_G);
    k = ada_mix(k ^ (((uint64_t)(uint32_t)rank << 32) | (uint64_t)(uint32_t)domain));
    k = ada_mix(k ^ (uint64_t)iteration);
    k = ada_mix(k ^ (ADA_DIFF_LINK | (uint64_t)(uint32_t)role));
    const uint64_t k2 = ada_mix(k ^ ADA_GATE_LINK);
    hipLaunchKernelGGL(diffaug_draw_p_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, k, k2, n, S, ada_T(S), flags, p, recs);
    DG_CHECK_LAUNCH("diffaug_draw_p");
    return DG_OK;
}

__device__ __forceinline__ int ada_wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// ONE block of 256 threads.  Thread t takes the values t, t + 256, ...; the partials are integers (|sum| <= n <= 65536), so the wave tree
// and the four-term sum behind it are exact whatever their order; lane 0 does the read-modify-write of the two window fields.
__global__ __launch_bounds__(256) void ada_accumulate_kernel(const float* __restrict__ d_out, int n, float thr, float* __restrict__ acc) {
    __shared__ int red[4];
    int part = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = d_out[i];
        part += (int)(v > thr) - (int)(v < thr);                        // by comparisons: a NaN and v == thr count 0
    }
    part = ada_wave_sum_i(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int sum = (red[0] + red[1]) + (red[2] + red[3]);
        acc[0] = acc[0] + (float)sum;
        acc[1] = acc[1] + (float)n;
    }
}

extern "C" int dg_ada_accumulate(const float* d_out, int n, float threshold, float* acc, dg_stream_t s) {
    DG_CHECK_ARG(d_out != nullptr && acc != nullptr, "dg_ada_accumulate: null pointer");
    DG_CHECK_ARG((((uintptr_t)d_out | (uintptr_t)acc) & 3) == 0, "dg_ada_accumulate: float pointers must be 4-byte aligned");
    DG_CHECK_ARG(n >= 1 && n <= ADA_MAX_OUTPUTS, "dg_ada_accumulate: 1 <= n <= %d discriminator outputs, got %d", ADA_MAX_OUTPUTS, n);
    DG_CHECK_ARG(threshold == threshold, "dg_ada_accumulate: the threshold is NaN");
    hipLaunchKernelGGL(ada_accumulate_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, d_out, n, threshold, acc);
    DG_CHECK_LAUNCH("ada_accumulate");
    return DG_OK;
}

// One lane.  Every operation is rounded once, in the order of the header (no contraction of acc[1] * step into the sum behind it).
__global__ __launch_bounds__(64) void ada_update_kernel(double* __restrict__ ctl, float* __restrict__ acc, double target, double step,
                                                        double p_max) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    const double sum = (double)acc[0], cnt = (double)acc[1];
    if (cnt == 0.0) return;                                             // an empty window: nothing changes
    const double rt = sum / cnt;
    const double adj = cnt * step;
    const double applied = rt > target ? adj : (rt < target ? -adj : 0.0);
    double p = ctl[0] + applied;
    if (!(p >= 0.0)) p = 0.0;                                           // max(0, .), then min(p_max, .)
    if (p > p_max) p = p_max;
    ctl[0] = p;
    ctl[1] = rt;
    ctl[2] = ctl[2] + 1.0;
    ctl[3] = ctl[3] + cnt;
    ctl[4] = applied;
    acc[0] = 0.0f;
    acc[1] = 0.0f;
}

extern "C" int dg_ada_update(double* ctl, float* acc, double target, double step_per_image, double p_max, dg_stream_t s) {
    DG_CHECK_ARG(ctl != nullptr && acc != nullptr, "dg_ada_update: null pointer");
    DG_CHECK_ARG(((uintptr_t)ctl & 7) == 0, "dg_ada_update: the control block (device double[8]) must be 8-byte aligned");
    DG_CHECK_ARG(((uintptr_t)acc & 3) == 0, "dg_ada_update: the window (device float[2]) must be 4-byte aligned");
    DG_CHECK_ARG(target > -1.0 && target < 1.0, "dg_ada_update: the target of r_t lies in (-1, 1), got %g", target);
    DG_CHECK_ARG(step_per_image >= 0.0 && step_per_image <= 1.0, "dg_ada_update: 0 <= step_per_image <= 1, got %g", step_per_image);
    DG_CHECK_ARG(p_max >= 0.0 && p_max <= 1.0, "dg_ada_update: 0 <= p_max <= 1, got %g", p_max);
    hipLaunchKernelGGL(ada_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, ctl, acc, target, step_per_image, p_max);
    DG_CHECK_LAUNCH("ada_update");
    return DG_OK;
}
