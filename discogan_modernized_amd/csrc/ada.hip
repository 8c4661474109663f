// Adaptive discriminator augmentation (Karras et al., NeurIPS 2020, "Training Generative Adversarial Networks with Limited Data"): the
// probability p of every stage of the differentiable augmentation, the overfitting measure r_t = E[sign(D(real) - threshold)] and the
// controller that moves p towards a target r_t, all in device memory.  include/discogan_hip.h ("adaptive discriminator augmentation")
// defines the state, the gate words and the order of the controller's operations; tests/ada_ref.py restates them in numpy.
//
// Two kernels, neither a hot path.  ada_accumulate_kernel adds the signs of one batch of discriminator outputs to a window: ONE block,
// integer partials, a fixed tree, no atomics.  ada_update_kernel closes a window: one lane.  The draw that reads p (dg_diffaug_draw_p:
// each stage of a sample kept with probability (float)*p, read from device memory by the kernel) is the GATED form of diffaug.hip's one
// record builder and lives there.
#include "dg_common.h"

#define ADA_MAX_OUTPUTS 65536                     // values of one dg_ada_accumulate call

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
