// Shared helpers for the gfx950 DiscoGAN kernels (internal; the public ABI is include/discogan_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/discogan_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 dg_bf16x4_t __attribute__((ext_vector_type(4)));

// ---- error plumbing (thread-local message, never abort) ---------------------------------------
extern thread_local char dg_err_buf[512];
int dg_fail(int code, const char* fmt, ...);

#define DG_CHECK_ARG(cond, ...)                                   \
    do {                                                          \
        if (!(cond)) return dg_fail(DG_ERR_INVALID, __VA_ARGS__); \
    } while (0)

#define DG_CHECK_LAUNCH(name)                                                                    \
    do {                                                                                         \
        hipError_t e__ = hipGetLastError();                                                      \
        if (e__ != hipSuccess) return dg_fail(DG_ERR_HIP, "%s: %s", name, hipGetErrorString(e__)); \
    } while (0)

static inline int dg_ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}
static inline bool dg_is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
static inline size_t dg_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int dg_get_option(int idx);
enum { DG_OPT_SPLITK = 0, DG_OPT_KT = 1, DG_OPT_TARGET_WGS = 2, DG_OPT_RESERVED = 3, DG_OPT_SPLIT_BELOW = 4, DG_OPT_POINTER_PATH = 5, DG_OPT_BF16 = 6, DG_OPT_DBG_ZERO = 7, DG_OPT_NO_DMA = 8, DG_OPT_DMA_MFMA = 9, DG_OPT_X3_MFMA = 10, DG_OPT_DGW_PERSIST = 11, DG_OPT_UNDERSTORY = 12, DG_OPT_BN_ITEMS = 13, DG_OPT_COUNT = 14 };
// Arithmetic of the conv products (DG_PREC_*): an argument all the way down.  DG_PREC_DEFAULT -> the process default
// dg_set_option("bf16", n), resolved once, where a call enters the library (the `prec` of a *_p / *_g entry point; the forms without one
// pass DG_PREC_DEFAULT).  Nothing below an entry point reads the option, and no per-thread state carries it.
static inline int dg_resolve_prec(int prec) { return prec >= 0 ? prec : dg_get_option(DG_OPT_BF16); }
// The tiled 3 -> K forward (igemm.hip, MODE_FWD_C3; wide: the 128-channel tile for K > 64): the form behind edge.hip's streaming kernels.
// Arguments are validated by the caller, which also collects the launch status.
__attribute__((visibility("hidden"))) void dg_c3_fwd_tiled(const float* x_nchw, const float* w, float* y_nhwc, int N, int H, int W, int K, int act,
                                                           float slope, bool wide, hipStream_t st);

// ---- grouped launches (round 4): one tensor per problem, picked by a block index (wave-uniform: scalar loads) ------------------
struct DgPtrs {
    const void* p[DG_MAX_GROUPS];
};
static inline DgPtrs dg_ptrs(const void* const* arr, int n) {
    DgPtrs r;
    for (int i = 0; i < DG_MAX_GROUPS; ++i) r.p[i] = (arr != nullptr && i < n) ? arr[i] : nullptr;
    return r;
}
static inline DgPtrs dg_ptrs1(const void* p0) {
    DgPtrs r;
    for (int i = 0; i < DG_MAX_GROUPS; ++i) r.p[i] = nullptr;
    r.p[0] = p0;
    return r;
}
template <typename T>
__device__ __forceinline__ T* dg_pick(const DgPtrs& t, int g) { return (T*)t.p[g]; }

// ---- device helpers ----------------------------------------------------------------------------
__device__ __forceinline__ float dg_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ double dg_wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// block-wide sum for blockDim.x == 256 (4 waves); result valid in thread 0
__device__ __forceinline__ float dg_block_sum256(float v, float* red /*>=4 floats LDS*/) {
    v = dg_wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w] = v;
    __syncthreads();
    float r = 0.f;
    if (threadIdx.x == 0) r = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return r;
}

// fp64 block sums for blockDim.x == 256 (4 waves): the wave sum of each of the N values, lane 0 of every wave to red[c][wave]; a barrier
// before (the previous use of red is read: item loops) and after.  The four wave sums of value c are then added by ONE of the two
// combiners below -- every site keeps the order it was written with, which its bits depend on: pairwise in metrics, recon, swd,
// diffaug and optim, sequential in loss and ganloss.
template <int N>
__device__ __forceinline__ void dg_block_stage_d(double (&a)[N], double (*red)[4]) {
#pragma unroll
    for (int c = 0; c < N; ++c) a[c] = dg_wave_sum_d(a[c]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < N; ++c) red[c][threadIdx.x >> 6] = a[c];
    }
    __syncthreads();
}
__device__ __forceinline__ void dg_block_stage_d(double v, double* red /*4 doubles LDS*/) {      // one value
    double a[1] = {v};
    dg_block_stage_d(a, (double (*)[4])red);
}
__device__ __forceinline__ double dg_sum4_pair(const double* r) { return (r[0] + r[1]) + (r[2] + r[3]); }
__device__ __forceinline__ double dg_sum4_seq(const double* r) { return r[0] + r[1] + r[2] + r[3]; }

__device__ __forceinline__ float dg_apply_act(float u, int act, float slope) {
    if (act == DG_ACT_LEAKY) return u > 0.f ? u : u * slope;
    if (act == DG_ACT_RELU) return u > 0.f ? u : 0.f;
    if (act == DG_ACT_SIGMOID) return 1.f / (1.f + __expf(-u));
    return u;
}

// BatchNorm apply, gs = gamma * invstd (one fp32 product): norm_act.hip's kernels, and the 3-channel kernels of edge.hip that apply the
// last decoder BatchNorm + ReLU to the values they load (BNL) -- one text, so the two agree bit for bit
__device__ __forceinline__ float bn_norm(float y, float mean, float gs, float beta) { return fmaf(y - mean, gs, beta); }

// fp32 -> three bf16 planes (the "f32x3" operand form of igemm.hip PREC 2 / igemm_dma_x3.hip): hi = bf16(v) (RNE),
// mid = bf16(v - hi), lo = bf16(v - hi - mid); both subtractions are exact in fp32, hi + mid + lo carries 24 significand bits
__device__ __forceinline__ void dg_split3(const f32x4& v, dg_bf16x4_t& hi, dg_bf16x4_t& mid, dg_bf16x4_t& lo) {
    hi = __builtin_convertvector(v, dg_bf16x4_t);
    const f32x4 r = v - __builtin_convertvector(hi, f32x4);
    mid = __builtin_convertvector(r, dg_bf16x4_t);
    lo = __builtin_convertvector(r - __builtin_convertvector(mid, f32x4), dg_bf16x4_t);
}
