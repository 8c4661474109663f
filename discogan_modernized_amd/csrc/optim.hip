// optim.Adam over flat fp32 buffers (image_translation.py:275-287: lr 2e-4, betas (0.5, 0.999), eps 1e-8,
// coupled L2 weight_decay 1e-5).  One launch per optimiser step over the whole flat parameter group
// (G_A+G_B or D_A+D_B): 28 B/param of HBM traffic, 16-byte accesses.
// The step counter and the bias-correction scalars live in DEVICE memory and are advanced by a
// one-thread kernel, so an optimiser step is capturable in a hipGraph and replays correctly.
// Operation order follows torch/optim/adam.py::_single_tensor_adam:
//   g' = g + wd*p ; m = m + (g'-m)*(1-b1) ; v = v*b2 + (1-b2)*g'*g' ;
//   denom = sqrt(v)/sqrt(1-b2^t) + eps ; p = p - (lr/(1-b1^t)) * m/denom
#include "dg_common.h"

// ctl: the step's device control block (dg_grad_clip_finalize), or nullptr; ctl[3] != 0 = this step is skipped, the count stays
__global__ void adam_advance_kernel(double* state, double lr, double b1, double b2, const double* ctl) {
    if (ctl != nullptr && ctl[3] != 0.0) return;
    const double t = state[0] + 1.0;
    state[0] = t;
    state[1] = lr / (1.0 - pow(b1, t));
    state[2] = sqrt(1.0 - pow(b2, t));
}

typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
// One parameter's update, every operation rounded on its own (no fused multiply-adds chosen by the compiler): the kernel's code paths
// (4 or 8 parameters per trip, the scalar tail, the three output forms) must give the same bits, and the reference's CPU ops round
// op by op as well.
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float gscale, float wd, float omb1, float b2, float omb2,
                                         float bc2_sqrt, float eps, float step_size) {
#pragma clang fp contract(off)
    const float gr = g * gscale + wd * p;
    m = m + (gr - m) * omb1;
    v = v * b2 + omb2 * gr * gr;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);
}
// The update of one flat range by blocks bid = 0 .. nb - 1 of 256 threads (grid-stride): the body of adam_step_kernel, and of one range of
// adam_step_ranges_x3_kernel.
// P16 = 1: also write a bf16 (RNE) shadow of the updated parameters for the bf16 matrix path (+2 B/param on 28);
// P16 = 3: the three bf16 planes of the f32x3 matrix path (dg_split3; planes `pstride` elements apart, +6 B/param)
template <int P16>
__device__ __forceinline__ void adam_range(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, long n, float step_size, float bc2_sqrt, float omb1, float b2, float omb2,
                                           float eps, float wd, float gscale, __bf16* __restrict__ p16, long pstride, long bid, long nb) {
    const long n4 = n >> 2;
    long i0 = bid * 256 + threadIdx.x;
    if constexpr (P16 == 3) {
        // plane outputs: 8 parameters per thread and trip, so that every plane store is 16 bytes (the 8-byte plane stores of the 4-parameter
        // trip made this form 15 % slower per byte than the plain one: 4.73 against 5.55 TB/s alone at 460 M parameters); same arithmetic
        typedef __bf16 bf16x8_a __attribute__((ext_vector_type(8)));
        const long n8 = (((size_t)p16 | (size_t)(pstride * 2)) & 15) == 0 ? n >> 3 : 0;      // a range that starts 8 bytes into a 16-byte plane granule keeps the 4-parameter trip
        for (long i = i0; i < n8; i += nb * 256) {
            f32x4 pp[2], gg[2], mm[2], vv[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                pp[h] = *(const f32x4*)(p + i * 8 + 4 * h);
                gg[h] = *(const f32x4*)(g + i * 8 + 4 * h);
                mm[h] = *(const f32x4*)(m + i * 8 + 4 * h);
                vv[h] = *(const f32x4*)(v + i * 8 + 4 * h);
            }
            dg_bf16x4_t hh[2], md[2], ll[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float a = pp[h][j], b = mm[h][j], c = vv[h][j];
                    adam_one(a, gg[h][j], b, c, gscale, wd, omb1, b2, omb2, bc2_sqrt, eps, step_size);
                    pp[h][j] = a; mm[h][j] = b; vv[h][j] = c;
                }
                *(f32x4*)(p + i * 8 + 4 * h) = pp[h];
                *(f32x4*)(m + i * 8 + 4 * h) = mm[h];
                *(f32x4*)(v + i * 8 + 4 * h) = vv[h];
                dg_split3(pp[h], hh[h], md[h], ll[h]);
            }
            *(bf16x8_a*)(p16 + i * 8) = __builtin_shufflevector(hh[0], hh[1], 0, 1, 2, 3, 4, 5, 6, 7);
            *(bf16x8_a*)(p16 + pstride + i * 8) = __builtin_shufflevector(md[0], md[1], 0, 1, 2, 3, 4, 5, 6, 7);
            *(bf16x8_a*)(p16 + 2 * pstride + i * 8) = __builtin_shufflevector(ll[0], ll[1], 0, 1, 2, 3, 4, 5, 6, 7);
        }
        i0 += n8 * 2;                 // the 4-parameter loop below takes what is left (n8 > 0: at most one trip of one thread)
    }
    for (long i = i0; i < n4; i += nb * 256) {
        f32x4 pp = *(const f32x4*)(p + i * 4);
        const f32x4 gg = *(const f32x4*)(g + i * 4);
        f32x4 mm = *(const f32x4*)(m + i * 4);
        f32x4 vv = *(const f32x4*)(v + i * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a = pp[j], b = mm[j], c = vv[j];
            adam_one(a, gg[j], b, c, gscale, wd, omb1, b2, omb2, bc2_sqrt, eps, step_size);
            pp[j] = a; mm[j] = b; vv[j] = c;
        }
        *(f32x4*)(p + i * 4) = pp;
        *(f32x4*)(m + i * 4) = mm;
        *(f32x4*)(v + i * 4) = vv;
        if (P16 == 1) *(bf16x4_t*)(p16 + i * 4) = __builtin_convertvector(pp, bf16x4_t);
        if (P16 == 3) {
            dg_bf16x4_t h, md, l;
            dg_split3(pp, h, md, l);
            *(dg_bf16x4_t*)(p16 + i * 4) = h;
            *(dg_bf16x4_t*)(p16 + pstride + i * 4) = md;
            *(dg_bf16x4_t*)(p16 + 2 * pstride + i * 4) = l;
        }
    }
    if (bid == 0 && threadIdx.x == 0) {
        for (long e = n4 * 4; e < n; ++e) {
            float a = p[e], b = m[e], c = v[e];
            adam_one(a, g[e], b, c, gscale, wd, omb1, b2, omb2, bc2_sqrt, eps, step_size);
            p[e] = a; m[e] = b; v[e] = c;
            if (P16 == 1) p16[e] = (__bf16)p[e];
            if (P16 == 3) {
                const __bf16 h = (__bf16)p[e];
                const float r = p[e] - (float)h;
                const __bf16 md = (__bf16)r;
                p16[e] = h;
                p16[pstride + e] = md;
                p16[2 * pstride + e] = (__bf16)(r - (float)md);
            }
        }
    }
}

template <int P16>
__global__ __launch_bounds__(256) void adam_step_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, long n,
                                                        const double* __restrict__ state, float b1, float b2, float eps,
                                                        float wd, float gscale, __bf16* __restrict__ p16, long pstride,
                                                        const double* __restrict__ ctl) {
    // ctl (or nullptr): the gradient scale and the go / no-go of this step come from device memory (dg_grad_clip_finalize on the same
    // stream) instead of the host.  A skipped step returns before its first load: p, m, v and every derived form keep their bits.
    if (ctl != nullptr) {
        if (ctl[3] != 0.0) return;
        gscale = (float)ctl[2];
    }
    adam_range<P16>(p, g, m, v, n, (float)state[1], (float)state[2], 1.f - b1, b2, 1.f - b2, eps, wd, gscale, p16, pstride, (long)blockIdx.x,
                    (long)gridDim.x);
}

static inline int flat_grid(size_t n) {
    size_t grid = (n / 4 + 255) / 256;
    if (grid > 4096) grid = 4096;
    if (grid < 1) grid = 1;
    return (int)grid;
}
// ctl == nullptr: an unconditional advance; otherwise state is left untouched when ctl[3] != 0
extern "C" int dg_adam_advance(double* state, double lr, double beta1, double beta2, const double* ctl, dg_stream_t stream) {
    DG_CHECK_ARG(state, "dg_adam_advance: null state");
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, state, lr, beta1, beta2, ctl);
    DG_CHECK_LAUNCH("adam_advance");
    return DG_OK;
}
// The one flat step.  ctl == nullptr: the host's grad_scale; otherwise the gradient scale (float)ctl[2] and the skip flag ctl[3] are
// read on the device and grad_scale is ignored.
// form 0: out unused; 1: out = the bf16 shadow; 3: out = plane 0 of the range (hi / mid / lo planes plane_elems elements apart).
extern "C" int dg_adam_step_flat(float* p, const float* g, float* m, float* v, size_t n, const double* state, float beta1, float beta2,
                                 float eps, float weight_decay, float grad_scale, const double* ctl, void* out, int form,
                                 size_t plane_elems, dg_stream_t stream) {
    DG_CHECK_ARG(p && g && m && v && state, "dg_adam_step_flat: null pointer");
    DG_CHECK_ARG(form == 0 || form == 1 || form == 3, "dg_adam_step_flat: form %d (0 plain, 1 bf16 shadow, 3 planes)", form);
    DG_CHECK_ARG(form == 0 || out, "dg_adam_step_flat: form %d without an output", form);
    DG_CHECK_ARG(form != 3 || (plane_elems >= n && plane_elems % 8 == 0), "dg_adam_step_flat: plane distance %zu for %zu parameters",
                 plane_elems, n);
    if (n == 0) return DG_OK;
    const dim3 grid(flat_grid(n)), block(256);
    const hipStream_t s = (hipStream_t)stream;
    const float gscale = ctl ? 1.f : grad_scale;
    if (form == 0)
        hipLaunchKernelGGL(adam_step_kernel<0>, grid, block, 0, s, p, g, m, v, (long)n, state, beta1, beta2, eps, weight_decay, gscale,
                           (__bf16*)nullptr, 0L, ctl);
    else if (form == 1)
        hipLaunchKernelGGL(adam_step_kernel<1>, grid, block, 0, s, p, g, m, v, (long)n, state, beta1, beta2, eps, weight_decay, gscale,
                           (__bf16*)out, 0L, ctl);
    else
        hipLaunchKernelGGL(adam_step_kernel<3>, grid, block, 0, s, p, g, m, v, (long)n, state, beta1, beta2, eps, weight_decay, gscale,
                           (__bf16*)out, (long)plane_elems, ctl);
    DG_CHECK_LAUNCH("adam_step");
    return DG_OK;
}
// fp32 -> bf16 (RNE) copy: initial weight shadow / shadows of tensors that have no fused producer
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* __restrict__ x, __bf16* __restrict__ y, long n) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256)
        *(bf16x4_t*)(y + i * 4) = __builtin_convertvector(*(const f32x4*)(x + i * 4), bf16x4_t);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long e = n4 * 4; e < n; ++e) y[e] = (__bf16)x[e];
}
extern "C" int dg_f32_to_bf16(const float* x, void* y, size_t n, dg_stream_t stream) {
    DG_CHECK_ARG(x && y, "dg_f32_to_bf16: null pointer");
    if (n == 0) return DG_OK;
    long grid = ((long)(n / 4) + 255) / 256;
    if (grid > 4096) grid = 4096;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, x, (__bf16*)y, (long)n);
    DG_CHECK_LAUNCH("f32_to_bf16");
    return DG_OK;
}
// fp32 -> three bf16 planes (dg_split3): plane operands of tensors that have no fused producer
__global__ __launch_bounds__(256) void f32_to_bf16x3_kernel(const float* __restrict__ x, __bf16* __restrict__ y, long n, long pstride) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        dg_bf16x4_t h, md, l;
        dg_split3(*(const f32x4*)(x + i * 4), h, md, l);
        *(dg_bf16x4_t*)(y + i * 4) = h;
        *(dg_bf16x4_t*)(y + pstride + i * 4) = md;
        *(dg_bf16x4_t*)(y + 2 * pstride + i * 4) = l;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long e = n4 * 4; e < n; ++e) {
            const __bf16 h = (__bf16)x[e];
            const float r = x[e] - (float)h;
            const __bf16 md = (__bf16)r;
            y[e] = h;
            y[pstride + e] = md;
            y[2 * pstride + e] = (__bf16)(r - (float)md);
        }
}
extern "C" int dg_f32_to_bf16x3(const float* x, void* y3, size_t n, size_t plane_elems, dg_stream_t stream) {
    DG_CHECK_ARG(x && y3, "dg_f32_to_bf16x3: null pointer");
    DG_CHECK_ARG(plane_elems >= n && plane_elems % 8 == 0, "dg_f32_to_bf16x3: plane distance %zu for %zu elements", plane_elems, n);
    if (n == 0) return DG_OK;
    long grid = ((long)(n / 4) + 255) / 256;
    if (grid > 8192) grid = 8192;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(f32_to_bf16x3_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, x, (__bf16*)y3, (long)n, (long)plane_elems);
    DG_CHECK_LAUNCH("f32_to_bf16x3");
    return DG_OK;
}

// ---- exponential moving average of a flat parameter buffer (optim.EMA) ---------------------------------------------------------
// ema += (p - ema) * w with w = 1 - decay, one launch over the whole flat generator group: 12 B/param (read p, read + write ema).
// Lerp form, every operation rounded on its own: p == ema leaves ema bitwise unchanged for every w (a generator outside the loss of
// recongan / gan keeps its EMA equal to itself), and the kernel's two code paths (16-byte trips, scalar tail) give the same bits as a
// host that rounds op by op.  Geometry of the Adam kernel above.
__device__ __forceinline__ float ema_one(float e, float p, float w) {
#pragma clang fp contract(off)
    const float d = p - e;
    const float s = d * w;
    return e + s;
}
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long n, float w) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        f32x4 ee = *(const f32x4*)(ema + i * 4);
        const f32x4 pp = *(const f32x4*)(p + i * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) ee[j] = ema_one(ee[j], pp[j], w);
        *(f32x4*)(ema + i * 4) = ee;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long e = n4 * 4; e < n; ++e) ema[e] = ema_one(ema[e], p[e], w);
}
// exchange the contents of two disjoint flat buffers bit for bit (integer lanes: NaN payloads pass untouched)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void swap_flat_kernel(unsigned int* __restrict__ a, unsigned int* __restrict__ b, long n) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const u32x4 x = *(const u32x4*)(a + i * 4);
        const u32x4 y = *(const u32x4*)(b + i * 4);
        *(u32x4*)(a + i * 4) = y;
        *(u32x4*)(b + i * 4) = x;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long e = n4 * 4; e < n; ++e) {
            const unsigned int x = a[e];
            a[e] = b[e];
            b[e] = x;
        }
}
extern "C" int dg_ema_update_flat(float* ema, const float* p, size_t n, float w, dg_stream_t stream) {
    DG_CHECK_ARG(ema && p, "dg_ema_update_flat: null pointer");
    DG_CHECK_ARG((((size_t)ema | (size_t)p) & 15) == 0, "dg_ema_update_flat: pointers must be 16-byte aligned (ema %p, p %p)", (void*)ema,
                 (const void*)p);
    DG_CHECK_ARG(w >= 0.f && w <= 1.f, "dg_ema_update_flat: weight %g outside [0, 1]", (double)w);      // (false for NaN)
    if (n == 0) return DG_OK;
    hipLaunchKernelGGL(ema_update_kernel, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, ema, p, (long)n, w);
    DG_CHECK_LAUNCH("ema_update");
    return DG_OK;
}
extern "C" int dg_swap_flat(float* a, float* b, size_t n, dg_stream_t stream) {
    DG_CHECK_ARG(a && b, "dg_swap_flat: null pointer");
    DG_CHECK_ARG((((size_t)a | (size_t)b) & 15) == 0, "dg_swap_flat: pointers must be 16-byte aligned (a %p, b %p)", (void*)a, (void*)b);
    if (n == 0 || a == b) return DG_OK;
    const size_t lo = (size_t)a < (size_t)b ? (size_t)a : (size_t)b, hi = (size_t)a < (size_t)b ? (size_t)b : (size_t)a;
    DG_CHECK_ARG((hi - lo) / sizeof(float) >= n, "dg_swap_flat: the two ranges of %zu floats overlap", n);
    hipLaunchKernelGGL(swap_flat_kernel, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, (unsigned int*)a, (unsigned int*)b, (long)n);
    DG_CHECK_LAUNCH("swap_flat");
    return DG_OK;
}

// ---- gradient statistics and step control (optim.Adam.enable_grad_control) --------------------------------------------------------
// Global gradient norm, clipping by it and a guard against a non-finite gradient, with no host round trip: a read-only pass over the flat
// gradient leaves one fp64 partial per block, one workgroup folds the partials into the device control block `ctl` (layout:
// include/discogan_hip.h), and the Adam kernels above take their gradient scale and their go / no-go from ctl.
// Every element is widened to double before it is squared: the product of two fp32 values is exact in fp64 and at most 2^256, so a finite
// gradient cannot overflow or underflow the sum, and only inf / NaN elements make it non-finite.  No atomics and a fixed summation order
// (per thread, per wave, per block, then over the slots in index order): the same gradient gives the same bits on every run.
#define DG_GRAD_STATS_SLOTS 16384            // workspace capacity in partials: four ranges at the full grid
static_assert(DG_GRAD_STATS_SLOTS >= 4096, "one full-grid range must fit");

__device__ __forceinline__ void sumsq4(double (&a)[4], const f32x4& x) {
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] += (double)x[j] * (double)x[j];      // (an exact product: fused or not, the same bits)
}
__global__ __launch_bounds__(256) void grad_sumsq_partial_kernel(const float* __restrict__ g, long n, double* __restrict__ ws) {
    __shared__ double red[4];
    const long n4 = n >> 2;
    const long stride = (long)gridDim.x * 256;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    // four trips of the grid-stride loop at a time: four independent 16-byte loads in flight per thread (a read-only stream has no
    // stores to overlap them with); the additions keep the order of the plain loop below
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const f32x4 x0 = *(const f32x4*)(g + i * 4);
        const f32x4 x1 = *(const f32x4*)(g + (i + stride) * 4);
        const f32x4 x2 = *(const f32x4*)(g + (i + 2 * stride) * 4);
        const f32x4 x3 = *(const f32x4*)(g + (i + 3 * stride) * 4);
        sumsq4(a, x0);
        sumsq4(a, x1);
        sumsq4(a, x2);
        sumsq4(a, x3);
    }
    for (; i < n4; i += stride) sumsq4(a, *(const f32x4*)(g + i * 4));
    double s = (a[0] + a[1]) + (a[2] + a[3]);
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long e = n4 * 4; e < n; ++e) s += (double)g[e] * (double)g[e];
    dg_block_stage_d(s, red);
    if (threadIdx.x == 0) ws[blockIdx.x] = dg_sum4_pair(red);
}
__global__ __launch_bounds__(256) void grad_clip_finalize_kernel(const double* __restrict__ ws, int slots, double pre_scale,
                                                                 double max_norm, int guard, double* __restrict__ ctl) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < slots; i += 256) s += ws[i];
    dg_block_stage_d(s, red);
    if (threadIdx.x != 0) return;
    const double sumsq = dg_sum4_pair(red);
    const double norm = sqrt(sumsq) * pre_scale;
    double scale = pre_scale;
    bool clipped = false;
    if (max_norm > 0.0) {
        // torch.nn.utils.clip_grad_norm_: coef = max_norm / (norm + 1e-6), clamped to at most 1 (a NaN stays a NaN, inf gives 0)
        const double coef = max_norm / (norm + 1e-6);
        if (!(coef >= 1.0)) {
            scale = pre_scale * coef;
            clipped = coef < 1.0;
        }
    }
    const bool finite = (sumsq - sumsq) == 0.0;      // false for inf and NaN
    const bool skip = guard != 0 && !finite;
    ctl[0] = sumsq;
    ctl[1] = norm;
    ctl[2] = scale;
    ctl[3] = skip ? 1.0 : 0.0;
    ctl[4] += 1.0;
    if (clipped && !skip) ctl[5] += 1.0;
    if (skip) ctl[6] += 1.0;
    if ((norm - norm) == 0.0 && norm > ctl[7]) ctl[7] = norm;
}

extern "C" size_t dg_grad_stats_workspace_bytes(void) { return (size_t)DG_GRAD_STATS_SLOTS * sizeof(double); }
extern "C" int dg_grad_sumsq_partial(const float* g, size_t n, double* ws, size_t ws_bytes, int slot0, int* slots_used, dg_stream_t stream) {
    DG_CHECK_ARG(slots_used, "dg_grad_sumsq_partial: null slots_used");
    *slots_used = 0;
    if (n == 0) return DG_OK;
    DG_CHECK_ARG(g && ws, "dg_grad_sumsq_partial: null pointer");
    DG_CHECK_ARG(((size_t)g & 15) == 0, "dg_grad_sumsq_partial: the gradient must be 16-byte aligned (%p)", (const void*)g);
    DG_CHECK_ARG(((size_t)ws & 7) == 0, "dg_grad_sumsq_partial: the workspace must be 8-byte aligned (%p)", (void*)ws);
    DG_CHECK_ARG(slot0 >= 0, "dg_grad_sumsq_partial: first slot %d", slot0);
    const int grid = flat_grid(n);
    DG_CHECK_ARG(((size_t)slot0 + (size_t)grid) * sizeof(double) <= ws_bytes,
                 "dg_grad_sumsq_partial: workspace of %zu bytes too small for slots %d..%ld (dg_grad_stats_workspace_bytes)", ws_bytes, slot0,
                 (long)slot0 + grid - 1);
    hipLaunchKernelGGL(grad_sumsq_partial_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, (long)n, ws + slot0);
    DG_CHECK_LAUNCH("grad_sumsq_partial");
    *slots_used = grid;
    return DG_OK;
}
extern "C" int dg_grad_clip_finalize(const double* ws, int slots, double pre_scale, double max_norm, int guard, double* ctl,
                                     dg_stream_t stream) {
    DG_CHECK_ARG(ctl, "dg_grad_clip_finalize: null ctl");
    DG_CHECK_ARG(slots >= 0 && slots <= DG_GRAD_STATS_SLOTS && (slots == 0 || ws), "dg_grad_clip_finalize: %d slots (workspace %p)", slots,
                 (const void*)ws);
    DG_CHECK_ARG(pre_scale == pre_scale && max_norm == max_norm, "dg_grad_clip_finalize: NaN pre_scale or max_norm");
    hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ws, slots, pre_scale, max_norm, guard, ctl);
    DG_CHECK_LAUNCH("grad_clip_finalize");
    return DG_OK;
}

// ---- the f32x3 step of a WHOLE group, transposed weight planes included (optim.Adam.step, active is None) -----------------------------
// dg_adam_step_flat (form 3) followed by dg_x3_transpose_planes reads back, microseconds later, the 6 B/param of planes the step wrote and
// writes them again transposed (12 B/param on top of the step's 34).  Here the step of a conv weight keeps its plane values in LDS and
// writes the transposed copy itself: 40 B/param, one pass.  One workgroup owns a 64 x TJ tile of a [K][J] weight image (J = 16 C;
// K % 64 == 0 and J % TJ == 0: no ragged tile, no scalar path).  Thread (lk, lv) updates the 8-parameter runs lv and lv + TJ / 16 of
// tile row lk -- adam_one / dg_split3 and the 16-byte plane stores of adam_range<3>'s 8-parameter trip --, then the tile leaves LDS
// column-wise exactly as x3_transpose_kernel stores it.  TJ = 128 on 512 threads wherever J % 128 == 0 (every interior conv of the
// model): rows of 512 contiguous bytes of p, g, m, v.  Alone on 224 M parameters of generator-shaped weights the 64 x 64 tile of the
// transpose pass (256-byte rows) ran at 3.70 TB/s of its 40 B/param and 32 x 128 at 3.87, where the flat kernel makes 4.6-4.8 TB/s of its
// 34 and the transpose pass 4.43 of its 12; 64 x 128 runs at 5.12 TB/s (1.75 ms against 1.58 + 0.61).  TJ = 64 on 256 threads serves
// the weights with J % 128 == 64.  Everything else of the group (BatchNorm vectors, 3-channel
// and ragged weights, the heads) goes through adam_step_ranges_x3_kernel: adam_range<3> over a table of ranges, ONE launch.
#include "x3_table.h"
template <int TJ>
__global__ __launch_bounds__(4 * TJ) void adam_step_x3t_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, const double* __restrict__ state, float b1, float b2,
                                                            float eps, float wd, float gscale, __bf16* __restrict__ p3,
                                                            __bf16* __restrict__ p3t, long plane, const double* __restrict__ ctl,
                                                            X3TransposeTable t) {
    // per plane the tile as 64 k rows x TJ / 2 words (a word = two neighbouring j of one k), pitch + 1: x3_transpose_kernel's tile
    constexpr int TPR = TJ / 16;                 // threads per tile row, two 8-parameter runs each
    __shared__ unsigned tile[3][64][TJ / 2 + 1];
    typedef __bf16 bf16x8_a __attribute__((ext_vector_type(8)));
    if (ctl != nullptr) {                 // (the same answer in every thread of the grid: nobody is left waiting at the barrier below)
        if (ctl[3] != 0.0) return;
        gscale = (float)ctl[2];
    }
    const float step_size = (float)state[1];
    const float bc2_sqrt = (float)state[2];
    const float omb1 = 1.f - b1, omb2 = 1.f - b2;
    int wi = 0;
    while (wi + 1 < t.n && (int)blockIdx.x >= t.tile0[wi + 1]) ++wi;
    const int K = t.K[wi], J = t.J[wi];
    const long base = t.off[wi];
    const int tj = J / TJ;
    const int b = blockIdx.x - t.tile0[wi];
    const int k0 = (b / tj) * 64, j0 = (b % tj) * TJ;
    const int lk = threadIdx.x / TPR, lv = threadIdx.x % TPR;        // update: row k, 8-parameter runs lv and lv + TPR of the row
    const int sq = threadIdx.x & 7, sjp = threadIdx.x >> 3;          // transposed store: k run 8 sq .. 8 sq + 7 of output rows 2 sjp, 2 sjp + 1
    f32x4 pp[2][2], gg[2][2], mm[2][2], vv[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const long e = base + (long)(k0 + lk) * J + j0 + (lv + TPR * h) * 8;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            pp[h][q] = *(const f32x4*)(p + e + 4 * q);
            gg[h][q] = *(const f32x4*)(g + e + 4 * q);
            mm[h][q] = *(const f32x4*)(m + e + 4 * q);
            vv[h][q] = *(const f32x4*)(v + e + 4 * q);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const long e = base + (long)(k0 + lk) * J + j0 + (lv + TPR * h) * 8;
        dg_bf16x4_t hh[2], md[2], ll[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = pp[h][q][j], bb = mm[h][q][j], c = vv[h][q][j];
                adam_one(a, gg[h][q][j], bb, c, gscale, wd, omb1, b2, omb2, bc2_sqrt, eps, step_size);
                pp[h][q][j] = a; mm[h][q][j] = bb; vv[h][q][j] = c;
            }
            *(f32x4*)(p + e + 4 * q) = pp[h][q];
            *(f32x4*)(m + e + 4 * q) = mm[h][q];
            *(f32x4*)(v + e + 4 * q) = vv[h][q];
            dg_split3(pp[h][q], hh[q], md[q], ll[q]);
        }
        const bf16x8_a pl3[3] = {__builtin_shufflevector(hh[0], hh[1], 0, 1, 2, 3, 4, 5, 6, 7),
                                 __builtin_shufflevector(md[0], md[1], 0, 1, 2, 3, 4, 5, 6, 7),
                                 __builtin_shufflevector(ll[0], ll[1], 0, 1, 2, 3, 4, 5, 6, 7)};
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            *(bf16x8_a*)(p3 + pl * plane + e) = pl3[pl];
            const u32x4 w = __builtin_bit_cast(u32x4, pl3[pl]);
#pragma unroll
            for (int i = 0; i < 4; ++i) tile[pl][lk][(lv + TPR * h) * 4 + i] = w[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        unsigned w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = tile[pl][8 * sq + i][sjp];
        u32x4 lo, hi;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            lo[i] = (w[2 * i] & 0xffffu) | (w[2 * i + 1] << 16);
            hi[i] = (w[2 * i] >> 16) | (w[2 * i + 1] & 0xffff0000u);
        }
        unsigned short* d = (unsigned short*)p3t + pl * plane + base + (long)(j0 + 2 * sjp) * K + k0 + 8 * sq;
        *(u32x4*)d = lo;
        *(u32x4*)(d + K) = hi;
    }
}

#define DG_ADAM_RANGES_MAX 64
struct AdamRangeTable {
    int n;
    int blk0[DG_ADAM_RANGES_MAX + 1];      // first block of range i (prefix sums); blk0[n] = grid
    long off[DG_ADAM_RANGES_MAX], len[DG_ADAM_RANGES_MAX];
};
__global__ __launch_bounds__(256) void adam_step_ranges_x3_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                  float* __restrict__ v, const double* __restrict__ state, float b1,
                                                                  float b2, float eps, float wd, float gscale, __bf16* __restrict__ p3,
                                                                  long plane, const double* __restrict__ ctl, AdamRangeTable t) {
    if (ctl != nullptr) {
        if (ctl[3] != 0.0) return;
        gscale = (float)ctl[2];
    }
    int ri = 0;
    while (ri + 1 < t.n && (int)blockIdx.x >= t.blk0[ri + 1]) ++ri;
    const long o = t.off[ri];
    adam_range<3>(p + o, g + o, m + o, v + o, t.len[ri], (float)state[1], (float)state[2], 1.f - b1, b2, 1.f - b2, eps, wd, gscale, p3 + o,
                  plane, (long)(blockIdx.x - t.blk0[ri]), (long)(t.blk0[ri + 1] - t.blk0[ri]));
}

// One f32x3 Adam step of a flat group of `numel` parameters as n_w tiled conv weights ([K][J] images at element offsets w_off: they
// also get their transposed planes in pt_planes) and n_r plain ranges [r_off, r_off + r_len) (plain planes only).  ctl == nullptr: the
// host's grad_scale; otherwise scale and go / no-go from the control block, as dg_adam_step_flat.  What neither list covers is left
// untouched.  Host arrays, each list ascending and disjoint in itself, and the two lists disjoint from each other (a weight that
// overlaps a range is refused: its elements would be stepped twice); r_len[i] == 0 is accepted and covers nothing.
extern "C" int dg_adam_step_group_x3(float* p, const float* g, float* m, float* v, size_t numel, const double* state, float beta1,
                                     float beta2, float eps, float weight_decay, float grad_scale, const double* ctl, void* p_planes,
                                     void* pt_planes, size_t plane_elems, const int64_t* w_off, const int* w_K, const int* w_J, int n_w,
                                     const int64_t* r_off, const int64_t* r_len, int n_r, dg_stream_t stream) {
    DG_CHECK_ARG(p && g && m && v && state && p_planes, "dg_adam_step_group_x3: null pointer");
    DG_CHECK_ARG(n_w >= 0 && n_r >= 0 && (n_w == 0 || (pt_planes && w_off && w_K && w_J)) && (n_r == 0 || (r_off && r_len)),
                 "dg_adam_step_group_x3: %d weights, %d ranges, or a null table", n_w, n_r);
    DG_CHECK_ARG(plane_elems >= numel && plane_elems % 8 == 0, "dg_adam_step_group_x3: plane distance %zu for %zu parameters", plane_elems,
                 numel);
    DG_CHECK_ARG((((size_t)p | (size_t)g | (size_t)m | (size_t)v | (size_t)p_planes | (size_t)pt_planes) & 15) == 0,
                 "dg_adam_step_group_x3: buffers must be 16-byte aligned");
    int64_t end = 0;
    for (int i = 0; i < n_w; ++i) {
        const int K = w_K[i], J = w_J[i];
        DG_CHECK_ARG(K >= 64 && J >= 64 && K % 64 == 0 && J % 64 == 0 && w_off[i] % 8 == 0 && w_off[i] >= end &&
                         (size_t)(w_off[i] + (int64_t)K * J) <= numel,
                     "dg_adam_step_group_x3: weight %d (K=%d, J=%d, offset %ld): K and J multiples of 64, offset a multiple of 8, ascending, "
                     "inside %zu parameters", i, K, J, (long)w_off[i], numel);
        end = w_off[i] + (int64_t)K * J;
    }
    end = 0;
    for (int i = 0; i < n_r; ++i) {
        DG_CHECK_ARG(r_len[i] >= 0 && r_off[i] % 8 == 0 && r_off[i] >= end && (size_t)(r_off[i] + r_len[i]) <= numel,
                     "dg_adam_step_group_x3: range %d (offset %ld, %ld parameters): offset a multiple of 8, ascending, inside %zu parameters", i,
                     (long)r_off[i], (long)r_len[i], numel);
        end = r_off[i] + r_len[i];
    }
    // ... and from each other: one merge walk over the two ascending lists (a range of no parameters covers nothing)
    for (int iw = 0, ir = 0; iw < n_w && ir < n_r;) {
        const int64_t wb = w_off[iw], we = wb + (int64_t)w_K[iw] * w_J[iw], rb = r_off[ir], re = rb + r_len[ir];
        if (r_len[ir] == 0 || re <= wb) ++ir;
        else if (we <= rb) ++iw;
        else
            DG_CHECK_ARG(false, "dg_adam_step_group_x3: weight %d (offset %ld, %ld parameters) overlaps range %d (offset %ld, %ld parameters)",
                         iw, (long)wb, (long)(we - wb), ir, (long)rb, (long)r_len[ir]);
    }
    const hipStream_t s = (hipStream_t)stream;
    for (int TJ = 128; TJ >= 64; TJ -= 64) {      // the 64 x 128 tile where J allows it, 64 x 64 for the rest; 48 weights per launch
        X3TransposeTable t;
        t.n = 0;
        long tiles = 0;
        for (int i = 0; i <= n_w; ++i) {
            if (i < n_w && (w_J[i] % 128 == 0) == (TJ == 128)) {
                t.tile0[t.n] = (int)tiles;
                t.K[t.n] = w_K[i]; t.J[t.n] = w_J[i]; t.off[t.n] = w_off[i];
                tiles += (long)(w_K[i] / 64) * (w_J[i] / TJ);
                ++t.n;
            }
            if (t.n == 0 || (i < n_w && t.n < DG_X3T_MAX)) continue;
            DG_CHECK_ARG(tiles <= 0x7fffffffL, "dg_adam_step_group_x3: %ld tiles in one launch", tiles);
            t.tile0[t.n] = (int)tiles;
            if (TJ == 128)
                hipLaunchKernelGGL(adam_step_x3t_kernel<128>, dim3((unsigned)tiles), dim3(512), 0, s, p, g, m, v, state, beta1, beta2, eps,
                                   weight_decay, grad_scale, (__bf16*)p_planes, (__bf16*)pt_planes, (long)plane_elems, ctl, t);
            else
                hipLaunchKernelGGL(adam_step_x3t_kernel<64>, dim3((unsigned)tiles), dim3(256), 0, s, p, g, m, v, state, beta1, beta2, eps,
                                   weight_decay, grad_scale, (__bf16*)p_planes, (__bf16*)pt_planes, (long)plane_elems, ctl, t);
            DG_CHECK_LAUNCH("adam_step_x3t");
            t.n = 0;
            tiles = 0;
        }
    }
    for (int i = 0; i < n_r;) {      // a table takes the next 64 ranges that hold parameters; the next one starts at the first range it left
        AdamRangeTable t;
        t.n = 0;
        int blocks = 0;
        for (; i < n_r && t.n < DG_ADAM_RANGES_MAX; ++i) {
            if (r_len[i] == 0) continue;
            t.blk0[t.n] = blocks;
            t.off[t.n] = r_off[i]; t.len[t.n] = r_len[i];
            blocks += flat_grid((size_t)r_len[i] / 2);      // 8 parameters per thread and trip
            ++t.n;
        }
        if (t.n == 0) continue;
        t.blk0[t.n] = blocks;
        hipLaunchKernelGGL(adam_step_ranges_x3_kernel, dim3(blocks), dim3(256), 0, s, p, g, m, v, state, beta1, beta2, eps, weight_decay,
                           grad_scale, (__bf16*)p_planes, (long)plane_elems, ctl, t);
        DG_CHECK_LAUNCH("adam_step_ranges_x3");
    }
    return DG_OK;
}
