// Training-mode BatchNorm2d + activation on NHWC [M][C] tensors, and stand-alone activations.
// Replaces nn.BatchNorm2d + in-place LeakyReLU(0.2)/ReLU (model.py:12-13,...,115-116) and their
// autograd backward; nn.Sigmoid / first-layer LeakyReLU backward (model.py:9,36).
// All kernels are HBM-bound streaming passes: 16-byte loads, lanes along the channel axis.
//
//   stats   : per-channel sum / sum-of-squares, fp32 per-thread partials over short row runs,
//             block partials to the workspace, finalised in fp64 (fixed order -> deterministic)
//   apply   : z = act((y - mean) * (gamma*invstd) + beta)
//   backward: g = dz * act'(u) with u recomputed bit-identically from y;
//             dbeta = sum g, dgamma = sum g*xhat, dy = gamma*invstd*(g - dbeta/M - xhat*dgamma/M)
#include "dg_common.h"
#include <string.h>
#include <initializer_list>

#define BN_U 8     // independent row loads in flight per thread (same-box A/B of the whole iteration: U=2 13.46 ms, 4 13.17, 8 13.13)

// Activation tensors are fp32 or bf16 (bf16 activation storage of the bf16 matrix path: statistics, normalisation and the
// backward expression stay fp32 / fp64; only what is STORED is rounded, RNE).  Every thread moves 16 bytes per access:
// V = 4 fp32 or 8 bf16 channels.
typedef __bf16 bf16x8_n __attribute__((ext_vector_type(8)));
typedef float f32x8_n __attribute__((ext_vector_type(8)));
template <typename T> struct BnV;
template <> struct BnV<float> { static constexpr int V = 4; };
template <> struct BnV<__bf16> { static constexpr int V = 8; };
__device__ __forceinline__ void bn_ld(const float* p, float (&v)[4]) {
    const f32x4 t = *(const f32x4*)p;
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
}
__device__ __forceinline__ void bn_ld(const __bf16* p, float (&v)[8]) {
    const f32x8_n t = __builtin_convertvector(*(const bf16x8_n*)p, f32x8_n);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = t[j];
}
// per-channel fp32 parameters (mean, invstd, gamma, beta): V consecutive channels as 16-byte loads
template <int V>
__device__ __forceinline__ void bn_ldp(const float* p, float (&v)[V]) {
#pragma unroll
    for (int h = 0; h < V / 4; ++h) {
        const f32x4 t = *(const f32x4*)(p + 4 * h);
        v[4 * h] = t[0]; v[4 * h + 1] = t[1]; v[4 * h + 2] = t[2]; v[4 * h + 3] = t[3];
    }
}
__device__ __forceinline__ void bn_st(float* p, const float (&v)[4]) { *(f32x4*)p = (f32x4){v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ void bn_st(__bf16* p, const float (&v)[8]) {
    f32x8_n t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = v[j];
    *(bf16x8_n*)p = __builtin_convertvector(t, bf16x8_n);
}

template <int V>
__device__ __forceinline__ void bn_stp(float* p, const float (&v)[V]) {
#pragma unroll
    for (int h = 0; h < V / 4; ++h) *(f32x4*)(p + 4 * h) = (f32x4){v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
}

// (bn_norm, the apply expression of every kernel here, lives in dg_common.h: edge.hip's on-load forms evaluate the same text)

// Grouped launches (dg_bn_*_g; round 4): the problems of one launch -- the same BatchNorm layer of the A-side and the B-side network, a
// discriminator layer's real and fake pass (image_translation.py:342-361) -- share M, C and every launch parameter; each has its own
// tensors.  A block index picks the problem (wave-uniform: scalar loads from the kernel arguments); the kernel bodies are the
// one-problem bodies, so a problem's result is bitwise what its own launch computes.
struct BnProb {
    const void* y;        // conv output (statistics, apply, backward)
    const void* dz;       // backward: gradient of the layer's output
    void* out;            // apply: z; backward apply: dy
    void* out16;          // bf16 shadow / plane triple of `out` (one-problem forms only)
    void* ws;             // this problem's workspace: partials [+ backward coefficients]
    float* saved;         // [2][C] mean, invstd
    const float* gamma;
    const float* beta;
    float* rmean;
    float* rvar;
    int64_t* nbt;
    float* dgamma;
    float* dbeta;
};
struct BnGroup {
    BnProb p[DG_MAX_GROUPS];
};

// Reduction-pass geometry: a 256-thread block is TX float4 lanes along channels x TY = 256/TX row lanes, with
// TX = the power of two covering C/4 (capped at 64), so every thread is busy for C = 64 as for C = 512.
// grid = (cchunks, rchunks); each block walks rows r0 + ty + k*TY of its row chunk.
struct BnGrid { int tx, ty, cchunks, rchunks; };
static BnGrid bn_grid(int M, int C, int V = 4) {
    BnGrid g;
    int q = C / V, tx = 1;
    while (tx < q && tx < 64) tx <<= 1;
    g.tx = tx;
    g.ty = 256 / tx;
    g.cchunks = (q + tx - 1) / tx;
    int rc = M / (g.ty * BN_U);            // at least one unrolled trip per row lane
    int cap = 2048 / g.cchunks;
    if (cap > 512) cap = 512;              // the finalize kernels walk this many partials per channel
    if (rc > cap) rc = cap;
    if (rc < 1) rc = 1;
    g.rchunks = rc;
    return g;
}

// part layout: [2][rchunks][C]  (0: sum of (y - shift), 1: sum of (y - shift)^2; shift = y[row 0])
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const BnGroup G, int M, int C, int rchunks, int TX) {
    constexpr int V = BnV<T>::V;
    const T* __restrict__ y = (const T*)G.p[blockIdx.z].y;
    float* __restrict__ part = (float*)G.p[blockIdx.z].ws;
    __shared__ float red[2][256][V];
    const int TY = 256 / TX;
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int c = (blockIdx.x * TX + tx) * V;
    const int rows_per = (M + rchunks - 1) / rchunks;
    const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
    float s[V], q[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = q[j] = 0.f;
    if (c < C) {
        // shifted sums: d = y - y[row 0]; var = E[d^2] - E[d]^2 has no catastrophic cancellation
        // because the shift is itself a sample of the channel (|mean - shift| ~ std).
        float sh[V];
        bn_ld(y + c, sh);
        const T* p = y + c;
        int r = r0 + ty;
        for (; r + (BN_U - 1) * TY < r1; r += BN_U * TY) {
            float v[BN_U][V];
#pragma unroll
            for (int u = 0; u < BN_U; ++u) bn_ld(p + (long)(r + u * TY) * C, v[u]);
#pragma unroll
            for (int u = 0; u < BN_U; ++u)
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    const float d = v[u][j] - sh[j];
                    s[j] += d;
                    q[j] += d * d;
                }
        }
        for (; r < r1; r += TY) {
            float v[V];
            bn_ld(p + (long)r * C, v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float d = v[j] - sh[j];
                s[j] += d;
                q[j] += d * d;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        red[0][threadIdx.x][j] = s[j];
        red[1][threadIdx.x][j] = q[j];
    }
    __syncthreads();
    for (int h = TY >> 1; h > 0; h >>= 1) {     // fixed-order tree over the row lanes
        if (ty < h) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                red[0][threadIdx.x][j] += red[0][threadIdx.x + h * TX][j];
                red[1][threadIdx.x][j] += red[1][threadIdx.x + h * TX][j];
            }
        }
        __syncthreads();
    }
    if (ty == 0 && c < C) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            part[(long)blockIdx.y * C + c + j] = red[0][tx][j];
            part[((long)rchunks + blockIdx.y) * C + c + j] = red[1][tx][j];
        }
    }
}

// Finalize helper: a 256-thread block owns 8 channels; 32 lanes per channel walk the row-chunk
// partials in a fixed order and are combined in fp64 through LDS (deterministic).  Returns the
// channel for the lane that holds the totals, -1 for every other thread.
#define BN_FIN_CH 8
__device__ __forceinline__ int bn_reduce_partials(const float* __restrict__ part, int C, int rchunks, double* s_out, double* q_out) {
    __shared__ double red[2][32][BN_FIN_CH];
    const int cl = threadIdx.x % BN_FIN_CH, pl = threadIdx.x / BN_FIN_CH;
    const int c = blockIdx.x * BN_FIN_CH + cl;
    double s = 0.0, q = 0.0;
    if (c < C) {
        int r = pl;
        for (; r + 96 < rchunks; r += 128) {       // 8 loads in flight, summed in row order
            float vs[4], vq[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                vs[u] = part[(long)(r + 32 * u) * C + c];
                vq[u] = part[((long)rchunks + r + 32 * u) * C + c];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                s += (double)vs[u];
                q += (double)vq[u];
            }
        }
        for (; r < rchunks; r += 32) {
            s += (double)part[(long)r * C + c];
            q += (double)part[((long)rchunks + r) * C + c];
        }
    }
    red[0][pl][cl] = s;
    red[1][pl][cl] = q;
    __syncthreads();
    if (pl != 0 || c >= C) return -1;
    for (int j = 1; j < 32; ++j) {
        s += red[0][j][cl];
        q += red[1][j][cl];
    }
    *s_out = s;
    *q_out = q;
    return c;
}

// blockIdx.y = output set; share > 1: `share` consecutive problems are passes through the SAME BatchNorm module (a discriminator's real
// and fake pass): their running-statistics updates are applied one after the other in problem order by the thread that owns the
// channel -- what `share` consecutive launches leave.
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_finalize_kernel(const BnGroup G, int share, int M, int C, int rchunks, float eps, float momentum) {
    for (int j = 0; j < share; ++j) {
        const BnProb& P = G.p[blockIdx.y * share + j];
        const T* __restrict__ y = (const T*)P.y;
        float* __restrict__ running_mean = P.rmean;
        float* __restrict__ running_var = P.rvar;
        int64_t* __restrict__ nbt = P.nbt;
        float* __restrict__ saved = P.saved;
        double s, q;
        const int c = bn_reduce_partials((const float*)P.ws, C, rchunks, &s, &q);
        if (c >= 0) {
            if (c == 0 && nbt) nbt[0] += 1;
            const double dm = s / M;
            const double mean = (double)y[c] + dm;
            double var = q / M - dm * dm;
            if (var < 0.0) var = 0.0;
            const float invstd = (float)(1.0 / sqrt(var + (double)eps));
            saved[c] = (float)mean;
            saved[C + c] = invstd;
            if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
            if (running_var) {
                const double unb = M > 1 ? var * ((double)M / (double)(M - 1)) : var;
                running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
            }
        }
        if (j + 1 < share) __syncthreads();       // the LDS rows of bn_reduce_partials are reused by the next problem
    }
}

// Finalize from the conv kernels' partial rows [P][3C+4] = {count,-,-,-, shift[C], sum[C], sumsq[C]}.
// Every partial is re-referenced to ONE global shift G (the first row's shift, itself a sample of the
// channel):  sum(y-G) = s_p + n_p*d,  sum((y-G)^2) = q_p + 2*d*s_p + n_p*d^2  with d = shift_p - G, all in
// fp64 FMAs (no divisions in the loop); block = 4 channels x 64 lanes, lanes combined in a fixed order.
__global__ __launch_bounds__(256) void bn_partials_finalize_kernel(const float* __restrict__ stat, int P, int rs, int M, int C,
                                                                  float eps, float momentum, float* __restrict__ running_mean,
                                                                  float* __restrict__ running_var, int64_t* __restrict__ nbt,
                                                                  float* __restrict__ saved) {
    // block = 4 channels (one 16-byte load per row and array), 256 row lanes; fixed-order tree reduction in fp64.
    // (Round 3: the first form gave every thread ONE channel and 64 row lanes -- 4-byte loads, P / 64 iterations -- and cost 41 us
    // per call on the 1024..4096 partial rows the plane kernels emit, more than the statistics pass it replaces.)
    __shared__ double red[256][8];
    const int t = threadIdx.x;
    const int c4 = blockIdx.x * 4;
    double S[4] = {0.0, 0.0, 0.0, 0.0}, Q[4] = {0.0, 0.0, 0.0, 0.0};
    const f32x4 G4 = *(const f32x4*)(stat + 4 + c4);                    // row 0 always has count > 0: the global shift
    for (int p = t; p < P; p += 256) {
        const float* row = stat + (long)p * rs;
        const double np = (double)row[0];
        if (np > 0.0) {
            const f32x4 sh = *(const f32x4*)(row + 4 + c4), s4 = *(const f32x4*)(row + 4 + C + c4), q4 = *(const f32x4*)(row + 4 + 2 * C + c4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double d = (double)sh[j] - (double)G4[j], s = (double)s4[j];
                S[j] += s + np * d;
                Q[j] += (double)q4[j] + d * (2.0 * s + np * d);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[t][j] = S[j];
        red[t][4 + j] = Q[j];
    }
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if (t < half) {
#pragma unroll
            for (int j = 0; j < 8; ++j) red[t][j] += red[t + half][j];
        }
        __syncthreads();
    }
    if (t >= 4) return;
    const int c = c4 + t;
    if (c >= C) return;
    if (c == 0 && nbt) nbt[0] += 1;
    const double dm = red[0][t] / M;
    const double mean = (double)G4[t] + dm;
    double var = red[0][4 + t] / M - dm * dm;
    if (var < 0.0) var = 0.0;
    saved[c] = (float)mean;
    saved[C + c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    if (running_var) {
        const double unb = M > 1 ? var * ((double)M / (double)(M - 1)) : var;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
    }
}

// Two-level form of the same merge for many partial rows.  Level 1: block (channel quad, row block rb of RB) takes rows
// rb * 256 + t, + RB * 256, ... re-referenced to the global shift like the one-launch form and leaves its eight fp64 sums in
// part[rb][0 = S, 1 = Q][C4].  Level 2: one thread per channel adds the RB rows in order and finishes.
__global__ __launch_bounds__(256) void bn_partials_reduce_kernel(const float* __restrict__ stat, int P, int rs, int C, int RB, double* __restrict__ part) {
    __shared__ double red[256][8];
    const int t = threadIdx.x, rb = blockIdx.y;
    const int c4 = blockIdx.x * 4;
    const int C4 = (C + 3) / 4 * 4;
    double S[4] = {0.0, 0.0, 0.0, 0.0}, Q[4] = {0.0, 0.0, 0.0, 0.0};
    const f32x4 G4 = *(const f32x4*)(stat + 4 + c4);
    for (int p = rb * 256 + t; p < P; p += RB * 256) {
        const float* row = stat + (long)p * rs;
        const double np = (double)row[0];
        if (np > 0.0) {
            const f32x4 sh = *(const f32x4*)(row + 4 + c4), s4 = *(const f32x4*)(row + 4 + C + c4), q4 = *(const f32x4*)(row + 4 + 2 * C + c4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double d = (double)sh[j] - (double)G4[j], s = (double)s4[j];
                S[j] += s + np * d;
                Q[j] += (double)q4[j] + d * (2.0 * s + np * d);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[t][j] = S[j];
        red[t][4 + j] = Q[j];
    }
    __syncthreads();
    for (int half = 128; half >= 1; half >>= 1) {
        if (t < half) {
#pragma unroll
            for (int j = 0; j < 8; ++j) red[t][j] += red[t + half][j];
        }
        __syncthreads();
    }
    if (t < 8) part[((long)rb * 2 + (t >> 2)) * C4 + c4 + (t & 3)] = red[0][t];
}
__global__ __launch_bounds__(64) void bn_partials_merge_kernel(const double* __restrict__ part, int RB, const float* __restrict__ stat, int M, int C,
                                                               float eps, float momentum, float* __restrict__ running_mean,
                                                               float* __restrict__ running_var, int64_t* __restrict__ nbt,
                                                               float* __restrict__ saved) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const int C4 = (C + 3) / 4 * 4;
    double S = 0.0, Q = 0.0;
    for (int rb = 0; rb < RB; ++rb) {
        S += part[((long)rb * 2 + 0) * C4 + c];
        Q += part[((long)rb * 2 + 1) * C4 + c];
    }
    if (c == 0 && nbt) nbt[0] += 1;
    const double dm = S / M;
    const double mean = (double)stat[4 + c] + dm;
    double var = Q / M - dm * dm;
    if (var < 0.0) var = 0.0;
    saved[c] = (float)mean;
    saved[C + c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    if (running_var) {
        const double unb = M > 1 ? var * ((double)M / (double)(M - 1)) : var;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
    }
}

typedef __bf16 bf16x4_n __attribute__((ext_vector_type(4)));
// TI / TO: element types of y and z.  Z16 (fp32 z only) = 1: also write a bf16 (RNE) shadow of z for the bf16 matrix path;
// = 3: the three bf16 planes of z for the f32x3 matrix path (dg_split3; planes `pstride` elements apart).  cm != 0: the planes
// are written in the QUAD-CHUNK layout [M / 4][C / 16][4 pixels][16 channels] instead of pixel-major [M][C] -- the layout the
// window input-grad kernel (igemm_dma_x3_dgw.hip) wants: the 16-channel chunk of 4 consecutive pixels is one 128-byte line, so
// a window row of a chunk uses every byte of the lines it touches, while a 4-pixel block of all channels stays one contiguous
// run (the weight-gradient kernel's 16-pixel tile is as contiguous as before).  The work items are then dealt so that 16
// consecutive lanes hold (4 pixels) x (the 4 channel quads of one chunk): a wave reads 4 x 256 contiguous bytes of the fp32
// tensors and writes whole 128-byte lines of every plane.
struct BnItem { long v; int c; long pi; };      // fp32 vector index (4 channels), first channel, plane element index
__device__ __forceinline__ BnItem bn_item(long i, int cvn, int cm) {
    BnItem it;
    if (!cm) {
        it.v = i;
        it.c = (int)(i % cvn) * 4;
        it.pi = i * 4;
        return it;
    }
    // i = ((grp * (cvn / 16) + h) * 4 + pp) * 16 + q16: pixel 4 grp + pp, channel quad 16 h + q16
    const int q16 = (int)(i & 15), pp = (int)((i >> 4) & 3);
    const long rest = i >> 6;
    const int hs = cvn >> 4;
    const int h = (int)(rest % hs);
    const long grp = rest / hs;
    const int cq = h * 16 + q16;
    it.v = (grp * 4 + pp) * cvn + cq;
    it.c = cq * 4;
    it.pi = ((grp * (cvn >> 2) + (cq >> 2)) * 4 + pp) * 16 + (cq & 3) * 4;
    return it;
}
template <typename TI, typename TO, int Z16>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const BnGroup G, long totalv, int C, int act, float slope, long pstride, int cm) {
    constexpr int V = BnV<TI>::V;
    const BnProb& P = G.p[blockIdx.y];
    const TI* __restrict__ y = (const TI*)P.y;
    TO* __restrict__ z = (TO*)P.out;
    const float* __restrict__ saved = P.saved;
    const float* __restrict__ gamma = P.gamma;
    const float* __restrict__ beta = P.beta;
    __bf16* __restrict__ z16 = (__bf16*)P.out16;
    static_assert(BnV<TI>::V == BnV<TO>::V, "same storage type on both sides");
    const int cvn = C / V;
    for (long lin = (long)blockIdx.x * 256 + threadIdx.x; lin < totalv; lin += (long)gridDim.x * 256) {
        long idx = lin, pi = lin * 4;
        int c = (int)(lin % cvn) * V;
        if constexpr (Z16 == 3) {
            const BnItem it = bn_item(lin, cvn, cm);
            idx = it.v; c = it.c; pi = it.pi;
        }
        float v[V], o[V], mean[V], istd[V], g[V], b[V];
        bn_ld(y + idx * V, v);
        bn_ldp<V>(saved + c, mean);
        bn_ldp<V>(saved + C + c, istd);
        bn_ldp<V>(gamma + c, g);
        bn_ldp<V>(beta + c, b);
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = dg_apply_act(bn_norm(v[j], mean[j], g[j] * istd[j], b[j]), act, slope);
        if (Z16 != 3 || z != nullptr) bn_st(z + idx * V, o);      // plane-only output (f32x3 path): the fp32 copy has no reader
        if constexpr (Z16 == 1) *(bf16x4_n*)(z16 + idx * 4) = __builtin_convertvector((f32x4){o[0], o[1], o[2], o[3]}, bf16x4_n);
        if constexpr (Z16 == 3) {
            dg_bf16x4_t h, md, l;
            dg_split3((f32x4){o[0], o[1], o[2], o[3]}, h, md, l);
            *(dg_bf16x4_t*)(z16 + pi) = h;
            *(dg_bf16x4_t*)(z16 + pstride + pi) = md;
            *(dg_bf16x4_t*)(z16 + 2 * pstride + pi) = l;
        }
    }
}

// fp32 storage in the reduction passes' geometry (round 4): fixed channels per thread -- mean / invstd / gamma / beta loaded ONCE instead
// of four 16-byte loads per item, no 64-bit index arithmetic per item --, BN_U rows in flight.  The per-element arithmetic is the
// item kernel's above, expression for expression: results are bitwise the same.  With the plane outputs of the f32x3 path the item
// kernel ran at 3.5 TB/s of its 10 B per element (five load and three store instructions per item) against 4.9 for the plain split
// kernel; this form: see DESIGN.md 3.3.  Plane element index of (row, c): pixel-major row * C + c; quad-chunk
// [M / 4][C / 16][4 pixels][16 channels].  For the quad-chunk layout the host picks TX = 16, so a wave is 4 pixels x 64 channels: whole
// 128-byte lines of every plane (rows_per is a multiple of 4).
__device__ __forceinline__ long bn_plane_index(int row, int c, int C, int cm) {
    if (!cm) return (long)row * C + c;
    return ((((long)(row >> 2)) * (C >> 4) + (c >> 4)) * 4 + (row & 3)) * 16 + (c & 15);
}
typedef __bf16 bf16x8_p __attribute__((ext_vector_type(8)));
// stores the three planes of V (4 | 8) consecutive channels: one 8- or 16-byte store per plane
template <int V>
__device__ __forceinline__ void bn_put_planes(__bf16* p3, long pstride, long pi, const float (&o)[V]) {
    dg_bf16x4_t h[V / 4], md[V / 4], l[V / 4];
#pragma unroll
    for (int q = 0; q < V / 4; ++q) dg_split3((f32x4){o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]}, h[q], md[q], l[q]);
    if constexpr (V == 4) {
        *(dg_bf16x4_t*)(p3 + pi) = h[0];
        *(dg_bf16x4_t*)(p3 + pstride + pi) = md[0];
        *(dg_bf16x4_t*)(p3 + 2 * pstride + pi) = l[0];
    } else {
        *(bf16x8_p*)(p3 + pi) = __builtin_shufflevector(h[0], h[1], 0, 1, 2, 3, 4, 5, 6, 7);
        *(bf16x8_p*)(p3 + pstride + pi) = __builtin_shufflevector(md[0], md[1], 0, 1, 2, 3, 4, 5, 6, 7);
        *(bf16x8_p*)(p3 + 2 * pstride + pi) = __builtin_shufflevector(l[0], l[1], 0, 1, 2, 3, 4, 5, 6, 7);
    }
}
// V = channels per thread: 4, or 8 with plane outputs (two 16-byte loads, ONE 16-byte store per plane: the plane stores of the V = 4
// form were 8-byte stores, three per item)
template <int Z16, int V>
__global__ __launch_bounds__(256) void bn_act_fwd_rows_kernel(const BnGroup G, int M, int C, int rows_per, int TX, int act, float slope, long pstride, int cm) {
    constexpr int U = V == 4 ? BN_U : BN_U / 2;
    const BnProb& P = G.p[blockIdx.z];
    const float* __restrict__ y = (const float*)P.y;
    float* __restrict__ z = (float*)P.out;
    __bf16* __restrict__ z16 = (__bf16*)P.out16;
    const int TY = 256 / TX;
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int c = (blockIdx.x * TX + tx) * V;
    if (c >= C) return;
    const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
    float mean[V], gs[V], b[V];
    bn_ldp<V>(P.saved + c, mean);
    bn_ldp<V>(P.saved + C + c, b);         // invstd for now
    bn_ldp<V>(P.gamma + c, gs);
#pragma unroll
    for (int j = 0; j < V; ++j) gs[j] = gs[j] * b[j];
    bn_ldp<V>(P.beta + c, b);
    auto put = [&](int row, const float (&v)[V]) {
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = dg_apply_act(bn_norm(v[j], mean[j], gs[j], b[j]), act, slope);
        if (Z16 != 3 || z != nullptr) bn_stp<V>(z + (long)row * C + c, o);      // plane-only output (f32x3 path): the fp32 copy has no reader
        if constexpr (Z16 == 1) *(bf16x4_n*)(z16 + (long)row * C + c) = __builtin_convertvector((f32x4){o[0], o[1], o[2], o[3]}, bf16x4_n);
        if constexpr (Z16 == 3) bn_put_planes<V>(z16, pstride, bn_plane_index(row, c, C, cm), o);
    };
    const float* py = y + c;
    int r = r0 + ty;
    for (; r + (U - 1) * TY < r1; r += U * TY) {
        float v[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) bn_ldp<V>(py + (long)(r + u * TY) * C, v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) put(r + u * TY, v[u]);
    }
    for (; r < r1; r += TY) {
        float v[V];
        bn_ldp<V>(py + (long)r * C, v);
        put(r, v);
    }
}

// bf16 storage, forward apply with the reduction passes' geometry: fixed channels per thread (parameters loaded once, no
// 64-bit modulo per access), U rows in flight
__global__ __launch_bounds__(256) void bn_act_fwd16_kernel(const BnGroup G, int M, int C, int rchunks, int TX, int act, float slope) {
    constexpr int V = 8, U = 4;
    const BnProb& P = G.p[blockIdx.z];
    const __bf16* __restrict__ y = (const __bf16*)P.y;
    __bf16* __restrict__ z = (__bf16*)P.out;
    const float* __restrict__ saved = P.saved;
    const float* __restrict__ gamma = P.gamma;
    const float* __restrict__ beta = P.beta;
    const int TY = 256 / TX;
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int c = (blockIdx.x * TX + tx) * V;
    if (c >= C) return;
    const int rows_per = (M + rchunks - 1) / rchunks;
    const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
    float mean[V], gs[V], b[V];
    bn_ldp<V>(saved + c, mean);
    bn_ldp<V>(saved + C + c, b);
    bn_ldp<V>(gamma + c, gs);
#pragma unroll
    for (int j = 0; j < V; ++j) gs[j] *= b[j];
    bn_ldp<V>(beta + c, b);
    const __bf16* py = y + c;
    __bf16* pz = z + c;
    int r = r0 + ty;
    for (; r + (U - 1) * TY < r1; r += U * TY) {
        float v[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) bn_ld(py + (long)(r + u * TY) * C, v[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int j = 0; j < V; ++j) v[u][j] = dg_apply_act(bn_norm(v[u][j], mean[j], gs[j], b[j]), act, slope);
            bn_st(pz + (long)(r + u * TY) * C, v[u]);
        }
    }
    for (; r < r1; r += TY) {
        float v[V];
        bn_ld(py + (long)r * C, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = dg_apply_act(bn_norm(v[j], mean[j], gs[j], b[j]), act, slope);
        bn_st(pz + (long)r * C, v);
    }
}

__device__ __forceinline__ float act_grad(float u, int act, float slope) {
    // derivative taken from the sign of the activation input == sign of its output (in-place
    // semantics of the reference: leaky_relu_backward(result), threshold_backward(result))
    if (act == DG_ACT_LEAKY) return u > 0.f ? 1.f : slope;
    if (act == DG_ACT_RELU) return u > 0.f ? 1.f : 0.f;
    return 1.f;
}

// BatchNorm backward reductions and the final expression run in fp64, like PyTorch's CPU kernels
// (accscalar_t = double): dy is a small difference of large terms whenever the incoming gradient is
// nearly constant within a channel (saturated discriminator), and fp32 there costs percents.
typedef double f64x4 __attribute__((ext_vector_type(4)));
// part layout (fp64): [2][rchunks][C]  (0: sum g, 1: sum g*xhat)
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const BnGroup G, int M, int C, int rchunks, int TX, int act, float slope) {
    constexpr int V = BnV<T>::V;
    const BnProb& P = G.p[blockIdx.z];
    const T* __restrict__ dz = (const T*)P.dz;
    const T* __restrict__ y = (const T*)P.y;
    double* __restrict__ part = (double*)P.ws;
    const float* __restrict__ saved = P.saved;
    const float* __restrict__ gamma = P.gamma;
    const float* __restrict__ beta = P.beta;
    __shared__ double red[2][256][V];
    const int TY = 256 / TX;
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int c = (blockIdx.x * TX + tx) * V;
    const int rows_per = (M + rchunks - 1) / rchunks;
    const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
    double s[V], q[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = q[j] = 0.;
    if (c < C) {
        float mean[V], istd[V], gs[V], b[V];
        bn_ldp<V>(saved + c, mean);
        bn_ldp<V>(saved + C + c, istd);
        bn_ldp<V>(gamma + c, gs);
        bn_ldp<V>(beta + c, b);
#pragma unroll
        for (int j = 0; j < V; ++j) gs[j] *= istd[j];
        auto acc = [&](const float (&v)[V], const float (&d)[V]) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float u = bn_norm(v[j], mean[j], gs[j], b[j]);
                const double gg = (double)(d[j] * act_grad(u, act, slope));
                s[j] += gg;
                q[j] += gg * (((double)v[j] - (double)mean[j]) * (double)istd[j]);
            }
        };
        const T* py = y + c;
        const T* pd = dz + c;
        constexpr int U = V == 4 ? BN_U : BN_U / 2;       // same bytes in flight per thread
        int r = r0 + ty;
        for (; r + (U - 1) * TY < r1; r += U * TY) {
            float v[U][V], d[U][V];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                bn_ld(py + (long)(r + u * TY) * C, v[u]);
                bn_ld(pd + (long)(r + u * TY) * C, d[u]);
            }
            if constexpr (V == 8) {
                // bf16 storage: the inputs carry 8 significant bits, so the U terms of a batch are summed in fp32 and only the
                // batch sums go into the fp64 accumulators (the per-element fp64 chain made this pass compute-bound)
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    float ls = 0.f, lq = 0.f;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const float um = v[u][j] - mean[j];
                        const float gg = d[u][j] * act_grad(fmaf(um, gs[j], b[j]), act, slope);
                        ls += gg;
                        lq = fmaf(gg, um * istd[j], lq);
                    }
                    s[j] += (double)ls;
                    q[j] += (double)lq;
                }
            } else {
#pragma unroll
            for (int u = 0; u < U; ++u) acc(v[u], d[u]);
            }
        }
        for (; r < r1; r += TY) {
            float v[V], d[V];
            bn_ld(py + (long)r * C, v);
            bn_ld(pd + (long)r * C, d);
            acc(v, d);
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        red[0][threadIdx.x][j] = s[j];
        red[1][threadIdx.x][j] = q[j];
    }
    __syncthreads();
    for (int h = TY >> 1; h > 0; h >>= 1) {
        if (ty < h) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                red[0][threadIdx.x][j] += red[0][threadIdx.x + h * TX][j];
                red[1][threadIdx.x][j] += red[1][threadIdx.x + h * TX][j];
            }
        }
        __syncthreads();
    }
    if (ty == 0 && c < C) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            part[(long)blockIdx.y * C + c + j] = red[0][tx][j];
            part[((long)rchunks + blockIdx.y) * C + c + j] = red[1][tx][j];
        }
    }
}

// coef (fp64): [2][C] = dbeta/M, dgamma/M  (kept in the workspace after the partials)
// blockIdx.y = output set; share > 1: `share` consecutive problems went through the SAME BatchNorm module (a discriminator's real and
// fake pass) and accumulate into the same dgamma / dbeta: added one after the other in problem order, as consecutive launches do.
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const BnGroup G, int share, int M, int C, int rchunks, int accumulate) {
    __shared__ double red[2][32][BN_FIN_CH];
    const int cl = threadIdx.x % BN_FIN_CH, pl = threadIdx.x / BN_FIN_CH;
    const int c = blockIdx.x * BN_FIN_CH + cl;
    for (int j = 0; j < share; ++j) {
        const BnProb& P = G.p[blockIdx.y * share + j];
        const double* __restrict__ part = (const double*)P.ws;
        double* __restrict__ coef = (double*)P.ws + (size_t)2 * rchunks * C;
        float* __restrict__ dgamma = P.dgamma;
        float* __restrict__ dbeta = P.dbeta;
        double s = 0.0, q = 0.0;
        if (c < C) {
            int r = pl;
            for (; r + 96 < rchunks; r += 128) {       // 8 loads in flight, summed in row order
                double vs[4], vq[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    vs[u] = part[(long)(r + 32 * u) * C + c];
                    vq[u] = part[((long)rchunks + r + 32 * u) * C + c];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    s += vs[u];
                    q += vq[u];
                }
            }
            for (; r < rchunks; r += 32) {
                s += part[(long)r * C + c];
                q += part[((long)rchunks + r) * C + c];
            }
        }
        if (j > 0) __syncthreads();
        red[0][pl][cl] = s;
        red[1][pl][cl] = q;
        __syncthreads();
        if (pl == 0 && c < C) {
            for (int k = 1; k < 32; ++k) {
                s += red[0][k][cl];
                q += red[1][k][cl];
            }
            coef[c] = s / M;
            coef[C + c] = q / M;
            const int acc = accumulate || j > 0;
            if (dbeta) dbeta[c] = (acc ? dbeta[c] : 0.f) + (float)s;
            if (dgamma) dgamma[c] = (acc ? dgamma[c] : 0.f) + (float)q;
        }
    }
}

// bf16 storage: dz, y in, dy out, all bf16.  The reduction geometry of the partial pass (fixed channels per thread, TY row
// lanes, U rows in flight), so the per-channel constants are loaded ONCE per thread; fp32 arithmetic in the subtraction-first
// form  dy = gs * ((g - c1) - (y - mean) * istd * c2)  -- the inputs carry 8 significant bits and dy is rounded to 8, which
// is what bounds the result, not the fp32 evaluation (the fp32-storage kernel below keeps fp64: there the fp32 chain would be
// the largest error).  Measured: the fp64 form ran at the SAME element rate as the fp32-storage kernel, i.e. compute-bound.
__global__ __launch_bounds__(256) void bn_bwd_apply16_kernel(const BnGroup G, int M, int C, int rchunks, int TX, int coef_rchunks, int act, float slope) {
    constexpr int V = 8, U = 4;
    const BnProb& P = G.p[blockIdx.z];
    const __bf16* __restrict__ dz = (const __bf16*)P.dz;
    const __bf16* __restrict__ y = (const __bf16*)P.y;
    __bf16* __restrict__ dy = (__bf16*)P.out;
    const float* __restrict__ saved = P.saved;
    const float* __restrict__ gamma = P.gamma;
    const float* __restrict__ beta = P.beta;
    const double* __restrict__ coef = (const double*)P.ws + (size_t)2 * coef_rchunks * C;
    const int TY = 256 / TX;
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int c = (blockIdx.x * TX + tx) * V;
    if (c >= C) return;
    const int rows_per = (M + rchunks - 1) / rchunks;
    const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
    float mean[V], gs[V], b[V], c1[V], k2[V];
    bn_ldp<V>(saved + c, mean);
    bn_ldp<V>(saved + C + c, k2);          // invstd for now
    bn_ldp<V>(gamma + c, gs);
    bn_ldp<V>(beta + c, b);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        gs[j] *= k2[j];
        c1[j] = (float)coef[c + j];
        k2[j] = (float)((double)gs[j] * (double)k2[j] * coef[C + c + j]);      // gs * invstd * c2
    }
    auto one = [&](const float (&v)[V], const float (&d)[V], float (&o)[V]) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float um = v[j] - mean[j];
            const float gg = d[j] * act_grad(fmaf(um, gs[j], b[j]), act, slope);
            o[j] = fmaf(-um, k2[j], gs[j] * (gg - c1[j]));
        }
    };
    const __bf16* py = y + c;
    const __bf16* pd = dz + c;
    __bf16* po = dy + c;
    int r = r0 + ty;
    for (; r + (U - 1) * TY < r1; r += U * TY) {
        float v[U][V], d[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            bn_ld(py + (long)(r + u * TY) * C, v[u]);
            bn_ld(pd + (long)(r + u * TY) * C, d[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float o[V];
            one(v[u], d[u], o);
            bn_st(po + (long)(r + u * TY) * C, o);
        }
    }
    for (; r < r1; r += TY) {
        float v[V], d[V], o[V];
        bn_ld(py + (long)r * C, v);
        bn_ld(pd + (long)r * C, d);
        one(v, d, o);
        bn_st(po + (long)r * C, o);
    }
}

// T: element type of dz / y / dy.  D16 (fp32 only) = 1: also write a bf16 shadow of dy; = 3: its three bf16 planes
template <typename T, int D16>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const BnGroup G, long totalv, int C, int coef_rchunks, int act, float slope, long pstride, int cm) {
    constexpr int V = BnV<T>::V;
    const BnProb& P = G.p[blockIdx.y];
    const T* __restrict__ dz = (const T*)P.dz;
    const T* __restrict__ y = (const T*)P.y;
    T* __restrict__ dy = (T*)P.out;
    const float* __restrict__ saved = P.saved;
    const float* __restrict__ gamma = P.gamma;
    const float* __restrict__ beta = P.beta;
    const double* __restrict__ coef = (const double*)P.ws + (size_t)2 * coef_rchunks * C;
    __bf16* __restrict__ dy16 = (__bf16*)P.out16;
    const int cvn = C / V;
    for (long lin = (long)blockIdx.x * 256 + threadIdx.x; lin < totalv; lin += (long)gridDim.x * 256) {
        long idx = lin, pi = lin * 4;
        int c = (int)(lin % cvn) * V;
        if constexpr (D16 == 3) {
            const BnItem it = bn_item(lin, cvn, cm);
            idx = it.v; c = it.c; pi = it.pi;
        }
        float v[V], d[V], o[V], mean[V], istd[V], g[V], b[V];
        bn_ld(y + idx * V, v);
        bn_ld(dz + idx * V, d);
        bn_ldp<V>(saved + c, mean);
        bn_ldp<V>(saved + C + c, istd);
        bn_ldp<V>(gamma + c, g);
        bn_ldp<V>(beta + c, b);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float gs = g[j] * istd[j];
            const float u = bn_norm(v[j], mean[j], gs, b[j]);
            const double gg = (double)(d[j] * act_grad(u, act, slope));
            const double xhat = ((double)v[j] - (double)mean[j]) * (double)istd[j];
            o[j] = (float)((double)g[j] * (double)istd[j] * (gg - coef[c + j] - xhat * coef[C + c + j]));
        }
        if (D16 != 3 || dy != nullptr) bn_st(dy + idx * V, o);   // plane-only output (f32x3 path): the fp32 copy has no reader
        if constexpr (D16 == 1) *(bf16x4_n*)(dy16 + idx * 4) = __builtin_convertvector((f32x4){o[0], o[1], o[2], o[3]}, bf16x4_n);
        if constexpr (D16 == 3) {
            dg_bf16x4_t h, md, l;
            dg_split3((f32x4){o[0], o[1], o[2], o[3]}, h, md, l);
            *(dg_bf16x4_t*)(dy16 + pi) = h;
            *(dg_bf16x4_t*)(dy16 + pstride + pi) = md;
            *(dg_bf16x4_t*)(dy16 + 2 * pstride + pi) = l;
        }
    }
}

// the fp32-storage backward apply in the same geometry (see bn_act_fwd_rows_kernel): per-channel constants -- the four parameters and the
// two fp64 coefficients -- once per thread instead of six 16-byte and eight 8-byte loads per item; the item kernel's fp64 expression.
template <int D16, int V>
__global__ __launch_bounds__(256) void bn_bwd_apply_rows_kernel(const BnGroup G, int M, int C, int rows_per, int TX, int coef_rchunks, int act, float slope,
                                                                long pstride, int cm) {
    constexpr int U = V == 4 ? BN_U / 2 : BN_U / 4;
    const BnProb& P = G.p[blockIdx.z];
    const float* __restrict__ dz = (const float*)P.dz;
    const float* __restrict__ y = (const float*)P.y;
    float* __restrict__ dy = (float*)P.out;
    __bf16* __restrict__ dy16 = (__bf16*)P.out16;
    const double* __restrict__ coef = (const double*)P.ws + (size_t)2 * coef_rchunks * C;
    const int TY = 256 / TX;
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int c = (blockIdx.x * TX + tx) * V;
    if (c >= C) return;
    const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
    float mean[V], istd[V], g[V], b[V], gs[V];
    double c1[V], c2[V];
    bn_ldp<V>(P.saved + c, mean);
    bn_ldp<V>(P.saved + C + c, istd);
    bn_ldp<V>(P.gamma + c, g);
    bn_ldp<V>(P.beta + c, b);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        gs[j] = g[j] * istd[j];
        c1[j] = coef[c + j];
        c2[j] = coef[C + c + j];
    }
    auto put = [&](int row, const float (&v)[V], const float (&d)[V]) {
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float u = bn_norm(v[j], mean[j], gs[j], b[j]);
            const double gg = (double)(d[j] * act_grad(u, act, slope));
            const double xhat = ((double)v[j] - (double)mean[j]) * (double)istd[j];
            o[j] = (float)((double)g[j] * (double)istd[j] * (gg - c1[j] - xhat * c2[j]));
        }
        if (D16 != 3 || dy != nullptr) bn_stp<V>(dy + (long)row * C + c, o);   // plane-only output (f32x3 path): the fp32 copy has no reader
        if constexpr (D16 == 1) *(bf16x4_n*)(dy16 + (long)row * C + c) = __builtin_convertvector((f32x4){o[0], o[1], o[2], o[3]}, bf16x4_n);
        if constexpr (D16 == 3) bn_put_planes<V>(dy16, pstride, bn_plane_index(row, c, C, cm), o);
    };
    const float* py = y + c;
    const float* pd = dz + c;
    int r = r0 + ty;
    for (; r + (U - 1) * TY < r1; r += U * TY) {
        float v[U][V], d[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            bn_ldp<V>(py + (long)(r + u * TY) * C, v[u]);
            bn_ldp<V>(pd + (long)(r + u * TY) * C, d[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) put(r + u * TY, v[u], d[u]);
    }
    for (; r < r1; r += TY) {
        float v[V], d[V];
        bn_ldp<V>(py + (long)r * C, v);
        bn_ldp<V>(pd + (long)r * C, d);
        put(r, v, d);
    }
}
// geometry of the two kernels above: TX channel lanes (16 for quad-chunk planes: a wave = 4 pixels x 64 channels), row chunks of a multiple of
// 8 rows.  Geometry only: bn_form() decides which shapes take these kernels (C a multiple of 64, M of 8).
struct BnRows { int tx, cchunks, rchunks, rows_per; };
static BnRows bn_rows(int M, int C, int cm, int V) {
    BnRows g;
    g.tx = 64 / V;                                  // quad-chunk planes: a wave = 4 (8) pixels x 64 channels
    if (!cm) while (g.tx < C / V && g.tx < 64) g.tx <<= 1;
    g.cchunks = (C / V + g.tx - 1) / g.tx;         // ragged last chunk (C = 192, 320, ...): the kernels return on c >= C
    const int ty = 256 / g.tx;
    long rc = M / ((long)ty * BN_U);
    long cap = 4096 / g.cchunks;
    if (rc > cap) rc = cap;
    if (rc < 1) rc = 1;
    g.rows_per = (int)(((M + rc - 1) / rc + 7) / 8 * 8);
    g.rchunks = (M + g.rows_per - 1) / g.rows_per;
    return g;
}

__global__ __launch_bounds__(256) void act_fwd_kernel(const DgPtrs xs, const DgPtrs ys, long total4, long n, int act, float slope) {
    const float* __restrict__ x = dg_pick<const float>(xs, blockIdx.y);
    float* __restrict__ y = dg_pick<float>(ys, blockIdx.y);
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total4; idx += (long)gridDim.x * 256) {
        if (idx * 4 + 3 < n) {
            const f32x4 v = *(const f32x4*)(x + idx * 4);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = act == DG_ACT_SIGMOID ? 1.f / (1.f + expf(-v[j])) : dg_apply_act(v[j], act, slope);
            *(f32x4*)(y + idx * 4) = o;
        } else {
            for (long e = idx * 4; e < n; ++e)
                y[e] = act == DG_ACT_SIGMOID ? 1.f / (1.f + expf(-x[e])) : dg_apply_act(x[e], act, slope);
        }
    }
}

__device__ __forceinline__ float act_bwd_one(float dy, float out, int act, float slope) {
    if (act == DG_ACT_SIGMOID) return dy * (1.f - out) * out;  // sigmoid_backward: grad * (1 - y) * y
    if (act == DG_ACT_LEAKY) return out > 0.f ? dy : dy * slope;
    if (act == DG_ACT_RELU) return out > 0.f ? dy : 0.f;
    return dy;
}
__global__ __launch_bounds__(256) void act_bwd_kernel(const DgPtrs dys, const DgPtrs outs, const DgPtrs dxs, long total4, long n, int act, float slope) {
    const float* __restrict__ dy = dg_pick<const float>(dys, blockIdx.y);
    const float* __restrict__ out = dg_pick<const float>(outs, blockIdx.y);
    float* __restrict__ dx = dg_pick<float>(dxs, blockIdx.y);
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total4; idx += (long)gridDim.x * 256) {
        if (idx * 4 + 3 < n) {
            const f32x4 d = *(const f32x4*)(dy + idx * 4), o = *(const f32x4*)(out + idx * 4);
            f32x4 r;
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = act_bwd_one(d[j], o[j], act, slope);
            *(f32x4*)(dx + idx * 4) = r;
        } else {
            for (long e = idx * 4; e < n; ++e) dx[e] = act_bwd_one(dy[e], out[e], act, slope);
        }
    }
}

// bf16 in / bf16 out (n % 8 == 0): the first layer's fused LeakyReLU backward on the bf16-stored gradient
__global__ __launch_bounds__(256) void act_bwd16_kernel(const __bf16* __restrict__ dy, const __bf16* __restrict__ out,
                                                        __bf16* __restrict__ dx, long total8, int act, float slope) {
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total8; idx += (long)gridDim.x * 256) {
        float d[8], o[8], r[8];
        bn_ld(dy + idx * 8, d);
        bn_ld(out + idx * 8, o);
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = act_bwd_one(d[j], o[j], act, slope);
        bn_st(dx + idx * 8, r);
    }
}

static int stream_grid(long total4) {
    long g = (total4 + 255) / 256;
    long cap = 2048;
#ifdef DG_EXPERIMENTS
    if (const int v = dg_get_option(DG_OPT_UNDERSTORY); v < 0) cap = -(long)v;      // probe: another cap on the workgroups of a streaming pass
#endif
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

extern "C" size_t dg_bn_workspace_bytes(int M, int C) {
    const BnGrid g = bn_grid(M, C);                                        // V = 4 needs the larger one (more channel lanes)
    return ((size_t)2 * g.rchunks * C + 2 * (size_t)C) * sizeof(double);   // fp64 partials in the backward
}

// ---- BatchNorm host layer: one call record, three passes ------------------------------------------------------------------------
// Every dg_bn_* entry point fills one BnCall on its stack and calls its pass (bn_stats, bn_fwd, bn_bwd); a pass validates the record once,
// names the apply form (bn_form) and launches.  Nothing below an entry point reads a process-wide option.
enum BnExtra { BN_EXTRA_NONE = 0, BN_EXTRA_SHADOW = 1, BN_EXTRA_PLANES = 2 };
struct BnCall {
    const char* who;                        // the entry point's public name, for messages
    int groups;                             // problems of this launch (1 .. DG_MAX_GROUPS)
    int share;                              // consecutive problems through the same module: one finalize block sums them (1: none)
    bool null_table;                        // a *_g entry point was handed a null pointer table (its problems are then not read)
    BnGroup G;                              // the problems' pointers: the kernel argument as it stands
    int M, C;                               // rows (N * H * W) and channels of every problem
    bool bf16;                              // activation storage: y / z / dz / dy are bf16 (io_bf16), else fp32; everything else stays fp32
    BnExtra extra;                          // second output beside p[0].out, at p[0].out16 (one problem): none | bf16 shadow | bf16 plane triple
    size_t plane_elems;                     // planes: elements from one plane to the next (>= M * C, % 8 == 0)
    int plane_layout;                       // planes: 0 pixel-major, 1 quad-chunk (C % 64 == 0, M % 4 == 0)
    bool write_out;                         // p[i].out is written; false (planes only): the plane triple is the only output
    int act;                                // apply passes: DG_ACT_NONE | _LEAKY | _RELU,
    float slope;                            // and LeakyReLU's slope
    float eps, momentum;                    // statistics pass
    int accumulate;                         // backward: add to dgamma / dbeta instead of overwriting them
    size_t ws_bytes;                        // bytes behind every p[i].ws (dg_bn_workspace_bytes)
    int items;                              // apply passes: option "bn_items", read where the call entered the library (item kernels everywhere)
    hipStream_t st;
};
// one fp32 problem, no second output: an entry point overwrites what it differs in
static BnCall bn_call(const char* who, int M, int C, dg_stream_t stream) {
    BnCall c = BnCall();
    c.who = who; c.groups = c.share = 1; c.M = M; c.C = C; c.write_out = true; c.st = (hipStream_t)stream;
    return c;
}
static BnCall bn_apply_call(const char* who, int M, int C, int act, float slope, dg_stream_t stream) {
    BnCall c = bn_call(who, M, C, stream);
    c.act = act; c.slope = slope; c.items = dg_get_option(DG_OPT_BN_ITEMS);
    return c;
}
// a *_g entry point: groups, share (< 1 -> 1) and how many problems to read from its tables (none when a table is missing)
static int bn_grouped(BnCall& c, int groups, int share, bool tables) {
    c.groups = groups; c.share = share < 1 ? 1 : share; c.null_table = !tables;
    return tables && groups >= 1 && groups <= DG_MAX_GROUPS ? groups : 0;
}

// What a pass needs of a call: per-problem pointers beyond y and saved, and the checks that not every pass makes.
enum { BN_NEED_DZ = 1, BN_NEED_OUT = 2, BN_NEED_AFFINE = 4, BN_NEED_WS = 8, BN_NEED_ROWS2 = 16, BN_NEED_ACT = 32 };
// The one validation.  Every refusal is DG_ERR_INVALID, except the workspace's (DG_ERR_WORKSPACE), which comes last.
static int bn_validate(const BnCall& c, int need) {
    const int M = c.M, C = c.C, V = c.bf16 ? 8 : 4;
    DG_CHECK_ARG(c.groups >= 1 && c.groups <= DG_MAX_GROUPS && !c.null_table, "%s: groups=%d (1..%d) or a null table", c.who, c.groups, DG_MAX_GROUPS);
    DG_CHECK_ARG(c.share >= 1 && c.groups % c.share == 0, "%s: groups=%d share=%d", c.who, c.groups, c.share);
    DG_CHECK_ARG(c.groups == 1 || c.extra == BN_EXTRA_NONE, "%s: shadow / plane outputs exist in the one-problem forms only", c.who);
    for (int i = 0; i < c.groups; ++i) {
        const BnProb &P = c.G.p[i], &S = c.G.p[i / c.share * c.share];
        DG_CHECK_ARG(P.rmean == S.rmean && P.dgamma == S.dgamma && P.dbeta == S.dbeta,
                     "%s: problems of one share set must name the same module buffers (running_mean, dgamma, dbeta)", c.who);
        DG_CHECK_ARG(P.y && P.saved && (!(need & BN_NEED_DZ) || P.dz) && (!(need & BN_NEED_OUT) || !c.write_out || P.out) &&
                         (!(need & BN_NEED_AFFINE) || (P.gamma && P.beta)),
                     "%s: null pointer (problem %d)", c.who, i);
    }
    if (c.extra != BN_EXTRA_NONE)
        DG_CHECK_ARG(c.G.p[0].out16, "%s: null %s pointer", c.who, c.extra == BN_EXTRA_PLANES ? "plane" : "shadow");
    if (c.extra == BN_EXTRA_PLANES) {
        DG_CHECK_ARG(c.plane_layout == 0 || c.plane_layout == 1, "%s: plane_layout 0 (pixel-major) or 1 (quad-chunk)", c.who);
        DG_CHECK_ARG(c.plane_elems >= (size_t)M * C && c.plane_elems % 8 == 0, "%s: plane distance %zu for %ld elements", c.who, c.plane_elems, (long)M * C);
        DG_CHECK_ARG(!c.plane_layout || (C % 64 == 0 && M % 4 == 0), "%s: quad-chunk planes need C %% 64 == 0 and M %% 4 == 0 (C=%d, M=%d)", c.who, C, M);
    }
    if (need & BN_NEED_ROWS2) DG_CHECK_ARG(M >= 2, "%s: Expected more than 1 value per channel when training (M=%d)", c.who, M);
    DG_CHECK_ARG(C >= V && C % V == 0, "%s: C=%d must be a multiple of %d", c.who, C, V);
    if (need & BN_NEED_ACT) DG_CHECK_ARG(c.act == DG_ACT_NONE || c.act == DG_ACT_LEAKY || c.act == DG_ACT_RELU, "%s: bad act %d", c.who, c.act);
    if (need & BN_NEED_WS) {
        const size_t want = dg_bn_workspace_bytes(M, C);
        for (int i = 0; i < c.groups; ++i)
            if (c.G.p[i].ws == nullptr || c.ws_bytes < want) return dg_fail(DG_ERR_WORKSPACE, "%s: workspace %zu < %zu", c.who, c.ws_bytes, want);
    }
    return DG_OK;
}

// The apply form of a forward / backward pass: the kernel that moves the activations, and what it writes beside `out`.
enum BnApply {
    BN_APPLY_BF16,                                                              // bf16 storage
    BN_APPLY_ROWS, BN_APPLY_ROWS_SHADOW, BN_APPLY_ROWS_PLANES,                  // rows kernels + BnExtra
    BN_APPLY_ITEMS, BN_APPLY_ITEMS_SHADOW, BN_APPLY_ITEMS_PLANES                // item kernels + BnExtra
};
struct BnForm { BnApply apply; BnRows rows; };                                  // rows: the rows kernels' geometry (BN_APPLY_ROWS* only)
// Pure: no option, no global.  In priority order:
//   1. bf16 storage has one kernel per pass (8 channels per lane on the reduction passes' grid) and no second output;
//   2. the rows kernels take C % 64 == 0 && M % 8 == 0, unless `items` asks for the item kernels; planes move V = 8 channels per lane, and
//      quad-chunk planes (layout 1) keep tx = 64 / V (bn_rows);
//   3. every other shape goes to the item kernels.
// Within 2 and 3 the second output picks the instantiation.
static BnForm bn_form(bool bf16, BnExtra extra, int layout, int M, int C, int items) {
    BnForm f = BnForm();
    const bool rows = !bf16 && C % 64 == 0 && M % 8 == 0 && !items;
    f.apply = bf16 ? BN_APPLY_BF16 : (BnApply)((rows ? BN_APPLY_ROWS : BN_APPLY_ITEMS) + extra);
    if (rows) f.rows = bn_rows(M, C, layout, extra == BN_EXTRA_PLANES ? 8 : 4);
    return f;
}

#define BN_LAUNCH(kernel, grid, ...) hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c.st, c.G, __VA_ARGS__)

static int bn_stats(const BnCall& c) {
    if (const int rc = bn_validate(c, BN_NEED_WS | BN_NEED_ROWS2)) return rc;
    const BnGrid g = bn_grid(c.M, c.C, c.bf16 ? 8 : 4);
    const dim3 pgrid(g.cchunks, g.rchunks, c.groups), fgrid((c.C + BN_FIN_CH - 1) / BN_FIN_CH, c.groups / c.share);
    if (c.bf16) BN_LAUNCH(bn_stats_partial_kernel<__bf16>, pgrid, c.M, c.C, g.rchunks, g.tx);
    else BN_LAUNCH(bn_stats_partial_kernel<float>, pgrid, c.M, c.C, g.rchunks, g.tx);
    DG_CHECK_LAUNCH("bn_stats_partial");
    if (c.bf16) BN_LAUNCH(bn_stats_finalize_kernel<__bf16>, fgrid, c.share, c.M, c.C, g.rchunks, c.eps, c.momentum);
    else BN_LAUNCH(bn_stats_finalize_kernel<float>, fgrid, c.share, c.M, c.C, g.rchunks, c.eps, c.momentum);
    DG_CHECK_LAUNCH("bn_stats_finalize");
    return DG_OK;
}

static int bn_fwd(const BnCall& c) {
    if (const int rc = bn_validate(c, BN_NEED_OUT | BN_NEED_AFFINE | BN_NEED_ACT)) return rc;
    const BnForm f = bn_form(c.bf16, c.extra, c.plane_layout, c.M, c.C, c.items);
    const BnRows& r = f.rows;
    const int M = c.M, C = c.C, act = c.act, cm = c.plane_layout;
    const float slope = c.slope;
    const long total4 = (long)M * C / 4, ps = (long)c.plane_elems;
    const dim3 rgrid(r.cchunks, r.rchunks, c.groups), igrid(stream_grid(total4), c.groups);
    switch (f.apply) {
    case BN_APPLY_BF16: {
        const BnGrid g = bn_grid(M, C, 8);
        BN_LAUNCH(bn_act_fwd16_kernel, dim3(g.cchunks, g.rchunks, c.groups), M, C, g.rchunks, g.tx, act, slope);
        break;
    }
    case BN_APPLY_ROWS:         BN_LAUNCH((bn_act_fwd_rows_kernel<0, 4>), rgrid, M, C, r.rows_per, r.tx, act, slope, 0L, 0); break;
    case BN_APPLY_ROWS_SHADOW:  BN_LAUNCH((bn_act_fwd_rows_kernel<1, 4>), rgrid, M, C, r.rows_per, r.tx, act, slope, 0L, 0); break;
    case BN_APPLY_ROWS_PLANES:  BN_LAUNCH((bn_act_fwd_rows_kernel<3, 8>), rgrid, M, C, r.rows_per, r.tx, act, slope, ps, cm); break;
    case BN_APPLY_ITEMS:        BN_LAUNCH((bn_act_fwd_kernel<float, float, 0>), igrid, total4, C, act, slope, 0L, 0); break;
    case BN_APPLY_ITEMS_SHADOW: BN_LAUNCH((bn_act_fwd_kernel<float, float, 1>), igrid, total4, C, act, slope, 0L, 0); break;
    case BN_APPLY_ITEMS_PLANES: BN_LAUNCH((bn_act_fwd_kernel<float, float, 3>), igrid, total4, C, act, slope, ps, cm); break;
    }
    DG_CHECK_LAUNCH("bn_act_fwd");
    return DG_OK;
}

static int bn_bwd(const BnCall& c) {
    if (const int rc = bn_validate(c, BN_NEED_DZ | BN_NEED_OUT | BN_NEED_AFFINE | BN_NEED_ACT | BN_NEED_WS)) return rc;
    const BnForm f = bn_form(c.bf16, c.extra, c.plane_layout, c.M, c.C, c.items);
    const BnRows& r = f.rows;
    const int M = c.M, C = c.C, act = c.act, cm = c.plane_layout;
    const float slope = c.slope;
    const BnGrid g = bn_grid(M, C, c.bf16 ? 8 : 4);
    const int rc = g.rchunks;                                                   // partials per channel: also what the apply kernels' coefficients came from
    const long total4 = (long)M * C / 4, ps = (long)c.plane_elems;
    const dim3 pgrid(g.cchunks, rc, c.groups), rgrid(r.cchunks, r.rchunks, c.groups), igrid(stream_grid(total4), c.groups);
    if (c.bf16) BN_LAUNCH(bn_bwd_partial_kernel<__bf16>, pgrid, M, C, rc, g.tx, act, slope);
    else BN_LAUNCH(bn_bwd_partial_kernel<float>, pgrid, M, C, rc, g.tx, act, slope);
    DG_CHECK_LAUNCH("bn_bwd_partial");
    BN_LAUNCH(bn_bwd_finalize_kernel, dim3((C + BN_FIN_CH - 1) / BN_FIN_CH, c.groups / c.share), c.share, M, C, rc, c.accumulate);
    DG_CHECK_LAUNCH("bn_bwd_finalize");
    switch (f.apply) {
    case BN_APPLY_BF16:         BN_LAUNCH(bn_bwd_apply16_kernel, pgrid, M, C, rc, g.tx, rc, act, slope); break;
    case BN_APPLY_ROWS:         BN_LAUNCH((bn_bwd_apply_rows_kernel<0, 4>), rgrid, M, C, r.rows_per, r.tx, rc, act, slope, 0L, 0); break;
    case BN_APPLY_ROWS_SHADOW:  BN_LAUNCH((bn_bwd_apply_rows_kernel<1, 4>), rgrid, M, C, r.rows_per, r.tx, rc, act, slope, 0L, 0); break;
    case BN_APPLY_ROWS_PLANES:  BN_LAUNCH((bn_bwd_apply_rows_kernel<3, 8>), rgrid, M, C, r.rows_per, r.tx, rc, act, slope, ps, cm); break;
    case BN_APPLY_ITEMS:        BN_LAUNCH((bn_bwd_apply_kernel<float, 0>), igrid, total4, C, rc, act, slope, 0L, 0); break;
    case BN_APPLY_ITEMS_SHADOW: BN_LAUNCH((bn_bwd_apply_kernel<float, 1>), igrid, total4, C, rc, act, slope, 0L, 0); break;
    case BN_APPLY_ITEMS_PLANES: BN_LAUNCH((bn_bwd_apply_kernel<float, 3>), igrid, total4, C, rc, act, slope, ps, cm); break;
    }
    DG_CHECK_LAUNCH("bn_bwd_apply");
    return DG_OK;
}
#undef BN_LAUNCH

// ---- entry points: fill the record, call the pass ---------------------------------------------------------------------------------
static int bn_stats_one(const char* who, const void* y, int io_bf16, int M, int C, float eps, float momentum, float* running_mean, float* running_var,
                        int64_t* nbt, float* saved, void* ws, size_t ws_bytes, dg_stream_t stream) {
    BnCall c = bn_call(who, M, C, stream);
    c.bf16 = io_bf16 != 0; c.eps = eps; c.momentum = momentum; c.ws_bytes = ws_bytes;
    BnProb& P = c.G.p[0];
    P.y = y; P.rmean = running_mean; P.rvar = running_var; P.nbt = nbt; P.saved = saved; P.ws = ws;
    return bn_stats(c);
}
extern "C" int dg_bn_train_stats_t(const void* y, int io_bf16, int M, int C, float eps, float momentum, float* running_mean,
                                   float* running_var, int64_t* nbt, float* saved, void* ws, size_t ws_bytes,
                                   dg_stream_t stream) {
    return bn_stats_one("dg_bn_train_stats_t", y, io_bf16, M, C, eps, momentum, running_mean, running_var, nbt, saved, ws, ws_bytes, stream);
}
extern "C" int dg_bn_train_stats(const float* y, int M, int C, float eps, float momentum, float* running_mean,
                                 float* running_var, int64_t* nbt, float* saved, void* ws, size_t ws_bytes,
                                 dg_stream_t stream) {
    return bn_stats_one("dg_bn_train_stats", y, 0, M, C, eps, momentum, running_mean, running_var, nbt, saved, ws, ws_bytes, stream);
}
extern "C" int dg_bn_train_stats_g(int groups, int share, const float* const* y, int M, int C, float eps, float momentum, float* const* running_mean,
                                   float* const* running_var, int64_t* const* nbt, float* const* saved, void* const* ws, size_t ws_bytes,
                                   dg_stream_t stream) {
    BnCall c = bn_call("dg_bn_train_stats_g", M, C, stream);
    c.eps = eps; c.momentum = momentum; c.ws_bytes = ws_bytes;
    for (int i = 0, n = bn_grouped(c, groups, share, y && saved && ws); i < n; ++i) {
        BnProb& P = c.G.p[i];
        P.y = y[i]; P.saved = saved[i]; P.ws = ws[i];
        P.rmean = running_mean ? running_mean[i] : nullptr;
        P.rvar = running_var ? running_var[i] : nullptr;
        P.nbt = nbt ? nbt[i] : nullptr;
    }
    return bn_stats(c);
}

static BnCall bn_fwd_call(const char* who, const void* y, void* z, int M, int C, const float* saved, const float* gamma, const float* beta, int act,
                          float slope, dg_stream_t stream) {
    BnCall c = bn_apply_call(who, M, C, act, slope, stream);
    BnProb& P = c.G.p[0];
    P.y = y; P.out = z; P.saved = (float*)saved; P.gamma = gamma; P.beta = beta;
    return c;
}
extern "C" int dg_bn_act_fwd(const float* y, float* z, int M, int C, const float* saved, const float* gamma,
                             const float* beta, int act, float slope, dg_stream_t stream) {
    return bn_fwd(bn_fwd_call("dg_bn_act_fwd", y, z, M, C, saved, gamma, beta, act, slope, stream));
}
extern "C" int dg_bn_act_fwd_g(int groups, const float* const* y, float* const* z, int M, int C, const float* const* saved, const float* const* gamma,
                               const float* const* beta, int act, float slope, dg_stream_t stream) {
    BnCall c = bn_apply_call("dg_bn_act_fwd_g", M, C, act, slope, stream);
    for (int i = 0, n = bn_grouped(c, groups, 1, y && z && saved && gamma && beta); i < n; ++i) {
        BnProb& P = c.G.p[i];
        P.y = y[i]; P.out = z[i]; P.saved = (float*)saved[i]; P.gamma = gamma[i]; P.beta = beta[i];
    }
    return bn_fwd(c);
}
extern "C" int dg_bn_act_fwd_bf16(const float* y, float* z, void* z_bf16, int M, int C, const float* saved, const float* gamma,
                                  const float* beta, int act, float slope, dg_stream_t stream) {
    BnCall c = bn_fwd_call("dg_bn_act_fwd_bf16", y, z, M, C, saved, gamma, beta, act, slope, stream);
    c.extra = BN_EXTRA_SHADOW; c.G.p[0].out16 = z_bf16;
    return bn_fwd(c);
}
// the same pass, also writing the three bf16 planes of z (plane_elems elements apart, >= M * C, % 8 == 0) for the f32x3 matrix path;
// z == nullptr: the planes only
extern "C" int dg_bn_act_fwd_x3(const float* y, float* z, void* z_planes, size_t plane_elems, int plane_layout, int M, int C, const float* saved,
                                const float* gamma, const float* beta, int act, float slope, dg_stream_t stream) {
    BnCall c = bn_fwd_call("dg_bn_act_fwd_x3", y, z, M, C, saved, gamma, beta, act, slope, stream);
    c.extra = BN_EXTRA_PLANES; c.G.p[0].out16 = z_planes; c.plane_elems = plane_elems; c.plane_layout = plane_layout; c.write_out = z != nullptr;
    return bn_fwd(c);
}
extern "C" int dg_bn_act_fwd_t(const void* y, void* z, int io_bf16, int M, int C, const float* saved, const float* gamma,
                               const float* beta, int act, float slope, dg_stream_t stream) {
    BnCall c = bn_fwd_call("dg_bn_act_fwd_t", y, z, M, C, saved, gamma, beta, act, slope, stream);
    c.bf16 = io_bf16 != 0;
    return bn_fwd(c);
}

static void bn_bwd_prob(BnProb& P, const void* dz, const void* y, void* dy, const float* saved, const float* gamma, const float* beta, float* dgamma,
                        float* dbeta, void* ws) {
    P.dz = dz; P.y = y; P.out = dy; P.saved = (float*)saved; P.gamma = gamma; P.beta = beta; P.dgamma = dgamma; P.dbeta = dbeta; P.ws = ws;
}
static BnCall bn_bwd_call(const char* who, const void* dz, const void* y, void* dy, int M, int C, const float* saved, const float* gamma,
                          const float* beta, int act, float slope, float* dgamma, float* dbeta, int accumulate, void* ws, size_t ws_bytes,
                          dg_stream_t stream) {
    BnCall c = bn_apply_call(who, M, C, act, slope, stream);
    c.accumulate = accumulate; c.ws_bytes = ws_bytes;
    bn_bwd_prob(c.G.p[0], dz, y, dy, saved, gamma, beta, dgamma, dbeta, ws);
    return c;
}
extern "C" int dg_bn_act_bwd(const float* dz, const float* y, float* dy, int M, int C, const float* saved,
                             const float* gamma, const float* beta, int act, float slope, float* dgamma, float* dbeta,
                             int accumulate, void* ws, size_t ws_bytes, dg_stream_t stream) {
    return bn_bwd(bn_bwd_call("dg_bn_act_bwd", dz, y, dy, M, C, saved, gamma, beta, act, slope, dgamma, dbeta, accumulate, ws, ws_bytes, stream));
}
extern "C" int dg_bn_act_bwd_g(int groups, int share, const float* const* dz, const float* const* y, float* const* dy, int M, int C,
                               const float* const* saved, const float* const* gamma, const float* const* beta, int act, float slope,
                               float* const* dgamma, float* const* dbeta, int accumulate, void* const* ws, size_t ws_bytes, dg_stream_t stream) {
    BnCall c = bn_apply_call("dg_bn_act_bwd_g", M, C, act, slope, stream);
    c.accumulate = accumulate; c.ws_bytes = ws_bytes;
    for (int i = 0, n = bn_grouped(c, groups, share, dz && y && dy && saved && gamma && beta && ws); i < n; ++i)
        bn_bwd_prob(c.G.p[i], dz[i], y[i], dy[i], saved[i], gamma[i], beta[i], dgamma ? dgamma[i] : nullptr, dbeta ? dbeta[i] : nullptr, ws[i]);
    return bn_bwd(c);
}
extern "C" int dg_bn_act_bwd_bf16(const float* dz, const float* y, float* dy, void* dy_bf16, int M, int C, const float* saved,
                                  const float* gamma, const float* beta, int act, float slope, float* dgamma, float* dbeta,
                                  int accumulate, void* ws, size_t ws_bytes, dg_stream_t stream) {
    BnCall c = bn_bwd_call("dg_bn_act_bwd_bf16", dz, y, dy, M, C, saved, gamma, beta, act, slope, dgamma, dbeta, accumulate, ws, ws_bytes, stream);
    c.extra = BN_EXTRA_SHADOW; c.G.p[0].out16 = dy_bf16;
    return bn_bwd(c);
}
extern "C" int dg_bn_act_bwd_x3(const float* dz, const float* y, float* dy, void* dy_planes, size_t plane_elems, int plane_layout, int M, int C,
                                const float* saved, const float* gamma, const float* beta, int act, float slope, float* dgamma,
                                float* dbeta, int accumulate, void* ws, size_t ws_bytes, dg_stream_t stream) {
    BnCall c = bn_bwd_call("dg_bn_act_bwd_x3", dz, y, dy, M, C, saved, gamma, beta, act, slope, dgamma, dbeta, accumulate, ws, ws_bytes, stream);
    c.extra = BN_EXTRA_PLANES; c.G.p[0].out16 = dy_planes; c.plane_elems = plane_elems; c.plane_layout = plane_layout; c.write_out = dy != nullptr;
    return bn_bwd(c);
}
extern "C" int dg_bn_act_bwd_t(const void* dz, const void* y, void* dy, int io_bf16, int M, int C, const float* saved,
                               const float* gamma, const float* beta, int act, float slope, float* dgamma, float* dbeta,
                               int accumulate, void* ws, size_t ws_bytes, dg_stream_t stream) {
    BnCall c = bn_bwd_call("dg_bn_act_bwd_t", dz, y, dy, M, C, saved, gamma, beta, act, slope, dgamma, dbeta, accumulate, ws, ws_bytes, stream);
    c.bf16 = io_bf16 != 0;
    return bn_bwd(c);
}

static int bn_partials_row_blocks(int P) {
    if (P < 4096) return 1;          // (tools/bench_partials.py: 16384 x 64: 83 -> 28 us, 4096 x 128: 25 -> 15 us; below that one launch wins)
    const int rb = P / 512;
    return rb < 2 ? 2 : (rb > 64 ? 64 : rb);
}
extern "C" size_t dg_bn_partials_workspace_bytes(int P, int C) {
    const int rb = bn_partials_row_blocks(P);
    return rb > 1 ? (size_t)rb * 2 * (size_t)((C + 3) / 4 * 4) * sizeof(double) : 0;
}
extern "C" int dg_bn_stats_from_partials(const float* stat, int P, int M, int C, float eps, float momentum,
                                         float* running_mean, float* running_var, int64_t* nbt, float* saved,
                                         void* ws, size_t ws_bytes, dg_stream_t stream) {
    DG_CHECK_ARG(stat && saved && P >= 1, "dg_bn_stats_from_partials: bad argument");
    DG_CHECK_ARG(M >= 2, "dg_bn_stats_from_partials: Expected more than 1 value per channel when training (M=%d)", M);
    DG_CHECK_ARG(C >= 4 && C % 4 == 0, "dg_bn_stats_from_partials: C=%d must be a multiple of 4", C);
    // few channels x many partial rows (the window input-grad at 64 channels: 16384 rows of 784 bytes = 12.8 MB for 16 blocks)
    // is a latency-bound crawl in one launch (20.6 us average, 119 us worst over the 512 px step): from 4096 rows on the rows
    // are first reduced by RB row blocks per channel quad, then merged -- two short launches, every sum still in a fixed order
    const int RB = bn_partials_row_blocks(P);
    if (RB > 1 && ws != nullptr && ws_bytes >= dg_bn_partials_workspace_bytes(P, C)) {
        hipLaunchKernelGGL(bn_partials_reduce_kernel, dim3((C + 3) / 4, RB), dim3(256), 0, (hipStream_t)stream, stat, P, 3 * C + 4, C, RB, (double*)ws);
        DG_CHECK_LAUNCH("bn_partials_reduce");
        hipLaunchKernelGGL(bn_partials_merge_kernel, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const double*)ws, RB, stat, M, C, eps,
                           momentum, running_mean, running_var, nbt, saved);
        DG_CHECK_LAUNCH("bn_partials_merge");
        return DG_OK;
    }
    hipLaunchKernelGGL(bn_partials_finalize_kernel, dim3((C + 3) / 4), dim3(256), 0, (hipStream_t)stream, stat, P, 3 * C + 4,
                       M, C, eps, momentum, running_mean, running_var, nbt, saved);
    DG_CHECK_LAUNCH("bn_partials_finalize");
    return DG_OK;
}

#ifdef DG_EXPERIMENTS
#include <utility>
template <int... Q, typename F>
__device__ __forceinline__ void bn_static_for(std::integer_sequence<int, Q...>, F&& f) {
    (f(std::integral_constant<int, Q>{}), ...);
}
// "Understory" form of a streaming kernel (experiment; tools/probe_corun.py): can an HBM-bound pass run BENEATH a saturating MFMA conv
// kernel instead of taking turns with it?  The conv kernels hold 2 waves x 217-240 registers per SIMD and 96-128 KB of LDS, so what is
// left on a CU is ONE wave of <= 32 registers per SIMD and 32-64 KB of LDS -- far too few registers for the loads in flight that HBM
// latency needs (the plain kernels reach 1 TB/s beside a conv kernel).  Here the loads in flight live in LDS: every wave keeps NP 1-KiB
// pieces under way with `buffer_load_dwordx4 ... lds` (no registers), takes the oldest with ONE ds_read_b128 per lane, and re-issues
// the slot.  A workgroup = 4 waves (one per SIMD), 4 NP KiB of LDS; vmcnt counts the DMA loads and the stores in issue order.
template <int NP>
__global__ __launch_bounds__(256) void act_fwd_understory_kernel(const float* __restrict__ x, float* __restrict__ y, long nbytes, long wgbytes, int act,
                                                                 float slope) {
    __shared__ __attribute__((aligned(1024))) char smem[4 * NP * 1024];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long base = (long)blockIdx.x * wgbytes;                       // this workgroup's byte range [base, base + span)
    const long left = nbytes - base;
    const int span = (int)(left < wgbytes ? left : wgbytes);
    const int npc = (span + 1023) >> 10;                                // 1-KiB pieces of the range; wave w takes pieces w, w + 4, ...
    const int cnt = npc > wave ? (npc - wave + 3) >> 2 : 0;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)x + base), 0, span, 0x00020000);
    const unsigned lds_w = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem + (unsigned)wave * NP * 1024;
    constexpr int OOR = (int)0x80000000;
    auto dma = [&](int slot, int voff) {
        unsigned keep;
        const unsigned dst = lds_w + (unsigned)slot * 1024;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(voff), "s"(rx), "s"(dst)
                     : "memory");
    };
    auto off_of = [&](int i) -> int { return i < cnt ? ((wave + 4 * i) << 10) + lane * 16 : OOR; };
#pragma unroll
    for (int k = 0; k < NP; ++k) dma(k, off_of(k));
    for (int i = 0; i < cnt; ++i) {
        // piece i's DMA is followed by (issue order) the rest of the prologue and one store + one DMA per earlier iteration
        if (i >= NP - 1) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (NP - 1)) : "memory");
        } else {
            bn_static_for(std::make_integer_sequence<int, NP - 1>{}, [&](auto q) {
                if (i == q) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP - 1 + (int)q) : "memory");
            });
        }
        const int slot = i % NP;
        f32x4 v;
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(lds_w + (unsigned)slot * 1024 + (unsigned)lane * 16) : "memory");
        const int o = off_of(i);
        dma(slot, off_of(i + NP));
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = act == DG_ACT_SIGMOID ? 1.f / (1.f + expf(-v[j])) : dg_apply_act(v[j], act, slope);
        if (o + 16 <= span) *(f32x4*)((char*)y + base + o) = r;
        else asm volatile("s_nop 0");                                  // (the skipped store only makes the next waits stricter than needed: never looser)
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the zero-fill DMAs of the tail still target this workgroup's LDS
}
template <int NP>
static int act_fwd_understory(const float* x, float* y, size_t n, int act, float slope, hipStream_t st, int wgs) {
    const long nbytes = (long)n * 4;
    long wgbytes = 4L * NP * 1024 * 4;                                   // >= 4 rounds of the ring per workgroup
    if (wgs > 0) wgbytes = ((nbytes + wgs - 1) / wgs + 4095) / 4096 * 4096;      // a fixed number of long-lived workgroups (one per CU: 256)
    else while ((nbytes + wgbytes - 1) / wgbytes > 2048) wgbytes *= 2;
    DG_CHECK_ARG(wgbytes < (1L << 31), "act_fwd_understory: range per workgroup");
    const int grid = (int)((nbytes + wgbytes - 1) / wgbytes);
    hipLaunchKernelGGL((act_fwd_understory_kernel<NP>), dim3(grid), dim3(256), 0, st, x, y, nbytes, wgbytes, act, slope);
    DG_CHECK_LAUNCH("act_fwd_understory");
    return DG_OK;
}
#endif

// ---- stand-alone activations: one validation, one launch site per kernel ---------------------------------------------------------
// tabs: the call's pointer tables, `groups` pointers each (a one-problem form passes the addresses of its arguments)
static int act_validate(const char* who, int groups, std::initializer_list<const void* const*> tabs, int act) {
    DG_CHECK_ARG(groups >= 1 && groups <= DG_MAX_GROUPS, "%s: groups=%d (1..%d)", who, groups, DG_MAX_GROUPS);
    for (const void* const* t : tabs) {
        DG_CHECK_ARG(t, "%s: null table", who);
        for (int i = 0; i < groups; ++i) DG_CHECK_ARG(t[i], "%s: null pointer", who);
    }
    DG_CHECK_ARG(act >= DG_ACT_NONE && act <= DG_ACT_SIGMOID, "%s: bad act %d", who, act);
    return DG_OK;
}
static int act_fwd(const char* who, int groups, const float* const* x, float* const* y, size_t n, int act, float slope, dg_stream_t stream) {
    if (const int rc = act_validate(who, groups, {(const void* const*)x, (const void* const*)y}, act)) return rc;
    if (n == 0) return DG_OK;
#ifdef DG_EXPERIMENTS
    if (const int np = dg_get_option(DG_OPT_UNDERSTORY); np && groups == 1 && n % 4 == 0) {
        const int wgs = np / 100, q = np % 100;                          // e.g. 25616: 256 long-lived workgroups, 16 pieces per wave
        if (q == 16) return act_fwd_understory<16>(x[0], y[0], n, act, slope, (hipStream_t)stream, wgs);
        if (q == 8) return act_fwd_understory<8>(x[0], y[0], n, act, slope, (hipStream_t)stream, wgs);
        return act_fwd_understory<4>(x[0], y[0], n, act, slope, (hipStream_t)stream, wgs);
    }
#endif
    const long total4 = (long)((n + 3) / 4);
    hipLaunchKernelGGL(act_fwd_kernel, dim3(stream_grid(total4), groups), dim3(256), 0, (hipStream_t)stream, dg_ptrs((const void* const*)x, groups),
                       dg_ptrs((const void* const*)y, groups), total4, (long)n, act, slope);
    DG_CHECK_LAUNCH("act_fwd");
    return DG_OK;
}
extern "C" int dg_act_fwd_g(int groups, const float* const* x, float* const* y, size_t n, int act, float slope, dg_stream_t stream) {
    return act_fwd("dg_act_fwd_g", groups, x, y, n, act, slope, stream);
}
extern "C" int dg_act_fwd(const float* x, float* y, size_t n, int act, float slope, dg_stream_t stream) {
    return act_fwd("dg_act_fwd", 1, &x, &y, n, act, slope, stream);
}
// io_bf16 (one problem): bf16 in, bf16 out, n % 8 == 0
static int act_bwd(const char* who, int groups, const void* const* dy, const void* const* out, void* const* dx, int io_bf16, size_t n, int act,
                   float slope, dg_stream_t stream) {
    if (const int rc = act_validate(who, groups, {dy, out, (const void* const*)dx}, act)) return rc;
    DG_CHECK_ARG(!io_bf16 || n % 8 == 0, "%s: bf16 tensors need n %% 8 == 0 (n=%zu)", who, n);
    if (n == 0) return DG_OK;
    const long total = (long)(io_bf16 ? n / 8 : (n + 3) / 4);
    if (io_bf16)
        hipLaunchKernelGGL(act_bwd16_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, (const __bf16*)dy[0], (const __bf16*)out[0],
                           (__bf16*)dx[0], total, act, slope);
    else
        hipLaunchKernelGGL(act_bwd_kernel, dim3(stream_grid(total), groups), dim3(256), 0, (hipStream_t)stream, dg_ptrs(dy, groups), dg_ptrs(out, groups),
                           dg_ptrs((const void* const*)dx, groups), total, (long)n, act, slope);
    DG_CHECK_LAUNCH("act_bwd");
    return DG_OK;
}
extern "C" int dg_act_bwd_g(int groups, const float* const* dy, const float* const* out, float* const* dx, size_t n, int act, float slope,
                            dg_stream_t stream) {
    return act_bwd("dg_act_bwd_g", groups, (const void* const*)dy, (const void* const*)out, (void* const*)dx, 0, n, act, slope, stream);
}
extern "C" int dg_act_bwd(const float* dy, const float* out, float* dx, size_t n, int act, float slope, dg_stream_t stream) {
    return act_bwd("dg_act_bwd", 1, (const void* const*)&dy, (const void* const*)&out, (void* const*)&dx, 0, n, act, slope, stream);
}
extern "C" int dg_act_bwd_t(const void* dy, const void* out, void* dx, int io_bf16, size_t n, int act, float slope, dg_stream_t stream) {
    return act_bwd("dg_act_bwd_t", 1, &dy, &out, &dx, io_bf16, n, act, slope, stream);
}
