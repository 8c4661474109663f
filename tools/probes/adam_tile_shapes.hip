// Probe: which tile should the f32x3 Adam step that also writes the transposed weight planes run (csrc/optim.hip adam_step_x3t_kernel)?
// The kernel's text with the tile (TK x TJ on NT threads) and the walk of the tiles (along j / down k) as template arguments, next to
// the flat plane form of the step (34 B/param) and the transpose pass alone (12 B/param), on twelve generator-shaped [K][J = 16 C]
// weights (224 M parameters, all-zero data; fixed step constants: timing only).  Prints best / mean of five launches and the TB/s of
// the bytes each form moves (fused: 40 B/param).  DESIGN.md 3.4, profiles/adam_fused_transpose_probe_tile_shapes.txt.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -o /tmp/adam_tile_shapes tools/probes/adam_tile_shapes.hip && /tmp/adam_tile_shapes
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float gscale, float wd, float omb1, float b2, float omb2,
                                         float bc2_sqrt, float eps, float step_size) {
#pragma clang fp contract(off)
    const float gr = g * gscale + wd * p;
    m = m + (gr - m) * omb1;
    v = v * b2 + omb2 * gr * gr;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p - step_size * (m / denom);
}
__device__ __forceinline__ void split3(const f32x4& v, bf16x4& hi, bf16x4& mid, bf16x4& lo) {
    hi = __builtin_convertvector(v, bf16x4);
    const f32x4 r = v - __builtin_convertvector(hi, f32x4);
    mid = __builtin_convertvector(r, bf16x4);
    lo = __builtin_convertvector(r - __builtin_convertvector(mid, f32x4), bf16x4);
}
#define TMAX 48
struct Table { int n; int tile0[TMAX + 1]; int K[TMAX], J[TMAX]; long off[TMAX]; };

__global__ __launch_bounds__(256) void flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   long n, __bf16* __restrict__ p16, long pstride) {
    const float gscale = 1.f, wd = 1e-5f, omb1 = 0.5f, b2 = 0.999f, omb2 = 0.001f, bc2_sqrt = 0.5f, eps = 1e-8f, step_size = 2e-4f;
    const long n8 = n >> 3;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        f32x4 pp[2], gg[2], mm[2], vv[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            pp[h] = *(const f32x4*)(p + i * 8 + 4 * h); gg[h] = *(const f32x4*)(g + i * 8 + 4 * h);
            mm[h] = *(const f32x4*)(m + i * 8 + 4 * h); vv[h] = *(const f32x4*)(v + i * 8 + 4 * h);
        }
        bf16x4 hh[2], md[2], ll[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = pp[h][j], b = mm[h][j], c = vv[h][j];
                adam_one(a, gg[h][j], b, c, gscale, wd, omb1, b2, omb2, bc2_sqrt, eps, step_size);
                pp[h][j] = a; mm[h][j] = b; vv[h][j] = c;
            }
            *(f32x4*)(p + i * 8 + 4 * h) = pp[h]; *(f32x4*)(m + i * 8 + 4 * h) = mm[h]; *(f32x4*)(v + i * 8 + 4 * h) = vv[h];
            split3(pp[h], hh[h], md[h], ll[h]);
        }
        *(bf16x8*)(p16 + i * 8) = __builtin_shufflevector(hh[0], hh[1], 0, 1, 2, 3, 4, 5, 6, 7);
        *(bf16x8*)(p16 + pstride + i * 8) = __builtin_shufflevector(md[0], md[1], 0, 1, 2, 3, 4, 5, 6, 7);
        *(bf16x8*)(p16 + 2 * pstride + i * 8) = __builtin_shufflevector(ll[0], ll[1], 0, 1, 2, 3, 4, 5, 6, 7);
    }
}

// TK x TJ tile, NT threads, KMAJOR: consecutive blocks walk down k instead of along j
template <int TK, int TJ, int NT, bool KMAJOR>
__global__ __launch_bounds__(NT) void fused_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   __bf16* __restrict__ p3, __bf16* __restrict__ p3t, long plane, Table t) {
    constexpr int RPR = TJ / 8, TPR = RPR / 2, SQN = TK / 8;
    static_assert(NT / TPR == TK && NT / SQN == TJ / 2, "shape");
    __shared__ unsigned tile[3][TK][TJ / 2 + 1];
    const float gscale = 1.f, wd = 1e-5f, omb1 = 0.5f, b2 = 0.999f, omb2 = 0.001f, bc2_sqrt = 0.5f, eps = 1e-8f, step_size = 2e-4f;
    int wi = 0;
    while (wi + 1 < t.n && (int)blockIdx.x >= t.tile0[wi + 1]) ++wi;
    const int K = t.K[wi], J = t.J[wi];
    const long base = t.off[wi];
    const int tj = J / TJ, tk = K / TK;
    const int b = blockIdx.x - t.tile0[wi];
    const int k0 = (KMAJOR ? b % tk : b / tj) * TK, j0 = (KMAJOR ? b / tk : b % tj) * TJ;
    const int lk = threadIdx.x / TPR, lv = threadIdx.x % TPR;
    const int sq = threadIdx.x % SQN, sjp = threadIdx.x / SQN;
    f32x4 pp[2][2], gg[2][2], mm[2][2], vv[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const long e = base + (long)(k0 + lk) * J + j0 + (lv + TPR * h) * 8;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            pp[h][q] = *(const f32x4*)(p + e + 4 * q); gg[h][q] = *(const f32x4*)(g + e + 4 * q);
            mm[h][q] = *(const f32x4*)(m + e + 4 * q); vv[h][q] = *(const f32x4*)(v + e + 4 * q);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const long e = base + (long)(k0 + lk) * J + j0 + (lv + TPR * h) * 8;
        bf16x4 hh[2], md[2], ll[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = pp[h][q][j], bb = mm[h][q][j], c = vv[h][q][j];
                adam_one(a, gg[h][q][j], bb, c, gscale, wd, omb1, b2, omb2, bc2_sqrt, eps, step_size);
                pp[h][q][j] = a; mm[h][q][j] = bb; vv[h][q][j] = c;
            }
            *(f32x4*)(p + e + 4 * q) = pp[h][q]; *(f32x4*)(m + e + 4 * q) = mm[h][q]; *(f32x4*)(v + e + 4 * q) = vv[h][q];
            split3(pp[h][q], hh[q], md[q], ll[q]);
        }
        const bf16x8 pl3[3] = {__builtin_shufflevector(hh[0], hh[1], 0, 1, 2, 3, 4, 5, 6, 7), __builtin_shufflevector(md[0], md[1], 0, 1, 2, 3, 4, 5, 6, 7),
                               __builtin_shufflevector(ll[0], ll[1], 0, 1, 2, 3, 4, 5, 6, 7)};
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            *(bf16x8*)(p3 + pl * plane + e) = pl3[pl];
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

// the transpose pass alone (vector path of x3_transpose_kernel)
__global__ __launch_bounds__(256) void transpose_kernel(const __bf16* __restrict__ src, __bf16* __restrict__ dst, long plane, Table t) {
    __shared__ unsigned tile[64][33];
    int wi = 0;
    while (wi + 1 < t.n && (int)blockIdx.x >= t.tile0[wi + 1]) ++wi;
    const int K = t.K[wi], J = t.J[wi];
    const int tj = J / 64;
    const int b = blockIdx.x - t.tile0[wi];
    const int k0 = (b / tj) * 64, j0 = (b % tj) * 64;
    const int lk = threadIdx.x >> 2, lv = threadIdx.x & 3, sq = threadIdx.x & 7, sjp = threadIdx.x >> 3;
    for (int pl = 0; pl < 3; ++pl) {
        const unsigned short* s = (const unsigned short*)src + pl * plane + t.off[wi];
        unsigned short* d = (unsigned short*)dst + pl * plane + t.off[wi];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const u32x4 v = *(const u32x4*)(s + (long)(k0 + lk) * J + j0 + (lv + 4 * h) * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[lk][(lv + 4 * h) * 4 + e] = v[e];
        }
        __syncthreads();
        unsigned w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] = tile[8 * sq + e][sjp];
        u32x4 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lo[e] = (w[2 * e] & 0xffffu) | (w[2 * e + 1] << 16);
            hi[e] = (w[2 * e] >> 16) | (w[2 * e + 1] & 0xffff0000u);
        }
        *(u32x4*)(d + (long)(j0 + 2 * sjp) * K + k0 + 8 * sq) = lo;
        *(u32x4*)(d + (long)(j0 + 2 * sjp + 1) * K + k0 + 8 * sq) = hi;
        __syncthreads();
    }
}

static Table make_table(const std::vector<std::pair<int, int>>& ws, int TK, int TJ, long* total) {
    Table t;
    t.n = (int)ws.size();
    long off = 0;
    int tiles = 0;
    for (int i = 0; i < t.n; ++i) {
        t.tile0[i] = tiles; t.K[i] = ws[i].first; t.J[i] = ws[i].second; t.off[i] = off;
        tiles += (ws[i].first / TK) * (ws[i].second / TJ);
        off += (long)ws[i].first * ws[i].second;
    }
    t.tile0[t.n] = tiles;
    *total = off;
    return t;
}

int main() {
    // a generator-like group: [K][J = 16 C] images, widest layers twice each
    std::vector<std::pair<int, int>> ws = {{128, 1024}, {256, 2048}, {512, 4096}, {1024, 8192}, {2048, 16384}, {2048, 32768}, {2048, 32768},
                                           {1024, 32768}, {512, 16384}, {256, 8192}, {128, 4096}, {64, 2048}};
    long n = 0;
    make_table(ws, 64, 64, &n);
    printf("parameters: %ld\n", n);
    float *p, *g, *m, *v;
    __bf16 *p3, *p3t;
    CK(hipMalloc(&p, n * 4)); CK(hipMalloc(&g, n * 4)); CK(hipMalloc(&m, n * 4)); CK(hipMalloc(&v, n * 4));
    CK(hipMalloc(&p3, n * 6)); CK(hipMalloc(&p3t, n * 6));
    CK(hipMemset(p, 0, n * 4)); CK(hipMemset(g, 0, n * 4)); CK(hipMemset(m, 0, n * 4)); CK(hipMemset(v, 0, n * 4));
    CK(hipMemset(p3, 0, n * 6)); CK(hipMemset(p3t, 0, n * 6));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto timeit = [&](const char* name, double bytes_per_param, auto&& launch) {
        float best = 1e30f, sum = 0.f;
        for (int r = 0; r < 7; ++r) {
            CK(hipEventRecord(e0));
            launch();
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 2) { sum += ms; if (ms < best) best = ms; }
        }
        printf("%-34s best %.3f ms  mean %.3f ms  %.2f TB/s (best)\n", name, best, sum / 5, bytes_per_param * n / best * 1e-9);
        fflush(stdout);
    };
    for (int round = 0; round < 2; ++round) {
        timeit("flat adam<3> (34 B)", 34, [&] { hipLaunchKernelGGL(flat_kernel, dim3(4096), dim3(256), 0, 0, p, g, m, v, n, p3, n); });
        { long tt; Table t = make_table(ws, 64, 64, &tt);
          timeit("transpose alone (12 B)", 12, [&] { hipLaunchKernelGGL(transpose_kernel, dim3(t.tile0[t.n]), dim3(256), 0, 0, p3, p3t, n, t); });
          timeit("fused 64x64 /256 (40 B)", 40, [&] { hipLaunchKernelGGL((fused_kernel<64, 64, 256, false>), dim3(t.tile0[t.n]), dim3(256), 0, 0, p, g, m, v, p3, p3t, n, t); });
          timeit("fused 64x64 /256 k-major", 40, [&] { hipLaunchKernelGGL((fused_kernel<64, 64, 256, true>), dim3(t.tile0[t.n]), dim3(256), 0, 0, p, g, m, v, p3, p3t, n, t); }); }
        { long tt; Table t = make_table(ws, 64, 128, &tt);
          timeit("fused 64x128 /512", 40, [&] { hipLaunchKernelGGL((fused_kernel<64, 128, 512, false>), dim3(t.tile0[t.n]), dim3(512), 0, 0, p, g, m, v, p3, p3t, n, t); });
          timeit("fused 64x128 /512 k-major", 40, [&] { hipLaunchKernelGGL((fused_kernel<64, 128, 512, true>), dim3(t.tile0[t.n]), dim3(512), 0, 0, p, g, m, v, p3, p3t, n, t); }); }
        { long tt; Table t = make_table(ws, 32, 128, &tt);
          timeit("fused 32x128 /256", 40, [&] { hipLaunchKernelGGL((fused_kernel<32, 128, 256, false>), dim3(t.tile0[t.n]), dim3(256), 0, 0, p, g, m, v, p3, p3t, n, t); }); }
        { long tt; Table t = make_table(ws, 128, 64, &tt);
          timeit("fused 128x64 /512", 40, [&] { hipLaunchKernelGGL((fused_kernel<128, 64, 512, false>), dim3(t.tile0[t.n]), dim3(512), 0, 0, p, g, m, v, p3, p3t, n, t); }); }
        { long tt; Table t = make_table(ws, 32, 64, &tt);
          timeit("fused 32x64 /128", 40, [&] { hipLaunchKernelGGL((fused_kernel<32, 64, 128, false>), dim3(t.tile0[t.n]), dim3(128), 0, 0, p, g, m, v, p3, p3t, n, t); }); }
    }
    return 0;
}
