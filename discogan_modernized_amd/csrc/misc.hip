// Error plumbing, options, and NCHW <-> NHWC layout helpers (tests / ingest of foreign tensors;
// not on the training hot path).
#include "dg_common.h"
#include <string.h>

thread_local char dg_err_buf[512] = "";
static int g_options[DG_OPT_COUNT] = {0};

int dg_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dg_err_buf, sizeof(dg_err_buf), fmt, ap);
    va_end(ap);
    return code;
}
int dg_get_option(int idx) { return (idx >= 0 && idx < DG_OPT_COUNT) ? g_options[idx] : 0; }

extern "C" int dg_version(void) { return 101; }
// bit 0: the experiments build (kernels that lost their A/B: window forward kernel, register-staged plane reader, persistent window
// input-grad, paired-plane 16x16x32 body); bit 1: the timing build (operand-dropping switch).  The product library returns 0.
extern "C" int dg_build_flags(void) {
    int f = 0;
#ifdef DG_EXPERIMENTS
    f |= 1;
#endif
#ifdef DG_TIMING_KNOBS
    f |= 2;
#endif
    return f;
}
extern "C" const char* dg_last_error(void) { return dg_err_buf; }
extern "C" int dg_set_option(const char* name, int value) {
    if (!name) return dg_fail(DG_ERR_INVALID, "dg_set_option: null name");
    if (!strcmp(name, "splitk")) g_options[DG_OPT_SPLITK] = value;
    else if (!strcmp(name, "kt")) g_options[DG_OPT_KT] = value;
    else if (!strcmp(name, "target_wgs")) g_options[DG_OPT_TARGET_WGS] = value;
    else if (!strcmp(name, "split_below")) g_options[DG_OPT_SPLIT_BELOW] = value;
    else if (!strcmp(name, "no_xcd_group")) g_options[DG_OPT_RESERVED] = value;   // 1: plain blockIdx -> tile order; 3: only the per-XCD row-tile blocks of single-column forward convs off
    else if (!strcmp(name, "bf16")) g_options[DG_OPT_BF16] = value;   // 1: interior conv GEMMs on bf16 MFMA, fp32 accumulate; 2: fp32 operands as three bf16 planes
#ifdef DG_TIMING_KNOBS
    // timing builds only (make TIMING=1 -> libdiscogan_hip_timing.so, tools/bench_ops.py --dbg_zero): 1|2|3 drop operand loads (WRONG
    // results), 4 / 8 select older reduction walks (correct results, another summation order).  The product library has no such switch.
    else if (!strcmp(name, "dbg_zero")) g_options[DG_OPT_DBG_ZERO] = value;
#endif
    else if (!strcmp(name, "no_dma")) g_options[DG_OPT_NO_DMA] = value;   // 1: bf16-operand convs stay on the register-staged tiles (igemm.hip) instead of the LDS-DMA kernel
    else if (!strcmp(name, "dma_mfma")) g_options[DG_OPT_DMA_MFMA] = value;   // 32: the LDS-DMA kernel's 32x32x16 body instead of 16x16x32; 1: no window kernels (A/B)
#ifdef DG_EXPERIMENTS
    // experiments library only (make EXPERIMENTS=1): kernels that were built, verified and measured not faster
    else if (!strcmp(name, "x3_mfma")) g_options[DG_OPT_X3_MFMA] = value;   // 16: the f32x3 plane kernel's 16x16x32 body (planes paired along k) instead of 32x32x16
    else if (!strcmp(name, "understory")) g_options[DG_OPT_UNDERSTORY] = value;   // 16 | 8 | 4: dg_act_fwd through the LDS-DMA-fed low-register streaming kernel with that many 1-KiB pieces in flight per wave (tools/probe_corun.py)
    else if (!strcmp(name, "dgw_persist")) g_options[DG_OPT_DGW_PERSIST] = value;   // 1: the f32x3 window input-grad kernel as one persistent workgroup per CU
#endif
    else if (!strcmp(name, "bn_items")) g_options[DG_OPT_BN_ITEMS] = value;   // 1: the fp32 BatchNorm apply passes on the item kernels instead of the row-geometry ones (tests, A/B: same results); read where a call enters the library
    else if (!strcmp(name, "pointer_path")) g_options[DG_OPT_POINTER_PATH] = value;   // 1: 64-bit addressing kernels (tests)
    else return dg_fail(DG_ERR_INVALID, "dg_set_option: unknown option '%s'", name);
    return DG_OK;
}

extern "C" int dg_device_cu_count(void) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
    return n;
}

// 32x32 tile transpose through LDS between the [C] and [H*W] axes of one image.  The tiles of one image are numbered along grid.x,
// column tile fastest (tiles_c = ceil(Cn / 32)): grid.y and grid.z stop at 65536, and R = H*W of a single-channel plane of
// 1449 x 1449 pixels already has 65613 row tiles.
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ x, float* __restrict__ y, int R, int Cn, int tiles_c) {
    // x: [B][R][Cn] -> y: [B][Cn][R]
    __shared__ float tile[32][33];
    const long boff = (long)blockIdx.z * R * Cn;
    const int tr = blockIdx.x / tiles_c;
    const int c0 = (blockIdx.x - tr * tiles_c) * 32, r0 = tr * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8) {
        const int r = r0 + j, c = c0 + tx;
        if (r < R && c < Cn) tile[j][tx] = x[boff + (long)r * Cn + c];
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, r = r0 + tx;
        if (r < R && c < Cn) y[boff + (long)c * R + r] = tile[tx][j];
    }
}
#define TRANSPOSE_MAX_TILES 16777215L   // grid.x * 256 threads must stay below 2^32
static int launch_transpose(const char* who, const float* x, float* y, int B, long R, long Cn, hipStream_t st) {
    DG_CHECK_ARG(R <= 2147483647L && Cn <= 2147483647L && R * Cn <= 2147483647L, "%s: C*H*W of one image must not exceed 2^31 - 1", who);
    const long tiles_c = (Cn + 31) / 32, tiles_r = (R + 31) / 32;
    DG_CHECK_ARG(tiles_c * tiles_r <= TRANSPOSE_MAX_TILES,
                 "%s: one image takes ceil(C/32) * ceil(H*W/32) = %ld tiles of 32 x 32, more than %ld (grid.x of 256-thread blocks)", who,
                 tiles_c * tiles_r, TRANSPOSE_MAX_TILES);
    dim3 grid((unsigned)(tiles_c * tiles_r), 1, B);
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, st, x, y, (int)R, (int)Cn, (int)tiles_c);
    DG_CHECK_LAUNCH("transpose");
    return DG_OK;
}
extern "C" int dg_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, dg_stream_t s) {
    DG_CHECK_ARG(x && y && N > 0 && C > 0 && H > 0 && W > 0 && N < 65536, "dg_nchw_to_nhwc: bad argument");
    return launch_transpose("dg_nchw_to_nhwc", x, y, N, C, (long)H * W, (hipStream_t)s);  // [N][C][HW] -> [N][HW][C]
}
extern "C" int dg_nhwc_to_nchw(const float* x, float* y, int N, int C, int H, int W, dg_stream_t s) {
    DG_CHECK_ARG(x && y && N > 0 && C > 0 && H > 0 && W > 0 && N < 65536, "dg_nhwc_to_nchw: bad argument");
    return launch_transpose("dg_nhwc_to_nchw", x, y, N, (long)H * W, C, (hipStream_t)s);  // [N][HW][C] -> [N][C][HW]
}

// ---- image ingest (dataset.py:62-66): uint8 [N][H][W][3] (decoded image rows) -> float [N][3][H][W] in [0,1] ----
// The reference does `/255.` and `transpose(2,0,1)` per image on the host and copies 4 B/channel over PCIe; here the
// uint8 batch crosses PCIe (1 B/channel) and one pass on the device normalises and re-lays it out.  Each thread
// produces 4 consecutive x of one (n, y): reads 12 contiguous bytes, writes one float4 into each channel plane.
__global__ __launch_bounds__(256) void u8hwc_to_f32chw_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, long npix4,
                                                              int HW4, int HW, int bgr) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix4; i += (long)gridDim.x * 256) {
        const long n = i / HW4;
        const int q = (int)(i - n * HW4);                 // group of 4 pixels inside the image
        const uint32_t* s = (const uint32_t*)(src + (n * HW + (long)q * 4) * 3);   // 12 bytes, 4-byte aligned
        const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
        uint8_t b[12];
#pragma unroll
        for (int j = 0; j < 4; ++j) { b[j] = (w0 >> (8 * j)) & 255; b[4 + j] = (w1 >> (8 * j)) & 255; b[8 + j] = (w2 >> (8 * j)) & 255; }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int cs = bgr ? 2 - c : c;
            // dataset.py:65: image.astype(np.float32) / 255. -- a correctly rounded fp32 division (a multiply by
            // 1/255.f can differ by one ulp), so divide
            const f32x4 v = {(float)b[cs] / 255.f, (float)b[3 + cs] / 255.f, (float)b[6 + cs] / 255.f, (float)b[9 + cs] / 255.f};
            *(f32x4*)(dst + (n * 3 + c) * HW + (long)q * 4) = v;
        }
    }
}
extern "C" int dg_u8hwc_to_f32chw(const uint8_t* src, float* dst, int N, int H, int W, int bgr, dg_stream_t s) {
    DG_CHECK_ARG(src && dst && N > 0 && H > 0 && W > 0 && (H * W) % 4 == 0, "dg_u8hwc_to_f32chw: bad argument (H*W must be a multiple of 4)");
    const int HW = H * W;
    const long npix4 = (long)N * (HW / 4);
    long g = (npix4 + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(u8hwc_to_f32chw_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)s, src, dst, npix4, HW / 4, HW, bgr);
    DG_CHECK_LAUNCH("u8hwc_to_f32chw");
    return DG_OK;
}
