// Image ingest on the device: decoded uint8 rows -> the float NCHW batch the networks take.
// Replaces (reference file:line) the per-image host work of dataset.py:52-66 (read_images) / :239-254 (DiscoGANDataset):
//   domain 'A' (edges2*):  image[:, :256]; 255 - cv2.dilate(255 - image, ones(3,3))  == a 3x3 EROSION of the left half
//   domain 'B':            image[:, 256:]
//   cv2.resize(image, (S, S))  (INTER_LINEAR: half-pixel centres, edge clamp)
//   image.astype(np.float32) / 255. ; transpose(2, 0, 1)
// One launch per batch: a thread owns one output pixel (all 3 channels), reads its 2 x 2 source taps (each the minimum over
// the in-bounds 3 x 3 neighbourhood when `erode`), interpolates, normalises and writes one float into each channel plane
// (consecutive threads = consecutive x: coalesced stores; the uint8 reads hit L2).  The batch crosses PCIe as uint8
// (1 B / channel of the SOURCE size) instead of float32 of the output size.
//
// Arithmetic (mode):
//   0  float: coefficients in fp32, horizontal pass then vertical pass like cv2's generic path; the reference's domain 'A' image is
//      float64 at cv2.resize (255. - image), so its result is not rounded to uint8 -- neither is this one.
//   1  8-bit fixed point, cv2's CV_8U path: coefficients round(2048 a) as int16, rows S0 a0 + S1 a1 (int32), output
//      (((b0 (R0 >> 4)) >> 16) + ((b1 (R1 >> 4)) >> 16) + 2) >> 2, a uint8; then / 255 (correctly rounded fp32 division).
#include "dg_draw.h"

struct PrepArgs {
    const uint8_t* src;
    float* dst;
    int N, H, W;        // source images [N][H][W][3]
    int x0, cw;         // crop: columns x0 .. x0 + cw - 1 (rows: all H)
    int erode, mode, S;
    double sx, sy;      // cw / S, H / S
};

__device__ __forceinline__ void prep_axis(int d, double scale, int n, int* i0, float* f) {
    // cv2 resize.cpp: fx = (dx + 0.5) * scale - 0.5; sx = floor(fx); fx -= sx; clamp at both ends with fx = 0
    float fx = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(fx);
    fx -= (float)s;
    if (s < 0) { fx = 0.f; s = 0; }
    if (s >= n - 1) { fx = 0.f; s = n - 1; }
    *i0 = s;
    *f = fx;
}

__device__ __forceinline__ void prep_tap(const PrepArgs& p, const uint8_t* img, int y, int x, int v[3]) {
    // pixel (y, x) of the CROPPED image, eroded over its in-bounds 3 x 3 neighbourhood when p.erode
    if (!p.erode) {
        const uint8_t* q = img + ((long)y * p.W + p.x0 + x) * 3;
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
        return;
    }
    int m0 = 255, m1 = 255, m2 = 255;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if ((unsigned)yy >= (unsigned)p.H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if ((unsigned)xx >= (unsigned)p.cw) continue;        // the crop edge is an image border for cv2.dilate
            const uint8_t* q = img + ((long)yy * p.W + p.x0 + xx) * 3;
            m0 = min(m0, (int)q[0]); m1 = min(m1, (int)q[1]); m2 = min(m2, (int)q[2]);
        }
    }
    v[0] = m0; v[1] = m1; v[2] = m2;
}

__global__ __launch_bounds__(256) void image_prep_kernel(const PrepArgs p) {
    const long total = (long)p.N * p.S * p.S;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ox = (int)(i % p.S);
        const int oy = (int)((i / p.S) % p.S);
        const long n = i / ((long)p.S * p.S);
        const uint8_t* img = p.src + n * (long)p.H * p.W * 3;
        int x0, y0;
        float fx, fy;
        prep_axis(ox, p.sx, p.cw, &x0, &fx);
        prep_axis(oy, p.sy, p.H, &y0, &fy);
        const int x1 = min(x0 + 1, p.cw - 1), y1 = min(y0 + 1, p.H - 1);
        int t00[3], t01[3], t10[3], t11[3];
        prep_tap(p, img, y0, x0, t00);
        prep_tap(p, img, y0, x1, t01);
        prep_tap(p, img, y1, x0, t10);
        prep_tap(p, img, y1, x1, t11);
        float out[3];
        if (p.mode == 1) {
            const int a1 = (int)rintf(fx * 2048.f), a0 = (int)rintf((1.f - fx) * 2048.f);
            const int b1 = (int)rintf(fy * 2048.f), b0 = (int)rintf((1.f - fy) * 2048.f);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int r0 = t00[c] * a0 + t01[c] * a1, r1 = t10[c] * a0 + t11[c] * a1;
                int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
                v = min(max(v, 0), 255);
                out[c] = (float)v / 255.f;
            }
        } else {
            const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float r0 = (float)t00[c] * a0 + (float)t01[c] * a1, r1 = (float)t10[c] * a0 + (float)t11[c] * a1;
                out[c] = (r0 * b0 + r1 * b1) / 255.f;
            }
        }
        float* d = p.dst + (n * 3) * (long)p.S * p.S + (long)oy * p.S + ox;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[(long)c * p.S * p.S] = out[c];
    }
}

extern "C" int dg_image_prep(const uint8_t* src, float* dst, int N, int H, int W, int x0, int cw, int erode, int mode, int S,
                             dg_stream_t s) {
    DG_CHECK_ARG(src && dst && N > 0 && H > 0 && W > 0 && S > 0, "dg_image_prep: bad argument");
    DG_CHECK_ARG(x0 >= 0 && cw > 0 && x0 + cw <= W, "dg_image_prep: crop [%d, %d) outside the %d-pixel rows", x0, x0 + cw, W);
    DG_CHECK_ARG(mode == 0 || mode == 1, "dg_image_prep: mode 0 (float) or 1 (cv2 8-bit fixed point)");
    PrepArgs p;
    p.src = src; p.dst = dst; p.N = N; p.H = H; p.W = W; p.x0 = x0; p.cw = cw; p.erode = erode ? 1 : 0; p.mode = mode; p.S = S;
    p.sx = (double)cw / S; p.sy = (double)H / S;
    const long total = (long)N * S * S;
    long g = (total + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(image_prep_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)s, p);
    DG_CHECK_LAUNCH("image_prep");
    return DG_OK;
}

// ---- training augmentation: random mirror and scale-jitter crop, fused into the preparation ---------------------------------------------
// "Prepare at L >= S, take the S x S window at (ox, oy), mirror it when flip" with only the S x S output pixels computed: output pixel
// (y, x) of sample n IS pixel (oy + y, ox + (flip ? S - 1 - x : x)) of the size-L preparation, so the kernel evaluates prep_axis / prep_tap
// and the interpolation below at that coordinate with scale = cw / L and H / L.  image_prep_kernel above stays as it is; prep_pixel restates
// its arithmetic expression by expression, and the result is bitwise dg_image_prep at L, sliced and flipped (tests/test_augment_gpu.py).
//
// The per-sample record (ox, oy, flip, 0) comes from a table dg_augment_draw fills on the device: dg_draw.h's generator (its key, two
// words per record, range) with
//   a = mix(k + G * (2 j + 1));   b = mix(k + G * (2 j + 2))                 (j = position in the batch)
//   w0 = a >> 32,  w1 = a & 0xFFFFFFFF,  w2 = b >> 32
//   flip = w0 >> 31;   ox = (uint64(w1) * (L - S + 1)) >> 32;   oy = (uint64(w2) * (L - S + 1)) >> 32
// flip is 0 without DG_AUG_FLIP, both offsets are 0 without DG_AUG_CROP.  tests/augment_ref.py restates this in numpy.
__global__ __launch_bounds__(256) void augment_draw_kernel(uint64_t key, int n, uint32_t range, int flags, int* __restrict__ recs) {
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        const uint64_t a = dg_mix(key + DG_DRAW_G * (2ull * (uint64_t)j + 1ull)), b = dg_mix(key + DG_DRAW_G * (2ull * (uint64_t)j + 2ull));
        const uint32_t w0 = (uint32_t)(a >> 32), w1 = (uint32_t)a, w2 = (uint32_t)(b >> 32);
        const bool crop = (flags & DG_AUG_CROP) != 0;
        int4 r;
        r.x = crop ? dg_draw_range(w1, 0, range) : 0;
        r.y = crop ? dg_draw_range(w2, 0, range) : 0;
        r.z = (flags & DG_AUG_FLIP) ? (int)(w0 >> 31) : 0;
        r.w = 0;
        reinterpret_cast<int4*>(recs)[j] = r;                    // one 16-byte store per record
    }
}

extern "C" int dg_augment_draw(uint64_t seed, int rank, int64_t iteration, int domain, int n, int S, int L, int flags, int32_t* recs,
                               dg_stream_t s) {
    DG_CHECK_ARG(recs != nullptr, "dg_augment_draw: null record table");
    DG_CHECK_ARG(((uintptr_t)recs & 15) == 0, "dg_augment_draw: the record table must be 16-byte aligned");
    DG_CHECK_ARG(n >= 0 && S > 0, "dg_augment_draw: n >= 0 records for S > 0 pixels, got n = %d, S = %d", n, S);
    DG_CHECK_ARG(L >= S, "dg_augment_draw: the prepared size L = %d is smaller than the output size S = %d", L, S);
    DG_CHECK_ARG(rank >= 0 && iteration >= 0 && (domain == 0 || domain == 1), "dg_augment_draw: rank >= 0, iteration >= 0, domain 0 (A) or 1 (B)");
    DG_CHECK_ARG((flags & ~(DG_AUG_FLIP | DG_AUG_CROP)) == 0, "dg_augment_draw: flags is a sum of DG_AUG_FLIP and DG_AUG_CROP, got %d", flags);
    if (n == 0) return DG_OK;
    int g = (n + 255) / 256;
    if (g > 1024) g = 1024;
    hipLaunchKernelGGL(augment_draw_kernel, dim3(g), dim3(256), 0, (hipStream_t)s, dg_draw_key(seed, rank, iteration, domain), n,
                       (uint32_t)(L - S + 1), flags, recs);
    DG_CHECK_LAUNCH("augment_draw");
    return DG_OK;
}

struct AugRec {
    int ox, oy, flip;
};

// Record of sample n, made safe: offsets clamped to [0, L - S] (a stale or foreign table cannot move the window off the size-L image), flip
// taken as zero / non-zero.
__device__ __forceinline__ AugRec aug_rec(const int* __restrict__ recs, const int* __restrict__ rec_index, long n, int S, int L) {
    const int4 r = reinterpret_cast<const int4*>(recs)[rec_index ? rec_index[n] : n];
    AugRec a;
    a.ox = min(max(r.x, 0), L - S);
    a.oy = min(max(r.y, 0), L - S);
    a.flip = r.z != 0;
    return a;
}

// Pixel (py, px) of the size-L preparation of one image: image_prep_kernel's arithmetic at an arbitrary destination coordinate
// (p.sx = cw / L, p.sy = H / L).
__device__ __forceinline__ void prep_pixel(const PrepArgs& p, const uint8_t* img, int py, int px, float out[3]) {
    int x0, y0;
    float fx, fy;
    prep_axis(px, p.sx, p.cw, &x0, &fx);
    prep_axis(py, p.sy, p.H, &y0, &fy);
    const int x1 = min(x0 + 1, p.cw - 1), y1 = min(y0 + 1, p.H - 1);
    int t00[3], t01[3], t10[3], t11[3];
    prep_tap(p, img, y0, x0, t00);
    prep_tap(p, img, y0, x1, t01);
    prep_tap(p, img, y1, x0, t10);
    prep_tap(p, img, y1, x1, t11);
    if (p.mode == 1) {
        const int a1 = (int)rintf(fx * 2048.f), a0 = (int)rintf((1.f - fx) * 2048.f);
        const int b1 = (int)rintf(fy * 2048.f), b0 = (int)rintf((1.f - fy) * 2048.f);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int r0 = t00[c] * a0 + t01[c] * a1, r1 = t10[c] * a0 + t11[c] * a1;
            int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
            v = min(max(v, 0), 255);
            out[c] = (float)v / 255.f;
        }
    } else {
        const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float r0 = (float)t00[c] * a0 + (float)t01[c] * a1, r1 = (float)t10[c] * a0 + (float)t11[c] * a1;
            out[c] = (r0 * b0 + r1 * b1) / 255.f;
        }
    }
}

// One thread per OUTPUT pixel, as image_prep_kernel: consecutive threads = consecutive output x, so the three channel-plane stores stay
// coalesced whatever the record says; a mirrored sample walks its uint8 taps right to left (L2 hits, like the forward walk).
// Reads stay inside the source for EVERY record value: prep_axis clamps the first tap of each axis to [0, n - 1] whatever destination
// coordinate it is given, the second tap is min(first + 1, n - 1), prep_tap skips neighbours outside [0, H) x [0, cw), and the launcher has
// checked x0 + cw <= W; aug_rec's clamp only keeps the window where the caller asked for it.  rec_index values are the caller's contract
// (rows of `recs`).
__global__ __launch_bounds__(256) void image_prep_aug_kernel(const PrepArgs p, const int L, const int* __restrict__ recs,
                                                             const int* __restrict__ rec_index) {
    const long total = (long)p.N * p.S * p.S;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int x = (int)(i % p.S);
        const int y = (int)((i / p.S) % p.S);
        const long n = i / ((long)p.S * p.S);
        const AugRec a = aug_rec(recs, rec_index, n, p.S, L);
        float out[3];
        prep_pixel(p, p.src + n * (long)p.H * p.W * 3, a.oy + y, a.ox + (a.flip ? p.S - 1 - x : x), out);
        float* d = p.dst + (n * 3) * (long)p.S * p.S + (long)y * p.S + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[(long)c * p.S * p.S] = out[c];
    }
}

static inline int aug_grid(long total) {
    long g = (total + 255) / 256;
    return (int)(g > 8192 ? 8192 : g);
}

extern "C" int dg_image_prep_aug(const uint8_t* src, float* dst, int N, int H, int W, int x0, int cw, int erode, int mode, int S, int L,
                                 const int32_t* recs, const int32_t* rec_index, dg_stream_t s) {
    DG_CHECK_ARG(src && dst && N > 0 && H > 0 && W > 0 && S > 0, "dg_image_prep_aug: bad argument");
    DG_CHECK_ARG(L >= S, "dg_image_prep_aug: the prepared size L = %d is smaller than the output size S = %d", L, S);
    DG_CHECK_ARG(recs != nullptr, "dg_image_prep_aug: null record table");
    DG_CHECK_ARG(((uintptr_t)recs & 15) == 0 && ((uintptr_t)rec_index & 3) == 0, "dg_image_prep_aug: the record table must be 16-byte aligned, rec_index 4-byte");
    DG_CHECK_ARG(x0 >= 0 && cw > 0 && x0 + cw <= W, "dg_image_prep_aug: crop [%d, %d) outside the %d-pixel rows", x0, x0 + cw, W);
    DG_CHECK_ARG(mode == 0 || mode == 1, "dg_image_prep_aug: mode 0 (float) or 1 (cv2 8-bit fixed point)");
    PrepArgs p;
    p.src = src; p.dst = dst; p.N = N; p.H = H; p.W = W; p.x0 = x0; p.cw = cw; p.erode = erode ? 1 : 0; p.mode = mode; p.S = S;
    p.sx = (double)cw / L; p.sy = (double)H / L;
    hipLaunchKernelGGL(image_prep_aug_kernel, dim3(aug_grid((long)N * S * S)), dim3(256), 0, (hipStream_t)s, p, L, recs, rec_index);
    DG_CHECK_LAUNCH("image_prep_aug");
    return DG_OK;
}

// The same operation on a resident float batch [N][3][S][S] (tensor files, synthetic data): float bilinear resize S -> L with the sampling of
// prep_axis and mode-0 arithmetic on the float taps (no / 255), window, mirror.  One thread per output ELEMENT (consecutive threads =
// consecutive x of one channel plane: coalesced stores, the four taps of a row pair come from L2).  A tap whose weight is exactly 0 is not
// read into the sum, so with L = S (every fraction 0) the output is the input bit for bit, -0.0, inf and NaN included; for finite taps
// t0 * 1 + t1 * 0 == t0 anyway.  Taps are clamped to [0, S - 1] by prep_axis for every record value.
__global__ __launch_bounds__(256) void augment_f32_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int S, int L,
                                                          double scale, const int* __restrict__ recs) {
    const long plane = (long)S * S, total = (long)N * 3 * plane;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int x = (int)(i % S);
        const int y = (int)((i / S) % S);
        const long nc = i / plane;
        const AugRec a = aug_rec(recs, nullptr, nc / 3, S, L);
        int x0, y0;
        float fx, fy;
        prep_axis(a.ox + (a.flip ? S - 1 - x : x), scale, S, &x0, &fx);
        prep_axis(a.oy + y, scale, S, &y0, &fy);
        const int x1 = min(x0 + 1, S - 1), y1 = min(y0 + 1, S - 1);
        const float* q = src + nc * plane;
        const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
        const float* q0 = q + (long)y0 * S;
        float r0 = q0[x0];
        if (fx != 0.f) r0 = r0 * a0 + q0[x1] * a1;
        float v = r0;
        if (fy != 0.f) {
            const float* q1 = q + (long)y1 * S;
            float r1 = q1[x0];
            if (fx != 0.f) r1 = r1 * a0 + q1[x1] * a1;
            v = r0 * b0 + r1 * b1;
        }
        dst[i] = v;
    }
}

extern "C" int dg_augment_f32(const float* src, float* dst, int N, int S, int L, const int32_t* recs, dg_stream_t s) {
    DG_CHECK_ARG(src && dst && N > 0 && S > 0, "dg_augment_f32: bad argument");
    DG_CHECK_ARG(L >= S, "dg_augment_f32: the resized size L = %d is smaller than the output size S = %d", L, S);
    DG_CHECK_ARG(recs != nullptr, "dg_augment_f32: null record table");
    DG_CHECK_ARG(((uintptr_t)recs & 15) == 0, "dg_augment_f32: the record table must be 16-byte aligned");
    const size_t bytes = (size_t)N * 3 * S * S * sizeof(float);
    DG_CHECK_ARG((const char*)dst + bytes <= (const char*)src || (const char*)src + bytes <= (const char*)dst,
                 "dg_augment_f32: source and destination overlap (every output reads up to four other pixels)");
    hipLaunchKernelGGL(augment_f32_kernel, dim3(aug_grid((long)N * 3 * S * S)), dim3(256), 0, (hipStream_t)s, src, dst, N, S, L,
                       (double)S / L, recs);
    DG_CHECK_LAUNCH("augment_f32");
    return DG_OK;
}
