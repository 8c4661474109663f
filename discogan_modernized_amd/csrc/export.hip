// Sample grids on the device: float NCHW batches -> ONE uint8 HWC canvas (the inverse of the ingest in misc.hip, tiled).
// Replaces (reference file:line) the host work of image_translation.py:170-209 (save_sample_images): every batch to the host as
// float32, a transpose per image, matplotlib's own float -> pixel conversion.  Here the six columns of a sampling event are laid out
// by one launch and cross PCIe once, as the uint8 canvas.
//
//   canvas [Hc][Wc][3], Hc = rows (S + gap) + gap, Wc = cols (S + gap) + gap; cell (r, c) = image r of batch c at
//   (gap + r (S + gap), gap + c (S + gap)); every other byte = bg.
//   pixel = (uint8) rintf(clamp(x, 0, 1) * 255.0f): round half to even, NaN -> 0, so that u8 -> / 255 -> this is the identity.
//
// One grid-stride index space covers the whole canvas, every byte written exactly once (no memset in front):
//   [0, n_cell)            (c, r, y, q): pixels 4q .. 4q + 3 of row y of cell (r, c): three 16-byte plane loads where the addresses
//                          allow (S % 4 == 0 and an aligned batch), 12 interleaved bytes out -- whole dwords at a 4-byte aligned canvas
//                          address; else head bytes, two re-aligned dwords, tail bytes (a cell row starts 3 (c (S + gap) + gap) bytes
//                          into a 3 Wc-byte canvas row: any alignment occurs).  A short last quad (S % 4 != 0) goes out bytewise.
//   [n_cell, + n_band)     the rows + 1 horizontal gutters: gap whole canvas rows each = one contiguous byte range, as aligned dwords
//   [.., + n_strip)        the cols + 1 vertical gutters of every cell row: 3 gap bytes each
#include "dg_common.h"

#define DG_GRID_MAX_COLS 8

struct GridArgs {
    const float* src[DG_GRID_MAX_COLS];
    uint8_t* canvas;
    int cols, rows, S, gap;
    int nq;                 // quads per cell row: ceil(S / 4)
    int Wc;
    uint32_t bg4;           // bg in every byte
    long n_cell, n_band, n_strip;
    long band_bytes;        // gap * Wc * 3
    long band_dwords;       // aligned dwords that can touch one band (band_bytes / 4 + 2)
};

__device__ __forceinline__ uint32_t grid_px(float x) {
    x = x > 0.f ? x : 0.f;          // NaN, -inf -> 0
    x = x < 1.f ? x : 1.f;
    return (uint32_t)rintf(x * 255.0f);
}

__global__ __launch_bounds__(256) void sample_grid_kernel(const GridArgs a) {
    const long total = a.n_cell + a.n_band + a.n_strip;
    const int S = a.S, pitch = a.S + a.gap;
    const long row_bytes = (long)a.Wc * 3;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        if (i < a.n_cell) {
            const int q = (int)(i % a.nq);
            long t = i / a.nq;
            const int y = (int)(t % S);
            t /= S;
            const int r = (int)(t % a.rows);
            const int c = (int)(t / a.rows);
            const float* base = a.src[0];
#pragma unroll
            for (int j = 1; j < DG_GRID_MAX_COLS; ++j) base = (j == c) ? a.src[j] : base;
            const long plane = (long)S * S;
            const float* p = base + (long)r * 3 * plane + (long)y * S + 4 * q;
            uint8_t* d = a.canvas + ((long)(a.gap + r * (long)pitch + y)) * row_bytes + ((long)a.gap + (long)c * pitch + 4 * q) * 3;
            const int npx = min(4, S - 4 * q);
            if (npx == 4) {
                uint32_t v[3][4];
                if ((S & 3) == 0 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const f32x4 f = *(const f32x4*)(p + ch * plane);
                        v[ch][0] = grid_px(f.x); v[ch][1] = grid_px(f.y); v[ch][2] = grid_px(f.z); v[ch][3] = grid_px(f.w);
                    }
                } else {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[ch][k] = grid_px(p[ch * plane + k]);
                }
                // bytes 0 .. 11: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3 (little endian dwords)
                const uint32_t w0 = v[0][0] | (v[1][0] << 8) | (v[2][0] << 16) | (v[0][1] << 24);
                const uint32_t w1 = v[1][1] | (v[2][1] << 8) | (v[0][2] << 16) | (v[1][2] << 24);
                const uint32_t w2 = v[2][2] | (v[0][3] << 8) | (v[1][3] << 16) | (v[2][3] << 24);
                const int m = (int)((uintptr_t)d & 3);
                if (m == 0) {
                    uint32_t* o = (uint32_t*)d;
                    o[0] = w0; o[1] = w1; o[2] = w2;
                } else {
                    const int h = 4 - m;                               // head bytes in front of the first aligned dword
                    for (int k = 0; k < h; ++k) d[k] = (uint8_t)(w0 >> (8 * k));
                    const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32), hi = (uint64_t)w1 | ((uint64_t)w2 << 32);
                    uint32_t* o = (uint32_t*)(d + h);
                    o[0] = (uint32_t)(lo >> (8 * h));
                    o[1] = (uint32_t)(hi >> (8 * h));
                    for (int k = 0; k < m; ++k) d[8 + h + k] = (uint8_t)(w2 >> (8 * (h + k)));
                }
            } else {
                for (int k = 0; k < npx; ++k)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) d[3 * k + ch] = (uint8_t)grid_px(p[ch * plane + k]);
            }
        } else if (i < a.n_cell + a.n_band) {
            const long j = i - a.n_cell;
            const long b = j / a.band_dwords, w = j - b * a.band_dwords;
            const long lo = b * (long)pitch * row_bytes, hi = lo + a.band_bytes;      // byte range of band b inside the canvas
            const uintptr_t first = ((uintptr_t)a.canvas + lo) & ~(uintptr_t)3;       // aligned dword holding the band's first byte
            const long o = (long)(first - (uintptr_t)a.canvas) + 4 * w;               // canvas offset of this thread's dword (may be < lo)
            if (o >= lo && o + 4 <= hi) {
                *(uint32_t*)(a.canvas + o) = a.bg4;
            } else {
                for (int k = 0; k < 4; ++k)
                    if (o + k >= lo && o + k < hi) a.canvas[o + k] = (uint8_t)a.bg4;
            }
        } else {
            const long j = i - a.n_cell - a.n_band;
            const int sc = (int)(j % (a.cols + 1));                 // strip in front of column sc (the last one: behind the last column)
            const long yy = j / (a.cols + 1);                       // cell row index: r * S + y
            const long r = yy / S, y = yy - r * S;
            uint8_t* d = a.canvas + (a.gap + r * pitch + y) * row_bytes + (long)sc * pitch * 3;
            for (int k = 0; k < 3 * a.gap; ++k) d[k] = (uint8_t)a.bg4;
        }
    }
}

extern "C" int dg_sample_grid_u8(const float* const* src, int cols, int rows, int S, int gap, int bg, uint8_t* canvas, dg_stream_t s) {
    DG_CHECK_ARG(src != nullptr, "dg_sample_grid_u8: null pointer table");
    DG_CHECK_ARG(canvas != nullptr, "dg_sample_grid_u8: null canvas");
    DG_CHECK_ARG(cols >= 1 && cols <= DG_GRID_MAX_COLS, "dg_sample_grid_u8: cols %d outside 1..%d", cols, DG_GRID_MAX_COLS);
    DG_CHECK_ARG(rows >= 1, "dg_sample_grid_u8: rows %d < 1", rows);
    DG_CHECK_ARG(S >= 1, "dg_sample_grid_u8: S %d < 1", S);
    DG_CHECK_ARG(gap >= 0, "dg_sample_grid_u8: gap %d < 0", gap);
    DG_CHECK_ARG(bg >= 0 && bg <= 255, "dg_sample_grid_u8: bg %d outside 0..255", bg);
    for (int c = 0; c < cols; ++c) DG_CHECK_ARG(src[c] != nullptr, "dg_sample_grid_u8: null batch pointer in column %d", c);
    const long pitch = (long)S + gap;
    const long Hc = rows * pitch + gap, Wc = cols * pitch + gap;
    DG_CHECK_ARG(pitch <= 0x7fffffffL && Hc <= 0x7fffffffL && Wc * 3 <= 0x7fffffffL && (long)rows * S <= 0x7fffffffL,
                 "dg_sample_grid_u8: a %ld x %ld canvas is too large", Hc, Wc);
    GridArgs a;
    for (int c = 0; c < DG_GRID_MAX_COLS; ++c) a.src[c] = c < cols ? src[c] : nullptr;
    a.canvas = canvas;
    a.cols = cols; a.rows = rows; a.S = S; a.gap = gap;
    a.nq = (S + 3) / 4;
    a.Wc = (int)Wc;
    a.bg4 = (uint32_t)bg * 0x01010101u;
    a.n_cell = (long)cols * rows * S * a.nq;
    a.band_bytes = (long)gap * Wc * 3;
    a.band_dwords = gap > 0 ? a.band_bytes / 4 + 2 : 0;
    a.n_band = (long)(rows + 1) * a.band_dwords;
    a.n_strip = gap > 0 ? (long)rows * S * (cols + 1) : 0;
    const long total = a.n_cell + a.n_band + a.n_strip;
    long g = (total + 255) / 256;
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL(sample_grid_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)s, a);
    DG_CHECK_LAUNCH("sample_grid");
    return DG_OK;
}
