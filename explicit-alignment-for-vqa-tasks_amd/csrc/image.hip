// CLIP image preprocessing: raw uint8 RGB images of any size -> the resized, centre-cropped, normalised pixels of the reference's
// image_preprocessor (extract_clip_embeddings_conceptual_captions.py:61), bit for bit.  PIL's 8-bit bicubic resampler is integer
// arithmetic: per axis a window [xmin, xmin + count) of 22-bit fixed-point weights, acc = 2^21 + sum src * k in int32, acc >> 22 clamped
// to a byte; a horizontal pass, then a vertical pass over its uint8 result.  The host plan (models/clip_preprocess.py) builds the weight
// tables for the cropped output range only; the kernels here are the two passes, the second one also looking the byte up in the
// ToTensor + Normalize table and writing either NCHW float32 or eavqa_patchify's patch rows.
//
// Both kernels check every descriptor and table entry against the buffer sizes they are given before they use it: whatever the tables
// hold, no load or store leaves src / mid / tables (a block or a column with a bad entry writes nothing).
#include "common.h"

namespace {

constexpr int IMG_H_TILE = 16;      // rows of the horizontal pass per workgroup (models/clip_preprocess.py: H_TILE_ROWS)
constexpr int IMG_H_ROWS = 4;       // rows per thread: one weight load feeds 4 rows x 3 channels
constexpr int IMG_V_TILE = 4;       // output rows of the vertical pass per workgroup (V_TILE_ROWS)
constexpr int IMG_PRECISION = 22;
constexpr int IMG_MAX_NPX = 4096;   // the vertical pass keeps IMG_V_TILE byte rows of the output in LDS

struct img_desc {                   // one row of the plan's int64 descriptor table
    int64_t src_off, W, H, row0, nrows, mid_off, tab_x, tab_y;
};

// a table block is [ksize, xmin[n_px], count[n_px], k[n_px * ksize]] at word offset `off`
__device__ __forceinline__ bool table_ok(const int32_t* tables, int64_t n_words, int64_t off, int n_px, int* ks) {
    if (off < 0 || off + 1 + 2 * (int64_t)n_px > n_words) return false;
    const int k = tables[off];
    if (k <= 0 || off + 1 + 2 * (int64_t)n_px + (int64_t)n_px * k > n_words) return false;
    *ks = k;
    return true;
}

__device__ __forceinline__ bool desc_ok(const img_desc& d, int64_t mid_bytes, int64_t mid_stride) {
    return d.W > 0 && d.H > 0 && d.W <= (1 << 24) && d.H <= (1 << 24) && d.row0 >= 0 && d.nrows > 0 && d.row0 + d.nrows <= d.H && d.mid_off >= 0 && (d.mid_off & 3) == 0 &&
           d.mid_off + d.nrows * mid_stride <= mid_bytes;
}

__device__ __forceinline__ uint32_t clip8(int acc) {
    const int v = acc >> IMG_PRECISION;                         // arithmetic shift, as PIL's clip8
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// Horizontal pass.  A workgroup owns IMG_H_TILE input rows of one image (tile table: the batch is ragged); a thread owns one output
// column of IMG_H_ROWS rows, keeps their 3-channel sums in registers and walks the column's weights once.  Neighbouring lanes read
// neighbouring windows of the same source rows and write neighbouring 3-byte pixels.
__global__ __launch_bounds__(256) void clip_resize_rows_kernel(int n_px, int n_images, const uint8_t* __restrict__ src, int64_t src_bytes,
                                                               const img_desc* __restrict__ desc, const int32_t* __restrict__ tables,
                                                               int64_t n_words, const int32_t* __restrict__ tiles, uint8_t* __restrict__ mid,
                                                               int64_t mid_bytes, int64_t mid_stride) {
    const int img = tiles[2 * blockIdx.x], r0 = tiles[2 * blockIdx.x + 1];
    if (img < 0 || img >= n_images || r0 < 0) return;
    const img_desc d = desc[img];
    int ks;
    if (!desc_ok(d, mid_bytes, mid_stride) || r0 >= d.nrows || d.src_off < 0 ||
        d.src_off + d.H * d.W * 3 > src_bytes || !table_ok(tables, n_words, d.tab_x, n_px, &ks))
        return;
    const int32_t* xmin = tables + d.tab_x + 1;
    const int32_t* count = xmin + n_px;
    const int32_t* kk = count + n_px;
    const int rows = min(IMG_H_TILE, (int)(d.nrows - r0));
    const int groups = (rows + IMG_H_ROWS - 1) / IMG_H_ROWS;
    const int64_t rs = d.W * 3;
    for (int it = threadIdx.x; it < groups * n_px; it += 256) {
        const int x = it % n_px, rg = it / n_px;
        const int xm = xmin[x], c = count[x];
        if (xm < 0 || c < 0 || c > ks || xm + (int64_t)c > d.W) continue;
        const int32_t* k = kk + (int64_t)x * ks;
        const int rbase = r0 + rg * IMG_H_ROWS;
        const int nr = min(IMG_H_ROWS, rows - rg * IMG_H_ROWS);
        const uint8_t* p = src + d.src_off + ((d.row0 + rbase) * d.W + xm) * 3;
        int acc[IMG_H_ROWS][3];
#pragma unroll
        for (int j = 0; j < IMG_H_ROWS; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << (IMG_PRECISION - 1);
        for (int t = 0; t < c; ++t) {
            const int kv = k[t];
#pragma unroll
            for (int j = 0; j < IMG_H_ROWS; ++j) {
                if (j < nr) {
                    const uint8_t* q = p + j * rs + t * 3;
                    acc[j][0] += (int)q[0] * kv;
                    acc[j][1] += (int)q[1] * kv;
                    acc[j][2] += (int)q[2] * kv;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < IMG_H_ROWS; ++j) {
            if (j < nr) {
                uint8_t* o = mid + d.mid_off + (rbase + j) * mid_stride + x * 3;
                o[0] = (uint8_t)clip8(acc[j][0]);
                o[1] = (uint8_t)clip8(acc[j][1]);
                o[2] = (uint8_t)clip8(acc[j][2]);
            }
        }
    }
}

// Vertical pass + crop + normalise + emit.  A workgroup owns IMG_V_TILE output rows of one image.  Step 1: a thread sums four
// consecutive bytes of an output row over the row's window (one 4-byte load per tap, lanes side by side along the intermediate row, the
// tap's weight the same for the whole row) and leaves the clamped bytes in LDS.  Step 2: the threads walk the OUTPUT layout, so the
// stores run along x (form (a)) or along a patch's ps-long pixel runs (form (b)), and look each byte up in the normalisation table.
// PATCH: eavqa_patchify's rows - [B * g * g, ldp], column (c * ps + i) * ps + j; the workgroup that owns a patch row's first pixel
// row (i == 0) also zeroes its pad columns [3 * ps * ps, ldp).
template <typename T, bool PATCH>
__global__ __launch_bounds__(256) void clip_resize_emit_kernel(int n_px, int n_images, const img_desc* __restrict__ desc,
                                                               const int32_t* __restrict__ tables, int64_t n_words,
                                                               const uint8_t* __restrict__ mid, int64_t mid_bytes, int64_t mid_stride,
                                                               const float* __restrict__ lut, int ps, T* __restrict__ out, int64_t ldp) {
    extern __shared__ __align__(16) unsigned char lds[];
    float* s_lut = reinterpret_cast<float*>(lds);                            // [3][256]
    uint32_t* s_rows = reinterpret_cast<uint32_t*>(lds + 3 * 256 * sizeof(float));   // [IMG_V_TILE][mid_stride / 4]
    const int tiles_per_image = (n_px + IMG_V_TILE - 1) / IMG_V_TILE;
    const int b = blockIdx.x / tiles_per_image, y0 = (blockIdx.x % tiles_per_image) * IMG_V_TILE;
    if (b >= n_images) return;
    const img_desc d = desc[b];
    int ks;
    if (!desc_ok(d, mid_bytes, mid_stride) || !table_ok(tables, n_words, d.tab_y, n_px, &ks)) return;     // uniform over the workgroup
    for (int i = threadIdx.x; i < 3 * 256; i += 256) s_lut[i] = lut[i];
    const int32_t* ymin = tables + d.tab_y + 1;
    const int32_t* count = ymin + n_px;
    const int32_t* kk = count + n_px;
    const int ty = min(IMG_V_TILE, n_px - y0);
    const int wpr = (int)(mid_stride >> 2);
    for (int e = threadIdx.x; e < ty * wpr; e += 256) {
        const int yl = e / wpr, w = e - yl * wpr, y = y0 + yl;
        const int ym = ymin[y], c = count[y];
        uint32_t packed = 0;
        if (ym >= d.row0 && c >= 0 && c <= ks && ym + (int64_t)c <= d.row0 + d.nrows) {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(mid + d.mid_off + (ym - d.row0) * mid_stride) + w;
            const int32_t* k = kk + (int64_t)y * ks;
            int a0 = 1 << (IMG_PRECISION - 1), a1 = a0, a2 = a0, a3 = a0;
            for (int t = 0; t < c; ++t) {
                const uint32_t v = p[(int64_t)t * wpr];
                const int kv = k[t];
                a0 += (int)(v & 255u) * kv;
                a1 += (int)((v >> 8) & 255u) * kv;
                a2 += (int)((v >> 16) & 255u) * kv;
                a3 += (int)(v >> 24) * kv;
            }
            packed = clip8(a0) | (clip8(a1) << 8) | (clip8(a2) << 16) | (clip8(a3) << 24);
        }
        s_rows[yl * wpr + w] = packed;
    }
    __syncthreads();
    const uint8_t* s_bytes = reinterpret_cast<const uint8_t*>(s_rows);
    const int g = PATCH ? n_px / ps : 0;
    for (int o = threadIdx.x; o < ty * 3 * n_px; o += 256) {
        const int x = o % n_px, t = o / n_px;
        const int c = t % 3, yl = t / 3, y = y0 + yl;
        const float v = s_lut[c * 256 + s_bytes[yl * mid_stride + x * 3 + c]];
        if (PATCH) {
            const int gy = y / ps, gx = x / ps;
            const int64_t row = ((int64_t)b * g + gy) * g + gx;
            elem<T>::st(out + row * ldp + (c * ps + (y - gy * ps)) * ps + (x - gx * ps), v);
        } else {
            elem<T>::st(out + (((int64_t)b * 3 + c) * n_px + y) * n_px + x, v);
        }
    }
    if (PATCH) {
        const int kreal = 3 * ps * ps, padw = (int)ldp - kreal;
        for (int yl = 0; yl < ty && padw > 0; ++yl) {
            const int y = y0 + yl;
            if (y % ps) continue;
            for (int o = threadIdx.x; o < g * padw; o += 256) {
                const int gx = o / padw;
                elem<T>::st(out + (((int64_t)b * g + y / ps) * g + gx) * ldp + kreal + (o - gx * padw), 0.f);
            }
        }
    }
}

int check_common(int n_px, int n_images, const void* desc, const void* tables, int64_t n_table_words, const void* mid, int64_t mid_bytes,
                 int64_t mid_stride) {
    if (n_px <= 0 || n_images <= 0 || !desc || !tables || n_table_words <= 0 || !mid || mid_bytes <= 0 || mid_stride <= 0) return EAVQA_E_ARG;
    return EAVQA_OK;
}

int check_layout(int n_px, const void* mid, int64_t mid_stride) {
    if (n_px > IMG_MAX_NPX) return EAVQA_E_SHAPE;
    if (mid_stride % 4 || (reinterpret_cast<uintptr_t>(mid) & 3u)) return EAVQA_E_ALIGN;
    if (mid_stride < 3 * (int64_t)n_px) return EAVQA_E_ARG;
    return EAVQA_OK;
}

}  // namespace

extern "C" int eavqa_clip_resize_rows(int n_px, int n_images, int n_tiles, const uint8_t* src, int64_t src_bytes, const int64_t* desc,
                                      const int32_t* tables, int64_t n_table_words, const int32_t* tiles, uint8_t* mid, int64_t mid_bytes,
                                      int64_t mid_stride, void* stream) {
    if (int rc = check_common(n_px, n_images, desc, tables, n_table_words, mid, mid_bytes, mid_stride)) return rc;
    if (n_tiles <= 0 || !src || src_bytes <= 0 || !tiles) return EAVQA_E_ARG;
    if (int rc = check_layout(n_px, mid, mid_stride)) return rc;
    hipLaunchKernelGGL(clip_resize_rows_kernel, dim3(n_tiles), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), n_px, n_images, src,
                       src_bytes, reinterpret_cast<const img_desc*>(desc), tables, n_table_words, tiles, mid, mid_bytes, mid_stride);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}

extern "C" int eavqa_clip_resize_emit(int dtype, int n_px, int ps, int n_images, const int64_t* desc, const int32_t* tables,
                                      int64_t n_table_words, const uint8_t* mid, int64_t mid_bytes, int64_t mid_stride, const float* lut,
                                      void* out, int64_t ldp, void* stream) {
    if (int rc = check_common(n_px, n_images, desc, tables, n_table_words, mid, mid_bytes, mid_stride)) return rc;
    if (ps < 0 || !lut || !out) return EAVQA_E_ARG;
    if (dtype != EAVQA_F32 && !(ps > 0 && dtype == EAVQA_BF16)) return EAVQA_E_DTYPE;
    if (ps > 0 && n_px % ps) return EAVQA_E_SHAPE;
    if (int rc = check_layout(n_px, mid, mid_stride)) return rc;
    if (ps > 0 && ldp < 3 * (int64_t)ps * ps) return EAVQA_E_ARG;
    const int64_t blocks = (int64_t)n_images * ((n_px + IMG_V_TILE - 1) / IMG_V_TILE);
    if (blocks > 0x7fffffff) return EAVQA_E_SHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = 3 * 256 * sizeof(float) + (size_t)IMG_V_TILE * mid_stride;
    const img_desc* dd = reinterpret_cast<const img_desc*>(desc);
    if (ps == 0)
        hipLaunchKernelGGL((clip_resize_emit_kernel<float, false>), dim3((unsigned)blocks), dim3(256), lds, s, n_px, n_images, dd, tables,
                           n_table_words, mid, mid_bytes, mid_stride, lut, 0, (float*)out, 0);
    else if (dtype == EAVQA_F32)
        hipLaunchKernelGGL((clip_resize_emit_kernel<float, true>), dim3((unsigned)blocks), dim3(256), lds, s, n_px, n_images, dd, tables,
                           n_table_words, mid, mid_bytes, mid_stride, lut, ps, (float*)out, ldp);
    else
        hipLaunchKernelGGL((clip_resize_emit_kernel<bf16_t, true>), dim3((unsigned)blocks), dim3(256), lds, s, n_px, n_images, dd, tables,
                           n_table_words, mid, mid_bytes, mid_stride, lut, ps, (bf16_t*)out, ldp);
    EAVQA_LAUNCH_CHECK();
    return EAVQA_OK;
}
