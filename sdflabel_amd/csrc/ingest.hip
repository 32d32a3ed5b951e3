// Frame ingest on the device (gfx950): the sparse depth map of the lidar, the matching of detector boxes to annotations and the CSS
// network's input, i.e. what pipelines/refine_css.py:101-138 does on the host before the first crop exists.
//
// sdfr_depth_map   utils/refinement.py:87-105 (compute_depth_map): frustum test, pinhole projection, truncation to a pixel, and the loop's
//                  overwrite rule -- the LAST point in input order that lands on a pixel sets its depth.  Pass A is an integer atomicMax of
//                  the point index, pass B a gather, so the image does not depend on scheduling and no float atomic exists.
//                  sdfr_depth_map_masked: the same over the points a uint8 mask keeps (the road-removed map of get_kitti_frame).
// sdfr_match_boxes refine_css.py:101-114: get_iou (utils/refinement.py:128-165) of every detector box against every annotation in float64,
//                  the first maximum per annotation (np.argmax), kept when iou >= 0.5.
// sdfr_css_input   utils/refinement.py:60-84 (transform_bgr_crop) for all annotations of a frame, reading the frame image in place:
//                  uint8(crop * 255), BGR -> RGB, Pillow's 8-bit bilinear resample to 128 x 128 (ImagingResample: horizontal pass over all
//                  rows, vertical pass over its uint8 result, 22-bit integer coefficients), ToTensor and Normalize.
// Compiled with -ffp-contract=off: every multiply / add rounds separately, as in numpy, Pillow's C and ATen.
#include "sdfr_common.h"

// ---- depth map ---------------------------------------------------------------------------------------------------------------------------
struct DmCam {
    float pl[12];            // the four plane normals (top, right, bottom, left), float32 as build_view_frustum leaves them
    double fx, fy, cx, cy;
};

__global__ __launch_bounds__(256) void sdfr_dm_init_kernel(int32_t* __restrict__ winner, int64_t npix, int32_t* __restrict__ info) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < npix) winner[i] = -1;
    if (i < 2) info[i] = 0;
}

template <typename T>
__global__ __launch_bounds__(256) void sdfr_dm_scatter_kernel(const T* __restrict__ lidar, const uint8_t* __restrict__ mask, int N, DmCam cam,
                                                             int w, int h, int32_t* __restrict__ winner, int32_t* __restrict__ info) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool kept = false, dropped = false;
    if (i < N && (!mask || mask[i])) {                                  // a masked-out point is as good as absent from the cloud
        const double X = (double)lidar[3 * (int64_t)i], Y = (double)lidar[3 * (int64_t)i + 1], Z = (double)lidar[3 * (int64_t)i + 2];
        bool in = true;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            in = in && (((double)cam.pl[3 * k] * X + (double)cam.pl[3 * k + 1] * Y) + (double)cam.pl[3 * k + 2] * Z > 0.0);
        if (in) {
            // project(...).astype(np.int32): the float64 pinhole rounded to float32, then truncated toward zero
            const float xf = (float)(cam.fx * (X / Z) + cam.cx), yf = (float)(cam.fy * (Y / Z) + cam.cy);
            // (a NaN or a value beyond int32 fails the range test below in float, before any conversion)
            if (xf > -1.f && xf < (float)w && yf > -1.f && yf < (float)h) {
                const int x = (int)xf, y = (int)yf;                     // in (-1, 0) truncates to 0, as astype does
                kept = true;
                atomicMax(&winner[(int64_t)y * w + x], i);
            } else {
                dropped = true;                                          // the reference's loop would raise IndexError (or wrap) here
            }
        }
    }
    const unsigned long long bk = __ballot(kept), bd = __ballot(dropped);
    if ((threadIdx.x & 63) == 0) {
        if (bk) atomicAdd(&info[0], __popcll(bk));
        if (bd) atomicAdd(&info[1], __popcll(bd));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void sdfr_dm_gather_kernel(const T* __restrict__ lidar, const int32_t* __restrict__ winner, int64_t npix,
                                                            float* __restrict__ depth) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int i = winner[p];
    depth[p] = i >= 0 ? (float)lidar[3 * (int64_t)i + 2] : 0.f;
}

static int dm_run(const void* lidar, int lidar_f64, int N, const uint8_t* mask, const float* planes, const double* cam, int w, int h, float* depth,
                  int32_t* winner, int32_t* info, void* stream) {
    SDFR_REQUIRE(N >= 0 && w > 0 && h > 0, "sdfr_depth_map: bad size");
    SDFR_REQUIRE((int64_t)w * h < ((int64_t)1 << 31), "sdfr_depth_map: image too large");
    SDFR_REQUIRE(planes && cam && depth && winner && info, "sdfr_depth_map: NULL argument");
    SDFR_REQUIRE(lidar || N == 0, "sdfr_depth_map: NULL points");
    hipStream_t s = (hipStream_t)stream;
    DmCam c;
    for (int i = 0; i < 12; ++i) c.pl[i] = planes[i];
    c.fx = cam[0]; c.fy = cam[1]; c.cx = cam[2]; c.cy = cam[3];
    const int64_t npix = (int64_t)w * h;
    hipLaunchKernelGGL(sdfr_dm_init_kernel, dim3(sdfr_cdiv(npix, 256)), dim3(256), 0, s, winner, npix, info);
    SDFR_LAUNCH_CHECK();
    if (N > 0) {
        if (lidar_f64)
            hipLaunchKernelGGL(sdfr_dm_scatter_kernel<double>, dim3(sdfr_cdiv(N, 256)), dim3(256), 0, s, (const double*)lidar, mask, N, c, w, h, winner, info);
        else
            hipLaunchKernelGGL(sdfr_dm_scatter_kernel<float>, dim3(sdfr_cdiv(N, 256)), dim3(256), 0, s, (const float*)lidar, mask, N, c, w, h, winner, info);
        SDFR_LAUNCH_CHECK();
    }
    if (lidar_f64)
        hipLaunchKernelGGL(sdfr_dm_gather_kernel<double>, dim3(sdfr_cdiv(npix, 256)), dim3(256), 0, s, (const double*)lidar, winner, npix, depth);
    else
        hipLaunchKernelGGL(sdfr_dm_gather_kernel<float>, dim3(sdfr_cdiv(npix, 256)), dim3(256), 0, s, (const float*)lidar, winner, npix, depth);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_depth_map(const void* lidar, int lidar_f64, int N, const float* planes, const double* cam, int w, int h, float* depth,
                              int32_t* winner, int32_t* info, void* stream) {
    return dm_run(lidar, lidar_f64, N, nullptr, planes, cam, w, h, depth, winner, info, stream);
}

// the depth map of the points with mask[i] != 0, indices and overwrite order those of the whole cloud (get_kitti_frame's road-removed map)
extern "C" int sdfr_depth_map_masked(const void* lidar, int lidar_f64, int N, const uint8_t* mask, const float* planes, const double* cam, int w,
                                     int h, float* depth, int32_t* winner, int32_t* info, void* stream) {
    SDFR_REQUIRE(mask || N <= 0, "sdfr_depth_map_masked: NULL mask");
    return dm_run(lidar, lidar_f64, N, mask, planes, cam, w, h, depth, winner, info, stream);
}

// ---- box matching ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void sdfr_match_boxes_kernel(const double* __restrict__ anno, int A, const double* __restrict__ det, int M,
                                                             int32_t* __restrict__ best, double* __restrict__ iou, int32_t* __restrict__ keep) {
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= A) return;
    const double b0 = anno[4 * a], b1 = anno[4 * a + 1], b2 = anno[4 * a + 2], b3 = anno[4 * a + 3];
    const double area_b = (b2 - b0) * (b3 - b1);
    int arg = -1;
    double top = 0.0;
    for (int m = 0; m < M; ++m) {                                       // get_iou(detector box, annotation box)
        const double a0 = det[4 * m], a1 = det[4 * m + 1], a2 = det[4 * m + 2], a3 = det[4 * m + 3];
        const double width = fmin(a2, b2) - fmax(a0, b0), height = fmin(a3, b3) - fmax(a1, b1);
        double v = 0.0;
        if (!(width < 0.0 || height < 0.0)) {
            const double over = width * height;
            const double area_a = (a2 - a0) * (a3 - a1);
            v = over / (((area_a + area_b) - over) + 1e-5);
        }
        if (arg < 0 || v > top) { arg = m; top = v; }                   // the first maximum, as np.argmax
    }
    best[a] = arg;
    iou[a] = top;
    keep[a] = (arg >= 0 && top >= 0.5) ? 1 : 0;                         // refine_css.py:110 skips iou < 0.5
}

extern "C" int sdfr_match_boxes(const double* anno, int A, const double* det, int M, int32_t* best, double* iou, int32_t* keep, void* stream) {
    SDFR_REQUIRE(A >= 0 && M >= 0, "sdfr_match_boxes: negative size");
    if (A == 0) return SDFR_OK;
    SDFR_REQUIRE(anno && best && iou && keep, "sdfr_match_boxes: NULL argument");
    SDFR_REQUIRE(det || M == 0, "sdfr_match_boxes: NULL detector boxes");
    hipLaunchKernelGGL(sdfr_match_boxes_kernel, dim3(sdfr_cdiv(A, 64)), dim3(64), 0, (hipStream_t)stream, anno, A, det, M, best, iou, keep);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

// ---- CSS input ---------------------------------------------------------------------------------------------------------------------------
#include "css_resample.h"             // CSS_OUT, CSS_PRECISION_BITS, css_coef_row, css_clip8: shared with augment.hip
#define CSS_META 8                   // int32 per annotation: l, t, crop width, crop height, first mask element (-1: none), first row of the
                                     // annotation in tmp, first workgroup of the annotation in the horizontal pass, unused

// One thread per output index of one pass (pass 0: horizontal, crop width -> 128; pass 1: vertical, crop height -> 128) of one annotation.
// coef[a][pass][xx] = { xmin, n, kk[0 .. ksize) }.
__global__ __launch_bounds__(CSS_OUT) void sdfr_css_coef_kernel(const int32_t* __restrict__ meta, int ksize, int32_t* __restrict__ coef) {
    const int a = blockIdx.x >> 1, pass = blockIdx.x & 1, xx = threadIdx.x;
    css_coef_row(meta[CSS_META * a + 2 + pass], xx, ksize, coef + ((int64_t)blockIdx.x * CSS_OUT + xx) * (2 + ksize));
}

// Horizontal pass: thread = (row of the crop, four neighbouring output columns), 8 rows per workgroup; a flat list of workgroups over the
// annotations (meta[6] = the annotation's first workgroup), so no workgroup is empty.  The crop's pixels are converted on the way in:
// (mask *) value, uint8(trunc(v * 255.0f)), channel order reversed.  12 result bytes per thread leave as three 32-bit stores.
__global__ __launch_bounds__(256) void sdfr_css_hpass_kernel(const float* __restrict__ image, int H, int W, const int32_t* __restrict__ meta,
                                                            int A, const float* __restrict__ masks, int ksize,
                                                            const int32_t* __restrict__ coef, uint8_t* __restrict__ tmp) {
    int a = 0;
    while (a + 1 < A && (int)blockIdx.x >= meta[CSS_META * (a + 1) + 6]) ++a;
    const int32_t* m = meta + CSS_META * a;
    const int l = m[0], t = m[1], cw = m[2], ch = m[3], moff = m[4];
    const int row = ((int)blockIdx.x - m[6]) * 8 + (threadIdx.x >> 5), xq = threadIdx.x & 31;
    if (row >= ch) return;
    int iy = t + row;
    iy = iy < 0 ? 0 : (iy >= H ? H - 1 : iy);                           // (a box outside the image is refused by the caller; never read out of bounds)
    const float* src = image + (int64_t)iy * W * 3;
    const float* mrow = (masks && moff >= 0) ? masks + moff + (int64_t)row * cw : nullptr;
    uint32_t px[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int32_t* k = coef + (((int64_t)a * 2 + 0) * CSS_OUT + (4 * xq + j)) * (2 + ksize);
        const int xmin = k[0], n = k[1];
        int acc[3] = {1 << (CSS_PRECISION_BITS - 1), 1 << (CSS_PRECISION_BITS - 1), 1 << (CSS_PRECISION_BITS - 1)};
        for (int x = 0; x < n; ++x) {
            int ix = l + xmin + x;
            ix = ix < 0 ? 0 : (ix >= W ? W - 1 : ix);
            const int kk = k[2 + x];
            const float mv = mrow ? mrow[xmin + x] : 1.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = src[3 * (int64_t)ix + (2 - c)];                // BGR -> RGB
                if (mrow) v = v * mv;
                acc[c] += (int)(uint8_t)(int)(v * 255.0f) * kk;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) px[3 * j + c] = css_clip8(acc[c]);
    }
    uint32_t* dst = (uint32_t*)(tmp + ((int64_t)m[5] + row) * (CSS_OUT * 3) + 12 * xq);
#pragma unroll
    for (int q = 0; q < 3; ++q) dst[q] = px[4 * q] | (px[4 * q + 1] << 8) | (px[4 * q + 2] << 16) | (px[4 * q + 3] << 24);
}

// Vertical pass over the horizontal pass' uint8 rows, then ToTensor (float32(u8) / 255.0f) and Normalize ((x - mean) / std, a subtraction and
// a division in float32).  Thread = (output row, four neighbouring output columns): 16-byte stores into each channel plane.
__global__ __launch_bounds__(256) void sdfr_css_vpass_kernel(const int32_t* __restrict__ meta, int ksize, const int32_t* __restrict__ coef,
                                                            const uint8_t* __restrict__ tmp, float* __restrict__ im,
                                                            float* __restrict__ im_orig, uint8_t* __restrict__ u8) {
    const int a = blockIdx.y;
    const int yy = blockIdx.x * 8 + (threadIdx.x >> 5), xq = threadIdx.x & 31;
    const int32_t* k = coef + (((int64_t)a * 2 + 1) * CSS_OUT + yy) * (2 + ksize);
    const int ymin = k[0], n = k[1];
    int acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 1 << (CSS_PRECISION_BITS - 1);
    const uint8_t* base = tmp + ((int64_t)meta[CSS_META * a + 5] + ymin) * (CSS_OUT * 3) + 12 * xq;
    for (int y = 0; y < n; ++y) {
        const uint32_t* r = (const uint32_t*)(base + (int64_t)y * (CSS_OUT * 3));
        const uint32_t w0 = r[0], w1 = r[1], w2 = r[2];
        const int kk = k[2 + y];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[i] += (int)((w0 >> (8 * i)) & 255u) * kk;
            acc[4 + i] += (int)((w1 >> (8 * i)) & 255u) * kk;
            acc[8 + i] += (int)((w2 >> (8 * i)) & 255u) * kk;
        }
    }
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    uint32_t b[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) b[i] = css_clip8(acc[i]);              // b[3 * j + c]: column 4 xq + j, channel c
    if (u8) {
        uint32_t* d = (uint32_t*)(u8 + (((int64_t)a * CSS_OUT + yy) * CSS_OUT) * 3 + 12 * xq);
#pragma unroll
        for (int q = 0; q < 3; ++q) d[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float4 o, nrm;
        float* po = &o.x;
        float* pn = &nrm.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            po[j] = __fdiv_rn((float)b[3 * j + c], 255.0f);
            pn[j] = __fdiv_rn(__fsub_rn(po[j], mean[c]), sd[c]);
        }
        const int64_t e = (((int64_t)a * 3 + c) * CSS_OUT + yy) * CSS_OUT + 4 * xq;
        if (im) *(float4*)(im + e) = nrm;
        if (im_orig) *(float4*)(im_orig + e) = o;
    }
}

extern "C" int sdfr_css_input(const float* image, int H, int W, const int32_t* meta, int A, const float* masks, int ksize, int n_hblocks,
                              int32_t* coef, uint8_t* tmp, float* im, float* im_orig, uint8_t* u8, void* stream) {
    SDFR_REQUIRE(A >= 0 && H > 0 && W > 0 && ksize >= 3 && n_hblocks >= 0, "sdfr_css_input: bad size");
    if (A == 0) return SDFR_OK;
    SDFR_REQUIRE(image && meta && coef && tmp, "sdfr_css_input: NULL argument");
    SDFR_REQUIRE(im || im_orig || u8, "sdfr_css_input: no output");
    SDFR_REQUIRE(n_hblocks >= A, "sdfr_css_input: every annotation needs a workgroup of the horizontal pass");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sdfr_css_coef_kernel, dim3(2 * A), dim3(CSS_OUT), 0, s, meta, ksize, coef);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_css_hpass_kernel, dim3(n_hblocks), dim3(256), 0, s, image, H, W, meta, A, masks, ksize, coef, tmp);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_css_vpass_kernel, dim3(CSS_OUT / 8, A), dim3(256), 0, s, meta, ksize, coef, tmp, im, im_orig, u8);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
