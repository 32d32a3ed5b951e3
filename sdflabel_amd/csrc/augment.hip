// Augmentation of the CSS network's training crops on the device (gfx950): what the reference's datasets/crops.py asks of torchvision's PIL
// backend per sample, i.e. of Pillow -- ColorJitter in a drawn order, RandomRotation(expand=True), Resize((128, 128)), RandomResizedCrop(128)
// and ToTensor / Normalize for the RGB image (bilinear), the same geometry with nearest-neighbour sampling for the UVW label image --
// reproduced byte for byte for given random parameters, for a ragged batch of source crops.
//
// sdfr_augment, four launches whatever the batch size:
//   jitter   one workgroup per sample.  Brightness / contrast / saturation are Image.blend(degenerate, image, f) in float32; contrast needs
//            the mean of the L image as it stands at that point of the order, an integer sum over the workgroup (the same on every run).
//            Hue is convert('HSV'), H += shift (byte wrap-around), convert('RGB').  Result: uint8, the size of the source.
//   tables   per sample and resample pass (rotated width -> 128, rotated height -> 128, crop width -> 128, crop height -> 128) Pillow's
//            22-bit bilinear coefficients (css_resample.h) and ImagingScaleAffine's nearest source index.
//   stage 1  one thread per pixel of the 128 x 128 intermediate.  RGB: the vertical resample pass over the horizontal pass' uint8 values,
//            each of which is recomputed from the rotated image, each pixel of which is evaluated on the fly (Image.transform AFFINE,
//            bilinear, float64) -- every 8-bit rounding where Pillow has it, no rotated image and no row buffer stored.
//            UVW: the nearest scale of the 16.16 fixed-point nearest rotation, two index look-ups.
//   stage 2  one thread per output pixel: crop((j, i, j + w, i + h)) and the same two resamples of the intermediate; ToTensor / Normalize,
//            the label bytes and mask = (u + v + w > 0).
// No atomics, no host synchronisation; a sample's bits depend on its own row of meta / params alone.
// Compiled with -ffp-contract=off: every multiply / add rounds separately, as in Pillow's C.
#include "sdfr_common.h"
#include "css_resample.h"

#define AUG_META 8                   // int32 per sample: h, w, first pixel of the sample in the packed sources, rotated width, rotated
                                     // height, 1 when the rotation is Pillow's copy shortcut, unused, unused
#define AUG_PARAMS SDFR_AUG_PARAMS   // float64 per sample: SDFR_AUG_* of include/sdfr.h
#define AUG_ROW(ksize) (3 + (ksize)) // int32 per table entry: nearest index, xmin, n, kk[ksize]
#define AUG_JIT_THREADS 1024

// ---- colour jitter ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int aug_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(a, b, f) of one byte: a + f (b - a) in float32; truncated for 0 <= f <= 1, else clipped and truncated
__device__ __forceinline__ int aug_blend(int a, int b, float f) {
    const float t = __fadd_rn((float)a, __fmul_rn(f, (float)(b - a)));
    if (f >= 0.f && f <= 1.0f) return (int)(uint8_t)(int)t;
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ int aug_clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// convert('HSV'), H += shift, convert('RGB') of one pixel (Pillow's rgb2hsv_row / hsv2rgb: float32 quotients, float64 where its C has
// double constants)
__device__ __forceinline__ void aug_hue(int& r, int& g, int& b, int shift) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    const int v = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = __fdiv_rn(cr, (float)maxc);
        const float rc = __fdiv_rn((float)(maxc - r), cr), gc = __fdiv_rn((float)(maxc - g), cr), bc = __fdiv_rn((float)(maxc - b), cr);
        float h;
        if (r == maxc) h = __fsub_rn(bc, gc);
        else if (g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
        else h = (float)((4.0 + (double)gc) - (double)rc);
        const double t = (double)h / 6.0 + 1.0;                         // in [5/6, 11/6]: fmod(t, 1.0) = t - floor(t), exact
        h = (float)(t - floor(t));
        uh = aug_clip255((int)((double)h * 255.0));
        us = aug_clip255((int)((double)s * 255.0));
    }
    uh = (uh + shift) & 255;
    if (us == 0) { r = g = b = v; return; }
    const double hf = (double)(float)uh * 6.0 / 255.0;
    const int i = (int)floor(hf);
    const double f = (double)(float)(hf - (double)(float)i);
    const double fs = (double)(float)((double)(float)us / 255.0);
    const double vf = (double)v;
    const int p = aug_clip255((int)floor(vf * (1.0 - fs) + 0.5));
    const int q = aug_clip255((int)floor(vf * (1.0 - fs * f) + 0.5));
    const int t2 = aug_clip255((int)floor(vf * (1.0 - fs * (1.0 - f)) + 0.5));
    switch (i % 6) {
        case 0: r = v; g = t2; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t2; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t2; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

struct AugJitter {
    float fb, fc, fs;                // brightness, contrast, saturation factors (the float Image.blend receives)
    int shift;                       // uint8(hue * 255); the hue step is skipped when the factor is 0
    int hue_on;
    int order;                       // operation ids in the order applied, two bits each from bit 0: 0 brightness, 1 contrast,
};                                   // 2 saturation, 3 hue (packed: an array indexed at run time would not stay in registers)

// operations order[first .. last) on one pixel; `mean` is the contrast operation's degenerate grey
__device__ __forceinline__ void aug_apply(const AugJitter& J, int first, int last, int mean, int& r, int& g, int& b) {
    for (int k = first; k < last; ++k) {
        const int op = (J.order >> (2 * k)) & 3;
        if (op == 0) {
            r = aug_blend(0, r, J.fb); g = aug_blend(0, g, J.fb); b = aug_blend(0, b, J.fb);
        } else if (op == 1) {
            r = aug_blend(mean, r, J.fc); g = aug_blend(mean, g, J.fc); b = aug_blend(mean, b, J.fc);
        } else if (op == 2) {
            const int L = aug_luma(r, g, b);
            r = aug_blend(L, r, J.fs); g = aug_blend(L, g, J.fs); b = aug_blend(L, b, J.fs);
        } else if (J.hue_on) {
            aug_hue(r, g, b, J.shift);
        }
    }
}

__global__ __launch_bounds__(AUG_JIT_THREADS) void sdfr_aug_jitter_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ meta,
                                                                         const double* __restrict__ params, uint8_t* __restrict__ jit) {
    __shared__ long long part[AUG_JIT_THREADS / 64];
    const int s = blockIdx.x;
    const int32_t* m = meta + AUG_META * s;
    const double* P = params + (int64_t)AUG_PARAMS * s;
    const int npix = m[0] * m[1];
    const uint8_t* in = src + 3 * (int64_t)m[2];
    uint8_t* out = jit + 3 * (int64_t)m[2];
    AugJitter J;
    J.fb = (float)P[SDFR_AUG_BRIGHTNESS]; J.fc = (float)P[SDFR_AUG_CONTRAST]; J.fs = (float)P[SDFR_AUG_SATURATION];
    J.hue_on = P[SDFR_AUG_HUE] != 0.0;
    J.shift = (int)(P[SDFR_AUG_HUE] * 255.0) & 255;
    int kc = 4;                                                          // position of the contrast operation in the order
    J.order = 0;
    for (int k = 0; k < 4; ++k) {
        const int op = (int)P[SDFR_AUG_ORDER + k] & 3;
        J.order |= op << (2 * k);
        if (op == 1 && kc == 4) kc = k;
    }
    // the L sum of the image as it stands when contrast is applied: exact integers, any summation order gives the same value
    long long sum = 0;
    if (kc < 4) {
        for (int p = threadIdx.x; p < npix; p += AUG_JIT_THREADS) {
            int r = in[3 * p], g = in[3 * p + 1], b = in[3 * p + 2];
            aug_apply(J, 0, kc, 0, r, g, b);
            sum += aug_luma(r, g, b);
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
        __syncthreads();
        sum = 0;
        for (int k = 0; k < AUG_JIT_THREADS / 64; ++k) sum += part[k];
    }
    const int mean = npix > 0 ? (int)((2 * sum + npix) / (2 * (long long)npix)) : 0;      // int(sum / n + 0.5)
    for (int p = threadIdx.x; p < npix; p += AUG_JIT_THREADS) {
        int r = in[3 * p], g = in[3 * p + 1], b = in[3 * p + 2];
        aug_apply(J, 0, 4, mean, r, g, b);
        out[3 * p] = (uint8_t)r; out[3 * p + 1] = (uint8_t)g; out[3 * p + 2] = (uint8_t)b;
    }
}

// ---- tables -------------------------------------------------------------------------------------------------------------------------------
// block = (sample, pass), thread = output index.  Input sizes: rotated width, rotated height, crop width, crop height.
__global__ __launch_bounds__(CSS_OUT) void sdfr_aug_table_kernel(const int32_t* __restrict__ meta, const double* __restrict__ params, int ksize,
                                                                int32_t* __restrict__ tab) {
    const int s = blockIdx.x >> 2, pass = blockIdx.x & 3, xx = threadIdx.x;
    const double* P = params + (int64_t)AUG_PARAMS * s;
    int inS;
    if (pass < 2) inS = meta[AUG_META * s + 3 + pass];
    else inS = (int)P[pass == 2 ? SDFR_AUG_BOX_W : SDFR_AUG_BOX_H];
    int32_t* row = tab + ((int64_t)blockIdx.x * CSS_OUT + xx) * AUG_ROW(ksize);
    css_coef_row(inS, xx, ksize, row + 1);
    // ImagingScaleAffine: the source coordinate starts at step / 2 and grows by one float64 addition per output index
    const double step = (double)inS / (double)CSS_OUT;
    double o = 0.0 + step * 0.5;
    for (int x = 0; x < xx; ++x) o += step;
    int idx = o < 0.0 ? -1 : (int)o;
    row[0] = idx < 0 ? 0 : (idx >= inS ? inS - 1 : idx);                 // (never outside for out = 128; the clamp guards the reads)
}

// ---- stage 1: rotate + resize to 128 x 128 ------------------------------------------------------------------------------------------------
// pixel (x, y) of Image.rotate(angle, BILINEAR, expand=True) of the h x w image `im`: ImagingGenericTransform with affine_transform and
// bilinear_filter32RGB
__device__ __forceinline__ void aug_rot_pixel(const uint8_t* __restrict__ im, int h, int w, const double* __restrict__ a, int copy, int x,
                                              int y, int* px) {
    if (copy) {
        const uint8_t* p = im + 3 * ((int64_t)min(y, h - 1) * w + min(x, w - 1));
        px[0] = p[0]; px[1] = p[1]; px[2] = p[2];
        return;
    }
    const double xi = x + 0.5, yi = y + 0.5;
    double xin = (a[0] * xi + a[1] * yi) + a[2];
    double yin = (a[3] * xi + a[4] * yi) + a[5];
    if (!(xin >= 0.0 && xin < (double)w && yin >= 0.0 && yin < (double)h)) { px[0] = px[1] = px[2] = 0; return; }
    xin -= 0.5; yin -= 0.5;
    const int x0f = (int)floor(xin), y0f = (int)floor(yin);             // in [-1, size - 1]
    const double dx = xin - x0f, dy = yin - y0f;
    const int x0 = max(x0f, 0), x1 = min(x0f + 1, w - 1);
    const uint8_t* r0 = im + 3 * (int64_t)max(y0f, 0) * w;
    const bool lower = y0f + 1 < h;                                     // y + 1 >= 0 always
    const uint8_t* r1 = im + 3 * (int64_t)(lower ? y0f + 1 : max(y0f, 0)) * w;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double p00 = r0[3 * x0 + c], p01 = r0[3 * x1 + c];
        double v1 = p00 + (p01 - p00) * dx;
        double v2 = v1;
        if (lower) {
            const double p10 = r1[3 * x0 + c], p11 = r1[3 * x1 + c];
            v2 = p10 + (p11 - p10) * dx;
        }
        v1 = v1 + (v2 - v1) * dy;
        px[c] = (int)(uint8_t)(int)v1;
    }
}

__device__ __forceinline__ long long aug_fix16(double v) { return (long long)floor(v * 65536.0 + 0.5); }

__global__ __launch_bounds__(256) void sdfr_aug_stage1_kernel(const uint8_t* __restrict__ jit, const uint8_t* __restrict__ uvw_src,
                                                             const int32_t* __restrict__ meta, const double* __restrict__ params, int ksize,
                                                             const int32_t* __restrict__ tab, uint8_t* __restrict__ mid_rgb,
                                                             uint8_t* __restrict__ mid_uvw) {
    const int s = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x, yy = pix >> 7, xx = pix & (CSS_OUT - 1);
    const int32_t* m = meta + AUG_META * s;
    const int h = m[0], w = m[1], nw = m[3], nh = m[4], copy = m[5];
    const double* a = params + (int64_t)AUG_PARAMS * s + SDFR_AUG_MATRIX;
    const int32_t* kh = tab + (((int64_t)s * 4 + 0) * CSS_OUT + xx) * AUG_ROW(ksize);
    const int32_t* kv = tab + (((int64_t)s * 4 + 1) * CSS_OUT + yy) * AUG_ROW(ksize);
    const int64_t o = (((int64_t)s * CSS_OUT + yy) * CSS_OUT + xx) * 3;
    {   // RGB: vertical pass over the horizontal pass' bytes
        const uint8_t* im = jit + 3 * (int64_t)m[2];
        const int xmin = kh[1], nx = kh[2], ymin = kv[1], ny = kv[2];
        int av[3] = {1 << (CSS_PRECISION_BITS - 1), 1 << (CSS_PRECISION_BITS - 1), 1 << (CSS_PRECISION_BITS - 1)};
        for (int y = 0; y < ny; ++y) {
            int ah[3] = {1 << (CSS_PRECISION_BITS - 1), 1 << (CSS_PRECISION_BITS - 1), 1 << (CSS_PRECISION_BITS - 1)};
            const int ry = min(ymin + y, nh - 1);
            for (int x = 0; x < nx; ++x) {
                int px[3];
                aug_rot_pixel(im, h, w, a, copy, min(xmin + x, nw - 1), ry, px);
                const int kk = kh[3 + x];
#pragma unroll
                for (int c = 0; c < 3; ++c) ah[c] += px[c] * kk;
            }
            const int kk = kv[3 + y];
#pragma unroll
            for (int c = 0; c < 3; ++c) av[c] += (int)css_clip8(ah[c]) * kk;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) mid_rgb[o + c] = (uint8_t)css_clip8(av[c]);
    }
    {   // UVW: nearest scale of the nearest rotation (Pillow's affine_fixed: 16.16 integers, one addition per pixel and per row)
        const uint8_t* im = uvw_src + 3 * (int64_t)m[2];
        const int sx = kh[0], sy = kv[0];
        int u[3] = {0, 0, 0};
        if (copy) {
            const uint8_t* p = im + 3 * ((int64_t)min(sy, h - 1) * w + min(sx, w - 1));
            u[0] = p[0]; u[1] = p[1]; u[2] = p[2];
        } else {
            const long long a0 = aug_fix16(a[0]), a1 = aug_fix16(a[1]), a3 = aug_fix16(a[3]), a4 = aug_fix16(a[4]);
            const long long a2 = aug_fix16((a[2] + a[0] * 0.5) + a[1] * 0.5), a5 = aug_fix16((a[5] + a[3] * 0.5) + a[4] * 0.5);
            const long long xin = (a2 + a1 * sy + a0 * sx) >> 16, yin = (a5 + a4 * sy + a3 * sx) >> 16;
            if (xin >= 0 && xin < w && yin >= 0 && yin < h) {
                const uint8_t* p = im + 3 * (yin * w + xin);
                u[0] = p[0]; u[1] = p[1]; u[2] = p[2];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) mid_uvw[o + c] = (uint8_t)u[c];
    }
}

// ---- stage 2: crop + resize to 128 x 128, tensors -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sdfr_aug_stage2_kernel(const uint8_t* __restrict__ mid_rgb, const uint8_t* __restrict__ mid_uvw,
                                                             const double* __restrict__ params, int ksize, const int32_t* __restrict__ tab,
                                                             float* __restrict__ rgb, uint8_t* __restrict__ uvw, uint8_t* __restrict__ mask,
                                                             uint8_t* __restrict__ rgb_u8) {
    const int s = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x, yy = pix >> 7, xx = pix & (CSS_OUT - 1);
    const double* P = params + (int64_t)AUG_PARAMS * s;
    const int bi = (int)P[SDFR_AUG_BOX_I], bj = (int)P[SDFR_AUG_BOX_J];
    const int32_t* kh = tab + (((int64_t)s * 4 + 2) * CSS_OUT + xx) * AUG_ROW(ksize);
    const int32_t* kv = tab + (((int64_t)s * 4 + 3) * CSS_OUT + yy) * AUG_ROW(ksize);
    const int64_t img = (int64_t)s * CSS_OUT * CSS_OUT * 3;
    const int xmin = kh[1], nx = kh[2], ymin = kv[1], ny = kv[2];
    int av[3] = {1 << (CSS_PRECISION_BITS - 1), 1 << (CSS_PRECISION_BITS - 1), 1 << (CSS_PRECISION_BITS - 1)};
    for (int y = 0; y < ny; ++y) {
        int ah[3] = {1 << (CSS_PRECISION_BITS - 1), 1 << (CSS_PRECISION_BITS - 1), 1 << (CSS_PRECISION_BITS - 1)};
        const uint8_t* r = mid_rgb + img + (int64_t)min(bi + ymin + y, CSS_OUT - 1) * (CSS_OUT * 3);
        for (int x = 0; x < nx; ++x) {
            const uint8_t* p = r + 3 * min(bj + xmin + x, CSS_OUT - 1);
            const int kk = kh[3 + x];
#pragma unroll
            for (int c = 0; c < 3; ++c) ah[c] += (int)p[c] * kk;
        }
        const int kk = kv[3 + y];
#pragma unroll
        for (int c = 0; c < 3; ++c) av[c] += (int)css_clip8(ah[c]) * kk;
    }
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    const uint8_t* q = mid_uvw + img + ((int64_t)min(bi + kv[0], CSS_OUT - 1) * CSS_OUT + min(bj + kh[0], CSS_OUT - 1)) * 3;
    int lab = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t b = css_clip8(av[c]);
        const int64_t e = (((int64_t)s * 3 + c) * CSS_OUT + yy) * CSS_OUT + xx;
        rgb[e] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)b, 255.0f), mean[c]), sd[c]);
        if (rgb_u8) rgb_u8[((int64_t)s * CSS_OUT * CSS_OUT + pix) * 3 + c] = (uint8_t)b;
        uvw[e] = q[c];
        lab += q[c];
    }
    mask[(int64_t)s * CSS_OUT * CSS_OUT + pix] = lab > 0 ? 1 : 0;
}

extern "C" int sdfr_augment(const uint8_t* rgb_src, const uint8_t* uvw_src, const int32_t* meta, const double* params, int B, int ksize,
                            int32_t* tab, uint8_t* jit, uint8_t* mid_rgb, uint8_t* mid_uvw, float* rgb, uint8_t* uvw, uint8_t* mask,
                            uint8_t* rgb_u8, void* stream) {
    SDFR_REQUIRE(B >= 0 && B <= 65535 && ksize >= 3, "sdfr_augment: bad size");
    if (B == 0) return SDFR_OK;
    SDFR_REQUIRE(rgb_src && uvw_src && meta && params && tab && jit && mid_rgb && mid_uvw && rgb && uvw && mask, "sdfr_augment: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sdfr_aug_jitter_kernel, dim3(B), dim3(AUG_JIT_THREADS), 0, s, rgb_src, meta, params, jit);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_aug_table_kernel, dim3(4 * B), dim3(CSS_OUT), 0, s, meta, params, ksize, tab);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_aug_stage1_kernel, dim3(CSS_OUT * CSS_OUT / 256, B), dim3(256), 0, s, jit, uvw_src, meta, params, ksize, tab, mid_rgb,
                       mid_uvw);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_aug_stage2_kernel, dim3(CSS_OUT * CSS_OUT / 256, B), dim3(256), 0, s, mid_rgb, mid_uvw, params, ksize, tab, rgb, uvw,
                       mask, rgb_u8);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
