// Pillow's 8-bit bilinear ImagingResample, the parts every user shares: the coefficient row of one output index and the final clip of an
// accumulator.  Included by ingest.hip (the CSS network's input) and augment.hip (the training crops); both compile with -ffp-contract=off.
#pragma once
#include <stdint.h>

#define CSS_OUT 128                  // transforms.Resize((128, 128))
#define CSS_PRECISION_BITS 22        // Pillow's 32 - 8 - 2

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter (support 1), in double like its C: output index xx of a pass
// from inS to CSS_OUT samples.  out = { xmin, n, kk[0 .. ksize) }.
__device__ __forceinline__ void css_coef_row(int inS, int xx, int ksize, int32_t* __restrict__ out) {
    const double scale = (double)inS / (double)CSS_OUT;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    const double center = 0.0 + (xx + 0.5) * scale;
    const double ss = 1.0 / fs;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > inS) xmax = inS;
    int n = xmax - xmin;
    if (n > ksize) n = ksize;                                           // cannot happen for ksize = ceil(support) * 2 + 1; guards the table
    if (n < 0) n = 0;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
        double t = (x + xmin - center + 0.5) * ss;
        if (t < 0.0) t = -t;
        const double wgt = t < 1.0 ? 1.0 - t : 0.0;
        ww += wgt;
    }
    out[0] = xmin;
    out[1] = n;
    for (int x = 0; x < n; ++x) {
        double t = (x + xmin - center + 0.5) * ss;                      // the same operations as above: the same bits
        if (t < 0.0) t = -t;
        double wgt = t < 1.0 ? 1.0 - t : 0.0;
        if (ww != 0.0) wgt /= ww;
        out[2 + x] = (int)(0.5 + wgt * (double)(1 << CSS_PRECISION_BITS));      // no negative taps in the triangle filter
    }
}

__device__ __forceinline__ uint32_t css_clip8(int v) {
    v >>= CSS_PRECISION_BITS;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
