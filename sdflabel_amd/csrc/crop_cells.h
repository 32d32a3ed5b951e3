// Per-pixel code of the training-crop export (crops.hip).  DESIGN.md ("Training crops") has the rules.
// Everything here is a plain function of one pixel, compiled for the device by crops.hip and for the host by
// tests/export_host/export_host.cpp, which loops over every pixel and is compared with the numpy restatement (tests/_export_ref.py) bit
// for bit.  Both translation units are compiled with -ffp-contract=off: every operation rounds separately.
//
// The rasteriser (verify_cells.h) has already decided which triangle wins a pixel and at what depth.  Here the winner's three per-vertex
// attributes -- the lattice-frame vertex positions, i.e. NOCS -- are interpolated perspective-correctly at the pixel and coloured as the
// reference colours NOCS, (x + 1) / 2 of 255; a frame's annotations occlude each other by the rasteriser's own key idiom.
#pragma once
#include "verify_cells.h"

#define CROP_COUNTS 4            // int32 per annotation: box pixels, covered, visible, flag word

// val -> byte: 0 for val <= 0 or NaN, 255 for val >= 255, else rint(val), ties to even
VERIFY_HD uint8_t crop_byte(double val) {
    if (!(val > 0.0)) return 0;
    if (val >= 255.0) return 255;
    return (uint8_t)(int)rint(val);
}

// The three NOCS bytes of a COVERED pixel (x, y) of triangle T (verify_tri_setup for the raster's window, K and z_min) with the float32
// attributes a0, a1, a2 [3] of its vertices.  E is verify_edges', as the rasteriser's own; q_i = E_i / z_i; D = (q0 + q1) + q2;
// n_k = (q0 a0[k] + q1 a1[k]) + q2 a2[k], every product rounded on its own; c_k = n_k / D; val = (c_k + 1) 127.5.  Three zero bytes become
// (0, 0, 1): the loader's mask u + v + w > 0 is then exactly the set of labelled pixels.
VERIFY_HD void crop_shade(const VerifyTri* T, int x, int y, const float* a0, const float* a1, const float* a2, uint8_t* out) {
    double E[3], q[3];
    verify_edges(T, x, y, E);
    for (int i = 0; i < 3; ++i) q[i] = E[i] / T->z[i];
    const double D = (q[0] + q[1]) + q[2];
    for (int k = 0; k < 3; ++k) {
        const double t0 = q[0] * (double)a0[k], t1 = q[1] * (double)a1[k], t2 = q[2] * (double)a2[k];
        const double n = (t0 + t1) + t2;
        const double c = n / D;
        const double val = (c + 1.0) * 127.5;
        out[k] = crop_byte(val);
    }
    if (out[0] == 0 && out[1] == 0 && out[2] == 0) out[2] = 1;
}

// one float32 colour value (0 ... 1) -> rintf(255 v) in float32, clamped to 0 ... 255; NaN gives 0.  k / 255 returns k.
VERIFY_HD uint8_t crop_rgb_byte(float v) {
    const float m = 255.0f * v;
    if (!(m > 0.0f)) return 0;
    if (m >= 255.0f) return 255;
    return (uint8_t)(int)rintf(m);
}

// the key of a covered window pixel of annotation b: the minimum over a frame's annotations is the nearest, and on an exact tie the lowest index
VERIFY_HD uint64_t crop_owner_key(float depth, uint32_t b) {
    uint32_t bits;
    memcpy(&bits, &depth, 4);
    return (uint64_t)bits << 32 | (uint64_t)b;
}

// the half-open box lies inside the window and its pixels are exactly off[0] .. off[1] of an array of Q
VERIFY_HD bool crop_box_ok(const int32_t* box, const int32_t* w, const int64_t* off, int64_t Q) {
    if (!(w[0] <= box[0] && box[0] <= box[2] && box[2] <= w[2] && w[1] <= box[1] && box[1] <= box[3] && box[3] <= w[3])) return false;
    return off[0] >= 0 && off[1] <= Q && off[1] - off[0] == (int64_t)(box[2] - box[0]) * (box[3] - box[1]);
}

// mesh offsets inside the arrays
VERIFY_HD bool crop_range_ok(const int64_t* off, int64_t N) { return off[0] >= 0 && off[0] <= off[1] && off[1] <= N; }

// The owner of window pixel i (global index into the packed rasters) of annotation b at image pixel (x, y): -1 where b's own mask does not
// cover, else the annotation with the minimum key among those whose (usable) window contains the pixel and whose mask covers it there.
VERIFY_HD int32_t crop_owner_pixel(const uint8_t* mask, const float* depth, const int32_t* windows, const int64_t* poff, int64_t P, int B, int W,
                                   int H, int b, int64_t i, int x, int y) {
    if (mask[i] == 0) return -1;
    uint64_t best = crop_owner_key(depth[i], (uint32_t)b);
    for (int c = 0; c < B; ++c) {
        if (c == b) continue;
        const int32_t* w = windows + 4 * c;
        if (!verify_window_ok(w, poff + c, P, W, H)) continue;
        if (!(w[0] <= x && x < w[2] && w[1] <= y && y < w[3])) continue;
        const int64_t j = verify_window_pixel(w, poff[c], x, y);
        if (mask[j] == 0) continue;
        const uint64_t key = crop_owner_key(depth[j], (uint32_t)c);
        if (key < best) best = key;
    }
    return (int32_t)(uint32_t)(best & 0xffffffffull);
}

// The raster's batch and what the export adds to it; all pointers as the entry points take them.
struct CropArgs : RasterArgs {
    const float* attributes;     // [V][3] per-vertex attributes (lattice-frame positions)
    const int32_t* boxes;        // [B][4] l, t, r, b inside the window
    const int64_t* qoff;         // [B + 1]
    int64_t Q;
};

// annotation b's window, box and offsets fit together and stay inside what the caller allocated
VERIFY_HD bool crop_anno_ok(const CropArgs* a, int b) {
    return verify_window_ok(a->windows + 4 * b, a->poff + b, a->P, a->W, a->H) && crop_box_ok(a->boxes + 4 * b, a->windows + 4 * b, a->qoff + b, a->Q) &&
           crop_range_ok(a->voff + b, a->V) && crop_range_ok(a->toff + b, a->T);
}

// Output pixel g (global index into the packed crops): the NOCS bytes of its annotation's winning triangle where the annotation is
// visible, else zeros.  Returns the flag bits to raise in the annotation's flag word (*anno; -1 when g belongs to no usable annotation).
// triangle: the raster's winning triangle per window pixel; owner: crop_owner_pixel's output or NULL (occlusion off).
VERIFY_HD int crop_export_pixel(const CropArgs* a, const int32_t* triangle, const int32_t* owner, int64_t g, uint8_t* out, int* anno,
                                int64_t* window_pixel) {
    out[0] = out[1] = out[2] = 0;
    *window_pixel = -1;
    const int b = verify_owner(a->qoff, a->B, g);
    *anno = -1;
    if (!crop_anno_ok(a, b) || g < a->qoff[b] || g >= a->qoff[b + 1]) return 0;            // (the flag of an unusable annotation is raised by the init launch)
    *anno = b;
    const int32_t* w = a->windows + 4 * b;
    const int32_t* box = a->boxes + 4 * b;
    const int64_t local = g - a->qoff[b];
    const int bw = box[2] - box[0];
    const int x = box[0] + (int)(local % bw), y = box[1] + (int)(local / bw);
    const int64_t i = verify_window_pixel(w, a->poff[b], x, y);                            // inside poff[b] .. poff[b + 1]: the box is inside the window
    *window_pixel = i;
    const int32_t tri = triangle[i];
    if (tri == -1) return 0;
    const int64_t t0 = a->toff[b], nt = a->toff[b + 1] - t0, v0 = a->voff[b], nv = a->voff[b + 1] - v0;
    if (tri < 0 || tri >= nt) return VERIFY_FLAG_INVALID;
    const int32_t* f = a->faces + 3 * (t0 + tri);
    if (!verify_face_ok(f, nv)) return VERIFY_FLAG_INVALID;
    if (owner && owner[i] != b) return 0;
    VerifyTri T;
    // a triangle the rasteriser would have skipped cannot have won a pixel: the triangle image does not belong to this mesh
    if (verify_tri_setup(a->vertices + 3 * (v0 + f[0]), a->vertices + 3 * (v0 + f[1]), a->vertices + 3 * (v0 + f[2]), a->K, a->z_min, w[0], w[1],
                         w[2], w[3], &T) != VERIFY_TRI_OK)
        return VERIFY_FLAG_INVALID;
    crop_shade(&T, x, y, a->attributes + 3 * (v0 + f[0]), a->attributes + 3 * (v0 + f[1]), a->attributes + 3 * (v0 + f[2]), out);
    return 0;
}
