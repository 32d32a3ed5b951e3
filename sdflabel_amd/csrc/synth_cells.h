// Per-pixel code of the synthetic bootstrap crops (synth.hip).  DESIGN.md ("Synthetic crops") has the rules.
// Everything here is a plain function of one pixel, compiled for the device by synth.hip and for the host by
// tests/synth_host/synth_host.cpp, which loops over every pixel and is compared with the numpy restatement (tests/_synth_ref.py) bit for
// bit.  Both translation units are compiled with -ffp-contract=off: every operation rounds separately.
//
// The rasteriser (verify_cells.h) has decided which triangle wins a window pixel, the scene-aware owner below which of a scene's objects is
// nearest there.  The colour of a crop pixel is the owner's winning triangle shaded with its interpolated vertex normal (ambient + Lambert +
// Blinn-Phong with an integer exponent 2^shin: no pow, no exp), or the scene's background where nothing covers the pixel.
#pragma once
#include "crop_cells.h"

#define SYNTH_PAINT 5            // double per annotation: albedo r, g, b, ks, shin (0 .. 7; the exponent is 2^shin)
#define SYNTH_LIGHT 5            // double per scene: light x, y, z (a unit vector of the camera frame, taken as given), ambient, kd
#define SYNTH_RAMP 8             // int32 per scene: top r, g, b, bottom r, g, b, noise amplitude (each clamped to 0 .. 255), noise seed

// crop_owner_pixel among the annotations of b's scene: annotation c counts only when scene[c] == scene[b].  scene == NULL: crop_owner_pixel.
VERIFY_HD int32_t synth_owner_pixel(const uint8_t* mask, const float* depth, const int32_t* windows, const int64_t* poff, int64_t P,
                                    const int32_t* scene, int B, int W, int H, int b, int64_t i, int x, int y) {
    if (mask[i] == 0) return -1;
    uint64_t best = crop_owner_key(depth[i], (uint32_t)b);
    for (int c = 0; c < B; ++c) {
        if (c == b) continue;
        if (scene && scene[c] != scene[b]) continue;
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

VERIFY_HD uint64_t synth_mix64(uint64_t z) {          // splitmix64 finaliser (the mixer of pose.hip's device sampler)
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the noise word of channel k of image pixel (x, y): the high half of mix64(seed ^ mix64((x << 33 | y << 2 | k) * golden + 1))
VERIFY_HD uint32_t synth_hash32(uint32_t seed, int x, int y, int k) {
    const uint64_t key = (uint64_t)(uint32_t)x << 33 | (uint64_t)(uint32_t)y << 2 | (uint64_t)(uint32_t)k;
    return (uint32_t)(synth_mix64((uint64_t)seed ^ synth_mix64(key * 0x9E3779B97F4A7C15ull + 1ull)) >> 32);
}

VERIFY_HD int synth_clamp_byte(int64_t v) { return v < 0 ? 0 : v > 255 ? 255 : (int)v; }

// procedural background, integers only: a vertical ramp top + ((bottom - top) y) / max(H - 1, 1) (C division: towards zero) plus the noise
// ((hash >> 24) amp >> 8) - (amp >> 1), clamped to 0 .. 255
VERIFY_HD uint8_t synth_ramp_byte(const int32_t* ramp, int H, int x, int y, int k) {
    const int top = synth_clamp_byte(ramp[k]), bot = synth_clamp_byte(ramp[3 + k]), amp = synth_clamp_byte(ramp[6]);
    const int den = H - 1 > 1 ? H - 1 : 1;
    const int64_t base = top + ((int64_t)(bot - top) * y) / den;
    const uint32_t h = synth_hash32((uint32_t)ramp[7], x, y, k);
    const int noise = (int)(((h >> 24) * (uint32_t)amp) >> 8) - (amp >> 1);
    return (uint8_t)synth_clamp_byte(base + noise);
}

VERIFY_HD double synth_pos(double v) { return v > 0.0 ? v : 0.0; }          // max(0, v); 0 for NaN

// The three colour bytes of a COVERED pixel (x, y) of triangle T with the float32 camera-frame normals n0, n1, n2 [3] of its vertices.
// Weights as crop_shade: q_i = E_i / z_i, D = (q0 + q1) + q2, n_k = ((q0 n0k + q1 n1k) + q2 n2k) / D; the normal is normalised (0 when its
// squared length is not positive); view ray v = -p / |p| through p = ((x - cx) / fx, (y - cy) / fy, 1); half vector h = (l + v) / |l + v| (0
// when the length is not positive); d = max(0, n.l), s = max(0, n.h) squared shin times; val_k = albedo_k (ambient + kd d) + ks s.
// Dot products are summed left to right.
VERIFY_HD void synth_shade(const VerifyTri* T, int x, int y, const double* K, const float* n0, const float* n1, const float* n2,
                           const double* paint, const double* light, uint8_t* out) {
    double E[3], q[3], n[3];
    verify_edges(T, x, y, E);
    for (int i = 0; i < 3; ++i) q[i] = E[i] / T->z[i];
    const double D = (q[0] + q[1]) + q[2];
    for (int k = 0; k < 3; ++k) {
        const double t0 = q[0] * (double)n0[k], t1 = q[1] * (double)n1[k], t2 = q[2] * (double)n2[k];
        const double m = (t0 + t1) + t2;
        n[k] = m / D;
    }
    const double len2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (!(len2 > 0.0)) {
        n[0] = n[1] = n[2] = 0.0;
    } else {
        const double len = sqrt(len2);
        for (int k = 0; k < 3; ++k) n[k] = n[k] / len;
    }
    const double px = ((double)x - K[2]) / K[0], py = ((double)y - K[3]) / K[1];
    const double pl = sqrt((px * px + py * py) + 1.0);
    const double v[3] = {-(px / pl), -(py / pl), -(1.0 / pl)};
    const double* l = light;
    const double d = synth_pos((n[0] * l[0] + n[1] * l[1]) + n[2] * l[2]);
    double h[3];
    for (int k = 0; k < 3; ++k) h[k] = l[k] + v[k];
    const double hl2 = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2];
    if (!(hl2 > 0.0)) {
        h[0] = h[1] = h[2] = 0.0;
    } else {
        const double hl = sqrt(hl2);
        for (int k = 0; k < 3; ++k) h[k] = h[k] / hl;
    }
    double s = synth_pos((n[0] * h[0] + n[1] * h[1]) + n[2] * h[2]);
    const double sh = paint[4];
    const int shin = !(sh > 0.0) ? 0 : sh >= 7.0 ? 7 : (int)sh;
    for (int i = 0; i < shin; ++i) s = s * s;
    const double diffuse = light[3] + light[4] * d;
    const double spec = paint[3] * s;
    for (int k = 0; k < 3; ++k) {
        const double val = paint[k] * diffuse + spec;
        out[k] = crop_byte(255.0 * val);
    }
}

// The export's batch and what the shading adds to it; all pointers as sdfr_synth_shade takes them.
struct SynthArgs : CropArgs {
    const float* normals;        // [V][3] camera-frame vertex normals (CropArgs::attributes is not read)
    const int32_t* scene;        // [B] scene of every annotation, or NULL: all in scene 0
    const double* paint;         // [B][SYNTH_PAINT]
    const double* light;         // [S][SYNTH_LIGHT]
    const int32_t* bg_index;     // [S] which background image a scene uses (outside 0 .. NBG - 1: the procedural one), or NULL
    const uint8_t* bg;           // [NBG][H][W][3] RGB
    const int32_t* ramp;         // [S][SYNTH_RAMP]
    int S, NBG;
};

VERIFY_HD int synth_scene_of(const SynthArgs* a, int b) { return a->scene ? a->scene[b] : 0; }

// crop_anno_ok, and the annotation's scene is one of the S scenes
VERIFY_HD bool synth_anno_ok(const SynthArgs* a, int b) {
    const int s = synth_scene_of(a, b);
    return crop_anno_ok(a, b) && s >= 0 && s < a->S;
}

VERIFY_HD void synth_background(const SynthArgs* a, int s, int x, int y, uint8_t* out) {
    const int32_t at = a->bg_index ? a->bg_index[s] : -1;
    for (int k = 0; k < 3; ++k)
        out[k] = at >= 0 && at < a->NBG ? a->bg[(((int64_t)at * a->H + y) * a->W + x) * 3 + k] : synth_ramp_byte(a->ramp + SYNTH_RAMP * s, a->H, x, y, k);
}

// Output pixel g (global index into the packed crops) of annotation b: the shaded colour of the owner c of b's window pixel, read at c's
// own window pixel, or the background of b's scene where the owner is -1 or cannot be looked up (an index outside the batch, another scene,
// a window or mesh offsets that do not fit, a window that does not hold the pixel, no winning triangle there).  Returns the flag bits to
// raise in b's flag word (*anno; -1 when g belongs to no usable annotation, and the bytes are zero).
VERIFY_HD int synth_shade_pixel(const SynthArgs* a, const int32_t* triangle, const int32_t* owner, int64_t g, uint8_t* out, int* anno) {
    out[0] = out[1] = out[2] = 0;
    const int b = verify_owner(a->qoff, a->B, g);
    *anno = -1;
    if (!synth_anno_ok(a, b) || g < a->qoff[b] || g >= a->qoff[b + 1]) return 0;           // (the flag of an unusable annotation is raised by the init launch)
    *anno = b;
    const int32_t* box = a->boxes + 4 * b;
    const int64_t local = g - a->qoff[b];
    const int bw = box[2] - box[0];
    const int x = box[0] + (int)(local % bw), y = box[1] + (int)(local / bw);
    const int s = synth_scene_of(a, b);
    const int32_t c = owner[verify_window_pixel(a->windows + 4 * b, a->poff[b], x, y)];    // inside poff[b] .. poff[b + 1]: the box is inside the window
    if (c >= 0 && c < a->B && synth_scene_of(a, c) == s) {
        const int32_t* w = a->windows + 4 * c;
        if (verify_window_ok(w, a->poff + c, a->P, a->W, a->H) && crop_range_ok(a->voff + c, a->V) && crop_range_ok(a->toff + c, a->T) && w[0] <= x &&
            x < w[2] && w[1] <= y && y < w[3]) {
            const int32_t tri = triangle[verify_window_pixel(w, a->poff[c], x, y)];
            if (tri != -1) {
                const int64_t t0 = a->toff[c], nt = a->toff[c + 1] - t0, v0 = a->voff[c], nv = a->voff[c + 1] - v0;
                if (tri < 0 || tri >= nt) return VERIFY_FLAG_INVALID;
                const int32_t* f = a->faces + 3 * (t0 + tri);
                if (!verify_face_ok(f, nv)) return VERIFY_FLAG_INVALID;
                VerifyTri T;
                if (verify_tri_setup(a->vertices + 3 * (v0 + f[0]), a->vertices + 3 * (v0 + f[1]), a->vertices + 3 * (v0 + f[2]), a->K, a->z_min, w[0],
                                     w[1], w[2], w[3], &T) != VERIFY_TRI_OK)
                    return VERIFY_FLAG_INVALID;
                synth_shade(&T, x, y, a->K, a->normals + 3 * (v0 + f[0]), a->normals + 3 * (v0 + f[1]), a->normals + 3 * (v0 + f[2]),
                            a->paint + SYNTH_PAINT * c, a->light + SYNTH_LIGHT * s, out);
                return 0;
            }
        }
    }
    synth_background(a, s, x, y, out);
    return 0;
}
