// Host harness of sdflabel_amd/csrc/synth_cells.h: rasterises every mesh with verify_cells.h (the atomic minimum done sequentially), then runs
// the scene-aware owner for every window pixel and the shading for every box pixel and writes what the kernels of synth.hip would write.
// tests/test_synth_cpu.py compares the output with the numpy restatement (tests/_synth_ref.py).
//   synth_host IN OUT
//   IN : int32 B, W, H, S, NBG, has_scene, has_triangle, has_qoff; float32 z_min; float64 K[4]; int64 voff[B + 1], toff[B + 1];
//        int32 windows[B][4], boxes[B][4]; int32 scene[B] (if has_scene); int64 qoff[B + 1] (if has_qoff: passed in place of the boxes' own);
//        float64 paint[B][5], light[S][5]; int32 ramp[S][8]; int32 bg_index[S] and uint8 bg[NBG][H][W][3] (if NBG > 0);
//        float32 vertices[V][3], normals[V][3]; int32 faces[T][3]; int32 triangle[P] (if has_triangle: used in place of the raster's)
//   OUT: int32 owner[P]; uint8 rgb[Q][3]; int32 flags[B]
// Every buffer has exactly the size the kernels' caller would allocate, so a sanitizer build of this program checks the index arithmetic.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "synth_cells.h"

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t h[8];
    float z_min;
    double K[4];
    if (!f || fread(h, 4, 8, f) != 8 || fread(&z_min, 4, 1, f) != 1 || fread(K, 8, 4, f) != 4) return 3;
    const int B = h[0], W = h[1], H = h[2], S = h[3], NBG = h[4];
    const bool has_scene = h[5] != 0, has_triangle = h[6] != 0, has_qoff = h[7] != 0;
    if (B < 0 || W < 1 || H < 1 || S < 1 || NBG < 0) return 3;
    std::vector<int64_t> voff, toff, qoff_in;
    std::vector<int32_t> windows, boxes, scene, ramp, bg_index, faces, triangle_in;
    std::vector<double> paint, light;
    std::vector<uint8_t> bg;
    std::vector<float> vertices, normals;
    if (!rd(f, voff, B + 1) || !rd(f, toff, B + 1) || !rd(f, windows, 4 * (size_t)B) || !rd(f, boxes, 4 * (size_t)B)) return 3;
    if (has_scene && !rd(f, scene, (size_t)B)) return 3;
    if (has_qoff && !rd(f, qoff_in, (size_t)B + 1)) return 3;
    if (!rd(f, paint, SYNTH_PAINT * (size_t)B) || !rd(f, light, SYNTH_LIGHT * (size_t)S) || !rd(f, ramp, SYNTH_RAMP * (size_t)S)) return 3;
    if (NBG > 0 && (!rd(f, bg_index, (size_t)S) || !rd(f, bg, (size_t)NBG * H * W * 3))) return 3;
    const int64_t V = voff[B], T = toff[B];
    if (voff[0] != 0 || toff[0] != 0 || V < 0 || T < 0) return 3;
    std::vector<int64_t> poff(B + 1, 0), qoff(B + 1, 0);
    for (int b = 0; b < B; ++b) {
        const int32_t* w = &windows[4 * b];
        const int32_t* x = &boxes[4 * b];
        if (!(x[0] <= x[2] && x[1] <= x[3])) return 3;                   // (a box outside its window is a case: the flag is expected)
        poff[b + 1] = poff[b] + (int64_t)(w[2] - w[0]) * (w[3] - w[1]);
        qoff[b + 1] = qoff[b] + (int64_t)(x[2] - x[0]) * (x[3] - x[1]);
        if (voff[b + 1] < voff[b] || toff[b + 1] < toff[b] || poff[b + 1] < poff[b]) return 3;
    }
    const int64_t P = poff[B], Q = qoff[B];                               // the buffers' sizes, whatever offset table is passed
    if (has_qoff) qoff = qoff_in;
    if (!rd(f, vertices, 3 * (size_t)V) || !rd(f, normals, 3 * (size_t)V) || !rd(f, faces, 3 * (size_t)T)) return 3;
    if (has_triangle && !rd(f, triangle_in, (size_t)P)) return 3;
    fclose(f);
    // raster: keys by a sequential minimum (as tests/verify_host/verify_host.cpp)
    std::vector<uint64_t> keys((size_t)P, VERIFY_NO_KEY);
    for (int64_t g = 0; g < T; ++g) {
        const int b = verify_owner(toff.data(), B, g);
        const int64_t v0 = voff[b], nv = voff[b + 1] - v0;
        const int32_t* w = &windows[4 * b];
        const int32_t* fc = &faces[3 * g];
        if (!verify_face_ok(fc, nv) || !verify_window_ok(w, &poff[b], P, W, H)) continue;
        VerifyTri tri;
        if (verify_tri_setup(&vertices[3 * (v0 + fc[0])], &vertices[3 * (v0 + fc[1])], &vertices[3 * (v0 + fc[2])], K, z_min, w[0], w[1], w[2], w[3],
                             &tri) != VERIFY_TRI_OK)
            continue;
        for (int y = tri.y0; y <= tri.y1; ++y)
            for (int x = tri.x0; x <= tri.x1; ++x) {
                const uint64_t key = verify_pixel_key(&tri, x, y, (uint32_t)(g - toff[b]));
                const int64_t at = verify_window_pixel(w, poff[b], x, y);
                if (key < keys[at]) keys[at] = key;
            }
    }
    std::vector<uint8_t> mask((size_t)P);
    std::vector<float> depth((size_t)P);
    std::vector<int32_t> triangle((size_t)P);
    for (int64_t i = 0; i < P; ++i) verify_resolve(keys[i], &mask[i], &depth[i], &triangle[i]);
    if (has_triangle) triangle = triangle_in;
    // owner: the loop of sdfr_synth_owner_kernel over the window pixels
    std::vector<int32_t> owner((size_t)P);
    for (int64_t i = 0; i < P; ++i) {
        const int b = verify_owner(poff.data(), B, i);
        const int32_t* w = &windows[4 * b];
        if (!verify_window_ok(w, &poff[b], P, W, H) || i < poff[b] || i >= poff[b + 1]) {
            owner[i] = -1;
            continue;
        }
        const int64_t local = i - poff[b];
        const int ww = w[2] - w[0];
        owner[i] = synth_owner_pixel(mask.data(), depth.data(), windows.data(), poff.data(), P, has_scene ? scene.data() : nullptr, B, W, H, b, i,
                                     w[0] + (int)(local % ww), w[1] + (int)(local / ww));
    }
    // shade: init, per box pixel, scrub
    SynthArgs a;
    static_cast<CropArgs&>(a) = {raster_args(vertices.data(), V, faces.data(), T, voff.data(), toff.data(), windows.data(), poff.data(), P, B, W, H, K, z_min),
                                 nullptr, boxes.data(), qoff.data(), Q};
    a.normals = normals.data(), a.scene = has_scene ? scene.data() : nullptr, a.paint = paint.data(), a.light = light.data();
    a.bg_index = NBG ? bg_index.data() : nullptr, a.bg = bg.data(), a.ramp = ramp.data(), a.S = S, a.NBG = NBG;
    std::vector<int32_t> flags(B, 0);
    for (int b = 0; b < B; ++b) flags[b] = synth_anno_ok(&a, b) ? 0 : VERIFY_FLAG_INVALID;
    std::vector<uint8_t> rgb(3 * (size_t)Q);
    for (int64_t g = 0; g < Q; ++g) {
        int b;
        const int raise = synth_shade_pixel(&a, triangle.data(), owner.data(), g, &rgb[3 * g], &b);
        if (raise) flags[b] |= raise;
    }
    for (int64_t g = 0; g < Q; ++g) {
        const int b = verify_owner(qoff.data(), B, g);
        if (!(flags[b] & VERIFY_FLAG_INVALID)) continue;
        rgb[3 * g] = rgb[3 * g + 1] = rgb[3 * g + 2] = 0;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 4;
    wr(o, owner), wr(o, rgb), wr(o, flags);
    fclose(o);
    return 0;
}
