// Host harness of sdflabel_amd/csrc/crop_cells.h: rasterises every mesh with verify_cells.h (the atomic minimum done sequentially), then runs
// the export's per-pixel code for every window pixel and every box pixel and writes what the kernels of crops.hip would write.
// tests/test_export_cpu.py compares the output with the numpy restatement (tests/_export_ref.py).
//   export_host IN OUT
//   IN : int32 B, W, H, occlusion, has_colors, has_triangle; float32 z_min; float64 K[4]; int64 voff[B + 1], toff[B + 1];
//        int32 windows[B][4], boxes[B][4]; float32 vertices[V][3], attributes[V][3]; int32 faces[T][3]; float32 colors[Q][3] (if has_colors);
//        int32 triangle[P] (if has_triangle: used in place of the raster's winning triangles)
//   OUT: int32 owner[P] (if occlusion); uint8 uvw[Q][3]; uint8 rgb[Q][3] (if has_colors); int32 flags[B]; int32 counts[B][4]
// Every buffer has exactly the size the kernels' caller would allocate, so a sanitizer build of this program checks the index arithmetic.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "crop_cells.h"

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
    int32_t h[6];
    float z_min;
    double K[4];
    if (!f || fread(h, 4, 6, f) != 6 || fread(&z_min, 4, 1, f) != 1 || fread(K, 8, 4, f) != 4) return 3;
    const int B = h[0], W = h[1], H = h[2];
    const bool occlusion = h[3] != 0, has_colors = h[4] != 0, has_triangle = h[5] != 0;
    if (B < 0 || W < 1 || H < 1) return 3;
    std::vector<int64_t> voff, toff;
    std::vector<int32_t> windows, boxes, faces, triangle_in;
    std::vector<float> vertices, attributes, colors;
    if (!rd(f, voff, B + 1) || !rd(f, toff, B + 1) || !rd(f, windows, 4 * (size_t)B) || !rd(f, boxes, 4 * (size_t)B)) return 3;
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
    const int64_t P = poff[B], Q = qoff[B];
    if (!rd(f, vertices, 3 * (size_t)V) || !rd(f, attributes, 3 * (size_t)V) || !rd(f, faces, 3 * (size_t)T)) return 3;
    if (has_colors && !rd(f, colors, 3 * (size_t)Q)) return 3;
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
    // owner: the loop of sdfr_crop_owner_kernel over the window pixels
    std::vector<int32_t> owner;
    if (occlusion) {
        owner.resize((size_t)P);
        for (int64_t i = 0; i < P; ++i) {
            const int b = verify_owner(poff.data(), B, i);
            const int32_t* w = &windows[4 * b];
            if (!verify_window_ok(w, &poff[b], P, W, H) || i < poff[b] || i >= poff[b + 1]) {
                owner[i] = -1;
                continue;
            }
            const int64_t local = i - poff[b];
            const int ww = w[2] - w[0];
            owner[i] = crop_owner_pixel(mask.data(), depth.data(), windows.data(), poff.data(), P, B, W, H, b, i, w[0] + (int)(local % ww),
                                        w[1] + (int)(local / ww));
        }
    }
    // export: init, per box pixel, scrub
    const CropArgs a = {raster_args(vertices.data(), V, faces.data(), T, voff.data(), toff.data(), windows.data(), poff.data(), P, B, W, H, K, z_min),
                        attributes.data(), boxes.data(), qoff.data(), Q};
    std::vector<int32_t> flags(B, 0);
    for (int b = 0; b < B; ++b) flags[b] = crop_anno_ok(&a, b) ? 0 : VERIFY_FLAG_INVALID;
    std::vector<uint8_t> uvw(3 * (size_t)Q), rgb(has_colors ? 3 * (size_t)Q : 0);
    for (int64_t g = 0; g < Q; ++g) {
        int b;
        int64_t at;
        const int raise = crop_export_pixel(&a, triangle.data(), occlusion ? owner.data() : nullptr, g, &uvw[3 * g], &b, &at);
        if (raise) flags[b] |= raise;
        if (has_colors)
            for (int k = 0; k < 3; ++k) rgb[3 * g + k] = b >= 0 ? crop_rgb_byte(colors[3 * g + (2 - k)]) : (uint8_t)0;
    }
    for (int64_t g = 0; g < Q; ++g) {
        const int b = verify_owner(qoff.data(), B, g);
        if (!(flags[b] & VERIFY_FLAG_INVALID)) continue;
        uvw[3 * g] = uvw[3 * g + 1] = uvw[3 * g + 2] = 0;
        if (has_colors) rgb[3 * g] = rgb[3 * g + 1] = rgb[3 * g + 2] = 0;
    }
    // counts
    std::vector<int32_t> counts(CROP_COUNTS * (size_t)B, 0);
    for (int b = 0; b < B; ++b) {
        const int32_t* w = &windows[4 * b];
        const int32_t* box = &boxes[4 * b];
        int32_t* o = &counts[CROP_COUNTS * b];
        const bool fits = verify_window_ok(w, &poff[b], P, W, H) && crop_box_ok(box, w, &qoff[b], Q);
        const int32_t word = flags[b] | (fits ? 0 : VERIFY_FLAG_INVALID);
        o[3] = word;
        if (word & VERIFY_FLAG_INVALID) continue;
        const int bw = box[2] - box[0], n = bw * (box[3] - box[1]);
        for (int i = 0; i < n; ++i) {
            const int x = box[0] + i % bw, y = box[1] + i / bw;
            const int64_t at = verify_window_pixel(w, poff[b], x, y);
            const bool c = mask[at] != 0;
            o[1] += c;
            o[2] += c && (!occlusion || owner[at] == b);
        }
        o[0] = n;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 4;
    wr(o, owner), wr(o, uvw), wr(o, rgb), wr(o, flags), wr(o, counts);
    fclose(o);
    return 0;
}
