// Host harness of sdflabel_amd/csrc/verify_cells.h: runs the per-triangle, per-pixel and per-point code for every triangle of every mesh,
// every pixel of its clamped box and every point, with the atomic minimum and the sums done sequentially, and writes what the kernels would
// write.  tests/test_verify_cpu.py compares the output with the numpy restatement.
//   verify_host IN OUT
//   IN : int32 B, W, H, NA, L; float32 z_min, band; float64 K[4]; int64 voff[B + 1], toff[B + 1]; int32 windows[B][4]; int64 ptoff[NA + 1];
//        float32 vertices[V][3]; int32 faces[T][3]; float32 pose[NA][6], latents[NA][L], points[N][3], sdf[N]
//   OUT: uint8 mask[P]; float32 depth[P]; int32 triangle[P]; int32 flags[B]; int32 counts[B][8]; float32 rows[N][L + 3]; uint8 in_cube[N];
//        int32 band[NA][3]
// Every buffer has exactly the size the kernels' caller would allocate, so a sanitizer build of this program checks the index arithmetic.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "verify_cells.h"

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
    int32_t h[5];
    float zb[2];
    double K[4];
    if (!f || fread(h, 4, 5, f) != 5 || fread(zb, 4, 2, f) != 2 || fread(K, 8, 4, f) != 4) return 3;
    const int B = h[0], W = h[1], H = h[2], NA = h[3], L = h[4];
    if (B < 0 || W < 1 || H < 1 || NA < 0 || L < 0) return 3;
    std::vector<int64_t> voff, toff, ptoff;
    std::vector<int32_t> windows, faces;
    std::vector<float> vertices, pose, latents, points, sdf;
    if (!rd(f, voff, B + 1) || !rd(f, toff, B + 1) || !rd(f, windows, 4 * (size_t)B) || !rd(f, ptoff, NA + 1)) return 3;
    const int64_t V = voff[B], T = toff[B], N = ptoff[NA];
    if (voff[0] != 0 || toff[0] != 0 || ptoff[0] != 0 || V < 0 || T < 0 || N < 0) return 3;
    if (!rd(f, vertices, 3 * (size_t)V) || !rd(f, faces, 3 * (size_t)T) || !rd(f, pose, VERIFY_POSE * (size_t)NA) ||
        !rd(f, latents, (size_t)NA * L) || !rd(f, points, 3 * (size_t)N) || !rd(f, sdf, (size_t)N))
        return 3;
    fclose(f);
    std::vector<int64_t> poff(B + 1, 0);
    for (int b = 0; b < B; ++b) {
        const int32_t* w = &windows[4 * b];
        poff[b + 1] = poff[b] + (int64_t)(w[2] - w[0]) * (w[3] - w[1]);
        if (voff[b + 1] < voff[b] || toff[b + 1] < toff[b] || poff[b + 1] < poff[b]) return 3;
    }
    const int64_t P = poff[B];
    // raster: keys by a sequential minimum
    std::vector<uint64_t> keys((size_t)P, VERIFY_NO_KEY);
    std::vector<int32_t> flags(B, 0);
    for (int64_t g = 0; g < T; ++g) {
        const int b = verify_owner(toff.data(), B, g);
        const int64_t v0 = voff[b], nv = voff[b + 1] - v0;
        const int32_t* w = &windows[4 * b];
        const int32_t* fc = &faces[3 * g];
        if (!verify_face_ok(fc, nv) || !verify_window_ok(w, &poff[b], P, W, H)) {       // as verify_load_tri of verify.hip
            flags[b] |= VERIFY_FLAG_INVALID;
            continue;
        }
        VerifyTri tri;
        const int st = verify_tri_setup(&vertices[3 * (v0 + fc[0])], &vertices[3 * (v0 + fc[1])], &vertices[3 * (v0 + fc[2])], K, zb[0], w[0], w[1],
                                        w[2], w[3], &tri);
        if (st == VERIFY_TRI_BEHIND) flags[b] |= VERIFY_FLAG_BEHIND;
        if (st != VERIFY_TRI_OK) continue;
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
    // mask counts
    std::vector<int32_t> counts(8 * (size_t)B, 0);
    for (int b = 0; b < B; ++b) {
        const int32_t* w = &windows[4 * b];
        int32_t* o = &counts[8 * b];
        if (!verify_window_ok(w, &poff[b], P, W, H)) {
            o[7] = VERIFY_FLAG_INVALID;
            continue;
        }
        const int ww = w[2] - w[0], n = ww * (w[3] - w[1]);
        int area = 0, x0 = INT32_MAX, y0 = INT32_MAX, x1 = -1, y1 = -1;
        for (int i = 0; i < n; ++i)
            if (mask[poff[b] + i]) {
                const int x = w[0] + i % ww, y = w[1] + i / ww;
                ++area;
                x0 = x < x0 ? x : x0, x1 = x > x1 ? x : x1, y0 = y < y0 ? y : y0, y1 = y > y1 ? y : y1;
            }
        o[0] = area;
        if (area) o[1] = x0, o[2] = y0, o[3] = x1 + 1, o[4] = y1 + 1;
    }
    // point rows and band counts
    const int NI = L + 3;
    std::vector<float> rows((size_t)N * NI);
    std::vector<uint8_t> in_cube((size_t)N);
    std::vector<int32_t> band(3 * (size_t)NA, 0);
    for (int64_t g = 0; g < N; ++g) {
        const int a = verify_owner(ptoff.data(), NA, g);
        for (int c = 0; c < L; ++c) rows[g * NI + c] = latents[(size_t)a * L + c];
        in_cube[g] = verify_point_x(&points[3 * g], &pose[VERIFY_POSE * a], &rows[g * NI + L]);
        band[3 * a] += 1;
        band[3 * a + 1] += in_cube[g] != 0;
        band[3 * a + 2] += verify_in_band(sdf[g], in_cube[g], pose[VERIFY_POSE * a + 5], zb[1]);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 4;
    wr(o, mask), wr(o, depth), wr(o, triangle), wr(o, flags), wr(o, counts), wr(o, rows), wr(o, in_cube), wr(o, band);
    fclose(o);
    return 0;
}
