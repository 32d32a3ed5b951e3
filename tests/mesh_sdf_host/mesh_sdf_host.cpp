// Host harness of sdflabel_amd/csrc/mesh_sdf_cells.h: runs the per-triangle, per-point code for every query point and every triangle in the
// kernels' order (chunks of MSDF_CHUNK folded in chunk order; areas summed inside chunks of MSDF_AREA_CHUNK, then over the chunk totals) and
// writes what the kernels would write.  tests/test_mesh_sdf_cpu.py compares the output with the numpy restatement.
//   mesh_sdf_host IN OUT
//   IN : int32 B, want_sign; int64 V, T, N, S; int64 voff[B + 1], toff[B + 1], qoff[B + 1], soff[B + 1]; float32 vertices[V][3];
//        int32 faces[T][3]; float32 points[N][3]; float32 uniforms[S][3]
//   OUT: float32 sdf[N], dist[N]; float64 d2[N]; int32 nearest[N]; float64 winding[N]; int32 flags[B]; float32 spoints[S][3];
//        int32 striangle[S]; int32 sflags[B]
// Every buffer has exactly the size the kernels' caller would allocate, so a sanitizer build of this program checks the index arithmetic.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mesh_sdf_cells.h"

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
    int32_t h[2];
    int64_t sz[4];
    if (!f || fread(h, 4, 2, f) != 2 || fread(sz, 8, 4, f) != 4) return 3;
    const int B = h[0];
    const bool want_sign = h[1] != 0;
    const int64_t V = sz[0], T = sz[1], N = sz[2], S = sz[3];
    if (B < 0 || V < 0 || T < 0 || N < 0 || S < 0) return 3;
    std::vector<int64_t> voff, toff, qoff, soff;
    std::vector<float> vertices, points, uniforms;
    std::vector<int32_t> faces;
    if (!rd(f, voff, B + 1) || !rd(f, toff, B + 1) || !rd(f, qoff, B + 1) || !rd(f, soff, B + 1) || !rd(f, vertices, 3 * (size_t)V) ||
        !rd(f, faces, 3 * (size_t)T) || !rd(f, points, 3 * (size_t)N) || !rd(f, uniforms, 3 * (size_t)S))
        return 3;
    fclose(f);

    // ---- sdfr_mesh_sdf: defaults, flags, then every mesh with usable offsets and at least one triangle
    std::vector<float> sdf((size_t)N), dist((size_t)N);
    std::vector<double> d2((size_t)N), winding((size_t)N);
    std::vector<int32_t> nearest((size_t)N), flags(B, 0);
    for (int64_t i = 0; i < N; ++i) {
        MsdfRun r;
        msdf_run_init(&r);
        msdf_finish(&r, false, &sdf[i], &dist[i], &d2[i], &nearest[i], &winding[i]);
    }
    std::vector<double> tris;          // the mesh's triangles, nine doubles each, as the kernel stages them tile by tile
    std::vector<int> status;
    for (int b = 0; b < B; ++b) {
        if (!(msdf_run_ok(&voff[b], V) && msdf_run_ok(&toff[b], T))) {
            flags[b] = MSDF_FLAG_INVALID;
            continue;
        }
        const int64_t t0 = toff[b], nt = toff[b + 1] - t0, v0 = voff[b], nv = voff[b + 1] - v0;
        tris.assign(9 * (size_t)nt, 0.0);
        status.assign((size_t)nt, 0);
        for (int64_t t = 0; t < nt; ++t) {
            status[t] = msdf_tri_load(vertices.data() + 3 * v0, nv, &faces[3 * (t0 + t)], &tris[9 * t]);
            flags[b] |= status[t];
        }
        if (!msdf_run_ok(&qoff[b], N) || nt == 0) continue;
        for (int64_t q = qoff[b]; q < qoff[b + 1]; ++q) {
            const double p[3] = {(double)points[3 * q], (double)points[3 * q + 1], (double)points[3 * q + 2]};
            MsdfRun r;
            msdf_run_init(&r);
            if (verify_finite(p[0]) && verify_finite(p[1]) && verify_finite(p[2])) {
                for (int64_t c0 = 0; c0 < nt; c0 += MSDF_CHUNK) {
                    MsdfRun c;
                    msdf_run_init(&c);
                    for (int64_t t = c0; t < nt && t < c0 + MSDF_CHUNK; ++t)
                        if (status[t] == 0) msdf_run_tri(&c, p, &tris[9 * t], (int32_t)t, want_sign);
                    msdf_run_fold(&r, &c);
                }
            }
            msdf_finish(&r, want_sign, &sdf[q], &dist[q], &d2[q], &nearest[q], &winding[q]);
        }
    }

    // ---- sdfr_mesh_surface_points
    std::vector<float> spoints(3 * (size_t)S, 0.0f);
    std::vector<int32_t> striangle((size_t)S, -1), sflags(B, 0);
    std::vector<double> local((size_t)T, 0.0), base;
    std::vector<int64_t> coff(B + 1, 0);
    for (int b = 0; b < B; ++b) {
        const bool ok = msdf_run_ok(&voff[b], V) && msdf_run_ok(&toff[b], T);
        coff[b + 1] = coff[b] + (ok ? (toff[b + 1] - toff[b] + MSDF_AREA_CHUNK - 1) / MSDF_AREA_CHUNK : 0);
    }
    base.assign((size_t)coff[B], 0.0);
    for (int b = 0; b < B; ++b) {
        if (!(msdf_run_ok(&voff[b], V) && msdf_run_ok(&toff[b], T))) {
            sflags[b] = MSDF_FLAG_INVALID;
            continue;
        }
        const int64_t t0 = toff[b], nt = toff[b + 1] - t0, v0 = voff[b], nv = voff[b + 1] - v0;
        double s = 0.0;
        for (int64_t k = coff[b]; k < coff[b + 1]; ++k) {
            double l = 0.0;
            for (int64_t t = (k - coff[b]) * MSDF_AREA_CHUNK; t < nt && t < (k - coff[b] + 1) * MSDF_AREA_CHUNK; ++t) {
                double tri[9];
                const int st = msdf_tri_load(vertices.data() + 3 * v0, nv, &faces[3 * (t0 + t)], tri);
                sflags[b] |= st;
                l += st == 0 ? msdf_area(tri) : 0.0;
                local[t0 + t] = l;
            }
            base[k] = s;
            s += l;
        }
        if (!(s > 0.0)) sflags[b] |= MSDF_FLAG_INVALID;
    }
    for (int64_t s = 0; s < S; ++s) {
        const int b = verify_owner(soff.data(), B, s);
        if (!(msdf_run_ok(&voff[b], V) && msdf_run_ok(&toff[b], T))) continue;
        const int64_t t0 = toff[b], nt = toff[b + 1] - t0, v0 = voff[b], nv = voff[b + 1] - v0;
        const int64_t t = msdf_pick(local.data() + t0, base.data() + coff[b], nt, &uniforms[3 * s]);
        double tri[9];
        if (t >= 0 && msdf_tri_load(vertices.data() + 3 * v0, nv, &faces[3 * (t0 + t)], tri) == 0) {
            msdf_surface_point(tri, uniforms[3 * s + 1], uniforms[3 * s + 2], &spoints[3 * s]);
            striangle[s] = (int32_t)t;
        }
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 4;
    wr(o, sdf), wr(o, dist), wr(o, d2), wr(o, nearest), wr(o, winding), wr(o, flags), wr(o, spoints), wr(o, striangle), wr(o, sflags);
    fclose(o);
    return 0;
}
