// Per-triangle, per-point code of the signed distance to triangle meshes and of the surface sampler (mesh_sdf.hip).  DESIGN.md ("Signed
// distances to meshes") has the rules.  Everything here is a plain function of one triangle and one point, compiled for the device by
// mesh_sdf.hip and for the host by tests/mesh_sdf_host/mesh_sdf_host.cpp, which loops over every point and triangle in the kernels' order
// and is compared with the numpy restatement (tests/_mesh_sdf_ref.py) bit for bit.  Both translation units are compiled with
// -ffp-contract=off: every operation rounds separately.
//
// float32 vertices and points, float64 arithmetic.  A triangle is nine doubles a0 a1 a2 b0 b1 b2 c0 c1 c2.  THE COMPONENT ORDER:
//   dot(u, v)   = (u0 v0 + u1 v1) + u2 v2
//   cross(u, v) = (u1 v2 - u2 v1,  u2 v0 - u0 v2,  u0 v1 - u1 v0), both products rounded before the subtraction
//   seg(p, a, b): ab = b - a, ap = p - a, l2 = dot(ab, ab); t = l2 > 0 ? dot(ap, ab) / l2 : 0; t < 0 -> 0, t > 1 -> 1; d = ap - t ab (the
//                 product rounded first); result dot(d, d)
//   d2(p, tri)  : m = seg(p, a, b); s = seg(p, b, c), m = s if s < m; s = seg(p, c, a), m = s if s < m; then e1 = b - a, e2 = c - a,
//                 n = cross(e1, e2), nn = dot(n, n); if nn > 0 and dot(cross(e1, p - a), n) >= 0 and dot(cross(c - b, p - b), n) >= 0 and
//                 dot(cross(a - c, p - c), n) >= 0: h = dot(p - a, n), s = (h h) / nn, m = s if s < m
//   omega(p, tri): A = a - p, B = b - p, C = c - p; la = sqrt(dot(A, A)), lb, lc alike; det = dot(A, cross(B, C));
//                 den = (((la lb) lc + dot(A, B) lc) + dot(A, C) lb) + dot(B, C) la; det == 0 ? 0 : atan2(det, den) / (2 pi), 2 pi being the
//                 double 6.283185307179586
//   area(tri)   : sqrt(nn) / 2
//   surface point: s = sqrt(u1), w0 = 1 - s, w1 = s (1 - u2), w2 = s u2, x_k = (float)((w0 a_k + w1 b_k) + w2 c_k)
// Finite float32 inputs cannot overflow any of these in float64 (the largest intermediate, h h, stays below 1e240), so none of them is NaN.
#pragma once
#include <math.h>
#include <stdint.h>

#include "verify_cells.h"      // verify_finite, verify_owner

#if defined(__HIPCC__)
#define MSDF_HD __host__ __device__ inline
#else
#define MSDF_HD static inline
#endif

#define MSDF_FLAG_NONFINITE 1        // flag bit 0: a triangle with a non-finite vertex was skipped
#define MSDF_FLAG_INVALID 2          // flag bit 1: a face index outside the mesh, offsets that do not fit together, or (sampler) no area
#define MSDF_CHUNK 4096              // triangles per summation chunk of the winding number and of the nearest-triangle search
#define MSDF_TILE 256                // triangles staged per tile; divides MSDF_CHUNK
#define MSDF_AREA_CHUNK 256          // triangles per chunk of the cumulative area
#define MSDF_TWO_PI 6.283185307179586

MSDF_HD double msdf_dot(const double* u, const double* v) {
    const double m0 = u[0] * v[0], m1 = u[1] * v[1], m2 = u[2] * v[2];
    return (m0 + m1) + m2;
}

MSDF_HD void msdf_cross(const double* u, const double* v, double* o) {
    const double a0 = u[1] * v[2], b0 = u[2] * v[1];
    const double a1 = u[2] * v[0], b1 = u[0] * v[2];
    const double a2 = u[0] * v[1], b2 = u[1] * v[0];
    o[0] = a0 - b0, o[1] = a1 - b1, o[2] = a2 - b2;
}

MSDF_HD void msdf_sub(const double* u, const double* v, double* o) { o[0] = u[0] - v[0], o[1] = u[1] - v[1], o[2] = u[2] - v[2]; }

// The triangle of face f of a mesh of nv vertices starting at `verts`, as nine doubles.  Returns 0, or the flag bit of the reason it is
// skipped.  Nothing outside the mesh's vertices is read.
MSDF_HD int msdf_tri_load(const float* verts, int64_t nv, const int32_t* f, double* tri) {
    if (!(f[0] >= 0 && f[1] >= 0 && f[2] >= 0 && f[0] < nv && f[1] < nv && f[2] < nv)) return MSDF_FLAG_INVALID;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) tri[3 * i + k] = (double)verts[3 * (int64_t)f[i] + k];
    for (int i = 0; i < 9; ++i)
        if (!verify_finite(tri[i])) return MSDF_FLAG_NONFINITE;
    return 0;
}

MSDF_HD double msdf_seg(const double* p, const double* a, const double* b) {
    double ab[3], ap[3], d[3];
    msdf_sub(b, a, ab);
    msdf_sub(p, a, ap);
    const double l2 = msdf_dot(ab, ab);
    double t = l2 > 0.0 ? msdf_dot(ap, ab) / l2 : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    for (int k = 0; k < 3; ++k) {
        const double m = t * ab[k];
        d[k] = ap[k] - m;
    }
    return msdf_dot(d, d);
}

MSDF_HD double msdf_tri_d2(const double* p, const double* tri) {
    const double *a = tri, *b = tri + 3, *c = tri + 6;
    double m = msdf_seg(p, a, b);
    double s = msdf_seg(p, b, c);
    if (s < m) m = s;
    s = msdf_seg(p, c, a);
    if (s < m) m = s;
    double e1[3], e2[3], n[3], e[3], q[3], x[3];
    msdf_sub(b, a, e1);
    msdf_sub(c, a, e2);
    msdf_cross(e1, e2, n);
    const double nn = msdf_dot(n, n);
    if (!(nn > 0.0)) return m;
    double pa[3];
    msdf_sub(p, a, pa);
    msdf_cross(e1, pa, x);
    if (!(msdf_dot(x, n) >= 0.0)) return m;
    msdf_sub(c, b, e);
    msdf_sub(p, b, q);
    msdf_cross(e, q, x);
    if (!(msdf_dot(x, n) >= 0.0)) return m;
    msdf_sub(a, c, e);
    msdf_sub(p, c, q);
    msdf_cross(e, q, x);
    if (!(msdf_dot(x, n) >= 0.0)) return m;
    const double h = msdf_dot(pa, n);
    s = (h * h) / nn;
    if (s < m) m = s;
    return m;
}

MSDF_HD double msdf_omega(const double* p, const double* tri) {
    double A[3], B[3], C[3], x[3];
    msdf_sub(tri, p, A);
    msdf_sub(tri + 3, p, B);
    msdf_sub(tri + 6, p, C);
    const double la = sqrt(msdf_dot(A, A)), lb = sqrt(msdf_dot(B, B)), lc = sqrt(msdf_dot(C, C));
    msdf_cross(B, C, x);
    const double det = msdf_dot(A, x);
    const double t0 = (la * lb) * lc, t1 = msdf_dot(A, B) * lc, t2 = msdf_dot(A, C) * lb, t3 = msdf_dot(B, C) * la;
    const double den = ((t0 + t1) + t2) + t3;
    return det == 0.0 ? 0.0 : atan2(det, den) / MSDF_TWO_PI;
}

MSDF_HD double msdf_area(const double* tri) {
    double e1[3], e2[3], n[3];
    msdf_sub(tri + 3, tri, e1);
    msdf_sub(tri + 6, tri, e2);
    msdf_cross(e1, e2, n);
    return sqrt(msdf_dot(n, n)) / 2.0;
}

// The running values of one query point over one chunk of triangles, and over the chunks of a mesh.
struct MsdfRun {
    double d2;        // smallest squared distance so far (+inf: none)
    double sum;       // winding-number sum
    int32_t idx;      // its triangle (-1: none); the lowest index among equal distances
};

MSDF_HD void msdf_run_init(MsdfRun* r) { r->d2 = (double)INFINITY, r->sum = 0.0, r->idx = -1; }

// triangle `t` of the mesh, visited in index order
MSDF_HD void msdf_run_tri(MsdfRun* r, const double* p, const double* tri, int32_t t, bool want_sign) {
    const double d = msdf_tri_d2(p, tri);
    if (d < r->d2) r->d2 = d, r->idx = t;
    if (want_sign) r->sum += msdf_omega(p, tri);
}

// chunk result c folded into the mesh's result r, in chunk order
MSDF_HD void msdf_run_fold(MsdfRun* r, const MsdfRun* c) {
    if (c->d2 < r->d2) r->d2 = c->d2, r->idx = c->idx;
    r->sum += c->sum;
}

// the outputs of one query point from its folded result (every pointer but sdf may be NULL)
MSDF_HD void msdf_finish(const MsdfRun* r, bool want_sign, float* sdf, float* dist, double* d2, int32_t* nearest, double* winding) {
    const float df = (float)sqrt(r->d2);
    const bool inside = want_sign && fabs(r->sum) >= 0.5;
    *sdf = inside ? -df : df;
    if (dist) *dist = df;
    if (d2) *d2 = r->d2;
    if (nearest) *nearest = r->idx;
    if (winding) *winding = want_sign ? r->sum : 0.0;
}

// offsets off[b], off[b + 1] describe a run inside an array of n elements
MSDF_HD bool msdf_run_ok(const int64_t* off, int64_t n) { return off[0] >= 0 && off[1] >= off[0] && off[1] <= n; }

// ---- surface sampler ---------------------------------------------------------------------------------------------------------------------

// cum[t] of a mesh whose first triangle is local[0] / base[0]
MSDF_HD double msdf_cum(const double* local, const double* base, int64_t t) { return base[t / MSDF_AREA_CHUNK] + local[t]; }

// the first t in [0, nt) with cum[t] > target, or -1 (no such triangle: no area, or a uniform outside [0, 1))
MSDF_HD int64_t msdf_pick(const double* local, const double* base, int64_t nt, const float* u) {
    if (nt <= 0 || !(u[0] >= 0.0f && u[0] < 1.0f && u[1] >= 0.0f && u[1] < 1.0f && u[2] >= 0.0f && u[2] < 1.0f)) return -1;
    const double target = (double)u[0] * msdf_cum(local, base, nt - 1);
    if (!(msdf_cum(local, base, nt - 1) > target)) return -1;
    int64_t lo = -1, hi = nt - 1;                    // cum[lo] <= target < cum[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (msdf_cum(local, base, mid) > target) hi = mid; else lo = mid;
    }
    return hi;
}

MSDF_HD void msdf_surface_point(const double* tri, float u1, float u2, float* x) {
    const double s = sqrt((double)u1);
    const double w0 = 1.0 - s, r = 1.0 - (double)u2;
    const double w1 = s * r, w2 = s * (double)u2;
    for (int k = 0; k < 3; ++k) {
        const double m0 = w0 * tri[k], m1 = w1 * tri[3 + k], m2 = w2 * tri[6 + k];
        x[k] = (float)((m0 + m1) + m2);
    }
}
