// Per-triangle, per-pixel and per-point code of the autolabel verification (verify.hip).  DESIGN.md ("Verification") has the rules.
// Everything here is a plain function of one triangle, one pixel or one point, compiled for the device by verify.hip and for the host by
// tests/verify_host/verify_host.cpp, which loops over every triangle, pixel and point and is compared with the numpy restatement
// (tests/_verify_ref.py) bit for bit.  Both translation units are compiled with -ffp-contract=off: every operation rounds separately.
// It is also the header of everything that reads the packed rasters: crop_cells.h (crops.hip, tests/export_host/export_host.cpp) includes it
// for RasterArgs, the window and face predicates, the window-pixel index, the edge functions and the workgroup reduction.
//
// Rasteriser: float32 camera-frame vertices, float64 arithmetic.  u = fx (X / Z) + cx, v = fy (Y / Z) + cy; pixel (x, y) is sampled at the
// point (x, y); edges are inclusive, both windings count; the winner of a pixel is the minimum of (bits(depth) << 32) | triangle index.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define VERIFY_HD __host__ __device__ inline
#else
#define VERIFY_HD static inline
#endif

#define VERIFY_NO_KEY 0xffffffffffffffffull      // key of a pixel no triangle covers
#define VERIFY_FLAG_BEHIND 1                     // flag bit 0: a triangle with a vertex at Z <= z_min was skipped
#define VERIFY_FLAG_INVALID 2                    // flag bit 1: a face index outside the mesh, or a window / offsets that do not fit together
#define VERIFY_TRI_OK 0
#define VERIFY_TRI_SKIP 1                        // skipped silently: non-finite vertex or projection, zero area, box outside the window
#define VERIFY_TRI_BEHIND 2                      // skipped, flag bit 0

struct VerifyTri {
    double u[3], v[3], z[3];      // projections and depths of the three vertices
    double sgn;                   // sign(A2): +1 or -1
    int x0, y0, x1, y1;           // INCLUSIVE pixel box, already inside the window
};

VERIFY_HD bool verify_finite(double a) { return fabs(a) <= 1.7976931348623157e308; }          // false for NaN and the infinities

VERIFY_HD double verify_project(double f, double c, float X, float Z) {
    const double q = (double)X / (double)Z;
    const double m = f * q;
    return m + c;
}

// Set up one triangle for the window [l, r) x [t, b) (0 <= l <= r, 0 <= t <= b; the caller checked that).  K = fx, fy, cx, cy.
// The pixel box is clamped to the window IN FLOATING POINT, then converted: no vertex value gives a box outside the window.
VERIFY_HD int verify_tri_setup(const float* p0, const float* p1, const float* p2, const double* K, float z_min, int l, int t, int r, int b,
                               VerifyTri* T) {
    const float* p[3] = {p0, p1, p2};
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k)
            if (!verify_finite((double)p[i][k])) return VERIFY_TRI_SKIP;
    for (int i = 0; i < 3; ++i)
        if (p[i][2] <= z_min) return VERIFY_TRI_BEHIND;
    for (int i = 0; i < 3; ++i) {
        T->u[i] = verify_project(K[0], K[2], p[i][0], p[i][2]);
        T->v[i] = verify_project(K[1], K[3], p[i][1], p[i][2]);
        T->z[i] = (double)p[i][2];
        if (!verify_finite(T->u[i]) || !verify_finite(T->v[i])) return VERIFY_TRI_SKIP;
    }
    const double a = (T->u[1] - T->u[0]) * (T->v[2] - T->v[0]);
    const double c = (T->v[1] - T->v[0]) * (T->u[2] - T->u[0]);
    const double A2 = a - c;
    if (!(A2 != 0.0) || !verify_finite(A2)) return VERIFY_TRI_SKIP;
    T->sgn = A2 > 0.0 ? 1.0 : -1.0;
    if (r <= l || b <= t) return VERIFY_TRI_SKIP;
    double ulo = fmin(fmin(T->u[0], T->u[1]), T->u[2]), uhi = fmax(fmax(T->u[0], T->u[1]), T->u[2]);
    double vlo = fmin(fmin(T->v[0], T->v[1]), T->v[2]), vhi = fmax(fmax(T->v[0], T->v[1]), T->v[2]);
    ulo = ceil(ulo), uhi = floor(uhi), vlo = ceil(vlo), vhi = floor(vhi);
    if (ulo < (double)l) ulo = (double)l;
    if (uhi > (double)(r - 1)) uhi = (double)(r - 1);
    if (vlo < (double)t) vlo = (double)t;
    if (vhi > (double)(b - 1)) vhi = (double)(b - 1);
    if (!(ulo <= uhi && vlo <= vhi)) return VERIFY_TRI_SKIP;
    T->x0 = (int)ulo, T->x1 = (int)uhi, T->y0 = (int)vlo, T->y1 = (int)vhi;        // all four inside [l, r - 1] x [t, b - 1]
    return VERIFY_TRI_OK;
}

// The edge functions of pixel (x, y): E[i] belongs to the edge (a, b) opposite vertex i, every product rounded on its own.  The rasteriser's
// cover test and depth and the export's interpolation (crop_cells.h) both start from these values.
VERIFY_HD void verify_edges(const VerifyTri* T, int x, int y, double* E) {
    const double px = (double)x, py = (double)y;
    double du[3], dv[3];
    for (int i = 0; i < 3; ++i) du[i] = T->u[i] - px, dv[i] = T->v[i] - py;
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        const double m0 = du[a] * dv[b], m1 = dv[a] * du[b];
        E[i] = m0 - m1;
    }
}

// The triangle's key at pixel (x, y), or VERIFY_NO_KEY where it does not cover the pixel or its depth there is not a positive finite float.
VERIFY_HD uint64_t verify_pixel_key(const VerifyTri* T, int x, int y, uint32_t tri) {
    double E[3];
    verify_edges(T, x, y, E);
    for (int i = 0; i < 3; ++i)
        if (!(E[i] * T->sgn >= 0.0)) return VERIFY_NO_KEY;
    const double S = (E[0] + E[1]) + E[2];
    const double q0 = E[0] / T->z[0], q1 = E[1] / T->z[1], q2 = E[2] / T->z[2];
    const double D = (q0 + q1) + q2;
    const float depth = (float)(S / D);
    if (!(depth > 0.0f) || !(depth <= 3.4028234663852886e38f)) return VERIFY_NO_KEY;
    uint32_t bits;
    memcpy(&bits, &depth, 4);
    return (uint64_t)bits << 32 | (uint64_t)tri;
}

VERIFY_HD void verify_resolve(uint64_t key, uint8_t* mask, float* depth, int32_t* tri) {
    if (key == VERIFY_NO_KEY) {
        *mask = 0, *depth = 0.0f, *tri = -1;
        return;
    }
    const uint32_t bits = (uint32_t)(key >> 32);
    *mask = 1;
    memcpy(depth, &bits, 4);
    *tri = (int32_t)(uint32_t)(key & 0xffffffffull);
}

// A camera-frame point in the lattice frame of an annotation: x = diag(1, -1, 1) rot_yaw^T (p / scale - trans) in float64, rounded once.
// pose = cos(yaw), sin(yaw), trans x, y, z, scale (float32; the cosine and sine are the label's own float32 values).  Returns 1 when x lies
// in [-1, 1]^3 (a NaN does not).
#define VERIFY_POSE 6
// the float64 part of verify_point_x: x before its one rounding (complete_cells.h offsets it along normals and rays first)
VERIFY_HD void verify_point_x64(const float* p, const float* pose, double* x) {
    const double c = (double)pose[0], s = (double)pose[1], sc = (double)pose[5];
    const double q0 = (double)p[0] / sc - (double)pose[2];
    const double q1 = (double)p[1] / sc - (double)pose[3];
    const double q2 = (double)p[2] / sc - (double)pose[4];
    const double a0 = c * q0, a1 = s * q2, b0 = s * q0, b1 = c * q2;
    x[0] = a0 - a1;
    x[1] = -q1;
    x[2] = b0 + b1;
}

VERIFY_HD uint8_t verify_point_x(const float* p, const float* pose, float* x) {
    double d[3];
    verify_point_x64(p, pose, d);
    x[0] = (float)d[0];
    x[1] = (float)d[1];
    x[2] = (float)d[2];
    return (uint8_t)(fabsf(x[0]) <= 1.0f && fabsf(x[1]) <= 1.0f && fabsf(x[2]) <= 1.0f);
}

// in the band: inside the cube and |sdf| scale < band, compared in float32 (a NaN value is outside)
VERIFY_HD bool verify_in_band(float sdf, uint8_t in_cube, float scale, float band) {
    const float d = fabsf(sdf) * scale;
    return in_cube != 0 && d < band;
}

// largest i in [0, n) with off[i] <= g, for non-decreasing off[0 .. n] with off[0] <= g < off[n]: the owner of element g of a ragged batch
VERIFY_HD int verify_owner(const int64_t* off, int n, int64_t g) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) / 2;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// Everything the rasteriser and the kernels that read its packed output need to know about one ragged batch; all pointers as the entry
// points take them (NULL / 0 for what a kernel does not read).
struct RasterArgs {
    const float* vertices;       // [V][3] camera frame
    const int32_t* faces;        // [T][3], indices local to the mesh
    const int64_t* voff;         // [B + 1]
    const int64_t* toff;         // [B + 1]
    const int32_t* windows;      // [B][4] l, t, r, b
    const int64_t* poff;         // [B + 1]
    int B, W, H;
    int64_t V, T, P;
    double K[4];
    float z_min;
};

static inline RasterArgs raster_args(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const int64_t* voff, const int64_t* toff,
                                     const int32_t* windows, const int64_t* poff, int64_t P, int B, int W, int H, const double* K, float z_min) {
    RasterArgs a = {vertices, faces, voff, toff, windows, poff, B, W, H, V, T, P, {0, 0, 0, 0}, z_min};
    if (K)
        for (int i = 0; i < 4; ++i) a.K[i] = K[i];
    return a;
}

// the window [l, t, r, b) lies inside the W x H image and its pixels are exactly off[0] .. off[1] of an array of P
VERIFY_HD bool verify_window_ok(const int32_t* w, const int64_t* off, int64_t P, int W, int H) {
    const int l = w[0], t = w[1], r = w[2], b = w[3];
    if (!(0 <= l && l <= r && r <= W && 0 <= t && t <= b && b <= H)) return false;
    const int64_t p0 = off[0], p1 = off[1];
    return p0 >= 0 && p1 <= P && p1 - p0 == (int64_t)(r - l) * (b - t);
}

// the three vertex indices of a face lie inside a mesh of nv vertices
VERIFY_HD bool verify_face_ok(const int32_t* f, int64_t nv) { return f[0] >= 0 && f[1] >= 0 && f[2] >= 0 && f[0] < nv && f[1] < nv && f[2] < nv; }

// index into the packed rasters of image pixel (x, y) of the window w whose pixels start at poff_b; inside poff[b] .. poff[b + 1] for a
// pixel inside a window that passed verify_window_ok
VERIFY_HD int64_t verify_window_pixel(const int32_t* w, int64_t poff_b, int x, int y) { return poff_b + (int64_t)(y - w[1]) * (w[2] - w[0]) + (x - w[0]); }

#if defined(__HIPCC__)
#define VERIFY_BLOCK 256         // threads per workgroup of every kernel of verify.hip and crops.hip

// sum (OP 0), minimum (1) or maximum (2) of one int per thread over the workgroup, in a fixed tree; the result is valid in every thread
template <int OP>
__device__ __forceinline__ int verify_block_reduce(int v, int* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int o = VERIFY_BLOCK / 2; o > 0; o >>= 1) {
        if (t < o) {
            const int x = sh[t], y = sh[t + o];
            sh[t] = OP == 0 ? x + y : OP == 1 ? (x < y ? x : y) : (x > y ? x : y);
        }
        __syncthreads();
    }
    return sh[0];
}
#endif
