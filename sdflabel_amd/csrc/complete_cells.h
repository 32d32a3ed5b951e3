// Per-element rules of shape completion from one view (complete.hip): what a row with an interval target [lo, hi] contributes to its shape's
// loss and latent gradient, and the rows one observed point gives -- the point, two points offset along its normal, and free-space points
// on its sensor ray (cpl_point_rows: THE per-point function, which align_cells.h's camera-frame rows go through too) --, and the row policy
// and row rule the kernels of encode_kernels.h take for such rows.  Plain functions and structs, compiled for the device by complete.hip
// and for the host by tests/complete_host/complete_host.cpp, which is compared with the numpy restatement (tests/_complete_ref.py) bit for
// bit.  Every operation rounds on its own (-ffp-contract=off).  DESIGN.md 7l has the rules.
#pragma once
#include <math.h>
#include <stdint.h>

#include "encode_cells.h"
#include "verify_cells.h"

#define CPL_MAX_FREE 64          // free-space slots per point (F)
#define CPL_ROW 5                // floats of a row: x y z lo hi
#define CPL_BAD_POSE 4           // view flags, bit 2: a non-finite pose or a scale <= 0; every slot of the shape is invalid
#define CPL_BAD_TABLE 8          //             bit 3: ptoff is broken at this shape; nothing is read through it

// What row (pred p, bounds lo <= hi) adds to its shape: the distance from clamp(p) to [clamp(lo), clamp(hi)] in float64, and the sign of
// the side it lies on where p is inside the clamp.  A row inside its interval adds nothing but counts (ok = 1).  ok needs a finite p,
// lo <= hi (false for a NaN) and one finite bound.  With lo == hi == t this is enc_row(p, t, clamp) in every bit.
ENC_HD EncRow cpl_row(float p, float lo, float hi, float clamp) {
    EncRow r;
    r.ok = (isfinite(p) && lo <= hi && (isfinite(lo) || isfinite(hi))) ? 1 : 0;
    r.e = 0.0;
    r.w = 0.f;
    if (r.ok) {
        const float cp = fminf(fmaxf(p, -clamp), clamp), cl = fminf(fmaxf(lo, -clamp), clamp), ch = fminf(fmaxf(hi, -clamp), clamp);
        const double d = cp < cl ? (double)cp - (double)cl : (cp > ch ? (double)cp - (double)ch : 0.0);
        r.e = fabs(d);
        const float sg = d > 0.0 ? 1.f : (d < 0.0 ? -1.f : 0.f);
        r.w = (p >= -clamp && p <= clamp) ? sg : 0.f;
    }
    return r;
}

// ptoff at shape b is usable: 0 <= ptoff[b] <= ptoff[b + 1] <= N
ENC_HD bool cpl_table_ok(const int64_t* ptoff, int b, int64_t N) {
    const int64_t a = ptoff[b], e = ptoff[b + 1];
    return a >= 0 && e >= a && e <= N;
}

// the pose row is usable: six finite words and a positive scale
ENC_HD bool cpl_pose_ok(const float* pose) {
    for (int i = 0; i < VERIFY_POSE; ++i)
        if (!isfinite(pose[i])) return false;
    return pose[5] > 0.f;
}

// the flag word of shape b
ENC_HD int32_t cpl_view_flags(const int64_t* ptoff, const float* pose, int b, int64_t N) {
    if (!cpl_table_ok(ptoff, b, N)) return CPL_BAD_TABLE;
    return cpl_pose_ok(pose + VERIFY_POSE * b) ? 0 : CPL_BAD_POSE;
}

// The shape that owns point g < N, or -1: the search of verify_owner over the table as it is, then the check that the entry found is
// usable and holds g.  Reads ptoff[0 .. B] only.
ENC_HD int cpl_owner(const int64_t* ptoff, int B, int64_t N, int64_t g) {
    if (B < 1) return -1;
    const int b = verify_owner(ptoff, B, g);
    return (cpl_table_ok(ptoff, b, N) && ptoff[b] <= g && g < ptoff[b + 1]) ? b : -1;
}

// u in [0, 1) of free-space slot f of point i of shape `shape` (shape0 + b): 53 bits of the library's hash
ENC_HD double cpl_u(uint64_t seed, int shape, int64_t i, int f) {
    const uint64_t key = (uint64_t)shape << 40 | (uint64_t)i << 8 | (uint64_t)f;
    const uint64_t h = train_mix64(seed ^ train_mix64(key * 0x9E3779B97F4A7C15ull + 1ull));
    return (double)(h >> 11) * 1.1102230246251565e-16;          // 2^-53
}

// one slot: the float64 position rounded once; valid only if the caller says so and the float32 position passes the store rule -- in
// [-1, 1]^3 with `cube` (the lattice frame), finite without (the camera frame has no cube)
ENC_HD void cpl_store(float* row, bool valid, bool cube, const double* x, float lo, float hi) {
    const float f0 = (float)x[0], f1 = (float)x[1], f2 = (float)x[2];
    const bool in = valid && (cube ? fabsf(f0) <= 1.0f && fabsf(f1) <= 1.0f && fabsf(f2) <= 1.0f            // (a NaN or an infinity is not)
                                   : isfinite(f0) && isfinite(f1) && isfinite(f2));
    const float nan = nanf("");
    row[0] = in ? f0 : 0.f;
    row[1] = in ? f1 : 0.f;
    row[2] = in ? f2 : 0.f;
    row[3] = in ? lo : nan;
    row[4] = in ? hi : nan;
}

// THE P = 3 + F rows of one observed point, written to out[P][5]: the point at x and the sensor at o, both in the frame the rows are in
// (float64 [3]); m: the normal in that frame, of any length (float64 [3]), or NULL.  usable = false: every slot is invalid and nothing of
// x, o or m is used.  In float64, in this order:  len = sqrt((m0 m0 + m1 m1) + m2 m2), n^ = m / len;  slot 1, 2 = x +- eta n^ with
// [+-eta, +-eta];  d = x - o, r = sqrt((d0 d0 + d1 d1) + d2 d2), d^ = d / r, reach = fmin(s_max, r), s = ((f + u) / F) reach,
// slot 3 + f = x - s d^ with [0, float32(s)].
ENC_HD void cpl_point_rows(bool usable, const double* x, const double* o, const double* m, bool cube, uint64_t seed, int shape, int64_t i, int F,
                           double eta, double s_max, float* out) {
    if (!usable) {
        const double zero3[3] = {0.0, 0.0, 0.0};
        for (int j = 0; j < 3 + F; ++j) cpl_store(out + CPL_ROW * j, false, cube, zero3, 0.f, 0.f);
        return;
    }
    cpl_store(out, true, cube, x, 0.f, 0.f);
    bool n_ok = false;
    double nh[3] = {0.0, 0.0, 0.0};
    if (m) {
        const double len = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
        n_ok = verify_finite(len) && len > 0.0;
        if (n_ok) nh[0] = m[0] / len, nh[1] = m[1] / len, nh[2] = m[2] / len;
    }
    const float fe = (float)eta;
    double y[3];
    for (int a = 0; a < 3; ++a) y[a] = x[a] + eta * nh[a];
    cpl_store(out + CPL_ROW, n_ok, cube, y, fe, fe);
    for (int a = 0; a < 3; ++a) y[a] = x[a] - eta * nh[a];
    cpl_store(out + 2 * CPL_ROW, n_ok, cube, y, -fe, -fe);
    // the ray from the sensor to the point
    const double dx = x[0] - o[0], dy = x[1] - o[1], dz = x[2] - o[2];
    const double r = sqrt((dx * dx + dy * dy) + dz * dz);
    const bool r_ok = verify_finite(r) && r > 0.0;
    const double d0 = r_ok ? dx / r : 0.0, d1 = r_ok ? dy / r : 0.0, d2 = r_ok ? dz / r : 0.0;
    const double reach = fmin(s_max, r);
    for (int f = 0; f < F; ++f) {
        const double u = cpl_u(seed, shape, i, f);
        const double s = (((double)f + u) / (double)F) * reach;
        y[0] = x[0] - s * d0, y[1] = x[1] - s * d1, y[2] = x[2] - s * d2;
        cpl_store(out + CPL_ROW * (3 + f), r_ok, cube, y, 0.f, (float)s);
    }
}

// The rows of one observed point p (camera frame) of a shape with pose row `pose`, in the lattice frame: cpl_point_rows of
// verify_point_x64 of p and of the sensor `origin`, the normal n (camera frame, float64 [3], or NULL) taken through
// diag(1, -1, 1) rot_yaw^T, and the cube rule.  usable: the shape's pose is (cpl_pose_ok) and the point has an owner -- otherwise nothing
// of p, n or pose is used.
ENC_HD void cpl_view_row(const float* p, const double* n, const float* pose, const float* origin, bool usable, uint64_t seed, int shape, int64_t i,
                         int F, double eta, double s_max, float* out) {
    double x[3] = {0.0, 0.0, 0.0}, o[3] = {0.0, 0.0, 0.0}, m[3] = {0.0, 0.0, 0.0};
    if (usable) {
        verify_point_x64(p, pose, x);
        verify_point_x64(origin, pose, o);
        if (n) {
            const double c = (double)pose[0], s = (double)pose[1];
            const double a0 = c * n[0], a1 = s * n[2], b0 = s * n[0], b1 = c * n[2];
            m[0] = a0 - a1, m[1] = -n[1], m[2] = b0 + b1;
        }
    }
    cpl_point_rows(usable, x, o, (usable && n) ? m : nullptr, true, seed, shape, i, F, eta, s_max, out);
}

// the two fits to interval rows share the rows kernel's policy for samples of x y z lo hi, and the row rule
typedef EncTargetRows<CPL_ROW> CplBoundRows;

struct CplBoundRule {
    const float *lo, *hi;
    ENC_HDM EncRow operator()(float p, int64_t i, int, float clamp) const { return cpl_row(p, lo[i], hi[i], clamp); }
};
