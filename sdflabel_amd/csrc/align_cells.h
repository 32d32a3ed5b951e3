// Per-element rules of the pose-and-shape fit to one view (align.hip): the camera-frame observation rows one point gives, what a drawn row
// becomes under the iteration's pose, what a row adds to its shape's loss and to the gradient with respect to the latent AND the pose
// (yaw, trans, scale), and the update of the pose.  Plain functions, compiled for the device by align.hip and for the host by
// tests/align_host/align_host.cpp, which is compared with the numpy restatement (tests/_align_ref.py) bit for bit.  Every operation rounds
// on its own (-ffp-contract=off).  DESIGN.md 7m has the rules.
#pragma once
#include <math.h>
#include <stdint.h>

#include "complete_cells.h"

#define ALN_ROW 5                // floats of an observation row: qx qy qz (camera frame, metres) lo hi (metric signed distance)
#define ALN_POSE 5               // pose parameters theta = yaw, tx, ty, tz, scale; gradient columns L .. L + 4
#define ALN_BAD_POSE 16          // flags, bit 4: pose[b] fails cpl_pose_ok; every row of the shape is invalid.  (complete_cells.h's
                                 // CPL_BAD_POSE is 4, which in an iteration's flag word is ENC_SKIPPED; the fit keeps the two apart.)

// one observation slot: the float64 position rounded once; valid only if the caller says so and the float32 position is finite.  There is
// no cube in the camera frame.
ENC_HD void aln_store(float* row, bool valid, const double* q, float lo, float hi) {
    const float f0 = (float)q[0], f1 = (float)q[1], f2 = (float)q[2];
    const bool in = valid && isfinite(f0) && isfinite(f1) && isfinite(f2);
    const float nan = nanf("");
    row[0] = in ? f0 : 0.f;
    row[1] = in ? f1 : 0.f;
    row[2] = in ? f2 : 0.f;
    row[3] = in ? lo : nan;
    row[4] = in ? hi : nan;
}

// The P = 3 + F rows of one observed point p (camera frame, metres), written to out[P][5].  n: the camera-frame normal (float64 [3]) or
// NULL; origin: the sensor (camera frame); usable: the point has an owner -- otherwise every slot is invalid and nothing of p or n is used.
// In float64, in this order:  len = sqrt((n0 n0 + n1 n1) + n2 n2), n^ = n / len;  slot 1, 2 = p +- eta n^;  d = p - o,
// r = sqrt((d0 d0 + d1 d1) + d2 d2), d^ = d / r, reach = fmin(s_max, r), s = ((f + u) / F) reach, slot 3 + f = p - s d^ with [0, float32(s)].
ENC_HD void aln_sample_row(const float* p, const double* n, const float* origin, bool usable, uint64_t seed, int shape, int64_t i, int F, double eta,
                           double s_max, float* out) {
    const double zero3[3] = {0.0, 0.0, 0.0};
    const bool p_ok = usable && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    if (!p_ok) {
        for (int j = 0; j < 3 + F; ++j) aln_store(out + ALN_ROW * j, false, zero3, 0.f, 0.f);
        return;
    }
    const double x[3] = {(double)p[0], (double)p[1], (double)p[2]};
    aln_store(out, true, x, 0.f, 0.f);
    bool n_ok = false;
    double nh[3] = {0.0, 0.0, 0.0};
    if (n) {
        const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        n_ok = verify_finite(len) && len > 0.0;
        if (n_ok) nh[0] = n[0] / len, nh[1] = n[1] / len, nh[2] = n[2] / len;
    }
    const float fe = (float)eta;
    double y[3];
    for (int a = 0; a < 3; ++a) y[a] = x[a] + eta * nh[a];
    aln_store(out + ALN_ROW, n_ok, y, fe, fe);
    for (int a = 0; a < 3; ++a) y[a] = x[a] - eta * nh[a];
    aln_store(out + 2 * ALN_ROW, n_ok, y, -fe, -fe);
    const double dx = x[0] - (double)origin[0], dy = x[1] - (double)origin[1], dz = x[2] - (double)origin[2];
    const double r = sqrt((dx * dx + dy * dy) + dz * dz);
    const bool r_ok = verify_finite(r) && r > 0.0;
    const double d0 = r_ok ? dx / r : 0.0, d1 = r_ok ? dy / r : 0.0, d2 = r_ok ? dz / r : 0.0;
    const double reach = fmin(s_max, r);
    for (int f = 0; f < F; ++f) {
        const double u = cpl_u(seed, shape, i, f);
        const double s = (((double)f + u) / (double)F) * reach;
        y[0] = x[0] - s * d0, y[1] = x[1] - s * d1, y[2] = x[2] - s * d2;
        aln_store(out + ALN_ROW * (3 + f), r_ok, y, 0.f, (float)s);
    }
}

// The drawn observation (q, lo, hi) under the iteration's pose: x = float32(verify_point_x64(q, pose)).  A row whose x leaves [-1, 1]^3,
// or whose shape's pose is not usable, gets x = 0 and NaN bounds for this iteration.
ENC_HD void aln_row(const float* q, const float* pose, bool pose_ok, float* x, float* lo, float* hi) {
    uint8_t in = 0;
    if (pose_ok) in = verify_point_x(q, pose, x);
    if (!in) {
        x[0] = x[1] = x[2] = 0.f;
        *lo = *hi = nanf("");
    }
}

// the flag word sdfr_align_rows stores for a shape with `count` samples (-1: a broken table entry); `bad` includes draw = 0 with k > count
ENC_HD int32_t aln_rows_flags(bool bad, int64_t count, bool pose_ok) {
    return bad ? ENC_BAD_TABLE : (count == 0 ? ENC_EMPTY : (pose_ok ? 0 : ALN_BAD_POSE));
}

// the metric prediction the row rule sees: scale p, one float32 rounding
ENC_HD float aln_metric(float p, const float* pose) { return pose[5] * p; }

// d pm / d (column c) in float64 for a row with decoder value p, Jacobian row jrow (latent columns 0 .. L - 1, then gx gy gz), camera-frame
// point q and pose row pose = c, sn, t, scale.  x is verify_point_x64(q, pose).  Columns: c < L zn_c; L yaw; L + 1 .. L + 3 trans; L + 4 scale.
//   zn_i   sc * J[i]
//   yaw    sc * (gz * x0 - gx * x2)
//   tx     -(sc * (gx * c + gz * sn))
//   ty     sc * gy
//   tz     sc * (gx * sn - gz * c)
//   scale  p + sc * ((gx * (c * u0 - sn * u2) - gy * u1) + gz * (sn * u0 + c * u2)),  u_a = -(q_a / (sc * sc))
// every product, sum and quotient as written, left to right, one rounding each.
ENC_HD double aln_dpm(int col, int L, float p, const float* jrow, const float* q, const float* pose) {
    const double sc = (double)pose[5];
    if (col < L) return sc * (double)jrow[col];
    const double c = (double)pose[0], sn = (double)pose[1];
    const double gx = (double)jrow[L], gy = (double)jrow[L + 1], gz = (double)jrow[L + 2];
    switch (col - L) {
        case 0: {
            double x[3];
            verify_point_x64(q, pose, x);
            const double a = gz * x[0], b = gx * x[2];
            return sc * (a - b);
        }
        case 1: {
            const double a = gx * c, b = gz * sn;
            return -(sc * (a + b));
        }
        case 2: return sc * gy;
        case 3: {
            const double a = gx * sn, b = gz * c;
            return sc * (a - b);
        }
        default: {
            const double s2 = sc * sc;
            const double u0 = -((double)q[0] / s2), u1 = -((double)q[1] / s2), u2 = -((double)q[2] / s2);
            const double a0 = c * u0, a1 = sn * u2, b0 = sn * u0, b1 = c * u2;
            const double t0 = gx * (a0 - a1), t1 = gy * u1, t2 = gz * (b0 + b1);
            return (double)p + sc * ((t0 - t1) + t2);
        }
    }
}

// Column c of the L + 7 a chunk sums: c < L + 5 the gradient column (w d pm / d column, and nothing -- not 0 x inf -- where w is 0),
// c == L + 5 the loss, c == L + 6 the count of ok rows
ENC_HD double aln_value(int c, int L, float w, double e, int ok, float p, const float* jrow, const float* q, const float* pose) {
    const int G = L + ALN_POSE;
    if (c < G) return w != 0.f ? (double)w * aln_dpm(c, L, p, jrow, q, pose) : 0.0;
    return c == G ? e : (ok ? 1.0 : 0.0);
}

// the pose row of theta = yaw, tx, ty, tz, scale: cos and sin in double of the float32 yaw, rounded once
ENC_HD void aln_pose_row(const float* theta, float* pose) {
    pose[0] = (float)cos((double)theta[0]);
    pose[1] = (float)sin((double)theta[0]);
    pose[2] = theta[1];
    pose[3] = theta[2];
    pose[4] = theta[3];
    pose[5] = theta[4];
}

// float32(g[L .. L + 4]) are all finite
ENC_HD bool aln_pose_grad_ok(const double* g, int L) {
    for (int i = 0; i < ALN_POSE; ++i)
        if (!isfinite((float)g[L + i])) return false;
    return true;
}

// the scale one Adam update would leave (the state is not touched); lr == 0: the scale as it is
ENC_HD float aln_scale_after(const float* theta, const float* tm, const float* tv, const double* g, int L, float lr, float bc1, float bc2) {
    float s = theta[4], m = tm[4], v = tv[4];
    if (lr != 0.f) latent_adam(&s, &m, &v, (float)g[L + 4], lr, bc1, bc2);
    return s;
}

// latent_adam on every pose parameter whose rate is not 0 (a rate of 0 leaves the parameter and its state untouched), then the next pose row
ENC_HD void aln_pose_step(float* theta, float* tm, float* tv, const double* g, int L, const float* lr, float bc1, float bc2, float* pose) {
    for (int i = 0; i < ALN_POSE; ++i)
        if (lr[i] != 0.f) latent_adam(&theta[i], &tm[i], &tv[i], (float)g[L + i], lr[i], bc1, bc2);
    aln_pose_row(theta, pose);
}
