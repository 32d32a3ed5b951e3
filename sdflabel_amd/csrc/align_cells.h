// Per-element rules of the pose-and-shape fit to one view (align.hip): the camera-frame observation rows one point gives, what a drawn row
// becomes under the iteration's pose, what a row adds to its shape's loss and to the gradient with respect to the latent AND the pose
// (yaw, trans, scale), and the update of the pose -- and the policy structs (AlnPosedRows, AlnRowRule, AlnCols, AlnPoseStep) through which
// the kernels of encode_kernels.h see them.  Plain functions and structs, compiled for the device by align.hip and for the host by
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

// The P = 3 + F rows of one observed point p (camera frame, metres), written to out[P][5]: cpl_point_rows of p, the sensor `origin` and the
// normal n (float64 [3], or NULL) as they are, and the finite rule -- there is no cube in the camera frame.  usable: the point has an
// owner; a point that is not finite gives invalid slots too.
ENC_HD void aln_sample_row(const float* p, const double* n, const float* origin, bool usable, uint64_t seed, int shape, int64_t i, int F, double eta,
                           double s_max, float* out) {
    const bool p_ok = usable && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
    double x[3] = {0.0, 0.0, 0.0}, o[3] = {0.0, 0.0, 0.0};
    if (p_ok)
        for (int a = 0; a < 3; ++a) x[a] = (double)p[a], o[a] = (double)origin[a];
    cpl_point_rows(p_ok, x, o, p_ok ? n : nullptr, false, seed, shape, i, F, eta, s_max, out);
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

// The rows kernel's policy (encode_cells.h) for observation rows under pose[b]: the side arrays are the camera-frame point, lo and hi
// (aln_row), and the workgroup keeps the lattice position itself until the decoder's inputs are written.
struct AlnPosedRows {
    static constexpr int W = ALN_ROW;
    struct Shape {
        float ps[VERIFY_POSE];
        bool ok;
    };
    struct Staged {
        float x[3];
    };
    const float* pose;
    float *cam, *lo, *hi;
    ENC_HDM Shape shape(int b) const {
        Shape s;
        for (int a = 0; a < VERIFY_POSE; ++a) s.ps[a] = pose[VERIFY_POSE * b + a];
        s.ok = cpl_pose_ok(s.ps);
        return s;
    }
    ENC_HDM int32_t flags(const Shape& s, bool bad, int64_t count) const { return aln_rows_flags(bad, count, s.ok); }
    ENC_HDM Staged stage(const Shape& s, const float* samples, int64_t src, int64_t i) const {
        float q[3] = {0.f, 0.f, 0.f}, l = 0.f, h = 0.f;
        Staged st = {{0.f, 0.f, 0.f}};
        if (src >= 0) {
            const float* row = samples + src * W;
            q[0] = row[0], q[1] = row[1], q[2] = row[2], l = row[3], h = row[4];
            aln_row(q, s.ps, s.ok, st.x, &l, &h);
        }
        cam[3 * i] = q[0], cam[3 * i + 1] = q[1], cam[3 * i + 2] = q[2];
        lo[i] = l, hi[i] = h;
        return st;
    }
    ENC_HDM float xyz(const float*, const Staged& st, int a) const { return st.x[a]; }
};

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

// the reduce's row rule (encode_cells.h): the interval rule on the metric prediction
struct AlnRowRule {
    const float *lo, *hi, *pose;
    ENC_HDM EncRow operator()(float p, int64_t i, int b, float clamp) const { return cpl_row(aln_metric(p, pose + VERIFY_POSE * b), lo[i], hi[i], clamp); }
};

// The reduce's column rule: the L + 5 gradient columns.  The five pose columns of a row (float64 divisions and a rotation each) are formed
// once per row into the EXTRA words; the latent columns, one product each, where they are summed.
struct AlnCols {
    static constexpr int EXTRA = ALN_POSE;
    const float *pred, *J, *cam, *pose;
    int Jstride, L;
    ENC_HDM void prepare(double* x, float w, int64_t i, int b) const {
        for (int c = 0; c < ALN_POSE; ++c) x[c] = aln_value(L + c, L, w, 0.0, 0, pred[i], J + i * Jstride, cam + 3 * i, pose + VERIFY_POSE * b);
    }
    ENC_HDM double operator()(int c, int, float w, double e, int ok, int64_t i, int b, const double* x) const {
        if (c >= L && c < L + ALN_POSE) return x[c - L];
        return aln_value(c, L, w, e, ok, pred[i], J + i * Jstride, cam + 3 * i, pose + VERIFY_POSE * b);
    }
};

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

// latent_adam on every pose parameter whose rate is not 0 (a rate of 0 leaves the parameter and its state untouched), then the next pose row.
// The arrays do not overlap, and the signature says so: the device then loads the fifteen words of state at once, not parameter by parameter.
ENC_HD void aln_pose_step(float* __restrict__ theta, float* __restrict__ tm, float* __restrict__ tv, const double* __restrict__ g, int L,
                          const float* __restrict__ lr, float bc1, float bc2, float* __restrict__ pose) {
    for (int i = 0; i < ALN_POSE; ++i)
        if (lr[i] != 0.f) latent_adam(&theta[i], &tm[i], &tv[i], (float)g[L + i], lr[i], bc1, bc2);
    aln_pose_row(theta, pose);
}

// The step kernel's pose policy (encode_cells.h): five pose parameters after the latent.  A shape with an unusable pose, a pose gradient
// that is not finite or a scale the update would not leave positive is not stepped; a latent rate of 0 leaves z, m and v alone, as a pose
// rate of 0 does its parameter.
struct AlnPoseStep {
    static constexpr int EXTRA = ALN_POSE;
    static constexpr int SKIP = ENC_EMPTY | ENC_NO_ROWS | ENC_BAD_TABLE | ALN_BAD_POSE;
    float *theta, *tm, *tv, *pose;
    float lr[ALN_POSE];
    ENC_HDM bool ok(int b, const double* g, int L, float bc1, float bc2) const {
        const float sc = aln_scale_after(theta + ALN_POSE * b, tm + ALN_POSE * b, tv + ALN_POSE * b, g, L, lr[4], bc1, bc2);
        return aln_pose_grad_ok(g, L) && isfinite(sc) && sc > 0.f;
    }
    ENC_HDM bool steps_latent(float lr_latent) const { return lr_latent != 0.f; }
    ENC_HDM void step(int b, const double* g, int L, float bc1, float bc2) const {
        aln_pose_step(theta + ALN_POSE * b, tm + ALN_POSE * b, tv + ALN_POSE * b, g, L, lr, bc1, bc2, pose + VERIFY_POSE * b);
    }
};
