// Per-element rules of the RANSAC pose initialisation (pose.hip): the sampler's draw, one step of the colour-NN and the scoring-NN searches,
// the fits, the transformed point, the inlier decision, the select comparison and the per-point terms of the final fit.  Plain functions of
// one hypothesis, one (point, candidate) pair or one point, compiled for the device by pose.hip and for the host by
// tests/pose_host/pose_host.cpp, which runs the threads as loops and is compared with the numpy restatement (tests/_pose_ref.py) bit for bit.
// Both translation units are compiled with -ffp-contract=off: every float32 / float64 expression below rounds as written; the one fused
// operation is the explicit fmaf of rs_nn_step.
#pragma once
#include <math.h>
#include <stdint.h>

#include "jacobi3.h"

#if defined(__HIPCC__)
#include <hip/hip_fp16.h>
#define POSE_HD __host__ __device__ inline
#else
#define POSE_HD static inline
#endif

#define RS_TPB 256      // threads per workgroup (every kernel)
#define RS_HG 8         // passing hypotheses per scoring workgroup (registers: 3 + 2 per hypothesis)
#define RS_TRANS 12     // float32 [3][4] = [rot*scale | tra] of a hypothesis

struct PoseV3 {
    float x, y, z;
};

// ---- sampler ----------------------------------------------------------------------------------------------------------------------------
POSE_HD uint64_t rs_mix64(uint64_t z) {          // splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

POSE_HD uint64_t rs_sample_key(uint64_t seed, uint64_t key) { return rs_mix64(seed ^ rs_mix64(key * 0x9E3779B97F4A7C15ull + 1ull)); }

// the 4 distinct scene indices of hypothesis t (all zero when n < 4).  Draw k, attempt c: hi 32 bits of the hash scaled to [0, n) by
// multiply-shift.  Repeats of an earlier draw are rejected (next attempt); after 64 attempts the value steps forward to the next unused
// index (never reached in practice, keeps the loop bounded).
POSE_HD void rs_sample_draw(uint64_t hk, int t, int n, int d[4]) {
    d[0] = d[1] = d[2] = d[3] = 0;
    if (n >= 4) {
        for (int k = 0; k < 4; ++k) {
            int x = 0;
            for (int c = 0;; ++c) {
                const uint64_t h = rs_mix64(hk ^ (((uint64_t)t << 16) | ((uint64_t)k << 8) | (uint64_t)c));
                x = (int)(((h >> 32) * (uint64_t)n) >> 32);
                bool rep = false;
                for (int q = 0; q < k; ++q) rep |= d[q] == x;
                if (!rep) break;
                if (c == 63) {
                    for (;;) {
                        x = x + 1 == n ? 0 : x + 1;
                        rep = false;
                        for (int q = 0; q < k; ++q) rep |= d[q] == x;
                        if (!rep) break;
                    }
                    break;
                }
            }
            d[k] = x;
        }
    }
}

// ---- colour NN --------------------------------------------------------------------------------------------------------------------------
// KDTree(model_cls).query in float64: rdist = (dx^2 + dy^2) + dz^2; candidates come in index order and a later one must be strictly
// nearer, so ties go to the lowest model index.  The distance reported is sqrt(best).
POSE_HD void rs_cnn_step(double qx, double qy, double qz, float mx, float my, float mz, int j, double* best, int* bi) {
    const double dx = qx - (double)mx, dy = qy - (double)my, dz = qz - (double)mz;
    const double d2 = dx * dx + dy * dy + dz * dz;
    if (d2 < *best) { *best = d2; *bi = j; }
}

// ---- fits -------------------------------------------------------------------------------------------------------------------------------
POSE_HD float rs_half_round(float x) {              // float32 -> float16 (round to nearest even) -> float32
#if defined(__HIPCC__)
    return __half2float(__float2half_rn(x));
#else
    union { float f; uint32_t u; } v;
    v.f = x;
    const uint32_t sign = v.u & 0x80000000u, a = v.u & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) return x;                                  // infinities and NaN
    if (a >= 0x477FF000u) { v.u = sign | 0x7F800000u; return v.f; }  // rounds to 65536 or beyond: infinity
    if (a < 0x38800000u) {                                           // below 2^-14: the float16 grid is multiples of 2^-24
        const float m = 16777216.0f, r = 12582912.0f;                // x * 2^24 is exact; (. + 1.5 * 2^23) - 1.5 * 2^23 rounds it to an integer, ties to even
        union { float f; uint32_t u; } w;
        w.u = a;
        float s = w.f * m;
        s = (s + r) - r;
        w.f = s / m;
        w.u |= sign;
        return w.f;
    }
    uint32_t r = a + 0x00000FFFu + ((a >> 13) & 1u);                 // 13 mantissa bits go: round to nearest, ties to even
    r &= 0xFFFFE000u;
    v.u = sign | r;
    return v.f;
#endif
}

POSE_HD double rs_round(double x, bool f16) {     // a value stored in the numpy dtype of the array it belongs to
    return f16 ? (double)rs_half_round((float)x) : (double)(float)x;
}

// H = sum to_c from_c^T (H[i][j] = sum to_i from_j): the reference's cross-correlation (kabsch) / covariance times N (procrustes).
// R = U diag(1, 1, det V) V^T with u1 = H v1 / s1, u2 = H v2 / s2 (made orthogonal to u1), u3 = u1 x u2 -- the unique rotation both
// reference fits return whenever rank(H) >= 2, whatever sign convention their SVD picked.  s3' = u3 . H v3 (signed).
// type 1 (procrustes): returns false when numpy's matrix_rank of the float32 covariance (tol = s1 * 3 * eps_f32) is below 2;
// c = (s1 + s2 + det V s3') / sum |from_c|^2 (= (d * S.diag).sum() / sigma_from).  Translation: kabsch  R(pm - cm) - R pm + pm,
// procrustes  mean_to - c R mean_from.
// rs_fit in two parts.  rs_fit_basis: the frames U, V, the two largest singular values and det V.
POSE_HD void rs_fit_basis(const double H[3][3], double U[3][3], double V[3][3], double* s1_, double* s2_, double* detV_) {
    double S[3][3], lam[3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) S[i][j] = H[0][i] * H[0][j] + H[1][i] * H[1][j] + H[2][i] * H[2][j];
    sdfr_jacobi3(S, lam, V);
    const double s1 = sqrt(lam[0] > 0.0 ? lam[0] : 0.0), s2 = sqrt(lam[1] > 0.0 ? lam[1] : 0.0);
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 3; ++i) U[i][k] = H[i][0] * V[0][k] + H[i][1] * V[1][k] + H[i][2] * V[2][k];
    double n1 = sqrt(U[0][0] * U[0][0] + U[1][0] * U[1][0] + U[2][0] * U[2][0]);
    if (!(n1 > 0.0)) { U[0][0] = 1.0; U[1][0] = 0.0; U[2][0] = 0.0; n1 = 1.0; }
    for (int i = 0; i < 3; ++i) U[i][0] /= n1;
    const double d12 = U[0][0] * U[0][1] + U[1][0] * U[1][1] + U[2][0] * U[2][1];
    for (int i = 0; i < 3; ++i) U[i][1] -= d12 * U[i][0];
    double n2 = sqrt(U[0][1] * U[0][1] + U[1][1] * U[1][1] + U[2][1] * U[2][1]);
    if (!(n2 > 1e-300)) {                              // rank 1: any unit vector orthogonal to u1
        const int a = fabs(U[0][0]) < 0.6 ? 0 : 1;
        double e[3] = {0.0, 0.0, 0.0};
        e[a] = 1.0;
        const double d = e[0] * U[0][0] + e[1] * U[1][0] + e[2] * U[2][0];
        for (int i = 0; i < 3; ++i) U[i][1] = e[i] - d * U[i][0];
        n2 = sqrt(U[0][1] * U[0][1] + U[1][1] * U[1][1] + U[2][1] * U[2][1]);
    }
    for (int i = 0; i < 3; ++i) U[i][1] /= n2;
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    *detV_ = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
             V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
    *s1_ = s1;
    *s2_ = s2;
}

// rs_fit_pose: rotation, scale and translation from the frames and sv = sign of det V (-1 or 1)
POSE_HD bool rs_fit_pose(const double H[3][3], const double U[3][3], const double V[3][3], double s1, double s2, double sv, const double mf[3],
                         const double mt[3], double sig_from, int type, double R[3][3], double* c, double t[3], double* s_ratio) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = U[i][0] * V[j][0] + U[i][1] * V[j][1] + sv * U[i][2] * V[j][2];
    *s_ratio = s1 > 0.0 ? s2 / s1 : 0.0;
    if (type == 1) {
        if (!(s2 > s1 * 3.0 * 1.1920928955078125e-07 /* float32 eps */)) return false;
        double hv[3];
        for (int i = 0; i < 3; ++i) hv[i] = H[i][0] * V[0][2] + H[i][1] * V[1][2] + H[i][2] * V[2][2];
        const double s3 = U[0][2] * hv[0] + U[1][2] * hv[1] + U[2][2] * hv[2];
        *c = (s1 + s2 + sv * s3) / sig_from;
        for (int i = 0; i < 3; ++i) t[i] = mt[i] - *c * (R[i][0] * mf[0] + R[i][1] * mf[1] + R[i][2] * mf[2]);
    } else {
        *c = 1.0;
        for (int i = 0; i < 3; ++i) {
            const double a = R[i][0] * (mt[0] - mf[0]) + R[i][1] * (mt[1] - mf[1]) + R[i][2] * (mt[2] - mf[2]);
            const double bb = R[i][0] * mt[0] + R[i][1] * mt[1] + R[i][2] * mt[2];
            t[i] = a - bb + mt[i];
        }
    }
    return true;
}

POSE_HD bool rs_fit(const double H[3][3], const double mf[3], const double mt[3], double sig_from, int type, double R[3][3], double* c,
                    double t[3], double* s_ratio) {
    double U[3][3], V[3][3], s1, s2, detV;
    rs_fit_basis(H, U, V, &s1, &s2, &detV);
    return rs_fit_pose(H, U, V, s1, s2, detV < 0.0 ? -1.0 : 1.0, mf, mt, sig_from, type, R, c, t, s_ratio);
}

// ---- one hypothesis after the colour gate -----------------------------------------------------------------------------------------------
// from = the 4 scene points (float32), to = their colour-NN model points (the model's dtype); numpy means: float32 sums in order, / 4 in
// float32, stored in the dtype; centred values stored in the dtype.  The two halves, so that a caller can stand between them:
POSE_HD void rs_sample_moments(const float fp[4][3], const float tp[4][3], bool f16, double mf[3], double mt[3], double H[3][3], double* sig_) {
    double fc[4][3], tc[4][3], sig = 0.0;
    for (int d = 0; d < 3; ++d) {
        const float sf = ((fp[0][d] + fp[1][d]) + fp[2][d]) + fp[3][d];
        const float st = ((tp[0][d] + tp[1][d]) + tp[2][d]) + tp[3][d];
        mf[d] = (double)(sf / 4.0f);
        mt[d] = rs_round((double)(st / 4.0f), f16);
    }
    for (int k = 0; k < 4; ++k)
        for (int d = 0; d < 3; ++d) {
            fc[k][d] = rs_round((double)fp[k][d] - mf[d], false);
            tc[k][d] = rs_round((double)tp[k][d] - mt[d], f16);
            sig += fc[k][d] * fc[k][d];
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) H[i][j] = ((tc[0][i] * fc[0][j] + tc[1][i] * fc[1][j]) + tc[2][i] * fc[2][j]) + tc[3][i] * fc[3][j];
    *sig_ = sig;
}

// the float32 row [rot*scale | tra] of an accepted fit: the float64 product R c stored to float32, ONE rounding per entry.  That is the
// reference's: its procrustes returns float64 R and c (numpy promotes through S = np.eye(3)) and `trans[:3, :3] = rot * scale` rounds the
// float64 product once; its kabsch has scale = 1, where (float)(R * 1.0) is (float)R.
POSE_HD void rs_hyp_row(const double R[3][3], double c, const double tr[3], float h[RS_TRANS]) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) h[i * 4 + j] = (float)(R[i][j] * c);
        h[i * 4 + 3] = (float)tr[i];
    }
}

// What rs_hyp_kernel does for one hypothesis that passed the colour gate: returns whether the hypothesis is scored (then h holds its row);
// *bits gets gate bit 1 (fit accepted: not rejected by the rank rule, float32(c) <= 3) and bit 2 (s2 / s1 < 1e-3: rank-deficient sample).
POSE_HD bool pose_sample_fit(const float fp[4][3], const float tp[4][3], bool f16, int type, float h[RS_TRANS], int* bits) {
    double mf[3], mt[3], H[3][3], sig, R[3][3], c, tr[3], ratio;
    bool pass = false;
    *bits = 0;
    rs_sample_moments(fp, tp, f16, mf, mt, H, &sig);
    if (rs_fit(H, mf, mt, sig, type, R, &c, tr, &ratio) && !((float)c > 3.0f)) {
        *bits |= 2;
        pass = true;
        rs_hyp_row(R, c, tr, h);
    }
    if (ratio < 1e-3) *bits |= 4;           // rank-deficient sample (diagnostic)
    return pass;
}

// ---- scoring ----------------------------------------------------------------------------------------------------------------------------
// the reference's transformed scene point: (trans[:, :3] @ scene.T).T + trans[:, 3] in float32, separate roundings in the sum's order
POSE_HD PoseV3 rs_transform(const float* h, float x, float y, float z) {
    PoseV3 r;
    r.x = ((h[0] * x + h[1] * y) + h[2] * z) + h[3];
    r.y = ((h[4] * x + h[5] * y) + h[6] * z) + h[7];
    r.z = ((h[8] * x + h[9] * y) + h[10] * z) + h[11];
    return r;
}

// one candidate j of the scoring search: float32 squared distance with two fused multiply-adds, dz^2 rounded first; a later candidate must
// be strictly nearer, so exact ties go to the first index.  bd starts at INFINITY and bi at 0.
POSE_HD void rs_nn_step(PoseV3 tp, float mx, float my, float mz, int j, float* bd, int* bi) {
    const float dx = tp.x - mx, dy = tp.y - my, dz = tp.z - mz;
    const float d2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
    if (d2 < *bd) { *bd = d2; *bi = j; }
}

// the inlier decision of step 5 for the winner nn: KDTree distance recomputed in float64 (< metric_thr), colour norm in float32
POSE_HD bool rs_inlier(PoseV3 tp, int nn, const float* mp, const float* mc, float sx, float sy, float sz, double metric_thr, float nocs_thr32) {
    const double dx = (double)tp.x - (double)mp[(size_t)nn * 3], dy = (double)tp.y - (double)mp[(size_t)nn * 3 + 1],
                 dz = (double)tp.z - (double)mp[(size_t)nn * 3 + 2];
    const double d = sqrt(dx * dx + dy * dy + dz * dz);
    const float cx = sx - mc[(size_t)nn * 3], cy = sy - mc[(size_t)nn * 3 + 1], cz = sz - mc[(size_t)nn * 3 + 2];
    const float dc = sqrtf(cx * cx + cy * cy + cz * cz);
    return d < metric_thr && dc < nocs_thr32;
}

// ---- select -----------------------------------------------------------------------------------------------------------------------------
// A thread walks its hypotheses t = tid, tid + 256, ... upwards and takes a count only when it is strictly larger (it starts from count 0,
// t = -1: the reference starts from an empty inlier set).  The tree then folds lane tid + o into lane tid for o = 128, 64, ..., 1:
// the other lane wins with a larger count, or with an equal count and the lower (valid) hypothesis index.
POSE_HD bool rs_select_takes(int c, int bc) { return c > bc; }
POSE_HD bool rs_select_folds(int c2, int t2, int c1, int t1) { return c2 > c1 || (c2 == c1 && t2 >= 0 && (t1 < 0 || t2 < t1)); }

// ---- final fit --------------------------------------------------------------------------------------------------------------------------
// Both passes: thread tid adds its inliers p = tid, tid + 256, ... in that order to its own partial sums (starting from 0.0), and the 256
// partials are folded by the tree lane tid += lane tid + o for o = 128, 64, ..., 1 (rs_block_sum).  m: the point's colour-NN model point,
// s: the scene point.  Pass 1: sums of m, of s, and the inlier count.
POSE_HD void rs_final_sums(const float* m, const float* s, double v[7]) {
    for (int d = 0; d < 3; ++d) { v[d] += (double)m[d]; v[3 + d] += (double)s[d]; }
    v[6] += 1.0;
}

// numpy means in the arrays' dtypes (model: float16 / float32, scene: float32)
POSE_HD void rs_final_means(const double v[7], bool f16, double mf[3], double mt[3]) {
    const double n = v[6];
    for (int d = 0; d < 3; ++d) {
        mf[d] = rs_round(v[d] / n, f16);
        mt[d] = rs_round(v[3 + d] / n, false);
    }
}

// Pass 2: the cross-covariance to_c from_c^T (9 terms, row-major) and |from_c|^2 of centred values stored in the arrays' dtypes
POSE_HD void rs_final_cov(const float* m, const float* s, const double mf[3], const double mt[3], bool f16, double v[10]) {
    double fc[3], tc[3];
    for (int d = 0; d < 3; ++d) {
        fc[d] = rs_round((double)m[d] - mf[d], f16);
        tc[d] = rs_round((double)s[d] - mt[d], false);
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i * 3 + j] += tc[i] * fc[j];
    v[9] += (fc[0] * fc[0] + fc[1] * fc[1]) + fc[2] * fc[2];
}
