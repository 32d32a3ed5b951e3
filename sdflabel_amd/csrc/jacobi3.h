// Float64 eigen-decomposition of a symmetric 3x3 matrix, shared by the RANSAC fits (pose.hip) and the lidar normals (normals.hip).
// A plain function, compiled for the device by the two units and for the host by tests/pose_host/pose_host.cpp.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define J3_HD __host__ __device__ inline
#else
#define J3_HD static inline
#endif

// eigen-decomposition of the symmetric 3x3 S (cyclic Jacobi, float64): eigenvalues descending in lam, eigenvectors as COLUMNS of V.
// The stop test and the rotations square the entries: a matrix whose largest entry lies outside [1e-100, 1e100] is first scaled by an exact
// power of two (its eigenvalues scaled back at the end), so that neither `off` nor `1e-36 * dia` under- or overflows.  Inside that range --
// every matrix the two users form from metric data -- nothing is scaled and every bit is as it was without the scaling.
J3_HD void sdfr_jacobi3(double S[3][3], double lam[3], double V[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    double big = 0.0, unscale = 1.0;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) big = fabs(S[i][j]) > big ? fabs(S[i][j]) : big;          // (a NaN entry never wins: no scaling)
    if (big > 0.0 && (big < 1e-100 || big > 1e100) && big <= 1.7976931348623157e308) {
        int e = -ilogb(big);
        e = e > 1000 ? 1000 : e;
        const double sc = ldexp(1.0, e);
        unscale = ldexp(1.0, -e);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) S[i][j] *= sc;
    }
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = S[0][1] * S[0][1] + S[0][2] * S[0][2] + S[1][2] * S[1][2];
        const double dia = S[0][0] * S[0][0] + S[1][1] * S[1][1] + S[2][2] * S[2][2];
        if (!(off > 1e-36 * dia)) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = S[p][q];
                if (apq == 0.0) continue;
                const double theta = (S[q][q] - S[p][p]) / (2.0 * apq);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                for (int k = 0; k < 3; ++k) {          // S <- S J  (columns p, q)
                    const double skp = S[k][p], skq = S[k][q];
                    S[k][p] = c * skp - s * skq;
                    S[k][q] = s * skp + c * skq;
                }
                for (int k = 0; k < 3; ++k) {          // S <- J^T S  (rows p, q)
                    const double spk = S[p][k], sqk = S[q][k];
                    S[p][k] = c * spk - s * sqk;
                    S[q][k] = s * spk + c * sqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int o[3] = {0, 1, 2};
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (S[o[j]][o[j]] < S[o[j + 1]][o[j + 1]]) { const int x = o[j]; o[j] = o[j + 1]; o[j + 1] = x; }
    double W[3][3];
    for (int i = 0; i < 3; ++i) {
        lam[i] = S[o[i]][o[i]] * unscale;
        for (int k = 0; k < 3; ++k) W[k][i] = V[k][o[i]];
    }
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) V[k][i] = W[k][i];
}
