// Per-element rules of a latent's way to the decoder and back, shared by the refinement's parameter glue (params.hip), its solver (solver.h)
// and the shape encoder (encode.hip, encode_cells.h): the unit normalisation latent_ = F.normalize(latent) (pipelines/optimizer.py:96), its
// backward, and one Adam update.  Plain float32 statements, every operation rounded on its own (the including files are compiled with
// -ffp-contract=off); compiled for the host too (tests/encode_host/encode_host.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LAT_HD __host__ __device__ __forceinline__
#else
#define LAT_HD static inline
#endif

// ||z||_2 summed in index order, max(., 1e-12) as F.normalize does
LAT_HD float latent_norm(const float* z, int L) {
    float ss = 0.f;
    for (int c = 0; c < L; ++c) ss += z[c] * z[c];
    return fmaxf(sqrtf(ss), 1e-12f);
}

// sum_i (z_i / nrm) g_i in index order: the projection the backward of the normalisation removes
LAT_HD float latent_unit_dot(const float* z, const float* g, int L, float nrm) {
    float dot = 0.f;
    for (int i = 0; i < L; ++i) dot += (z[i] / nrm) * g[i];
    return dot;
}

// d / d z_i of a function of z / nrm whose gradient with respect to z / nrm is g
LAT_HD float latent_unit_grad(float zi, float gi, float nrm, float dot) { return (gi - (zi / nrm) * dot) / nrm; }

// One Adam update (betas 0.9 / 0.999, eps 1e-8) as torch.optim.Adam forms it.  bc1 = 1 - beta1^t, bc2 = 1 - beta2^t are the caller's.
// 1 - beta2 is the rounded double value: in float32, 1.f - 0.999f is 0.99998713e-3 and puts the second moment 1.3e-5 below torch's.
LAT_HD void latent_adam(float* p, float* m_io, float* v_io, float gi, float lr, float bc1, float bc2) {
    const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f, omb2 = 0.001f;
    float m = *m_io, v = *v_io;
    m = b1 * m + (1.f - b1) * gi;
    v = b2 * v + omb2 * gi * gi;
    *m_io = m; *v_io = v;
    const float denom = sqrtf(v) / sqrtf(bc2) + eps;
    *p -= (lr / bc1) * (m / denom);
}
