// Encoding shapes under a frozen decoder (DeepSDF's "reconstruct"): everything of one iteration of the batched latent fit that is not the
// decoder itself.  sdfr_encode_rows draws the iteration's rows and writes the decoder's inputs; sdfr_encode_reduce turns the decoder's values
// and the latent columns of its Jacobian into one clamped-L1 loss and one latent gradient per shape; sdfr_encode_step takes the gradient
// through the unit normalisation and applies Adam.  The per-element rules and THE summation order are csrc/encode_cells.h.
// No atomics, no memset, no host synchronisation; the same bits on every run; a shape's results do not depend on B or on its place in the
// batch.  Compiled with -ffp-contract=off: every float64 and float32 operation is rounded on its own.
#include "encode_kernels.h"

// The rows kernel (samples of 4 floats) and the reduce (the exact row rule enc_row) are instances of encode_kernels.h, which the interval
// fit of complete.hip shares.
extern "C" int sdfr_encode_rows(const float* samples, int64_t S, const int64_t* soff, int B, int shape0, int64_t k, int draw, int64_t seed, int64_t iter,
                                const float* z, int L, int unit, float* inputs, float* target, float* zn, int32_t* flags, void* stream) {
    return enc_rows_launch<4>("sdfr_encode_rows", samples, S, soff, B, shape0, k, draw, seed, iter, z, L, unit, inputs, target, nullptr, zn, flags, stream);
}

extern "C" int64_t sdfr_encode_ws_bytes(int B, int64_t k, int L) { return enc_ws_bytes(B, k, L); }

extern "C" int sdfr_encode_reduce(const float* pred, const float* target, const float* J, int Jstride, int L, int B, int64_t k, float clamp, void* ws,
                                  int64_t ws_bytes, double* loss, double* g_zn, int32_t* flags, void* stream) {
    return enc_reduce_launch("sdfr_encode_reduce", pred, EncExactRule{target}, target != nullptr, J, Jstride, L, B, k, clamp, ws, ws_bytes, loss, g_zn,
                             flags, stream);
}

// ---- step -----------------------------------------------------------------------------------------------------------------------------------
// grid (B), one workgroup per shape.  Thread 0 walks the latent once in index order (norm, projection, the finite check); then thread i
// updates element i.  A shape that is flagged or whose gradient is not finite keeps z, m and v and gets ENC_SKIPPED.
__global__ __launch_bounds__(ENC_THREADS) void sdfr_encode_step_kernel(float* __restrict__ z, float* __restrict__ m, float* __restrict__ v, int L,
                                                                      int unit, const double* __restrict__ g_zn, const double* __restrict__ loss,
                                                                      int32_t* __restrict__ flags, float code_reg, float lr, float bc1, float bc2,
                                                                      float* __restrict__ history_row) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ float s_g[ENC_MAX_L];
    __shared__ float s_nrm, s_dot, s_nz;
    __shared__ int s_skip;
    float* zb = z + (int64_t)b * L;
    if (tid < L) s_g[tid] = (float)g_zn[(int64_t)b * L + tid];
    __syncthreads();
    if (tid == 0) {
        const int fl = flags[b];
        const float nrm = unit ? latent_norm(zb, L) : 1.f;
        const float dot = unit ? latent_unit_dot(zb, s_g, L, nrm) : 0.f;
        const float nz = unit ? 0.f : enc_raw_norm(zb, L);
        int skip = (fl & (ENC_EMPTY | ENC_NO_ROWS | ENC_BAD_TABLE)) ? 1 : 0;
        for (int i = 0; i < L; ++i)
            if (!isfinite(enc_step_grad(zb[i], s_g[i], unit, nrm, dot, nz, code_reg))) skip = 1;
        s_nrm = nrm; s_dot = dot; s_nz = nz; s_skip = skip;
        if (skip) flags[b] = fl | ENC_SKIPPED;
        if (history_row) history_row[b] = (float)loss[b];
    }
    __syncthreads();
    if (s_skip || tid >= L) return;
    const float gi = enc_step_grad(zb[tid], s_g[tid], unit, s_nrm, s_dot, s_nz, code_reg);
    latent_adam(&zb[tid], &m[(int64_t)b * L + tid], &v[(int64_t)b * L + tid], gi, lr, bc1, bc2);
}

extern "C" int sdfr_encode_step(float* z, float* m, float* v, int L, int B, int unit, const double* g_zn, const double* loss, int32_t* flags,
                                float code_reg, float lr, int t, float* history, int64_t history_stride, void* stream) {
    SDFR_REQUIRE(z && m && v && g_zn && loss && flags, "sdfr_encode_step: NULL argument");
    SDFR_REQUIRE(L >= 1 && L <= ENC_MAX_L && B >= 0 && B <= ENC_MAX_B, "sdfr_encode_step: bad size (L = %d, B = %d)", L, B);
    SDFR_REQUIRE(t >= 1 && t <= ENC_MAX_ITER, "sdfr_encode_step: the step count t = %d starts at 1", t);
    SDFR_REQUIRE(!history || history_stride >= B, "sdfr_encode_step: history_stride %lld below B = %d", (long long)history_stride, B);
    SDFR_REQUIRE(isfinite(lr) && isfinite(code_reg), "sdfr_encode_step: non-finite learning rate or regulariser");
    if (B == 0) return SDFR_OK;
    float bc1, bc2;
    enc_bias(t, &bc1, &bc2);
    hipLaunchKernelGGL(sdfr_encode_step_kernel, dim3(B), dim3(ENC_THREADS), 0, (hipStream_t)stream, z, m, v, L, unit, g_zn, loss, flags, code_reg, lr,
                       bc1, bc2, history ? history + (int64_t)(t - 1) * history_stride : (float*)nullptr);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
