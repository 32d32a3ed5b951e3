// Encoding shapes under a frozen decoder (DeepSDF's "reconstruct"): everything of one iteration of the batched latent fit that is not the
// decoder itself.  sdfr_encode_rows draws the iteration's rows and writes the decoder's inputs; sdfr_encode_reduce turns the decoder's values
// and the latent columns of its Jacobian into one clamped-L1 loss and one latent gradient per shape; sdfr_encode_step takes the gradient
// through the unit normalisation and applies Adam.  The per-element rules and THE summation order are csrc/encode_cells.h.
// No atomics, no memset, no host synchronisation; the same bits on every run; a shape's results do not depend on B or on its place in the
// batch.  Compiled with -ffp-contract=off: every float64 and float32 operation is rounded on its own.
//
// The three are instances of the kernels of encode_kernels.h, which the interval fit of complete.hip and the pose-and-shape fit of
// align.hip share: the rows over EncExactRows (samples of 4 floats), the reduce over EncExactRule (enc_row) and the latent columns, the
// step over EncNoPose.
#include "encode_kernels.h"

extern "C" int sdfr_encode_rows(const float* samples, int64_t S, const int64_t* soff, int B, int shape0, int64_t k, int draw, int64_t seed, int64_t iter,
                                const float* z, int L, int unit, float* inputs, float* target, float* zn, int32_t* flags, void* stream) {
    return enc_rows_launch("sdfr_encode_rows", samples, S, soff, B, shape0, k, draw, seed, iter, z, L, unit, EncExactRows{target, nullptr}, true,
                           target != nullptr, inputs, zn, flags, stream);
}

extern "C" int64_t sdfr_encode_ws_bytes(int B, int64_t k, int L) { return enc_ws_bytes(B, k, L); }

extern "C" int sdfr_encode_reduce(const float* pred, const float* target, const float* J, int Jstride, int L, int B, int64_t k, float clamp, void* ws,
                                  int64_t ws_bytes, double* loss, double* g_zn, int32_t* flags, void* stream) {
    return enc_reduce_launch("sdfr_encode_reduce", pred, EncExactRule{target}, target != nullptr, J, Jstride, L, B, k, clamp, ws, ws_bytes, loss, g_zn,
                             flags, stream);
}

extern "C" int sdfr_encode_step(float* z, float* m, float* v, int L, int B, int unit, const double* g_zn, const double* loss, int32_t* flags,
                                float code_reg, float lr, int t, float* history, int64_t history_stride, void* stream) {
    return enc_step_launch("sdfr_encode_step", z, m, v, L, B, unit, EncNoPose{}, true, true, g_zn, loss, flags, code_reg, lr, t, history, history_stride,
                           stream);
}
