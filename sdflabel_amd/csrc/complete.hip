// Shape completion from one view (DeepSDF's other use of a frozen decoder): sdfr_view_samples turns observed points into sample rows with
// an interval target -- the point, two points offset along its normal, free-space points on its sensor ray --, sdfr_bound_rows and
// sdfr_bound_reduce are sdfr_encode_rows and sdfr_encode_reduce for such rows, and sdfr_encode_step is used as it is.  All three are
// instances of the kernels of encode_kernels.h: the samples with a pose, the rows over CplBoundRows (samples of 5 floats), the reduce
// over CplBoundRule (cpl_row).  The per-element rules are csrc/complete_cells.h.  No atomics, no memset, no host
// synchronisation; the same bits on every run; a shape's results do not depend on B or on its place in the batch.
// Compiled with -ffp-contract=off.
#include "encode_kernels.h"

extern "C" int sdfr_view_samples(const float* points, const double* normals, int64_t N, const int64_t* ptoff, int B, const float* pose, const float* origin,
                                 int shape0, int F, float eta, float s_max, int64_t seed, float* rows, int32_t* flags, void* stream) {
    return enc_samples_launch<true>("sdfr_view_samples", points, normals, N, ptoff, B, pose, origin, shape0, F, eta, s_max, seed, rows, flags, stream);
}

extern "C" int sdfr_bound_rows(const float* samples, int64_t S, const int64_t* soff, int B, int shape0, int64_t k, int draw, int64_t seed, int64_t iter,
                               const float* z, int L, int unit, float* inputs, float* lo, float* hi, float* zn, int32_t* flags, void* stream) {
    return enc_rows_launch("sdfr_bound_rows", samples, S, soff, B, shape0, k, draw, seed, iter, z, L, unit, CplBoundRows{lo, hi}, true, lo && hi, inputs, zn,
                           flags, stream);
}

extern "C" int sdfr_bound_reduce(const float* pred, const float* lo, const float* hi, const float* J, int Jstride, int L, int B, int64_t k, float clamp,
                                 void* ws, int64_t ws_bytes, double* loss, double* g_zn, int32_t* flags, void* stream) {
    return enc_reduce_launch("sdfr_bound_reduce", pred, CplBoundRule{lo, hi}, lo != nullptr && hi != nullptr, J, Jstride, L, B, k, clamp, ws, ws_bytes, loss,
                             g_zn, flags, stream);
}
