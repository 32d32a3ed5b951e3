// Pose and shape fitted to one view under a frozen decoder: everything of one iteration that is not the decoder itself, with the pose in the
// middle.  sdfr_align_samples turns observed points into camera-frame rows with a METRIC interval target, once; sdfr_align_rows draws the
// iteration's rows and takes them through the iteration's pose to the decoder's inputs; sdfr_align_reduce forms one loss and one gradient
// per shape with respect to the latent and to yaw, trans and scale -- the last three columns of the decoder's Jacobian are d sdf / d xyz;
// sdfr_align_step applies Adam to the latent and to the pose, and writes the next iteration's pose row.  All four are instances of the
// kernels of encode_kernels.h (THE summation order, once): the samples without a pose, the rows over AlnPosedRows, the reduce over
// AlnRowRule and AlnCols, the step over AlnPoseStep.  The per-element rules and the policies are csrc/align_cells.h.
// No atomics, no memset, no host synchronisation; the same bits on every run; a shape's results do not depend on B or on its place in the
// batch.  Compiled with -ffp-contract=off.
#include "encode_kernels.h"

extern "C" int sdfr_align_samples(const float* points, const double* normals, int64_t N, const int64_t* ptoff, int B, const float* origin, int shape0, int F,
                                  float eta, float s_max, int64_t seed, float* rows, int32_t* flags, void* stream) {
    return enc_samples_launch<false>("sdfr_align_samples", points, normals, N, ptoff, B, nullptr, origin, shape0, F, eta, s_max, seed, rows, flags, stream);
}

extern "C" int sdfr_align_rows(const float* samples, int64_t S, const int64_t* soff, int B, int shape0, int64_t k, int draw, int64_t seed, int64_t iter,
                               const float* z, int L, int unit, const float* pose, float* inputs, float* cam, float* lo, float* hi, float* zn,
                               int32_t* flags, void* stream) {
    return enc_rows_launch("sdfr_align_rows", samples, S, soff, B, shape0, k, draw, seed, iter, z, L, unit, AlnPosedRows{pose, cam, lo, hi}, pose != nullptr,
                           cam && lo && hi, inputs, zn, flags, stream);
}

extern "C" int64_t sdfr_align_ws_bytes(int B, int64_t k, int L) { return enc_ws_bytes(B, k, L, ALN_POSE); }

extern "C" int sdfr_align_reduce(const float* pred, const float* lo, const float* hi, const float* J, int Jstride, const float* cam, const float* pose, int L,
                                 int B, int64_t k, float clamp, void* ws, int64_t ws_bytes, double* loss, double* g, int32_t* flags, void* stream) {
    return enc_reduce_launch("sdfr_align_reduce", "sdfr_align_ws_bytes", pred, AlnRowRule{lo, hi, pose}, AlnCols{pred, J, cam, pose, Jstride, L},
                             lo != nullptr && hi != nullptr && cam != nullptr && pose != nullptr, J, Jstride, L + 3, L, ALN_POSE, B, k, clamp, ws, ws_bytes,
                             loss, g, flags, stream);
}

extern "C" int sdfr_align_step(float* z, float* m, float* v, int L, int B, int unit, float* theta, float* tm, float* tv, float* pose, const double* g,
                               const double* loss, int32_t* flags, float code_reg, float lr, const float* lr_pose, int t, float* history,
                               int64_t history_stride, void* stream) {
    AlnPoseStep step{theta, tm, tv, pose, {0.f, 0.f, 0.f, 0.f, 0.f}};
    bool finite = true;
    for (int i = 0; lr_pose && i < ALN_POSE; ++i) {
        step.lr[i] = lr_pose[i];
        finite = finite && isfinite(lr_pose[i]);
    }
    return enc_step_launch("sdfr_align_step", z, m, v, L, B, unit, step, theta && tm && tv && pose && lr_pose, finite, g, loss, flags, code_reg, lr, t,
                           history, history_stride, stream);
}
