// Shape completion from one view (DeepSDF's other use of a frozen decoder): sdfr_view_samples turns observed points into sample rows with
// an interval target -- the point, two points offset along its normal, free-space points on its sensor ray --, sdfr_bound_rows and
// sdfr_bound_reduce are sdfr_encode_rows and sdfr_encode_reduce for such rows (the kernels of encode_kernels.h with samples of 5 floats and
// the row rule cpl_row), and sdfr_encode_step is used as it is.  The per-element rules are csrc/complete_cells.h.  No atomics,
// no memset, no host synchronisation; the same bits on every run; a shape's results do not depend on B or on its place in the batch.
// Compiled with -ffp-contract=off.
#include "encode_kernels.h"
#include "complete_cells.h"

// One point per thread: thread g < N writes the P = 3 + F rows of point g, thread g < B the flag word of shape g.
__global__ __launch_bounds__(ENC_THREADS) void sdfr_view_samples_kernel(const float* __restrict__ points, const double* __restrict__ normals, int64_t N,
                                                                       const int64_t* __restrict__ ptoff, int B, const float* __restrict__ pose,
                                                                       const float* __restrict__ origin, int shape0, int F, double eta, double s_max,
                                                                       uint64_t seed, float* __restrict__ rows, int32_t* __restrict__ flags) {
    const int64_t g = (int64_t)blockIdx.x * ENC_THREADS + threadIdx.x;
    if (g < B) flags[g] = cpl_view_flags(ptoff, pose, (int)g, N);
    if (g >= N) return;
    const int b = cpl_owner(ptoff, B, N, g);
    const bool usable = b >= 0 && cpl_pose_ok(pose + VERIFY_POSE * (b < 0 ? 0 : b));
    const float org[3] = {origin[0], origin[1], origin[2]};
    cpl_view_row(points + 3 * g, normals ? normals + 3 * g : nullptr, pose + VERIFY_POSE * (b < 0 ? 0 : b), org, usable, seed, shape0 + (b < 0 ? 0 : b),
                 b < 0 ? 0 : g - ptoff[b], F, eta, s_max, rows + (int64_t)CPL_ROW * (3 + F) * g);
}

extern "C" int sdfr_view_samples(const float* points, const double* normals, int64_t N, const int64_t* ptoff, int B, const float* pose, const float* origin,
                                 int shape0, int F, float eta, float s_max, int64_t seed, float* rows, int32_t* flags, void* stream) {
    SDFR_REQUIRE(B >= 0 && N >= 0 && shape0 >= 0 && (int64_t)shape0 + B <= ENC_MAX_B, "sdfr_view_samples: bad size (B = %d, N = %lld, shape0 = %d)", B,
                 (long long)N, shape0);
    SDFR_REQUIRE(F >= 0 && F <= CPL_MAX_FREE, "sdfr_view_samples: F = %d free-space rows outside [0,%d]", F, CPL_MAX_FREE);
    SDFR_REQUIRE(isfinite(eta) && isfinite(s_max) && s_max >= 0.f, "sdfr_view_samples: eta must be finite and s_max finite and not negative");
    SDFR_REQUIRE(N <= ((int64_t)1 << 32), "sdfr_view_samples: at most 2^32 points");
    if (B == 0 && N == 0) return SDFR_OK;
    SDFR_REQUIRE(ptoff && pose && origin && flags && (N == 0 || (points && rows)) && B >= 1, "sdfr_view_samples: NULL argument, or points without a shape");
    const int64_t threads = N > B ? N : (int64_t)B;
    hipLaunchKernelGGL(sdfr_view_samples_kernel, dim3((unsigned)((threads + ENC_THREADS - 1) / ENC_THREADS)), dim3(ENC_THREADS), 0, (hipStream_t)stream,
                       points, normals, N, ptoff, B, pose, origin, shape0, F, (double)eta, (double)s_max, (uint64_t)seed, rows, flags);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_bound_rows(const float* samples, int64_t S, const int64_t* soff, int B, int shape0, int64_t k, int draw, int64_t seed, int64_t iter,
                               const float* z, int L, int unit, float* inputs, float* lo, float* hi, float* zn, int32_t* flags, void* stream) {
    return enc_rows_launch<5>("sdfr_bound_rows", samples, S, soff, B, shape0, k, draw, seed, iter, z, L, unit, inputs, lo, hi, zn, flags, stream);
}

struct CplBoundRule {
    const float *lo, *hi;
    __device__ EncRow operator()(float p, int64_t i, int, float clamp) const { return cpl_row(p, lo[i], hi[i], clamp); }
};

extern "C" int sdfr_bound_reduce(const float* pred, const float* lo, const float* hi, const float* J, int Jstride, int L, int B, int64_t k, float clamp,
                                 void* ws, int64_t ws_bytes, double* loss, double* g_zn, int32_t* flags, void* stream) {
    return enc_reduce_launch("sdfr_bound_reduce", pred, CplBoundRule{lo, hi}, lo != nullptr && hi != nullptr, J, Jstride, L, B, k, clamp, ws, ws_bytes, loss,
                             g_zn, flags, stream);
}
