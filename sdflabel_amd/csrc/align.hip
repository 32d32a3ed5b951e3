// Pose and shape fitted to one view under a frozen decoder: everything of one iteration that is not the decoder itself, with the pose in the
// middle.  sdfr_align_samples turns observed points into camera-frame rows with a METRIC interval target, once; sdfr_align_rows draws the
// iteration's rows and takes them through the iteration's pose to the decoder's inputs; sdfr_align_reduce forms one loss and one gradient
// per shape with respect to the latent and to yaw, trans and scale -- the last three columns of the decoder's Jacobian are d sdf / d xyz --
// through the reduce kernels of encode_kernels.h (THE summation order, once); sdfr_align_step applies Adam to the latent (the rule of
// sdfr_encode_step) and to the pose, and writes the next iteration's pose row.  The per-element rules are csrc/align_cells.h.
// No atomics, no memset, no host synchronisation; the same bits on every run; a shape's results do not depend on B or on its place in the
// batch.  Compiled with -ffp-contract=off.
#include "encode_kernels.h"
#include "align_cells.h"

// One point per thread: thread g < N writes the P = 3 + F rows of point g, thread g < B the flag word of shape g.
__global__ __launch_bounds__(ENC_THREADS) void sdfr_align_samples_kernel(const float* __restrict__ points, const double* __restrict__ normals, int64_t N,
                                                                        const int64_t* __restrict__ ptoff, int B, const float* __restrict__ origin,
                                                                        int shape0, int F, double eta, double s_max, uint64_t seed,
                                                                        float* __restrict__ rows, int32_t* __restrict__ flags) {
    const int64_t g = (int64_t)blockIdx.x * ENC_THREADS + threadIdx.x;
    if (g < B) flags[g] = cpl_table_ok(ptoff, (int)g, N) ? 0 : CPL_BAD_TABLE;
    if (g >= N) return;
    const int b = cpl_owner(ptoff, B, N, g);
    const float org[3] = {origin[0], origin[1], origin[2]};
    aln_sample_row(points + 3 * g, normals ? normals + 3 * g : nullptr, org, b >= 0, seed, shape0 + (b < 0 ? 0 : b), b < 0 ? 0 : g - ptoff[b], F, eta, s_max,
                   rows + (int64_t)ALN_ROW * (3 + F) * g);
}

extern "C" int sdfr_align_samples(const float* points, const double* normals, int64_t N, const int64_t* ptoff, int B, const float* origin, int shape0, int F,
                                  float eta, float s_max, int64_t seed, float* rows, int32_t* flags, void* stream) {
    SDFR_REQUIRE(B >= 0 && N >= 0 && shape0 >= 0 && (int64_t)shape0 + B <= ENC_MAX_B, "sdfr_align_samples: bad size (B = %d, N = %lld, shape0 = %d)", B,
                 (long long)N, shape0);
    SDFR_REQUIRE(F >= 0 && F <= CPL_MAX_FREE, "sdfr_align_samples: F = %d free-space rows outside [0,%d]", F, CPL_MAX_FREE);
    SDFR_REQUIRE(isfinite(eta) && isfinite(s_max) && s_max >= 0.f, "sdfr_align_samples: eta must be finite and s_max finite and not negative");
    SDFR_REQUIRE(N <= ((int64_t)1 << 32), "sdfr_align_samples: at most 2^32 points");
    if (B == 0 && N == 0) return SDFR_OK;
    SDFR_REQUIRE(ptoff && origin && flags && (N == 0 || (points && rows)) && B >= 1, "sdfr_align_samples: NULL argument, or points without a shape");
    const int64_t threads = N > B ? N : (int64_t)B;
    hipLaunchKernelGGL(sdfr_align_samples_kernel, dim3((unsigned)((threads + ENC_THREADS - 1) / ENC_THREADS)), dim3(ENC_THREADS), 0, (hipStream_t)stream,
                       points, normals, N, ptoff, B, origin, shape0, F, (double)eta, (double)s_max, (uint64_t)seed, rows, flags);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

// ---- rows -----------------------------------------------------------------------------------------------------------------------------------
// enc_rows_kernel<5> with a pose in the middle: grid (ceil(k / 256), B) -- or (1, B) without inputs: zn and flags only.  Thread tid of a
// workgroup draws row s0 + tid, takes its camera-frame point through pose[b] (aln_row) and keeps the lattice position in LDS; then the
// [256][L + 3] block is written element by element.
__global__ __launch_bounds__(ENC_THREADS) void sdfr_align_rows_kernel(const float* __restrict__ samples, int64_t S, const int64_t* __restrict__ soff,
                                                                     int shape0, int64_t k, int draw, uint64_t seed, int64_t iter,
                                                                     const float* __restrict__ z, int L, int unit, const float* __restrict__ pose,
                                                                     float* __restrict__ inputs, float* __restrict__ cam, float* __restrict__ lo,
                                                                     float* __restrict__ hi, float* __restrict__ zn, int32_t* __restrict__ flags) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int NI = L + 3;
    __shared__ float s_zn[ENC_MAX_L];
    __shared__ float s_nrm;
    __shared__ float s_x[ENC_THREADS * 3];
    const int64_t count = enc_count(soff, b, S);
    const bool bad = count < 0 || (!draw && inputs && count > 0 && k > count);
    const bool zero = bad || count == 0;
    const float ps[VERIFY_POSE] = {pose[VERIFY_POSE * b], pose[VERIFY_POSE * b + 1], pose[VERIFY_POSE * b + 2], pose[VERIFY_POSE * b + 3],
                                   pose[VERIFY_POSE * b + 4], pose[VERIFY_POSE * b + 5]};
    const bool pose_ok = cpl_pose_ok(ps);
    if (tid == 0) s_nrm = unit ? latent_norm(z + (int64_t)b * L, L) : 1.f;
    __syncthreads();
    if (tid < L) {
        const float v = unit ? z[(int64_t)b * L + tid] / s_nrm : z[(int64_t)b * L + tid];
        s_zn[tid] = v;
        if (blockIdx.x == 0) zn[(int64_t)b * L + tid] = v;
    }
    if (blockIdx.x == 0 && tid == 0) flags[b] = aln_rows_flags(bad, count, pose_ok);
    if (!inputs) return;
    const int64_t s0 = (int64_t)blockIdx.x * ENC_THREADS;
    const int rows = (int)((k - s0) < ENC_THREADS ? (k - s0) : ENC_THREADS);
    if (tid < rows) {
        const int64_t s = s0 + tid, i = (int64_t)b * k + s;
        float q[3] = {0.f, 0.f, 0.f}, x[3] = {0.f, 0.f, 0.f}, l = 0.f, h = 0.f;
        if (!zero) {
            const int64_t src = soff[b] + (draw ? enc_draw(seed, iter, shape0 + b, s, count) : s);
            const float* row = samples + src * ALN_ROW;
            q[0] = row[0], q[1] = row[1], q[2] = row[2], l = row[3], h = row[4];
            aln_row(q, ps, pose_ok, x, &l, &h);
        }
        cam[3 * i] = q[0], cam[3 * i + 1] = q[1], cam[3 * i + 2] = q[2];
        lo[i] = l, hi[i] = h;
        s_x[3 * tid] = x[0], s_x[3 * tid + 1] = x[1], s_x[3 * tid + 2] = x[2];
    }
    __syncthreads();
    float* out = inputs + ((int64_t)b * k + s0) * NI;
    for (int e = tid; e < rows * NI; e += ENC_THREADS) {
        const int r = e / NI, c = e - r * NI;
        out[e] = zero ? 0.f : (c < L ? s_zn[c] : s_x[3 * r + (c - L)]);
    }
}

extern "C" int sdfr_align_rows(const float* samples, int64_t S, const int64_t* soff, int B, int shape0, int64_t k, int draw, int64_t seed, int64_t iter,
                               const float* z, int L, int unit, const float* pose, float* inputs, float* cam, float* lo, float* hi, float* zn,
                               int32_t* flags, void* stream) {
    SDFR_REQUIRE(soff && z && pose && zn && flags && (!inputs || (cam && lo && hi && (samples || S == 0))), "sdfr_align_rows: NULL argument");
    SDFR_REQUIRE(L >= 1 && L <= ENC_MAX_L, "sdfr_align_rows: latent size %d outside [1,%d]", L, ENC_MAX_L);
    SDFR_REQUIRE(B >= 0 && shape0 >= 0 && (int64_t)shape0 + B <= ENC_MAX_B && S >= 0, "sdfr_align_rows: bad size (B = %d, shape0 = %d, S = %lld)", B, shape0,
                 (long long)S);
    SDFR_REQUIRE(!inputs || (k >= 1 && k <= ENC_MAX_K), "sdfr_align_rows: k = %lld outside [1,%d]", (long long)k, ENC_MAX_K);
    SDFR_REQUIRE(iter >= 0 && iter < ENC_MAX_ITER, "sdfr_align_rows: iter outside [0,2^24)");
    if (B == 0) return SDFR_OK;
    hipLaunchKernelGGL(sdfr_align_rows_kernel, dim3(inputs ? sdfr_cdiv(k, ENC_THREADS) : 1, B), dim3(ENC_THREADS), 0, (hipStream_t)stream, samples, S, soff,
                       shape0, k, draw, (uint64_t)seed, iter, z, L, unit, pose, inputs, cam, lo, hi, zn, flags);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

// ---- reduce ---------------------------------------------------------------------------------------------------------------------------------
// The interval rule on the metric prediction, and the L + 5 gradient columns of align_cells.h, in the chunk and fold kernels of
// encode_kernels.h.
struct AlnRowRule {
    const float *lo, *hi, *pose;
    __device__ EncRow operator()(float p, int64_t i, int b, float clamp) const { return cpl_row(aln_metric(p, pose + VERIFY_POSE * b), lo[i], hi[i], clamp); }
};

// The five pose columns of a row (float64 divisions and a rotation each) are formed once per row into LDS; the latent columns, one product
// each, where they are summed.
struct AlnCols {
    static constexpr int EXTRA = ALN_POSE;
    const float *pred, *J, *cam, *pose;
    int Jstride, L;
    __device__ void prepare(double* x, float w, int64_t i, int b) const {
        for (int c = 0; c < ALN_POSE; ++c) x[c] = aln_value(L + c, L, w, 0.0, 0, pred[i], J + i * Jstride, cam + 3 * i, pose + VERIFY_POSE * b);
    }
    __device__ double operator()(int c, int, float w, double e, int ok, int64_t i, int b, const double* x) const {
        if (c >= L && c < L + ALN_POSE) return x[c - L];
        return aln_value(c, L, w, e, ok, pred[i], J + i * Jstride, cam + 3 * i, pose + VERIFY_POSE * b);
    }
};

extern "C" int64_t sdfr_align_ws_bytes(int B, int64_t k, int L) { return enc_ws_bytes(B, k, L, ALN_POSE); }

extern "C" int sdfr_align_reduce(const float* pred, const float* lo, const float* hi, const float* J, int Jstride, const float* cam, const float* pose, int L,
                                 int B, int64_t k, float clamp, void* ws, int64_t ws_bytes, double* loss, double* g, int32_t* flags, void* stream) {
    return enc_reduce_launch("sdfr_align_reduce", "sdfr_align_ws_bytes", pred, AlnRowRule{lo, hi, pose}, AlnCols{pred, J, cam, pose, Jstride, L},
                             lo != nullptr && hi != nullptr && cam != nullptr && pose != nullptr, J, Jstride, L + 3, L, ALN_POSE, B, k, clamp, ws, ws_bytes,
                             loss, g, flags, stream);
}

// ---- step -----------------------------------------------------------------------------------------------------------------------------------
// grid (B), one workgroup per shape.  Thread 0 walks the latent once in index order (norm, projection, the finite checks, the scale the
// update would leave); then thread i updates latent element i and thread 0 the pose and the next pose row.  A skipped shape keeps
// everything and gets ENC_SKIPPED.
struct AlnRates {
    float lr[ALN_POSE];
};

__global__ __launch_bounds__(ENC_THREADS) void sdfr_align_step_kernel(float* __restrict__ z, float* __restrict__ m, float* __restrict__ v, int L, int unit,
                                                                     float* __restrict__ theta, float* __restrict__ tm, float* __restrict__ tv,
                                                                     float* __restrict__ pose, const double* __restrict__ g,
                                                                     const double* __restrict__ loss, int32_t* __restrict__ flags, float code_reg,
                                                                     float lr, AlnRates rates, float bc1, float bc2, float* __restrict__ history_row) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int G = L + ALN_POSE;
    __shared__ float s_g[ENC_MAX_L];
    __shared__ float s_nrm, s_dot, s_nz;
    __shared__ int s_skip;
    float* zb = z + (int64_t)b * L;
    const double* gb = g + (int64_t)b * G;
    if (tid < L) s_g[tid] = (float)gb[tid];
    __syncthreads();
    if (tid == 0) {
        const int fl = flags[b];
        const float nrm = unit ? latent_norm(zb, L) : 1.f;
        const float dot = unit ? latent_unit_dot(zb, s_g, L, nrm) : 0.f;
        const float nz = unit ? 0.f : enc_raw_norm(zb, L);
        int skip = (fl & (ENC_EMPTY | ENC_NO_ROWS | ENC_BAD_TABLE | ALN_BAD_POSE)) ? 1 : 0;
        for (int i = 0; i < L; ++i)
            if (!isfinite(enc_step_grad(zb[i], s_g[i], unit, nrm, dot, nz, code_reg))) skip = 1;
        if (!aln_pose_grad_ok(gb, L)) skip = 1;
        const float sc = aln_scale_after(theta + ALN_POSE * b, tm + ALN_POSE * b, tv + ALN_POSE * b, gb, L, rates.lr[4], bc1, bc2);
        if (!(isfinite(sc) && sc > 0.f)) skip = 1;
        s_nrm = nrm; s_dot = dot; s_nz = nz; s_skip = skip;
        if (skip) flags[b] = fl | ENC_SKIPPED;
        if (history_row) history_row[b] = (float)loss[b];
    }
    __syncthreads();
    if (s_skip) return;
    if (tid < L && lr != 0.f) {
        const float gi = enc_step_grad(zb[tid], s_g[tid], unit, s_nrm, s_dot, s_nz, code_reg);
        latent_adam(&zb[tid], &m[(int64_t)b * L + tid], &v[(int64_t)b * L + tid], gi, lr, bc1, bc2);
    }
    if (tid == 0) aln_pose_step(theta + ALN_POSE * b, tm + ALN_POSE * b, tv + ALN_POSE * b, gb, L, rates.lr, bc1, bc2, pose + VERIFY_POSE * b);
}

extern "C" int sdfr_align_step(float* z, float* m, float* v, int L, int B, int unit, float* theta, float* tm, float* tv, float* pose, const double* g,
                               const double* loss, int32_t* flags, float code_reg, float lr, const float* lr_pose, int t, float* history,
                               int64_t history_stride, void* stream) {
    SDFR_REQUIRE(z && m && v && theta && tm && tv && pose && g && loss && flags && lr_pose, "sdfr_align_step: NULL argument");
    SDFR_REQUIRE(L >= 1 && L <= ENC_MAX_L && B >= 0 && B <= ENC_MAX_B, "sdfr_align_step: bad size (L = %d, B = %d)", L, B);
    SDFR_REQUIRE(t >= 1 && t <= ENC_MAX_ITER, "sdfr_align_step: the step count t = %d starts at 1", t);
    SDFR_REQUIRE(!history || history_stride >= B, "sdfr_align_step: history_stride %lld below B = %d", (long long)history_stride, B);
    AlnRates rates;
    bool finite = isfinite(lr) && isfinite(code_reg);
    for (int i = 0; i < ALN_POSE; ++i) {
        rates.lr[i] = lr_pose[i];
        finite = finite && isfinite(lr_pose[i]);
    }
    SDFR_REQUIRE(finite, "sdfr_align_step: non-finite learning rate or regulariser");
    if (B == 0) return SDFR_OK;
    float bc1, bc2;
    enc_bias(t, &bc1, &bc2);
    hipLaunchKernelGGL(sdfr_align_step_kernel, dim3(B), dim3(ENC_THREADS), 0, (hipStream_t)stream, z, m, v, L, unit, theta, tm, tv, pose, g, loss, flags,
                       code_reg, lr, rates, bc1, bc2, history ? history + (int64_t)(t - 1) * history_stride : (float*)nullptr);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
