// The kernels of the frozen-decoder fits (encode.hip: exact targets; complete.hip: interval targets; align.hip: interval targets and a
// pose), each ONCE, over the policy structs of the cells headers: the observation rows of a view (with a pose or without), the iteration's
// rows over a row policy, the reduce -- the chunk kernel over a row rule and a column rule, and the fold, whose summation order is
// encode_cells.h's -- and the step over a pose policy.  Each comes with the launch that holds its argument checks; `name` is the entry
// point's.  Device code only; a translation unit that includes it is compiled with -ffp-contract=off.
#pragma once
#include "sdfr_common.h"
#include "align_cells.h"

#define ENC_MAX_G (ENC_MAX_L + ALN_POSE)   // gradient columns of a reduce at the most: the latent's and the five of a pose

// ---- samples --------------------------------------------------------------------------------------------------------------------------------
// One point per thread: thread g < N writes the P = 3 + F rows of point g, thread g < B the flag word of shape g.  POSED: lattice-frame
// rows through pose[b] (cpl_view_row); else camera-frame rows (aln_sample_row), and `pose` is not read.
template <bool POSED>
__global__ __launch_bounds__(ENC_THREADS) void enc_samples_kernel(const float* __restrict__ points, const double* __restrict__ normals, int64_t N,
                                                                 const int64_t* __restrict__ ptoff, int B, const float* __restrict__ pose,
                                                                 const float* __restrict__ origin, int shape0, int F, double eta, double s_max,
                                                                 uint64_t seed, float* __restrict__ rows, int32_t* __restrict__ flags) {
    const int64_t g = (int64_t)blockIdx.x * ENC_THREADS + threadIdx.x;
    if (g < B) flags[g] = POSED ? cpl_view_flags(ptoff, pose, (int)g, N) : (cpl_table_ok(ptoff, (int)g, N) ? 0 : CPL_BAD_TABLE);
    if (g >= N) return;
    const int b = cpl_owner(ptoff, B, N, g), bb = b < 0 ? 0 : b;
    const float org[3] = {origin[0], origin[1], origin[2]};
    const double* n = normals ? normals + 3 * g : nullptr;
    const int64_t i = b < 0 ? 0 : g - ptoff[b];
    float* out = rows + (int64_t)CPL_ROW * (3 + F) * g;
    if (POSED)
        cpl_view_row(points + 3 * g, n, pose + VERIFY_POSE * bb, org, b >= 0 && cpl_pose_ok(pose + VERIFY_POSE * bb), seed, shape0 + bb, i, F, eta, s_max, out);
    else
        aln_sample_row(points + 3 * g, n, org, b >= 0, seed, shape0 + bb, i, F, eta, s_max, out);
}

template <bool POSED>
static int enc_samples_launch(const char* name, const float* points, const double* normals, int64_t N, const int64_t* ptoff, int B, const float* pose,
                              const float* origin, int shape0, int F, float eta, float s_max, int64_t seed, float* rows, int32_t* flags, void* stream) {
    SDFR_REQUIRE(B >= 0 && N >= 0 && shape0 >= 0 && (int64_t)shape0 + B <= ENC_MAX_B, "%s: bad size (B = %d, N = %lld, shape0 = %d)", name, B, (long long)N,
                 shape0);
    SDFR_REQUIRE(F >= 0 && F <= CPL_MAX_FREE, "%s: F = %d free-space rows outside [0,%d]", name, F, CPL_MAX_FREE);
    SDFR_REQUIRE(isfinite(eta) && isfinite(s_max) && s_max >= 0.f, "%s: eta must be finite and s_max finite and not negative", name);
    SDFR_REQUIRE(N <= ((int64_t)1 << 32), "%s: at most 2^32 points", name);
    if (B == 0 && N == 0) return SDFR_OK;
    SDFR_REQUIRE(ptoff && (pose || !POSED) && origin && flags && (N == 0 || (points && rows)) && B >= 1, "%s: NULL argument, or points without a shape", name);
    const int64_t threads = N > B ? N : (int64_t)B;
    hipLaunchKernelGGL(enc_samples_kernel<POSED>, dim3((unsigned)((threads + ENC_THREADS - 1) / ENC_THREADS)), dim3(ENC_THREADS), 0, (hipStream_t)stream,
                       points, normals, N, ptoff, B, pose, origin, shape0, F, (double)eta, (double)s_max, (uint64_t)seed, rows, flags);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

// ---- rows -----------------------------------------------------------------------------------------------------------------------------------
// grid (ceil(k / 256), B) -- or (1, B) without inputs: zn and flags only.  A workgroup writes 256 rows of one shape: thread tid draws row
// s0 + tid, the row policy stores its side arrays and says what goes to LDS (the sample's index, or the position under the pose); then the
// [256][L + 3] block is written element by element (consecutive threads, consecutive words).  Workgroup b draws from the samples of shape
// b, unless the policy has an owner(): then from that shape's (search_cells.h: many starts on one shape's samples; -1: none, which counts
// as a broken table entry), while z, the policy's own arrays and every output stay indexed by b.
template <class Rows>
__host__ __device__ __forceinline__ auto enc_rows_owner(const Rows& rows, int b, int) -> decltype(rows.owner(b)) { return rows.owner(b); }
template <class Rows>
__host__ __device__ __forceinline__ int enc_rows_owner(const Rows&, int b, long) { return b; }

template <class Rows>
__global__ __launch_bounds__(ENC_THREADS) void enc_rows_kernel(const float* __restrict__ samples, int64_t S, const int64_t* __restrict__ soff, int shape0,
                                                              int64_t k, int draw, uint64_t seed, int64_t iter, const float* __restrict__ z, int L,
                                                              int unit, Rows rows, float* __restrict__ inputs, float* __restrict__ zn,
                                                              int32_t* __restrict__ flags) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int NI = L + 3;
    __shared__ float s_zn[ENC_MAX_L];
    __shared__ float s_nrm;
    __shared__ typename Rows::Staged s_row[ENC_THREADS];
    const int own = enc_rows_owner(rows, b, 0);
    const int64_t count = own < 0 ? -1 : enc_count(soff, own, S);
    const bool bad = count < 0 || (!draw && inputs && count > 0 && k > count);
    const bool zero = bad || count == 0;
    const typename Rows::Shape shape = rows.shape(b);
    if (tid == 0) s_nrm = unit ? latent_norm(z + (int64_t)b * L, L) : 1.f;
    __syncthreads();
    if (tid < L) {
        const float v = unit ? z[(int64_t)b * L + tid] / s_nrm : z[(int64_t)b * L + tid];
        s_zn[tid] = v;
        if (blockIdx.x == 0) zn[(int64_t)b * L + tid] = v;
    }
    if (blockIdx.x == 0 && tid == 0) flags[b] = rows.flags(shape, bad, count);
    if (!inputs) return;
    const int64_t s0 = (int64_t)blockIdx.x * ENC_THREADS;
    const int n = (int)((k - s0) < ENC_THREADS ? (k - s0) : ENC_THREADS);
    if (tid < n) {
        const int64_t s = s0 + tid;
        const int64_t src = zero ? -1 : soff[own] + (draw ? enc_draw(seed, iter, shape0 + own, s, count) : s);
        s_row[tid] = rows.stage(shape, samples, src, (int64_t)b * k + s);
    }
    __syncthreads();
    float* out = inputs + ((int64_t)b * k + s0) * NI;
    for (int e = tid; e < n * NI; e += ENC_THREADS) {
        const int r = e / NI, c = e - r * NI;
        out[e] = zero ? 0.f : (c < L ? s_zn[c] : rows.xyz(samples, s_row[r], c - L));
    }
}

// `always_ok`: what the policy reads on every call is not NULL; `sides_ok`: its side arrays are not
template <class Rows>
static int enc_rows_launch(const char* name, const float* samples, int64_t S, const int64_t* soff, int B, int shape0, int64_t k, int draw, int64_t seed,
                           int64_t iter, const float* z, int L, int unit, Rows rows, bool always_ok, bool sides_ok, float* inputs, float* zn,
                           int32_t* flags, void* stream) {
    SDFR_REQUIRE(soff && z && always_ok && zn && flags && (!inputs || (sides_ok && (samples || S == 0))), "%s: NULL argument", name);
    SDFR_REQUIRE(L >= 1 && L <= ENC_MAX_L, "%s: latent size %d outside [1,%d]", name, L, ENC_MAX_L);
    SDFR_REQUIRE(B >= 0 && shape0 >= 0 && (int64_t)shape0 + B <= ENC_MAX_B && S >= 0, "%s: bad size (B = %d, shape0 = %d, S = %lld)", name, B, shape0,
                 (long long)S);
    SDFR_REQUIRE(!inputs || (k >= 1 && k <= ENC_MAX_K), "%s: k = %lld outside [1,%d]", name, (long long)k, ENC_MAX_K);
    SDFR_REQUIRE(iter >= 0 && iter < ENC_MAX_ITER, "%s: iter outside [0,2^24)", name);
    if (B == 0) return SDFR_OK;
    hipLaunchKernelGGL(enc_rows_kernel<Rows>, dim3(inputs ? sdfr_cdiv(k, ENC_THREADS) : 1, B), dim3(ENC_THREADS), 0, (hipStream_t)stream, samples, S, soff,
                       shape0, k, draw, (uint64_t)seed, iter, z, L, unit, rows, inputs, zn, flags);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

// ---- reduce ---------------------------------------------------------------------------------------------------------------------------------
// grid (chunks, B): one workgroup sums one chunk of ENC_CHUNK rows of one shape into part[b][chunk][G + 2], in the order of encode_cells.h,
// over a row rule and a column rule (the cells headers).  The rows' weights go to LDS once; then, ENC_COLS columns at a time, accumulator
// (slot j, column c) belongs to thread j ncols + c, so the threads of a wave read consecutive words of a row of J.
template <class Rule, class Cols>
__global__ __launch_bounds__(ENC_THREADS) void enc_chunk_kernel(const float* __restrict__ pred, Rule rule, Cols cols, int G, int64_t k, float clamp,
                                                               double* __restrict__ part) {
    const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
    const int64_t chunks = gridDim.x;
    const int64_t row0 = (int64_t)ch * ENC_CHUNK;
    const int n = (int)((k - row0) < ENC_CHUNK ? (k - row0) : ENC_CHUNK);
    const int64_t base = (int64_t)b * k + row0;
    __shared__ double s_e[ENC_CHUNK];
    __shared__ float s_w[ENC_CHUNK];
    __shared__ unsigned char s_ok[ENC_CHUNK];
    __shared__ double s_acc[ENC_SLOTS * (ENC_COLS + 1)];
    __shared__ double s_x[Cols::EXTRA ? ENC_CHUNK * Cols::EXTRA : 1];
    for (int r = tid; r < n; r += ENC_THREADS) {
        const EncRow q = rule(pred[base + r], base + r, b, clamp);
        s_e[r] = q.e; s_w[r] = q.w; s_ok[r] = (unsigned char)q.ok;
        cols.prepare(s_x + r * Cols::EXTRA, q.w, base + r, b);
    }
    __syncthreads();
    const int NC = G + 2;
    double* out = part + ((int64_t)b * chunks + ch) * NC;
    for (int c0 = 0; c0 < NC; c0 += ENC_COLS) {
        const int nc = (NC - c0) < ENC_COLS ? (NC - c0) : ENC_COLS;
        for (int e = tid; e < ENC_SLOTS * nc; e += ENC_THREADS) {
            const int j = e / nc, c = c0 + (e - j * nc);
            double a = 0.0;
            ENC_SLOT_ROWS(r, j, n) a += cols(c, G, s_w[r], s_e[r], s_ok[r], base + r, b, s_x + r * Cols::EXTRA);
            s_acc[j * (ENC_COLS + 1) + (c - c0)] = a;
        }
        __syncthreads();
        for (int o = ENC_SLOTS / 2; o > 0; o >>= 1) {
            for (int e = tid; e < o * nc; e += ENC_THREADS) {
                const int j = e / nc, cc = e - j * nc;
                enc_tree_step(s_acc + cc, ENC_COLS + 1, j, o);
            }
            __syncthreads();
        }
        if (tid < nc) out[c0 + tid] = s_acc[tid];
        __syncthreads();
    }
}

// grid (B): the chunk sums in chunk order, the means, bit 1 of the flags
static __global__ __launch_bounds__(64) void enc_fold_kernel(const double* __restrict__ part, int64_t chunks, int G, double* __restrict__ loss,
                                                            double* __restrict__ g_zn, int32_t* __restrict__ flags) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int NC = G + 2;
    __shared__ double s_tot[ENC_MAX_G + 2];
    for (int c = tid; c < NC; c += 64) {
        double a = 0.0;
        for (int64_t ch = 0; ch < chunks; ++ch) a += part[((int64_t)b * chunks + ch) * NC + c];
        s_tot[c] = a;
    }
    __syncthreads();
    const double n_ok = s_tot[G + 1];
    for (int c = tid; c < G; c += 64) g_zn[(int64_t)b * G + c] = enc_mean(s_tot[c], n_ok);
    if (tid == 0) {
        loss[b] = enc_mean(s_tot[G], n_ok);
        if (!(n_ok > 0.0)) flags[b] |= ENC_NO_ROWS;
    }
}

// bytes of the partial sums of a reduce with `extra` gradient columns beyond the latent's (0: the latent fits; -1: sizes the kernels refuse)
static inline int64_t enc_ws_bytes(int B, int64_t k, int L, int extra = 0) {
    if (B < 0 || B > ENC_MAX_B || k < 1 || k > ENC_MAX_K || L < 1 || L > ENC_MAX_L) return -1;
    return (int64_t)B * enc_chunks(k) * (L + extra + 2) * (int64_t)sizeof(double);
}

// the argument checks and the two launches of a reduce over G = L + extra gradient columns; `targets_ok`: the rules' own pointers are not
// NULL; J has at least `need` words a row; `ws_name` is the entry point that gives the workspace's size
template <class Rule, class Cols>
static int enc_reduce_launch(const char* name, const char* ws_name, const float* pred, Rule rule, Cols cols, bool targets_ok, const float* J, int Jstride,
                             int need, int L, int extra, int B, int64_t k, float clamp, void* ws, int64_t ws_bytes, double* loss, double* g,
                             int32_t* flags, void* stream) {
    SDFR_REQUIRE(pred && targets_ok && J && ws && loss && g && flags, "%s: NULL argument", name);
    SDFR_REQUIRE(L >= 1 && L <= ENC_MAX_L && Jstride >= need, "%s: latent size %d outside [1,%d] or beyond the row stride %d", name, L, ENC_MAX_L, Jstride);
    SDFR_REQUIRE(B >= 0 && B <= ENC_MAX_B && k >= 1 && k <= ENC_MAX_K, "%s: bad size (B = %d, k = %lld)", name, B, (long long)k);
    SDFR_REQUIRE(clamp > 0.f, "%s: clamp must be positive", name);
    SDFR_REQUIRE(ws_bytes >= enc_ws_bytes(B, k, L, extra), "%s: the workspace holds %lld bytes, %s asks for %lld", name, (long long)ws_bytes, ws_name,
                 (long long)enc_ws_bytes(B, k, L, extra));
    SDFR_REQUIRE(((uintptr_t)ws & 7) == 0, "%s: the workspace must be aligned to 8 bytes", name);
    if (B == 0) return SDFR_OK;
    const int64_t chunks = enc_chunks(k);
    hipLaunchKernelGGL((enc_chunk_kernel<Rule, Cols>), dim3((unsigned)chunks, B), dim3(ENC_THREADS), 0, (hipStream_t)stream, pred, rule, cols, L + extra, k,
                       clamp, (double*)ws);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(enc_fold_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const double*)ws, chunks, L + extra, loss, g, flags);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

// the latent fits' reduce: the latent columns of J
template <class Rule>
static int enc_reduce_launch(const char* name, const float* pred, Rule rule, bool targets_ok, const float* J, int Jstride, int L, int B, int64_t k,
                             float clamp, void* ws, int64_t ws_bytes, double* loss, double* g_zn, int32_t* flags, void* stream) {
    return enc_reduce_launch(name, "sdfr_encode_ws_bytes", pred, rule, EncLatentCols{J, Jstride}, targets_ok, J, Jstride, L, L, 0, B, k, clamp, ws, ws_bytes,
                             loss, g_zn, flags, stream);
}

// ---- step -----------------------------------------------------------------------------------------------------------------------------------
// grid (B), one workgroup per shape; g has L + Pose::EXTRA columns a shape.  Thread 0 walks the latent once in index order (norm,
// projection, the finite check) and asks the pose policy; then thread i updates latent element i and thread 0 steps the pose.  A shape
// that is flagged, whose gradient is not finite or that the policy refuses keeps everything and gets ENC_SKIPPED.
template <class Pose>
__global__ __launch_bounds__(ENC_THREADS) void enc_step_kernel(float* __restrict__ z, float* __restrict__ m, float* __restrict__ v, int L, int unit, Pose pose,
                                                              const double* __restrict__ g, const double* __restrict__ loss,
                                                              int32_t* __restrict__ flags, float code_reg, float lr, float bc1, float bc2,
                                                              float* __restrict__ history_row) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ float s_g[ENC_MAX_L];
    __shared__ float s_nrm, s_dot, s_nz;
    __shared__ int s_skip;
    float* zb = z + (int64_t)b * L;
    const double* gb = g + (int64_t)b * (L + Pose::EXTRA);
    if (tid < L) s_g[tid] = (float)gb[tid];
    __syncthreads();
    if (tid == 0) {
        const int fl = flags[b];
        const float nrm = unit ? latent_norm(zb, L) : 1.f;
        const float dot = unit ? latent_unit_dot(zb, s_g, L, nrm) : 0.f;
        const float nz = unit ? 0.f : enc_raw_norm(zb, L);
        int skip = (fl & Pose::SKIP) ? 1 : 0;
        for (int i = 0; i < L; ++i)
            if (!isfinite(enc_step_grad(zb[i], s_g[i], unit, nrm, dot, nz, code_reg))) skip = 1;
        if (!pose.ok(b, gb, L, bc1, bc2)) skip = 1;
        s_nrm = nrm; s_dot = dot; s_nz = nz; s_skip = skip;
        if (skip) flags[b] = fl | ENC_SKIPPED;
        if (history_row) history_row[b] = (float)loss[b];
    }
    __syncthreads();
    if (s_skip) return;
    if (tid < L && pose.steps_latent(lr)) {
        const float gi = enc_step_grad(zb[tid], s_g[tid], unit, s_nrm, s_dot, s_nz, code_reg);
        latent_adam(&zb[tid], &m[(int64_t)b * L + tid], &v[(int64_t)b * L + tid], gi, lr, bc1, bc2);
    }
    if (tid == 0) pose.step(b, gb, L, bc1, bc2);
}

// `pose_ok`: the policy's pointers are not NULL; `rates_finite`: its learning rates are finite
template <class Pose>
static int enc_step_launch(const char* name, float* z, float* m, float* v, int L, int B, int unit, Pose pose, bool pose_ok, bool rates_finite, const double* g,
                           const double* loss, int32_t* flags, float code_reg, float lr, int t, float* history, int64_t history_stride, void* stream) {
    SDFR_REQUIRE(z && m && v && pose_ok && g && loss && flags, "%s: NULL argument", name);
    SDFR_REQUIRE(L >= 1 && L <= ENC_MAX_L && B >= 0 && B <= ENC_MAX_B, "%s: bad size (L = %d, B = %d)", name, L, B);
    SDFR_REQUIRE(t >= 1 && t <= ENC_MAX_ITER, "%s: the step count t = %d starts at 1", name, t);
    SDFR_REQUIRE(!history || history_stride >= B, "%s: history_stride %lld below B = %d", name, (long long)history_stride, B);
    SDFR_REQUIRE(isfinite(lr) && isfinite(code_reg) && rates_finite, "%s: non-finite learning rate or regulariser", name);
    if (B == 0) return SDFR_OK;
    float bc1, bc2;
    enc_bias(t, &bc1, &bc2);
    hipLaunchKernelGGL(enc_step_kernel<Pose>, dim3(B), dim3(ENC_THREADS), 0, (hipStream_t)stream, z, m, v, L, unit, pose, g, loss, flags, code_reg, lr, bc1, bc2,
                       history ? history + (int64_t)(t - 1) * history_stride : (float*)nullptr);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
