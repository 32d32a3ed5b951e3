// Encoding shapes under a frozen decoder (DeepSDF's "reconstruct"): everything of one iteration of the batched latent fit that is not the
// decoder itself.  sdfr_encode_rows draws the iteration's rows and writes the decoder's inputs; sdfr_encode_reduce turns the decoder's values
// and the latent columns of its Jacobian into one clamped-L1 loss and one latent gradient per shape; sdfr_encode_step takes the gradient
// through the unit normalisation and applies Adam.  The per-element rules and THE summation order are csrc/encode_cells.h.
// No atomics, no memset, no host synchronisation; the same bits on every run; a shape's results do not depend on B or on its place in the
// batch.  Compiled with -ffp-contract=off: every float64 and float32 operation is rounded on its own.
#include "sdfr_common.h"
#include "encode_cells.h"

#define ENC_THREADS 256

// grid (ceil(k / 256), B) -- or (1, B) without inputs: zn and flags only.  A workgroup writes 256 rows of one shape: the sample of each row
// goes to LDS first, then the [256][L + 3] block is written element by element (consecutive threads, consecutive words).
__global__ __launch_bounds__(ENC_THREADS) void sdfr_encode_rows_kernel(const float* __restrict__ samples, int64_t S, const int64_t* __restrict__ soff,
                                                                      int shape0, int64_t k, int draw, uint64_t seed, int64_t iter,
                                                                      const float* __restrict__ z, int L, int unit, float* __restrict__ inputs,
                                                                      float* __restrict__ target, float* __restrict__ zn,
                                                                      int32_t* __restrict__ flags) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int NI = L + 3;
    __shared__ float s_zn[ENC_MAX_L];
    __shared__ float s_nrm;
    __shared__ int64_t s_src[ENC_THREADS];
    const int64_t count = enc_count(soff, b, S);
    const bool bad = count < 0 || (!draw && inputs && count > 0 && k > count);
    const bool zero = bad || count == 0;
    if (tid == 0) s_nrm = unit ? latent_norm(z + (int64_t)b * L, L) : 1.f;
    __syncthreads();
    if (tid < L) {
        const float v = unit ? z[(int64_t)b * L + tid] / s_nrm : z[(int64_t)b * L + tid];
        s_zn[tid] = v;
        if (blockIdx.x == 0) zn[(int64_t)b * L + tid] = v;
    }
    if (blockIdx.x == 0 && tid == 0) flags[b] = bad ? ENC_BAD_TABLE : (count == 0 ? ENC_EMPTY : 0);
    if (!inputs) return;
    const int64_t s0 = (int64_t)blockIdx.x * ENC_THREADS;
    const int rows = (int)((k - s0) < ENC_THREADS ? (k - s0) : ENC_THREADS);
    if (tid < rows) {
        const int64_t s = s0 + tid;
        const int64_t src = zero ? -1 : soff[b] + (draw ? enc_draw(seed, iter, shape0 + b, s, count) : s);
        s_src[tid] = src;
        target[(int64_t)b * k + s] = zero ? 0.f : samples[src * 4 + 3];
    }
    __syncthreads();
    float* out = inputs + ((int64_t)b * k + s0) * NI;
    for (int e = tid; e < rows * NI; e += ENC_THREADS) {
        const int r = e / NI, c = e - r * NI;
        float v;
        if (zero) v = 0.f;
        else if (c < L) v = s_zn[c];
        else v = samples[s_src[r] * 4 + (c - L)];
        out[e] = v;
    }
}

extern "C" int sdfr_encode_rows(const float* samples, int64_t S, const int64_t* soff, int B, int shape0, int64_t k, int draw, int64_t seed, int64_t iter,
                                const float* z, int L, int unit, float* inputs, float* target, float* zn, int32_t* flags, void* stream) {
    SDFR_REQUIRE(soff && z && zn && flags && (!inputs || (target && (samples || S == 0))), "sdfr_encode_rows: NULL argument");
    SDFR_REQUIRE(L >= 1 && L <= ENC_MAX_L, "sdfr_encode_rows: latent size %d outside [1,%d]", L, ENC_MAX_L);
    SDFR_REQUIRE(B >= 0 && shape0 >= 0 && (int64_t)shape0 + B <= ENC_MAX_B && S >= 0, "sdfr_encode_rows: bad size (B = %d, shape0 = %d, S = %lld)", B, shape0,
                 (long long)S);
    SDFR_REQUIRE(!inputs || (k >= 1 && k <= ENC_MAX_K), "sdfr_encode_rows: k = %lld outside [1,%d]", (long long)k, ENC_MAX_K);
    SDFR_REQUIRE(iter >= 0 && iter < ENC_MAX_ITER, "sdfr_encode_rows: iter outside [0,2^24)");
    if (B == 0) return SDFR_OK;
    hipLaunchKernelGGL(sdfr_encode_rows_kernel, dim3(inputs ? sdfr_cdiv(k, ENC_THREADS) : 1, B), dim3(ENC_THREADS), 0, (hipStream_t)stream, samples, S,
                       soff, shape0, k, draw, (uint64_t)seed, iter, z, L, unit, inputs, target, zn, flags);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

// ---- reduce ---------------------------------------------------------------------------------------------------------------------------------
// grid (chunks, B): one workgroup sums one chunk of ENC_CHUNK rows of one shape into part[b][chunk][L + 2], in the order of encode_cells.h.
// The rows' weights go to LDS once; then, ENC_COLS columns at a time, accumulator (slot j, column c) belongs to thread j ncols + c, so the
// threads of a wave read consecutive words of a row of J.
__global__ __launch_bounds__(ENC_THREADS) void sdfr_encode_chunk_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                       const float* __restrict__ J, int Jstride, int L, int64_t k, float clamp,
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
    for (int r = tid; r < n; r += ENC_THREADS) {
        const EncRow q = enc_row(pred[base + r], target[base + r], clamp);
        s_e[r] = q.e; s_w[r] = q.w; s_ok[r] = (unsigned char)q.ok;
    }
    __syncthreads();
    const int NC = L + 2;
    double* out = part + ((int64_t)b * chunks + ch) * NC;
    for (int c0 = 0; c0 < NC; c0 += ENC_COLS) {
        const int nc = (NC - c0) < ENC_COLS ? (NC - c0) : ENC_COLS;
        for (int e = tid; e < ENC_SLOTS * nc; e += ENC_THREADS) {
            const int j = e / nc, c = c0 + (e - j * nc);
            double a = 0.0;
            ENC_SLOT_ROWS(r, j, n) a += enc_value(c, L, s_w[r], s_e[r], s_ok[r], J + (base + r) * Jstride);
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
__global__ __launch_bounds__(64) void sdfr_encode_fold_kernel(const double* __restrict__ part, int64_t chunks, int L, double* __restrict__ loss,
                                                             double* __restrict__ g_zn, int32_t* __restrict__ flags) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int NC = L + 2;
    __shared__ double s_tot[ENC_MAX_L + 2];
    for (int c = tid; c < NC; c += 64) {
        double a = 0.0;
        for (int64_t ch = 0; ch < chunks; ++ch) a += part[((int64_t)b * chunks + ch) * NC + c];
        s_tot[c] = a;
    }
    __syncthreads();
    const double n_ok = s_tot[L + 1];
    for (int c = tid; c < L; c += 64) g_zn[(int64_t)b * L + c] = enc_mean(s_tot[c], n_ok);
    if (tid == 0) {
        loss[b] = enc_mean(s_tot[L], n_ok);
        if (!(n_ok > 0.0)) flags[b] |= ENC_NO_ROWS;
    }
}

extern "C" int64_t sdfr_encode_ws_bytes(int B, int64_t k, int L) {
    if (B < 0 || B > ENC_MAX_B || k < 1 || k > ENC_MAX_K || L < 1 || L > ENC_MAX_L) return -1;
    return (int64_t)B * enc_chunks(k) * (L + 2) * (int64_t)sizeof(double);
}

extern "C" int sdfr_encode_reduce(const float* pred, const float* target, const float* J, int Jstride, int L, int B, int64_t k, float clamp, void* ws,
                                  int64_t ws_bytes, double* loss, double* g_zn, int32_t* flags, void* stream) {
    SDFR_REQUIRE(pred && target && J && ws && loss && g_zn && flags, "sdfr_encode_reduce: NULL argument");
    SDFR_REQUIRE(L >= 1 && L <= ENC_MAX_L && Jstride >= L, "sdfr_encode_reduce: latent size %d outside [1,%d] or beyond the row stride %d", L, ENC_MAX_L,
                 Jstride);
    SDFR_REQUIRE(B >= 0 && B <= ENC_MAX_B && k >= 1 && k <= ENC_MAX_K, "sdfr_encode_reduce: bad size (B = %d, k = %lld)", B, (long long)k);
    SDFR_REQUIRE(clamp > 0.f, "sdfr_encode_reduce: clamp must be positive");
    SDFR_REQUIRE(ws_bytes >= sdfr_encode_ws_bytes(B, k, L), "sdfr_encode_reduce: the workspace holds %lld bytes, sdfr_encode_ws_bytes asks for %lld",
                 (long long)ws_bytes, (long long)sdfr_encode_ws_bytes(B, k, L));
    SDFR_REQUIRE(((uintptr_t)ws & 7) == 0, "sdfr_encode_reduce: the workspace must be aligned to 8 bytes");
    if (B == 0) return SDFR_OK;
    const int64_t chunks = enc_chunks(k);
    hipLaunchKernelGGL(sdfr_encode_chunk_kernel, dim3((unsigned)chunks, B), dim3(ENC_THREADS), 0, (hipStream_t)stream, pred, target, J, Jstride, L, k,
                       clamp, (double*)ws);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_encode_fold_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const double*)ws, chunks, L, loss, g_zn, flags);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
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
