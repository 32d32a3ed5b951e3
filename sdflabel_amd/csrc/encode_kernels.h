// The kernels the frozen-decoder fits share (encode.hip: exact targets; complete.hip: interval targets; align.hip: interval targets and a
// pose): the iteration's rows for samples of W floats, and THE ONE COPY of the reduce -- the chunk kernel over a row rule and a column rule,
// and the fold -- whose summation order is encode_cells.h's.
// Device code only; a translation unit that includes it is compiled with -ffp-contract=off.
#pragma once
#include "sdfr_common.h"
#include "encode_cells.h"

#define ENC_THREADS 256
#define ENC_MAX_G (ENC_MAX_L + 5)          // gradient columns of a reduce at the most: the latent's and the five of a pose (align.hip)

// grid (ceil(k / 256), B) -- or (1, B) without inputs: zn and flags only.  A workgroup writes 256 rows of one shape: the sample of each row
// goes to LDS first, then the [256][L + 3] block is written element by element (consecutive threads, consecutive words).  Samples are
// [S][W] = x y z and W - 3 target words: word 3 goes to t0, word 4 (W = 5) to t1.
template <int W>
__global__ __launch_bounds__(ENC_THREADS) void enc_rows_kernel(const float* __restrict__ samples, int64_t S, const int64_t* __restrict__ soff, int shape0,
                                                              int64_t k, int draw, uint64_t seed, int64_t iter, const float* __restrict__ z, int L,
                                                              int unit, float* __restrict__ inputs, float* __restrict__ t0, float* __restrict__ t1,
                                                              float* __restrict__ zn, int32_t* __restrict__ flags) {
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
        t0[(int64_t)b * k + s] = zero ? 0.f : samples[src * W + 3];
        if (W == 5) t1[(int64_t)b * k + s] = zero ? 0.f : samples[src * W + 4];
    }
    __syncthreads();
    float* out = inputs + ((int64_t)b * k + s0) * NI;
    for (int e = tid; e < rows * NI; e += ENC_THREADS) {
        const int r = e / NI, c = e - r * NI;
        float v;
        if (zero) v = 0.f;
        else if (c < L) v = s_zn[c];
        else v = samples[s_src[r] * W + (c - L)];
        out[e] = v;
    }
}

// the argument checks and the launch of enc_rows_kernel<W>; `name` is the entry point's
template <int W>
static int enc_rows_launch(const char* name, const float* samples, int64_t S, const int64_t* soff, int B, int shape0, int64_t k, int draw, int64_t seed,
                           int64_t iter, const float* z, int L, int unit, float* inputs, float* t0, float* t1, float* zn, int32_t* flags, void* stream) {
    SDFR_REQUIRE(soff && z && zn && flags && (!inputs || (t0 && (W == 4 || t1) && (samples || S == 0))), "%s: NULL argument", name);
    SDFR_REQUIRE(L >= 1 && L <= ENC_MAX_L, "%s: latent size %d outside [1,%d]", name, L, ENC_MAX_L);
    SDFR_REQUIRE(B >= 0 && shape0 >= 0 && (int64_t)shape0 + B <= ENC_MAX_B && S >= 0, "%s: bad size (B = %d, shape0 = %d, S = %lld)", name, B, shape0,
                 (long long)S);
    SDFR_REQUIRE(!inputs || (k >= 1 && k <= ENC_MAX_K), "%s: k = %lld outside [1,%d]", name, (long long)k, ENC_MAX_K);
    SDFR_REQUIRE(iter >= 0 && iter < ENC_MAX_ITER, "%s: iter outside [0,2^24)", name);
    if (B == 0) return SDFR_OK;
    hipLaunchKernelGGL(enc_rows_kernel<W>, dim3(inputs ? sdfr_cdiv(k, ENC_THREADS) : 1, B), dim3(ENC_THREADS), 0, (hipStream_t)stream, samples, S, soff,
                       shape0, k, draw, (uint64_t)seed, iter, z, L, unit, inputs, t0, t1, zn, flags);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

// ---- reduce ---------------------------------------------------------------------------------------------------------------------------------
// A row rule gives the EncRow of row i (an index into the [B k] arrays) of shape b from its prediction: the exact rule reads one target, the
// interval rule two bounds.  A column rule gives the value of column c < G + 2 of that row (G gradient columns, then the loss and the count
// of ok rows): the latent fits take the latent columns of J (enc_value, G = L), the pose-and-shape fit of align.hip adds the pose's.
struct EncExactRule {
    const float* target;
    __device__ EncRow operator()(float p, int64_t i, int, float clamp) const { return enc_row(p, target[i], clamp); }
};

// A column rule may keep EXTRA float64 words a row in LDS, written once per row (prepare) before the columns are summed: values that are
// costly and shared by no other row.  What is summed, and in which order, does not depend on where a value was formed.
struct EncLatentCols {
    static constexpr int EXTRA = 0;
    const float* J;
    int Jstride;
    __device__ void prepare(double*, float, int64_t, int) const {}
    __device__ double operator()(int c, int G, float w, double e, int ok, int64_t i, int, const double*) const {
        return enc_value(c, G, w, e, ok, J + i * Jstride);
    }
};

// grid (chunks, B): one workgroup sums one chunk of ENC_CHUNK rows of one shape into part[b][chunk][G + 2], in the order of encode_cells.h.
// The rows' weights go to LDS once; then, ENC_COLS columns at a time, accumulator (slot j, column c) belongs to thread j ncols + c, so the
// threads of a wave read consecutive words of a row of J.
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
