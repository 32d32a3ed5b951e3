// The search for a fit's start: many candidate starts share one shape's samples, are scored by the loss alone on the same drawn rows, and
// are ranked per shape on the device.  sdfr_search_rows is the rows kernel of the fits (encode_kernels.h) over a policy with an owner
// (search_cells.h): start s reads the samples of shape own[s] and draws as that shape does, with its own latent and pose.
// sdfr_search_reduce is the chunk and fold kernels over the fits' own row rules and a column rule without gradient columns, so its loss is
// the loss word of sdfr_bound_reduce / sdfr_align_reduce in every bit, and no Jacobian is read.  sdfr_search_select ranks the usable starts
// of every shape by (loss, index) with rank counting over the shape's losses in LDS: no sort, nothing that depends on the schedule.
// The per-element rules are csrc/search_cells.h.  No atomics, no memset, no host synchronisation; the same bits on every
// run; a start's results depend neither on N nor on its place in the batch.  Compiled with -ffp-contract=off.
#include "encode_kernels.h"
#include "search_cells.h"

template <class Inner>
static int srch_rows_launch(Inner inner, bool sides_ok, const float* samples, int64_t S, const int64_t* soff, int B, const int32_t* own, int N,
                            int shape0, int64_t k, int draw, int64_t seed, int64_t iter, const float* z, int L, int unit, float* inputs, float* zn,
                            int32_t* flags, void* stream) {
    const char* name = "sdfr_search_rows";
    SDFR_REQUIRE(soff && own && z && zn && flags && (!inputs || (sides_ok && (samples || S == 0))), "%s: NULL argument", name);
    SDFR_REQUIRE(L >= 1 && L <= ENC_MAX_L, "%s: latent size %d outside [1,%d]", name, L, ENC_MAX_L);
    SDFR_REQUIRE(B >= 0 && N >= 0 && N <= ENC_MAX_B && shape0 >= 0 && (int64_t)shape0 + B <= ENC_MAX_B && S >= 0,
                 "%s: bad size (B = %d, N = %d, shape0 = %d, S = %lld)", name, B, N, shape0, (long long)S);
    SDFR_REQUIRE(!inputs || (k >= 1 && k <= ENC_MAX_K), "%s: k = %lld outside [1,%d]", name, (long long)k, ENC_MAX_K);
    SDFR_REQUIRE(iter >= 0 && iter < ENC_MAX_ITER, "%s: iter outside [0,2^24)", name);
    if (N == 0) return SDFR_OK;
    const SrchRows<Inner> rows{inner, own, B};
    hipLaunchKernelGGL(enc_rows_kernel<SrchRows<Inner>>, dim3(inputs ? sdfr_cdiv(k, ENC_THREADS) : 1, N), dim3(ENC_THREADS), 0, (hipStream_t)stream, samples, S,
                       soff, shape0, k, draw, (uint64_t)seed, iter, z, L, unit, rows, inputs, zn, flags);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_search_rows(const float* samples, int64_t S, const int64_t* soff, int B, const int32_t* own, int N, int shape0, int64_t k, int draw,
                                int64_t seed, int64_t iter, const float* z, int L, int unit, const float* pose, float* inputs, float* cam, float* lo, float* hi,
                                float* zn, int32_t* flags, void* stream) {
    if (pose) {
        SrchPosedRows inner;
        inner.pose = pose, inner.cam = cam, inner.lo = lo, inner.hi = hi;
        return srch_rows_launch(inner, lo && hi, samples, S, soff, B, own, N, shape0, k, draw, seed, iter, z, L, unit, inputs, zn, flags, stream);
    }
    return srch_rows_launch(CplBoundRows{lo, hi}, lo && hi, samples, S, soff, B, own, N, shape0, k, draw, seed, iter, z, L, unit, inputs, zn, flags,
                            stream);
}

extern "C" int64_t sdfr_search_ws_bytes(int N, int64_t k) {
    if (N < 0 || N > ENC_MAX_B || k < 1 || k > ENC_MAX_K) return -1;
    return (int64_t)N * enc_chunks(k) * 2 * (int64_t)sizeof(double);
}

template <class Rule>
static int srch_reduce_launch(const float* pred, Rule rule, int N, int64_t k, float clamp, void* ws, double* loss, int32_t* flags, void* stream) {
    const int64_t chunks = enc_chunks(k);
    hipLaunchKernelGGL((enc_chunk_kernel<Rule, SrchLossCols>), dim3((unsigned)chunks, N), dim3(ENC_THREADS), 0, (hipStream_t)stream, pred, rule, SrchLossCols(), 0,
                       k, clamp, (double*)ws);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(enc_fold_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, (const double*)ws, chunks, 0, loss, (double*)nullptr, flags);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_search_reduce(const float* pred, const float* lo, const float* hi, const float* pose, int N, int64_t k, float clamp, void* ws,
                                  int64_t ws_bytes, double* loss, int32_t* flags, void* stream) {
    const char* name = "sdfr_search_reduce";
    SDFR_REQUIRE(pred && lo && hi && ws && loss && flags, "%s: NULL argument", name);
    SDFR_REQUIRE(N >= 0 && N <= ENC_MAX_B && k >= 1 && k <= ENC_MAX_K, "%s: bad size (N = %d, k = %lld)", name, N, (long long)k);
    SDFR_REQUIRE(clamp > 0.f, "%s: clamp must be positive", name);
    SDFR_REQUIRE(ws_bytes >= sdfr_search_ws_bytes(N, k), "%s: the workspace holds %lld bytes, sdfr_search_ws_bytes asks for %lld", name, (long long)ws_bytes,
                 (long long)sdfr_search_ws_bytes(N, k));
    SDFR_REQUIRE(((uintptr_t)ws & 7) == 0, "%s: the workspace must be aligned to 8 bytes", name);
    if (N == 0) return SDFR_OK;
    if (pose) return srch_reduce_launch(pred, AlnRowRule{lo, hi, pose}, N, k, clamp, ws, loss, flags, stream);
    return srch_reduce_launch(pred, CplBoundRule{lo, hi}, N, k, clamp, ws, loss, flags, stream);
}

// grid (B), one workgroup a shape.  Phase 1, thread i (strided): the start's loss and usability byte to LDS, and the thread's count of
// usable starts.  Phase 2, thread 0: the counts in thread order (integers).  Phase 3, thread i (strided): a usable start counts the usable
// starts before it (srch_rank: every thread of a wave reads the same LDS word) and, with a rank below keep, stores its index; the ranks of
// the usable starts are a permutation, so every word of order[b] is written once -- the ranks from min(keep, usable) on by thread r.
__global__ __launch_bounds__(SRCH_THREADS) void srch_select_kernel(const double* __restrict__ loss, const int32_t* __restrict__ flags,
                                                                  const int64_t* __restrict__ coff, int64_t N, int keep, int32_t* __restrict__ order,
                                                                  int32_t* __restrict__ count) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ double s_loss[SRCH_MAX_STARTS];
    __shared__ unsigned char s_ok[SRCH_MAX_STARTS];
    __shared__ int s_cnt[SRCH_THREADS];
    __shared__ int s_usable;
    int32_t* ob = order + (int64_t)b * keep;
    const int64_t cnt = srch_count(coff, b, N);
    if (cnt < 0) {                                       // (the whole workgroup: nothing is read through the entry)
        if (tid < keep) ob[tid] = -1;
        if (tid == 0) count[b] = -1;
        return;
    }
    const int n = (int)cnt;
    const int64_t c0 = coff[b];
    int mine = 0;
    for (int i = tid; i < n; i += SRCH_THREADS) {
        const double l = loss[c0 + i];
        const bool ok = srch_usable(flags[c0 + i], l);
        s_loss[i] = l;
        s_ok[i] = ok ? 1 : 0;
        mine += ok ? 1 : 0;
    }
    s_cnt[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        int u = 0;
        for (int t = 0; t < SRCH_THREADS; ++t) u += s_cnt[t];
        s_usable = u;
        count[b] = u < keep ? u : keep;
    }
    __syncthreads();
    const int kept = s_usable < keep ? s_usable : keep;
    if (tid >= kept && tid < keep) ob[tid] = -1;
    for (int i = tid; i < n; i += SRCH_THREADS) {
        if (!s_ok[i]) continue;
        const int r = srch_rank(s_loss, s_ok, n, i);
        if (r < keep) ob[r] = (int32_t)(c0 + i);
    }
}

extern "C" int sdfr_search_select(const double* loss, const int32_t* flags, const int64_t* coff, int B, int64_t N, int keep, int32_t* order, int32_t* count,
                                  void* stream) {
    const char* name = "sdfr_search_select";
    SDFR_REQUIRE(coff && order && count && (N == 0 || (loss && flags)), "%s: NULL argument", name);
    SDFR_REQUIRE(B >= 0 && B <= ENC_MAX_B && N >= 0 && N <= 0x7FFFFFFF, "%s: bad size (B = %d, N = %lld)", name, B, (long long)N);
    SDFR_REQUIRE(keep >= 1 && keep <= SRCH_MAX_KEEP, "%s: keep = %d outside [1,%d]", name, keep, SRCH_MAX_KEEP);
    if (B == 0) return SDFR_OK;
    hipLaunchKernelGGL(srch_select_kernel, dim3(B), dim3(SRCH_THREADS), 0, (hipStream_t)stream, loss, flags, coff, N, keep, order, count);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
