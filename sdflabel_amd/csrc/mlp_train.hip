// Training the DeepSDF decoder on the device (gfx950): the forward that stores its activations, the gradient with respect to the input rows
// and the gradient with respect to the weights.  Exact float32 on v_mfma_f32_32x32x2_f32, k in order, bias last; DESIGN.md 7j.
//
// The weights change every step, so the entry points read plain [out][in] row-major DEVICE weights (nn.Linear.weight), not a packed
// sdfr_decoder image.  The work is layer at a time -- the activations have to be stored anyway -- and every layer is one of three products
// of ONE tile kernel (train_gemm_kernel: a workgroup of four waves owns 64 x 64 outputs, a wave one 32 x 32 accumulator; operands go through
// LDS as [k][64] tiles of 32 k, the next tile prefetched into registers while the current one is multiplied):
//   forward          z = xin_l W_l^T           A = xin_l [n][in] (k contiguous), B = W_l [out][in] (k contiguous), k = in
//                    epilogue: + bias, ReLU, the dropout decision of train_cells.h and its 1/(1-p) scale, stored at the row stride of the NEXT
//                    layer's input (its re-injected columns were copied behind by train_copy_kernel); the last linear writes sdf and the tail.
//   input gradient   h = d_l W_l               A = d_l [n][out] (k contiguous), B = W_l [out][in] (in contiguous), k = out
//                    epilogue: d_{l-1} = h * (a_{l-1} > 0 ? 1/(1-p) : 0) -- the stored activation IS the mask --, re-injected columns to ginj[l];
//                    layer 0 adds the ginj of the injection layers in ascending l and writes g_inputs.
//   weight gradient  dW_l = d_l^T xin_l        A = d_l (out contiguous), B = xin_l (in contiguous), k = the rows of one chunk of TRAIN_CHUNK
//                    blockIdx.z = chunk; a partial per chunk, summed in chunk order by train_reduce_kernel.  No atomics.
// An output element is one dot product in k order whatever tile it falls into: a row's sdf and g_inputs do not depend on its position
// or on the batch, dW / db depend on n and the shapes only, and every run gives the same bits.  Tails are predicated (zero operands).
#include "sdfr_common.h"
#include "train_cells.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define TG_TILE 64
#define TG_KT 32
#define TG_P 66                    // pitch of an LDS tile [k][64]: the transposing store of lane (k, m) hits bank 2 k + m
#define TG_ROW(r, h) (((r) & 3) + 8 * ((r) >> 2) + 4 * (h))

enum { TG_FWD = 0, TG_DX = 1, TG_DW = 2 };

struct TrainGemmArgs {
    const float* a;                // A operand
    const float* b;                // B operand
    int64_t lda, ldb;
    int64_t M, K;                  // rows of A's side, reduction length
    int N;                         // columns of B's side
    // forward
    const float* bias;
    float* out;                    // act_l (row stride ld_out), or NULL for the last linear
    int64_t ld_out;
    float* sdf;                    // last linear
    float* tail;
    int use_tanh, hidden;
    int layer, drop;               // drop: this layer takes the hash
    uint32_t threshold;
    uint64_t seed;
    float scale;
    // input gradient
    const float* header;           // the workspace header: [0] = 1/(1-p), [1] = drop_layers
    const float* act_prev;         // act_{l-1} (row stride = K's layer in_dim = N), NULL for layer 0
    int out_prev;                  // out_dim[l-1]
    float* d_prev;                 // [n][out_prev]
    float* ginj;                   // [n][N - out_prev]
    float* g_inputs;               // layer 0: [n][N]
    const float* inj_src[SDFR_MAX_LAYERS];   // layer 0: ginj of layer l or NULL
    int inj_cnt[SDFR_MAX_LAYERS], inj_off[SDFR_MAX_LAYERS];
    int n_lin;
    // weight gradient
    float* part_dw;                // [chunks][M][N]
    float* part_db;                // [chunks][M]
};

// 64 (m) x 32 (k) tile of an operand into 8 registers; KC: k is the contiguous index of the source (src[m ld + k]), else m (src[k ld + m])
template <bool KC>
__device__ __forceinline__ void tg_load(const float* __restrict__ src, int64_t ld, int64_t m0, int64_t M, int64_t k0, int64_t kend, int tid,
                                        float r[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t m = m0 + (KC ? (tid >> 5) + 8 * i : (tid & 63));
        const int64_t k = k0 + (KC ? (tid & 31) : (tid >> 6) + 4 * i);
        const bool ok = m < M && k < kend;
        r[i] = ok ? src[KC ? m * ld + k : k * ld + m] : 0.f;
    }
}

template <bool KC>
__device__ __forceinline__ void tg_store(float* __restrict__ lds, int tid, const float r[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int m = KC ? (tid >> 5) + 8 * i : (tid & 63);
        const int k = KC ? (tid & 31) : (tid >> 6) + 4 * i;
        lds[k * TG_P + m] = r[i];
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void train_gemm_kernel(TrainGemmArgs A) {
    __shared__ float As[TG_KT * TG_P];
    __shared__ float Bs[TG_KT * TG_P];
    constexpr bool AKC = MODE != TG_DW, BKC = MODE == TG_FWD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 31, h = lane >> 5, wm = wave & 1, wn = wave >> 1;
    const int64_t m0 = (int64_t)blockIdx.x * TG_TILE;
    const int64_t n0 = (int64_t)blockIdx.y * TG_TILE;
    int64_t kbeg = 0, kend = A.K;
    if (MODE == TG_DW) {
        kbeg = (int64_t)blockIdx.z * TRAIN_CHUNK;
        kend = kbeg + TRAIN_CHUNK < A.K ? kbeg + TRAIN_CHUNK : A.K;
    }
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float ra[8], rb[8];
    float dbs = 0.f;
    tg_load<AKC>(A.a, A.lda, m0, A.M, kbeg, kend, tid, ra);
    tg_load<BKC>(A.b, A.ldb, n0, A.N, kbeg, kend, tid, rb);
    const float* ap = As + h * TG_P + wm * 32 + col;
    const float* bp = Bs + h * TG_P + wn * 32 + col;
    for (int64_t kt = kbeg; kt < kend; kt += TG_KT) {
        __syncthreads();                                               // the previous tile's reads are done
        tg_store<AKC>(As, tid, ra);
        tg_store<BKC>(Bs, tid, rb);
        __syncthreads();
        if (kt + TG_KT < kend) {
            tg_load<AKC>(A.a, A.lda, m0, A.M, kt + TG_KT, kend, tid, ra);
            tg_load<BKC>(A.b, A.ldb, n0, A.N, kt + TG_KT, kend, tid, rb);
        }
        if (MODE == TG_DW && blockIdx.y == 0 && tid < TG_TILE) {       // db: the column sums of d from the A tile, the chunk's rows in order
#pragma unroll
            for (int k = 0; k < TG_KT; ++k) dbs += As[k * TG_P + tid];     // (rows past the chunk are zero in the tile)
        }
#pragma unroll
        for (int s = 0; s < TG_KT / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * s * TG_P], bp[2 * s * TG_P], acc, 0, 0, 0);
    }

    const int64_t j = n0 + wn * 32 + col;                              // the lane's column
    const bool jok = j < A.N;
    if (MODE == TG_FWD) {
        const float bias = jok ? A.bias[j] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = m0 + wm * 32 + TG_ROW(r, h);
            if (!jok || row >= A.M) continue;
            const float z = acc[r] + bias;
            if (A.hidden) {
                float a = z > 0.f ? z : 0.f;
                if (A.drop) a = train_keep(A.seed, A.layer, row, (int)j, A.threshold) ? a * A.scale : 0.f;
                A.out[row * A.ld_out + j] = a;
            } else {
                const float y1 = A.use_tanh ? tanhf(z) : z;
                const float o = tanhf(y1);
                A.sdf[row] = o;
                A.tail[2 * row] = y1;
                A.tail[2 * row + 1] = o;
            }
        }
    } else if (MODE == TG_DX) {
        const float scale = (A.act_prev != nullptr && ((reinterpret_cast<const int*>(A.header)[1] >> (A.layer - 1)) & 1)) ? A.header[0] : 1.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = m0 + wm * 32 + TG_ROW(r, h);
            if (!jok || row >= A.M) continue;
            if (A.act_prev != nullptr) {
                if (j < A.out_prev) {
                    const float a = A.act_prev[row * A.N + j];
                    A.d_prev[row * A.out_prev + j] = a > 0.f ? acc[r] * scale : 0.f;
                } else {
                    A.ginj[row * (A.N - A.out_prev) + (j - A.out_prev)] = acc[r];
                }
            } else {
                float g = acc[r];
                for (int l = 1; l < A.n_lin; ++l) {
                    const int c = (int)j - A.inj_off[l];
                    if (A.inj_src[l] != nullptr && c >= 0 && c < A.inj_cnt[l]) g += A.inj_src[l][row * A.inj_cnt[l] + c];
                }
                A.g_inputs[row * A.N + j] = g;
            }
        }
    } else {
        float* o = A.part_dw + (int64_t)blockIdx.z * A.M * A.N;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = m0 + wm * 32 + TG_ROW(r, h);
            if (jok && row < A.M) o[row * A.N + j] = acc[r];
        }
        if (blockIdx.y == 0 && tid < TG_TILE && m0 + tid < A.M) A.part_db[(int64_t)blockIdx.z * A.M + m0 + tid] = dbs;
    }
}

struct TrainCopyArgs {
    const float* inputs;
    float* header;
    float* x0;
    float* act[SDFR_MAX_LAYERS];   // act[l - 1] of an injection layer l, or NULL
    int64_t ld[SDFR_MAX_LAYERS];   // in_dim[l]
    int first[SDFR_MAX_LAYERS];    // out_dim[l - 1]
    int inj_cnt[SDFR_MAX_LAYERS], inj_off[SDFR_MAX_LAYERS];
    int n_lin, n_inputs, drop_layers;
    int64_t n;
    float scale;
};

// the input rows into the workspace: x0, and behind the activations of every layer that is followed by an injection
__global__ __launch_bounds__(256) void train_copy_kernel(TrainCopyArgs A) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) {
        A.header[0] = A.scale;
        reinterpret_cast<int*>(A.header)[1] = A.drop_layers;
    }
    if (e >= A.n * A.n_inputs) return;
    const int64_t row = e / A.n_inputs;
    const int c = (int)(e % A.n_inputs);
    const float v = A.inputs[e];
    A.x0[e] = v;
    for (int l = 1; l < A.n_lin; ++l) {
        const int k = c - A.inj_off[l];
        if (A.act[l] != nullptr && k >= 0 && k < A.inj_cnt[l]) A.act[l][row * A.ld[l] + A.first[l] + k] = v;
    }
}

// d of the last linear: g_sdf times the derivative of the final tanh (and of the inner one with use_tanh), formed from the stored tail
__global__ __launch_bounds__(256) void train_dy_kernel(const float* __restrict__ g_sdf, const float* __restrict__ tail, int64_t n, int use_tanh,
                                                       float* __restrict__ d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float y1 = tail[2 * i], o = tail[2 * i + 1];
    float gy = 1.f - o * o;
    if (use_tanh) gy = gy * (1.f - y1 * y1);
    d[i] = g_sdf[i] * gy;
}

__global__ __launch_bounds__(256) void train_reduce_kernel(const float* __restrict__ part_dw, const float* __restrict__ part_db, int64_t chunks,
                                                           int64_t n_dw, int64_t n_db, float* __restrict__ dw, float* __restrict__ db) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n_dw) {
        float s = 0.f;
        for (int64_t c = 0; c < chunks; ++c) s += part_dw[c * n_dw + e];
        dw[e] = s;
    } else if (e < n_dw + n_db) {
        const int64_t i = e - n_dw;
        float s = 0.f;
        for (int64_t c = 0; c < chunks; ++c) s += part_db[c * n_db + i];
        db[i] = s;
    }
}

static int train_check_desc(const char* what, int n_lin, const int* in_dim, const int* out_dim, const int* inj_n, const int* inj_off, int n_inputs,
                            int64_t n) {
    SDFR_REQUIRE(in_dim && out_dim && inj_n && inj_off, "%s: NULL decoder description", what);
    SDFR_REQUIRE(n_lin >= 2 && n_lin <= SDFR_MAX_LAYERS, "%s: n_lin = %d is outside 2 .. %d", what, n_lin, SDFR_MAX_LAYERS);
    SDFR_REQUIRE(n >= 0 && n <= (1ll << 26), "%s: n = %lld is outside 0 .. 2^26", what, (long long)n);
    SDFR_REQUIRE(n_inputs >= 1 && in_dim[0] == n_inputs && inj_n[0] == 0, "%s: layer 0 reads the %d input columns and nothing re-injected", what,
                 n_inputs);
    SDFR_REQUIRE(out_dim[n_lin - 1] == 1, "%s: the last linear must have out_dim 1", what);
    for (int l = 0; l < n_lin; ++l) {
        SDFR_REQUIRE(out_dim[l] >= 1 && out_dim[l] <= TRAIN_MAX_WIDTH && in_dim[l] >= 1 && in_dim[l] <= TRAIN_MAX_IN,
                     "%s: layer %d is %d x %d; widths up to %d (inputs of a layer up to %d) are supported", what, l, out_dim[l], in_dim[l],
                     TRAIN_MAX_WIDTH, TRAIN_MAX_IN);
        SDFR_REQUIRE(inj_n[l] >= 0 && inj_off[l] >= 0 && inj_off[l] + inj_n[l] <= n_inputs, "%s: layer %d re-injects columns outside the input row", what,
                     l);
        if (l > 0)
            SDFR_REQUIRE(in_dim[l] == out_dim[l - 1] + inj_n[l], "%s: in_dim[%d] = %d is not out_dim[%d] + inj_n[%d] = %d", what, l, in_dim[l], l - 1, l,
                         out_dim[l - 1] + inj_n[l]);
    }
    return SDFR_OK;
}

static int train_device_check(const void* p, const char* what) {
    int cur = -1;
    SDFR_HIP_CHECK(hipGetDevice(&cur));
    hipPointerAttribute_t at;
    SDFR_HIP_CHECK(hipPointerGetAttributes(&at, p));
    SDFR_REQUIRE(at.device == cur, "%s: the tensors live on device %d but the current device (the launch stream's) is %d", what, at.device, cur);
    return SDFR_OK;
}

extern "C" int64_t sdfr_decoder_train_bytes(int n_lin, const int* in_dim, const int* out_dim, const int* inj_n, const int* inj_off, int n_inputs,
                                            int64_t n) {
    if (train_check_desc("sdfr_decoder_train_bytes", n_lin, in_dim, out_dim, inj_n, inj_off, n_inputs, n) != SDFR_OK) return -1;
    return train_layout(n_lin, in_dim, out_dim, inj_n, n).total * 4;
}

extern "C" int sdfr_decoder_train_forward(int n_lin, const int* in_dim, const int* out_dim, const int* inj_n, const int* inj_off, int n_inputs,
                                          int use_tanh, const float* const* W, const float* const* b, const float* inputs, int64_t n, float drop_p,
                                          int drop_layers, int64_t seed, float* sdf, void* ws, int64_t ws_bytes, void* stream) {
    const char* what = "sdfr_decoder_train_forward";
    if (int rc = train_check_desc(what, n_lin, in_dim, out_dim, inj_n, inj_off, n_inputs, n)) return rc;
    SDFR_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: drop_p = %g is outside [0, 1)", what, (double)drop_p);
    if (n == 0) return SDFR_OK;
    SDFR_REQUIRE(W && b && inputs && sdf, "%s: NULL argument", what);
    for (int l = 0; l < n_lin; ++l) SDFR_REQUIRE(W[l] && b[l], "%s: NULL weights of layer %d", what, l);
    const TrainLayout L = train_layout(n_lin, in_dim, out_dim, inj_n, n);
    SDFR_REQUIRE(ws != nullptr && ws_bytes >= L.total * 4, "%s: the workspace needs %lld bytes for %lld rows, got %lld", what, (long long)(L.total * 4),
                 (long long)n, (long long)(ws ? ws_bytes : 0));
    if (int rc = train_device_check(inputs, what)) return rc;
    float* wf = reinterpret_cast<float*>(ws);
    const int nh = n_lin - 1;
    const bool dropping = drop_p > 0.f;
    const float scale = dropping ? 1.0f / (1.0f - drop_p) : 1.0f;
    const uint32_t threshold = (uint32_t)rint((double)drop_p * 16777216.0);

    TrainCopyArgs C = {};
    C.inputs = inputs; C.header = wf; C.x0 = wf + L.x0;
    for (int l = 1; l < n_lin; ++l) {
        C.act[l] = inj_n[l] > 0 ? wf + L.act[l - 1] : nullptr;
        C.ld[l] = in_dim[l]; C.first[l] = out_dim[l - 1]; C.inj_cnt[l] = inj_n[l]; C.inj_off[l] = inj_off[l];
    }
    C.n_lin = n_lin; C.n_inputs = n_inputs; C.drop_layers = dropping ? (drop_layers & 0xffff) : 0; C.n = n; C.scale = scale;
    hipLaunchKernelGGL(train_copy_kernel, dim3((unsigned)sdfr_cdiv(n * n_inputs, 256)), dim3(256), 0, (hipStream_t)stream, C);
    SDFR_LAUNCH_CHECK();

    for (int l = 0; l < n_lin; ++l) {
        TrainGemmArgs G = {};
        G.a = l == 0 ? wf + L.x0 : wf + L.act[l - 1];
        G.b = W[l];
        G.lda = G.ldb = in_dim[l];
        G.M = n; G.K = in_dim[l]; G.N = out_dim[l];
        G.bias = b[l];
        G.hidden = l < nh;
        G.out = l < nh ? wf + L.act[l] : nullptr;
        G.ld_out = l < nh ? in_dim[l + 1] : 0;
        G.sdf = sdf; G.tail = wf + L.tail; G.use_tanh = use_tanh;
        G.layer = l; G.drop = (dropping && l < nh && ((drop_layers >> l) & 1)) ? 1 : 0;
        G.threshold = threshold; G.seed = (uint64_t)seed; G.scale = scale;
        hipLaunchKernelGGL(train_gemm_kernel<TG_FWD>, dim3((unsigned)sdfr_cdiv(n, TG_TILE), (unsigned)sdfr_cdiv(out_dim[l], TG_TILE)), dim3(256), 0,
                           (hipStream_t)stream, G);
        SDFR_LAUNCH_CHECK();
    }
    return SDFR_OK;
}

extern "C" int sdfr_decoder_train_backward(int n_lin, const int* in_dim, const int* out_dim, const int* inj_n, const int* inj_off, int n_inputs,
                                           int use_tanh, const float* const* W, const float* g_sdf, int64_t n, void* ws, int64_t ws_bytes,
                                           float* const* dW, float* const* db, float* g_inputs, void* stream) {
    const char* what = "sdfr_decoder_train_backward";
    if (int rc = train_check_desc(what, n_lin, in_dim, out_dim, inj_n, inj_off, n_inputs, n)) return rc;
    SDFR_REQUIRE(n > 0, "%s: n = 0 rows leave no gradient to form (dW would be undefined): skip the call", what);
    SDFR_REQUIRE(W && g_sdf && dW && db && g_inputs, "%s: NULL argument", what);
    for (int l = 0; l < n_lin; ++l) SDFR_REQUIRE(W[l] && dW[l] && db[l], "%s: NULL weights or gradients of layer %d", what, l);
    const TrainLayout L = train_layout(n_lin, in_dim, out_dim, inj_n, n);
    SDFR_REQUIRE(ws != nullptr && ws_bytes >= L.total * 4, "%s: the workspace needs %lld bytes for %lld rows, got %lld", what, (long long)(L.total * 4),
                 (long long)n, (long long)(ws ? ws_bytes : 0));
    if (int rc = train_device_check(g_sdf, what)) return rc;
    float* wf = reinterpret_cast<float*>(ws);
    const int nh = n_lin - 1;
    const int64_t chunks = train_chunks(n);
    hipStream_t st = (hipStream_t)stream;

    hipLaunchKernelGGL(train_dy_kernel, dim3((unsigned)sdfr_cdiv(n, 256)), dim3(256), 0, st, g_sdf, wf + L.tail, n, use_tanh, wf + L.delta[nh & 1]);
    SDFR_LAUNCH_CHECK();
    for (int l = nh; l >= 0; --l) {
        const float* d = wf + L.delta[l & 1];
        const float* xin = l == 0 ? wf + L.x0 : wf + L.act[l - 1];
        const int64_t n_dw = (int64_t)out_dim[l] * in_dim[l];
        {   // dW_l, db_l
            TrainGemmArgs G = {};
            G.a = d; G.lda = out_dim[l]; G.M = out_dim[l];
            G.b = xin; G.ldb = in_dim[l]; G.N = in_dim[l];
            G.K = n;
            G.part_dw = wf + L.part;
            G.part_db = wf + L.part + chunks * n_dw;
            hipLaunchKernelGGL(train_gemm_kernel<TG_DW>,
                               dim3((unsigned)sdfr_cdiv(out_dim[l], TG_TILE), (unsigned)sdfr_cdiv(in_dim[l], TG_TILE), (unsigned)chunks), dim3(256), 0,
                               st, G);
            SDFR_LAUNCH_CHECK();
            hipLaunchKernelGGL(train_reduce_kernel, dim3((unsigned)sdfr_cdiv(n_dw + out_dim[l], 256)), dim3(256), 0, st, G.part_dw, G.part_db, chunks,
                               n_dw, (int64_t)out_dim[l], dW[l], db[l]);
            SDFR_LAUNCH_CHECK();
        }
        {   // d_{l-1} and the re-injected columns' gradient, or g_inputs
            TrainGemmArgs G = {};
            G.a = d; G.lda = out_dim[l]; G.M = n; G.K = out_dim[l];
            G.b = W[l]; G.ldb = in_dim[l]; G.N = in_dim[l];
            G.header = wf; G.layer = l; G.n_lin = n_lin;
            if (l > 0) {
                G.act_prev = wf + L.act[l - 1];
                G.out_prev = out_dim[l - 1];
                G.d_prev = wf + L.delta[(l - 1) & 1];
                G.ginj = wf + L.ginj[l];
            } else {
                G.g_inputs = g_inputs;
                for (int k = 1; k < n_lin; ++k) {
                    G.inj_src[k] = inj_n[k] > 0 ? wf + L.ginj[k] : nullptr;
                    G.inj_cnt[k] = inj_n[k];
                    G.inj_off[k] = inj_off[k];
                }
            }
            hipLaunchKernelGGL(train_gemm_kernel<TG_DX>, dim3((unsigned)sdfr_cdiv(n, TG_TILE), (unsigned)sdfr_cdiv(in_dim[l], TG_TILE)), dim3(256), 0, st,
                               G);
            SDFR_LAUNCH_CHECK();
        }
    }
    return SDFR_OK;
}
