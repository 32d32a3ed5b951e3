// RANSAC pose initialisation (Kabsch / Procrustes) of B crops at once: PoseEstimator.init_pose_3d of the reference
// (utils/pose.py:85-233) on the device.  Built with -ffp-contract=off: every float32 / float64 expression below rounds as written.
//
// Launch sequence of sdfr_ransac_pose (all on the caller's stream, no host synchronisation):
//   [sample]  device sampler (idx == NULL): 4 distinct scene indices per hypothesis from a counter-based hash
//   cnn       colour-NN table: nearest model colour (index + float64 distance) of every scene point, brute force, colours tiled in LDS
//   hyp       per hypothesis: colour gate (4 table lookups), Kabsch / Procrustes fit in float64, the reference's float32 [rot*scale | tra];
//             ballot compaction of the passing hypotheses into a per-crop list (order kept)
//   score     the hot kernel: (chunk of 256 scene points) x (group of RS_HG passing hypotheses) per workgroup, model points streamed
//             through LDS; inlier counts are integer (ballot + popcount, one LDS add per wave, one global add per workgroup)
//   select    first maximum count per crop (strict >, the reference's step 6) and the < 5 rule
//   mask      the winner's inlier mask, recomputed with the scoring kernel's own device function
//   final     means and cross-covariance of the inliers' colour-NN correspondences in float64 (fixed order), final fit model -> scene
// Every reduction is fixed-order or integer, so a crop gives the same bits in any batch.
#include "sdfr_common.h"
#include "pose_cells.h"       // RS_TPB, RS_HG, RS_TRANS and every per-element rule (rs_*, pose_sample_fit)

namespace {

struct Ws {
    double* cnn_d;      // [B][ncap] float64 distance to the nearest model colour
    float* hyp;         // [B][T][12]
    int32_t* plist;     // [B][T] passing hypotheses, in order
    int32_t* pcount;    // [B]
    int32_t* mask;      // [B][ncap] the winner's inlier mask
};

static inline size_t rs_align(size_t x) { return (x + 255) & ~(size_t)255; }

static size_t ws_layout(int B, int ncap, int T, char* base, Ws* w) {
    size_t off = 0;
    const size_t s_d = rs_align(sizeof(double) * (size_t)B * ncap), s_h = rs_align(sizeof(float) * RS_TRANS * (size_t)B * T),
                 s_l = rs_align(sizeof(int32_t) * (size_t)B * T), s_c = rs_align(sizeof(int32_t) * (size_t)B),
                 s_m = rs_align(sizeof(int32_t) * (size_t)B * ncap);
    if (w) {
        w->cnn_d = (double*)(base + off);
        w->hyp = (float*)(base + off + s_d);
        w->plist = (int32_t*)(base + off + s_d + s_h);
        w->pcount = (int32_t*)(base + off + s_d + s_h + s_l);
        w->mask = (int32_t*)(base + off + s_d + s_h + s_l + s_c);
    }
    return s_d + s_h + s_l + s_c + s_m;
}

// ---- device sampler -----------------------------------------------------------------------------------------------------------------
// rs_sample_draw (pose_cells.h): the 4 distinct indices of (seed, key, t)
__global__ __launch_bounds__(RS_TPB) void rs_sample_kernel(uint64_t seed, const int64_t* __restrict__ keys, const int32_t* __restrict__ ncnt,
                                                         int T, int32_t* __restrict__ idx) {
    const int b = blockIdx.y, t = blockIdx.x * RS_TPB + threadIdx.x;
    if (t >= T) return;
    const int n = ncnt[b];
    const uint64_t key = keys ? (uint64_t)keys[b] : (uint64_t)b;
    int d[4];
    rs_sample_draw(rs_sample_key(seed, key), t, n, d);
    int4 v = make_int4(d[0], d[1], d[2], d[3]);
    *(int4*)(idx + ((size_t)b * T + t) * 4) = v;
}

// ---- colour-NN table ------------------------------------------------------------------------------------------------------------------
// KDTree(model_cls).query in float64 (rs_cnn_step), distance sqrt(rdist); ties go to the lowest model index.
__global__ __launch_bounds__(RS_TPB) void rs_cnn_kernel(const float* __restrict__ mcls, const int32_t* __restrict__ mcnt, int mcap,
                                                      const float* __restrict__ scls, const int32_t* __restrict__ ncnt, int ncap,
                                                      int32_t* __restrict__ cnn_idx, double* __restrict__ cnn_d) {
    __shared__ float tx[RS_TPB], ty[RS_TPB], tz[RS_TPB];
    const int b = blockIdx.y, tid = threadIdx.x, p = blockIdx.x * RS_TPB + tid;
    const int N = ncnt[b], M = mcnt[b];
    if ((int)blockIdx.x * RS_TPB >= N) return;
    const float* sc = scls + ((size_t)b * ncap + (p < N ? p : 0)) * 3;
    const double qx = sc[0], qy = sc[1], qz = sc[2];
    double best = INFINITY;
    int bi = 0;
    const float* mc = mcls + (size_t)b * mcap * 3;
    for (int base = 0; base < M; base += RS_TPB) {
        const int j = base + tid;
        if (j < M) { tx[tid] = mc[(size_t)j * 3]; ty[tid] = mc[(size_t)j * 3 + 1]; tz[tid] = mc[(size_t)j * 3 + 2]; }
        __syncthreads();
        const int n = M - base < RS_TPB ? M - base : RS_TPB;
        for (int k = 0; k < n; ++k) {
            rs_cnn_step(qx, qy, qz, tx[k], ty[k], tz[k], base + k, &best, &bi);
        }
        __syncthreads();
    }
    if (p < N) {
        cnn_idx[(size_t)b * ncap + p] = bi;
        cnn_d[(size_t)b * ncap + p] = sqrt(best);
    }
}

// ---- hypotheses: gate, fit, compaction ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_TPB) void rs_hyp_kernel(const float* __restrict__ model, const int32_t* __restrict__ mcnt, int mcap, int model_f16,
                                                      const float* __restrict__ scene, const int32_t* __restrict__ ncnt, int ncap,
                                                      const int32_t* __restrict__ idx, int T, int type, double nocs_thr,
                                                      const int32_t* __restrict__ cnn_idx, const double* __restrict__ cnn_d, Ws w,
                                                      int32_t* __restrict__ gate, int32_t* __restrict__ counts) {
    __shared__ int wc[RS_TPB / 64];
    __shared__ int base_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = ncnt[b], M = mcnt[b];
    const bool f16 = model_f16 != 0;
    if (tid == 0) base_s = 0;
    __syncthreads();
    for (int t0 = 0; t0 < T; t0 += RS_TPB) {
        const int t = t0 + tid;
        bool pass = false;
        if (t < T) {
            int flag = 0, cnt = -1;
            if (N >= 5 && M >= 1) {
                const int4 q = *(const int4*)(idx + ((size_t)b * T + t) * 4);
                const int ii[4] = {q.x, q.y, q.z, q.w};
                bool ok = true;
                for (int k = 0; k < 4; ++k) ok &= ii[k] >= 0 && ii[k] < N;
                if (ok) {
                    bool g = true;
                    for (int k = 0; k < 4; ++k) g &= !(cnn_d[(size_t)b * ncap + ii[k]] > nocs_thr);
                    if (g) {
                        flag = 1;
                        // from = the 4 scene points (float32), to = their colour-NN model points (the model's dtype)
                        float fp[4][3], tp[4][3], h[RS_TRANS];
                        for (int k = 0; k < 4; ++k) {
                            const float* s = scene + ((size_t)b * ncap + ii[k]) * 3;
                            const float* m = model + ((size_t)b * mcap + cnn_idx[(size_t)b * ncap + ii[k]]) * 3;
                            for (int d = 0; d < 3; ++d) { fp[k][d] = s[d]; tp[k][d] = m[d]; }
                        }
                        int bits;
                        if (pose_sample_fit(fp, tp, f16, type, h, &bits)) {
                            cnt = 0;
                            pass = true;
                            float* hp = w.hyp + ((size_t)b * T + t) * RS_TRANS;
                            *(float4*)(hp) = make_float4(h[0], h[1], h[2], h[3]);
                            *(float4*)(hp + 4) = make_float4(h[4], h[5], h[6], h[7]);
                            *(float4*)(hp + 8) = make_float4(h[8], h[9], h[10], h[11]);
                        }
                        flag |= bits;
                    }
                }
            }
            gate[(size_t)b * T + t] = flag;
            counts[(size_t)b * T + t] = cnt;
        }
        const unsigned long long bal = __ballot(pass);
        if (lane == 0) wc[wv] = __popcll(bal);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int k = 0; k < RS_TPB / 64; ++k) {
            woff += k < wv ? wc[k] : 0;
            tot += wc[k];
        }
        const int base = base_s;
        if (pass) w.plist[(size_t)b * T + base + woff + __popcll(bal & ((1ull << lane) - 1ull))] = t;
        __syncthreads();
        if (tid == 0) base_s = base + tot;
        __syncthreads();
    }
    if (tid == 0) w.pcount[b] = base_s;
}

// ---- scoring ----------------------------------------------------------------------------------------------------------------------------
// nearest model point of HN transformed points, searched on float32 squared distances (first index on exact ties); model points
// stream through the workgroup's LDS tiles.  Every thread of the workgroup must call it (barriers).
template <int HN>
__device__ __forceinline__ void rs_nn_search(const PoseV3 (&tp)[HN], int (&bi)[HN], const float* __restrict__ mp, int M, float4* tile) {
    float bd[HN];
    for (int h = 0; h < HN; ++h) { bd[h] = INFINITY; bi[h] = 0; }
    const int tid = threadIdx.x;
    for (int base = 0; base < M; base += RS_TPB) {
        const int j = base + tid;
        if (j < M) tile[tid] = make_float4(mp[(size_t)j * 3], mp[(size_t)j * 3 + 1], mp[(size_t)j * 3 + 2], 0.0f);
        __syncthreads();
        const int n = M - base < RS_TPB ? M - base : RS_TPB;
        for (int k = 0; k < n; ++k) {
            const float4 m = tile[k];
#pragma unroll
            for (int h = 0; h < HN; ++h) {
                rs_nn_step(tp[h], m.x, m.y, m.z, base + k, &bd[h], &bi[h]);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(RS_TPB) void rs_score_kernel(const float* __restrict__ model, const float* __restrict__ mcls,
                                                        const int32_t* __restrict__ mcnt, int mcap, const float* __restrict__ scene,
                                                        const float* __restrict__ scls, const int32_t* __restrict__ ncnt, int ncap, int T,
                                                        double metric_thr, float nocs_thr32, Ws w, int32_t* __restrict__ counts) {
    __shared__ float4 tile[RS_TPB];
    __shared__ int hc[RS_HG];
    const int b = blockIdx.z, g0 = blockIdx.y * RS_HG, tid = threadIdx.x, lane = tid & 63;
    const int np = w.pcount[b], N = ncnt[b], M = mcnt[b];
    if (g0 >= np || (int)blockIdx.x * RS_TPB >= N) return;       // uniform over the workgroup
    const int nh = np - g0 < RS_HG ? np - g0 : RS_HG;
    const int p = blockIdx.x * RS_TPB + tid;
    const float* s = scene + ((size_t)b * ncap + (p < N ? p : 0)) * 3;
    const float sx = s[0], sy = s[1], sz = s[2];
    PoseV3 tp[RS_HG];
    int hid[RS_HG];
    for (int h = 0; h < RS_HG; ++h) {
        hid[h] = w.plist[(size_t)b * T + g0 + (h < nh ? h : 0)];
        tp[h] = rs_transform(w.hyp + ((size_t)b * T + hid[h]) * RS_TRANS, sx, sy, sz);
    }
    if (tid < RS_HG) hc[tid] = 0;
    const float* mp = model + (size_t)b * mcap * 3;
    const float* mc = mcls + (size_t)b * mcap * 3;
    int bi[RS_HG];
    rs_nn_search<RS_HG>(tp, bi, mp, M, tile);           // (its barriers also order the hc[] zeroing before the adds)
    const float* sc = scls + ((size_t)b * ncap + (p < N ? p : 0)) * 3;
    const float cx = sc[0], cy = sc[1], cz = sc[2];
    for (int h = 0; h < RS_HG; ++h) {
        const bool in = p < N && h < nh && rs_inlier(tp[h], bi[h], mp, mc, cx, cy, cz, metric_thr, nocs_thr32);
        const unsigned long long bal = __ballot(in);
        if (lane == 0 && bal) atomicAdd(&hc[h], (int)__popcll(bal));
    }
    __syncthreads();
    if (tid < nh && hc[tid] > 0) atomicAdd(counts + (size_t)b * T + hid[tid], hc[tid]);
}

// ---- select, mask, final fit ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_TPB) void rs_select_kernel(const int32_t* __restrict__ counts, int T, int32_t* __restrict__ best,
                                                         int32_t* __restrict__ n_inliers) {
    __shared__ int sc[RS_TPB], st[RS_TPB];
    const int b = blockIdx.x, tid = threadIdx.x;
    int bc = 0, bt = -1;             // the reference starts from an empty inlier set: a count must be > 0 to be taken
    for (int t = tid; t < T; t += RS_TPB) {
        const int c = counts[(size_t)b * T + t];
        if (rs_select_takes(c, bc)) { bc = c; bt = t; }
    }
    sc[tid] = bc;
    st[tid] = bt;
    __syncthreads();
    for (int o = RS_TPB / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const int c2 = sc[tid + o], t2 = st[tid + o];
            if (rs_select_folds(c2, t2, sc[tid], st[tid])) { sc[tid] = c2; st[tid] = t2; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        best[b] = st[0];
        n_inliers[b] = sc[0];
    }
}

__global__ __launch_bounds__(RS_TPB) void rs_mask_kernel(const float* __restrict__ model, const float* __restrict__ mcls,
                                                       const int32_t* __restrict__ mcnt, int mcap, const float* __restrict__ scene,
                                                       const float* __restrict__ scls, const int32_t* __restrict__ ncnt, int ncap, int T,
                                                       double metric_thr, float nocs_thr32, const int32_t* __restrict__ best, Ws w) {
    __shared__ float4 tile[RS_TPB];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int p = blockIdx.x * RS_TPB + tid, N = ncnt[b], M = mcnt[b], bt = best[b];
    if ((int)blockIdx.x * RS_TPB >= N) return;
    if (bt < 0) {
        if (p < N) w.mask[(size_t)b * ncap + p] = 0;
        return;
    }
    const float* s = scene + ((size_t)b * ncap + (p < N ? p : 0)) * 3;
    PoseV3 tp[1] = {rs_transform(w.hyp + ((size_t)b * T + bt) * RS_TRANS, s[0], s[1], s[2])};
    const float* mp = model + (size_t)b * mcap * 3;
    int bi[1];
    rs_nn_search<1>(tp, bi, mp, M, tile);
    const float* sc = scls + ((size_t)b * ncap + (p < N ? p : 0)) * 3;
    const bool in = p < N && rs_inlier(tp[0], bi[0], mp, mcls + (size_t)b * mcap * 3, sc[0], sc[1], sc[2], metric_thr, nocs_thr32);
    if (p < N) w.mask[(size_t)b * ncap + p] = in ? 1 : 0;
}

// fixed-order block sum of K doubles per thread (tree over the 256 lanes' partials)
template <int K>
__device__ __forceinline__ void rs_block_sum(double (&v)[K], double* red) {
    const int tid = threadIdx.x;
    for (int k = 0; k < K; ++k) red[k * RS_TPB + tid] = v[k];
    __syncthreads();
    for (int o = RS_TPB / 2; o > 0; o >>= 1) {
        if (tid < o)
            for (int k = 0; k < K; ++k) red[k * RS_TPB + tid] += red[k * RS_TPB + tid + o];
        __syncthreads();
    }
    for (int k = 0; k < K; ++k) v[k] = red[k * RS_TPB];
    __syncthreads();
}

// final fit model -> scene on the winner's inliers and their colour-NN model points (steps 6-7)
__global__ __launch_bounds__(RS_TPB) void rs_final_kernel(const float* __restrict__ model, int mcap, int model_f16, const float* __restrict__ scene,
                                                        const int32_t* __restrict__ ncnt, int ncap, int type, float scale_model,
                                                        const int32_t* __restrict__ cnn_idx, Ws w, int32_t* __restrict__ found,
                                                        int32_t* __restrict__ n_inliers, float* __restrict__ scale, float* __restrict__ rot,
                                                        float* __restrict__ tra) {
    __shared__ double red[10 * RS_TPB];
    const int b = blockIdx.x, tid = threadIdx.x, N = ncnt[b];
    const bool f16 = model_f16 != 0;
    const int ni = n_inliers[b];
    bool ok = N >= 5 && ni >= 5;
    double R[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, c = 0.0, t[3] = {0.0, 0.0, 0.0};
    if (ok) {       // uniform over the workgroup
        const int32_t* mk = w.mask + (size_t)b * ncap;
        double v6[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int p = tid; p < N; p += RS_TPB)
            if (mk[p]) {
                const float* s = scene + ((size_t)b * ncap + p) * 3;
                const float* m = model + ((size_t)b * mcap + cnn_idx[(size_t)b * ncap + p]) * 3;
                rs_final_sums(m, s, v6);
            }
        rs_block_sum<7>(v6, red);
        double mf[3], mt[3];
        rs_final_means(v6, f16, mf, mt);
        double v10[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int p = tid; p < N; p += RS_TPB)
            if (mk[p]) {
                const float* s = scene + ((size_t)b * ncap + p) * 3;
                const float* m = model + ((size_t)b * mcap + cnn_idx[(size_t)b * ncap + p]) * 3;
                rs_final_cov(m, s, mf, mt, f16, v10);
            }
        rs_block_sum<10>(v10, red);
        if (tid == 0) {
            double H[3][3], ratio;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) H[i][j] = v10[i * 3 + j];
            ok = rs_fit(H, mf, mt, v10[9], type, R, &c, t, &ratio);     // procrustes returning None here: the reference raises, we report "not found"
        }
    }
    if (tid == 0) {
        found[b] = ok ? 1 : 0;
        if (!ok) n_inliers[b] = ni > 0 ? ni : 0;
        scale[b] = ok ? (type == 1 ? (float)c : scale_model) : 0.0f;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) rot[(size_t)b * 9 + i * 3 + j] = ok ? (float)R[i][j] : 0.0f;
            tra[(size_t)b * 3 + i] = ok ? (float)t[i] : 0.0f;
        }
    }
}

}  // namespace

extern "C" int64_t sdfr_ransac_ws_bytes(int B, int ncap, int T) {
    if (B <= 0 || ncap <= 0 || T <= 0) return 0;
    return (int64_t)ws_layout(B, ncap, T, nullptr, nullptr);
}

extern "C" int sdfr_ransac_sample(int64_t seed, const int64_t* keys, const int32_t* ncnt, int B, int T, int32_t* idx, void* stream) {
    SDFR_REQUIRE(ncnt && idx, "sdfr_ransac_sample: NULL argument");
    SDFR_REQUIRE(T > 0, "sdfr_ransac_sample: T must be positive");
    SDFR_REQUIRE(((uintptr_t)idx & 15) == 0, "sdfr_ransac_sample: idx must be 16-byte aligned");
    if (B <= 0) return SDFR_OK;
    hipLaunchKernelGGL(rs_sample_kernel, dim3(sdfr_cdiv(T, RS_TPB), B), dim3(RS_TPB), 0, (hipStream_t)stream, (uint64_t)seed, keys, ncnt, T, idx);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_ransac_pose(const float* model, const float* model_cls, const int32_t* mcnt, int mcap, int model_f16, const float* scene,
                                const float* scene_cls, const int32_t* ncnt, int ncap, int B, const int32_t* idx, int64_t seed,
                                const int64_t* keys, int T, int type, float scale_model, const double* h_thr, void* ws, int32_t* found,
                                int32_t* best, int32_t* n_inliers, float* scale, float* rot, float* tra, int32_t* cnn_idx, int32_t* gate,
                                int32_t* counts, int32_t* idx_out, void* stream) {
    SDFR_REQUIRE(model && model_cls && mcnt && scene && scene_cls && ncnt && h_thr && ws && found && best && n_inliers && scale && rot && tra &&
                     cnn_idx && gate && counts,
                 "sdfr_ransac_pose: NULL argument");
    SDFR_REQUIRE(mcap > 0 && ncap > 0 && T > 0, "sdfr_ransac_pose: bad capacity");
    SDFR_REQUIRE(type == 0 || type == 1, "sdfr_ransac_pose: type must be 0 (kabsch) or 1 (procrustes)");
    SDFR_REQUIRE(idx || idx_out, "sdfr_ransac_pose: the device sampler (idx == NULL) needs idx_out");
    SDFR_REQUIRE(((uintptr_t)idx & 15) == 0 && ((uintptr_t)idx_out & 15) == 0, "sdfr_ransac_pose: idx / idx_out must be 16-byte aligned");
    if (B <= 0) return SDFR_OK;
    hipStream_t s = (hipStream_t)stream;
    Ws w;
    ws_layout(B, ncap, T, (char*)ws, &w);
    const double metric_thr = h_thr[0], nocs_thr = h_thr[1];
    const float nocs_thr32 = (float)nocs_thr;
    if (!idx) {
        hipLaunchKernelGGL(rs_sample_kernel, dim3(sdfr_cdiv(T, RS_TPB), B), dim3(RS_TPB), 0, s, (uint64_t)seed, keys, ncnt, T, idx_out);
        SDFR_LAUNCH_CHECK();
        idx = idx_out;
    }
    const int nb = sdfr_cdiv(ncap, RS_TPB);
    hipLaunchKernelGGL(rs_cnn_kernel, dim3(nb, B), dim3(RS_TPB), 0, s, model_cls, mcnt, mcap, scene_cls, ncnt, ncap, cnn_idx, w.cnn_d);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_hyp_kernel, dim3(B), dim3(RS_TPB), 0, s, model, mcnt, mcap, model_f16, scene, ncnt, ncap, idx, T, type, nocs_thr,
                       (const int32_t*)cnn_idx, (const double*)w.cnn_d, w, gate, counts);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_score_kernel, dim3(nb, sdfr_cdiv(T, RS_HG), B), dim3(RS_TPB), 0, s, model, model_cls, mcnt, mcap, scene, scene_cls, ncnt,
                       ncap, T, metric_thr, nocs_thr32, w, counts);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_select_kernel, dim3(B), dim3(RS_TPB), 0, s, (const int32_t*)counts, T, best, n_inliers);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_mask_kernel, dim3(nb, B), dim3(RS_TPB), 0, s, model, model_cls, mcnt, mcap, scene, scene_cls, ncnt, ncap, T, metric_thr,
                       nocs_thr32, (const int32_t*)best, w);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rs_final_kernel, dim3(B), dim3(RS_TPB), 0, s, model, mcap, model_f16, scene, ncnt, ncap, type, scale_model,
                       (const int32_t*)cnn_idx, w, found, n_inliers, scale, rot, tra);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
