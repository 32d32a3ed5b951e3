// One shape fitted to several views under a frozen decoder: the step that folds the views of an object into one latent and one scale.
// An iteration of the joint fit is sdfr_align_rows over the V views (each view's latent row a copy of its track's), the decoder pair,
// sdfr_align_reduce over the V views -- all unchanged -- and sdfr_track_step: per track, which views are usable, the weighted means of
// their losses and of their latent (and scale) gradient columns in ascending view order, the latent's step by the rule of enc_step_kernel,
// the shared scale's, each usable view's own pose step, and the next iteration's latent row and pose row of every view.  The per-element
// rules are csrc/track_cells.h.  One launch, grid (T), one workgroup a track; no atomics, no memset, no host
// synchronisation; the same bits on every run; a track's results do not depend on T or on its place in the batch.  Compiled with
// -ffp-contract=off.
#include "sdfr_common.h"
#include "track_cells.h"

struct TrkRates {
    float lr[ALN_POSE];
};

// Phase 1, thread i: view i's usability byte and weight to LDS, ENC_SKIPPED to an unusable view.  Phase 2, thread c: column c of the fold
// (c < L a latent column, c == L the scale's, c == L + 1 the loss); consecutive threads read consecutive words of a row of g.  Phase 3,
// thread 0: the latent's walk in index order, the scale's update, whether the track is stepped.  Phase 4: thread i < L steps latent
// element i and copies it to every view's row; thread i steps view i.
__global__ __launch_bounds__(ENC_THREADS) void trk_step_kernel(float* __restrict__ z, float* __restrict__ m, float* __restrict__ v, int L, int unit,
                                                              float* __restrict__ scale, float* __restrict__ sm, float* __restrict__ sv, int share,
                                                              const int64_t* __restrict__ voff, int V, const float* __restrict__ weight,
                                                              float* __restrict__ theta, float* __restrict__ tm, float* __restrict__ tv,
                                                              float* __restrict__ pose, float* __restrict__ z_view, const double* __restrict__ g,
                                                              const double* __restrict__ view_loss, int32_t* __restrict__ vflags,
                                                              double* __restrict__ loss, int32_t* __restrict__ tflags, float code_reg, float lr,
                                                              TrkRates rates, float bc1, float bc2, float* __restrict__ history_row) {
    const int t = blockIdx.x, tid = threadIdx.x;
    const int G = L + ALN_POSE;
    __shared__ unsigned char s_ok[TRK_MAX_VIEWS];
    __shared__ float s_w[TRK_MAX_VIEWS];
    __shared__ float s_g[ENC_MAX_L];
    __shared__ double s_loss;
    __shared__ float s_gs, s_nrm, s_dot, s_nz, s_scale;
    __shared__ int s_skip;
    const int64_t count = trk_count(voff, t, V);
    if (count < 0) {                                     // (the whole workgroup: nothing is read or written through the entry)
        if (tid == 0) tflags[t] = TRK_BAD_TABLE;
        return;
    }
    const int n = (int)count;
    const int64_t v0 = voff[t];
    for (int i = tid; i < n; i += ENC_THREADS) {
        const int64_t vi = v0 + i;
        const float w = weight ? weight[vi] : 1.f;
        const int32_t fl = vflags[vi];
        const bool ok = trk_view_usable(fl, w, g + vi * G, L, !share, theta + ALN_POSE * vi, tm + ALN_POSE * vi, tv + ALN_POSE * vi, rates.lr[4], bc1, bc2);
        s_ok[i] = ok ? 1 : 0;
        s_w[i] = w;
        if (!ok) vflags[vi] = fl | ENC_SKIPPED;
    }
    __syncthreads();
    int used;
    const double W = trk_weight_sum(s_w, s_ok, n, &used);
    if (used)
        for (int c = tid; c < L + 2; c += ENC_THREADS) {
            if (c < L) {
                s_g[c] = (float)(trk_fold(g + v0 * G + c, G, s_w, s_ok, n) / W);
            } else if (c == L) {
                s_gs = share ? (float)(trk_fold(g + v0 * G + L + 4, G, s_w, s_ok, n) / W) : 0.f;
            } else {
                s_loss = trk_fold(view_loss + v0, 1, s_w, s_ok, n) / W;
            }
        }
    __syncthreads();
    float* zb = z + (int64_t)t * L;
    if (tid == 0) {
        int skip = 1, fl = (n == 0 ? TRK_NO_VIEWS : 0) | TRK_NO_USABLE | TRK_SKIPPED;
        double ls = 0.0;
        if (used) {
            const float nrm = unit ? latent_norm(zb, L) : 1.f;
            const float dot = unit ? latent_unit_dot(zb, s_g, L, nrm) : 0.f;
            const float nz = unit ? 0.f : enc_raw_norm(zb, L);
            skip = 0;
            for (int i = 0; i < L; ++i)
                if (!isfinite(enc_step_grad(zb[i], s_g[i], unit, nrm, dot, nz, code_reg))) skip = 1;
            float sc = 0.f, scm = 0.f, scv = 0.f;
            if (share) {
                trk_scale_step(scale[t], sm[t], sv[t], s_gs, rates.lr[4], bc1, bc2, &sc, &scm, &scv);
                if (!(isfinite(sc) && sc > 0.f)) skip = 1;
                if (!skip && rates.lr[4] != 0.f) scale[t] = sc, sm[t] = scm, sv[t] = scv;
            }
            s_nrm = nrm; s_dot = dot; s_nz = nz; s_scale = sc;
            fl = skip ? TRK_SKIPPED : 0;
            ls = s_loss;
        }
        s_skip = skip;
        tflags[t] = fl;
        loss[t] = ls;
        if (history_row) history_row[t] = (float)ls;
    }
    __syncthreads();
    if (s_skip) {                                        // nothing of the track moves; its usable views say so
        for (int i = tid; i < n; i += ENC_THREADS)
            if (s_ok[i]) vflags[v0 + i] |= ENC_SKIPPED;
        return;
    }
    if (tid < L) {
        if (lr != 0.f) {
            const float gi = enc_step_grad(zb[tid], s_g[tid], unit, s_nrm, s_dot, s_nz, code_reg);
            latent_adam(&zb[tid], &m[(int64_t)t * L + tid], &v[(int64_t)t * L + tid], gi, lr, bc1, bc2);
        }
        const float zi = zb[tid];
        for (int i = 0; i < n; ++i) z_view[(v0 + i) * L + tid] = zi;
    }
    for (int i = tid; i < n; i += ENC_THREADS) {
        const int64_t vi = v0 + i;
        trk_view_step(s_ok[i] != 0, share != 0, s_scale, theta + ALN_POSE * vi, tm + ALN_POSE * vi, tv + ALN_POSE * vi, g + vi * G, L, rates.lr, bc1, bc2,
                      pose + VERIFY_POSE * vi);
    }
}

extern "C" int sdfr_track_step(float* z, float* m, float* v, int L, int T, int unit, float* scale, float* sm, float* sv, int share_scale,
                               const int64_t* voff, int V, const float* weight, float* theta, float* tm, float* tv, float* pose, float* z_view,
                               const double* g, const double* view_loss, int32_t* vflags, double* loss, int32_t* tflags, float code_reg, float lr,
                               const float* lr_pose, int t, float* history, int64_t history_stride, void* stream) {
    SDFR_REQUIRE(z && m && v && voff && theta && tm && tv && pose && z_view && g && view_loss && vflags && loss && tflags && lr_pose &&
                     (!share_scale || (scale && sm && sv)),
                 "sdfr_track_step: NULL argument");
    SDFR_REQUIRE(L >= 1 && L <= ENC_MAX_L && T >= 0 && T <= ENC_MAX_B && V >= 0 && V <= ENC_MAX_B, "sdfr_track_step: bad size (L = %d, T = %d, V = %d)", L, T, V);
    SDFR_REQUIRE(t >= 1 && t <= ENC_MAX_ITER, "sdfr_track_step: the step count t = %d starts at 1", t);
    SDFR_REQUIRE(!history || history_stride >= T, "sdfr_track_step: history_stride %lld below T = %d", (long long)history_stride, T);
    TrkRates rates;
    bool finite = isfinite(lr) && isfinite(code_reg);
    for (int i = 0; i < ALN_POSE; ++i) {
        rates.lr[i] = lr_pose[i];
        finite = finite && isfinite(lr_pose[i]);
    }
    SDFR_REQUIRE(finite, "sdfr_track_step: non-finite learning rate or regulariser");
    if (T == 0) return SDFR_OK;
    float bc1, bc2;
    enc_bias(t, &bc1, &bc2);
    hipLaunchKernelGGL(trk_step_kernel, dim3(T), dim3(ENC_THREADS), 0, (hipStream_t)stream, z, m, v, L, unit, scale, sm, sv, share_scale ? 1 : 0, voff, V, weight,
                       theta, tm, tv, pose, z_view, g, view_loss, vflags, loss, tflags, code_reg, lr, rates, bc1, bc2,
                       history ? history + (int64_t)(t - 1) * history_stride : (float*)nullptr);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
