// The evaluator's statistics on the device  --  replace compute_statistics_jit / get_thresholds / fused_compute_statistics (numba CPU JIT)
// and scipy's cdist of the reference's pipelines/detection_3d.py.  Layouts and conventions: include/sdfr.h, "Evaluator statistics".
//
// All comparisons and sums are float64; compiled with -ffp-contract=off so that every product and sum rounds where the source rounds.
//
// The matching is serial inside a frame (ground truths in annotation order, a detection once assigned is gone), but independent between
// frames, combinations c = (class, difficulty, overlap level) and score thresholds:
//   pass A (eval_scores_kernel): one lane per (frame, combination), no score threshold; writes the score of every true positive at its
//          ground truth's slot of out[c][NG] (NaN elsewhere), which the caller compacts by sorting;
//   thresholds (eval_thresholds_kernel): one workgroup per combination compacts and sorts its scores, one lane walks the recall targets;
//   pass B (eval_pr_kernel): one lane per (combination, threshold).  A workgroup owns a contiguous chunk of frames, stages one frame's
//          overlap block in LDS (read from global memory when it does not fit), keeps the seven running sums in registers over its
//          frames and writes ONE partial row per lane; eval_pr_reduce_kernel adds the chunks' rows in chunk order.  The chunking depends
//          on the frame count (and the caller's frames_per_chunk) only, never on the device, and no float is accumulated atomically:
//          two runs give the same bits.
// The set of assigned detections is a 64-bit mask in registers for frames of up to 64 detections; larger frames keep it as a bit array in
// the caller's workspace (global memory), so neither path indexes a private array (no scratch).
#include "sdfr_common.h"
#include <algorithm>

namespace {

constexpr int EV_TPB = 256;
constexpr int EV_OV_LDS = 4096;            // doubles of a staged overlap block (32 KB)
constexpr int EV_CHUNK = 8;                // frames per workgroup of pass B unless the caller chooses
constexpr double EV_NO_DETECTION = -10000000.0;
constexpr double EV_PI = 3.141592653589793;

__device__ __forceinline__ double ev_min(double a, double b) { return b < a ? b : a; }      // Python's min / max of two floats
__device__ __forceinline__ double ev_max(double a, double b) { return b > a ? b : a; }

// Python's float %: fmod, then the divisor's sign
__device__ __forceinline__ double ev_pymod(double a, double b) {
    double r = fmod(a, b);
    if (r != 0.0) {
        if ((b < 0.0) != (r < 0.0)) r += b;
    } else {
        r = copysign(0.0, b);
    }
    return r;
}

__device__ __forceinline__ double ev_angle_diff(double x, double y) {
    const double period = 2.0 * EV_PI;
    double d = ev_pymod(x - y + period / 2.0, period) - period / 2.0;
    if (d > EV_PI) d = d - 2.0 * EV_PI;
    return d;
}

// intersection of image box b with DontCare box q over b's area (image_box_overlap, criterion 0)
__device__ __forceinline__ double ev_dc_overlap(const double* b, const double* q) {
    const double iw = ev_min(b[2], q[2]) - ev_max(b[0], q[0]);
    if (iw > 0.0) {
        const double ih = ev_min(b[3], q[3]) - ev_max(b[1], q[1]);
        if (ih > 0.0) return iw * ih / ((b[2] - b[0]) * (b[3] - b[1]));
    }
    return 0.0;
}

struct Mask64 {            // detections 0..63 of a frame, in registers
    unsigned long long m = 0ull;
    __device__ __forceinline__ bool test(int j) const { return (m >> j) & 1ull; }
    __device__ __forceinline__ void set(int j) { m |= 1ull << j; }
};

struct MaskMem {           // any number of detections: `words` uint32 of the workspace, owned by this lane
    uint32_t* p;
    __device__ __forceinline__ bool test(int j) const { return (p[j >> 5] >> (j & 31)) & 1u; }
    __device__ __forceinline__ void set(int j) { p[j >> 5] |= 1u << (j & 31); }
};

struct Overlap {           // block [nd][ng] of a frame: staged in LDS, or float32 / float64 in global memory
    const double* lds;
    const float* g32;
    const double* g64;
    int ng;
    __device__ __forceinline__ double at(int j, int i) const {
        const int64_t k = (int64_t)j * ng + i;
        return lds ? lds[k] : g32 ? (double)g32[k] : g64[k];
    }
};

struct FrameView {
    int nd, ng;
    const double* score;       // [nd]
    const int8_t* ign_dt;      // [nd] of this lane's (class, difficulty)
    const int8_t* ign_gt;      // [ng]
    const double *dt_yaw, *dt_alpha, *gt_yaw, *gt_alpha;      // angular sums only
    const double* dt_bbox;     // [nd][4], DontCare rule only
    const double* dc;          // [ndc][4]
    int ndc;
};

struct Sums {
    long long tp = 0, fp = 0, fn = 0;
    double yaw = 0.0, sim = 0.0, md = 0.0, conf = 0.0;
};

// One greedy matching of a frame.  FP = false: pass A, writes the true positives' scores to score_out[i] (ground truth i).
// FP = true: pass B at score threshold `thresh`, adds the frame's sums to S (per-frame sums first, as the reference adds them).
template <bool FP, typename Mask>
__device__ __forceinline__ void match_frame(const FrameView& F, const Overlap& O, Mask& asg, double min_overlap, double thresh, bool angular,
                                            Sums& S, double* score_out) {
    long long tp = 0, fn = 0;
    double md = 0.0, conf = 0.0, yaw = 0.0, sim = 0.0;
    for (int i = 0; i < F.ng; ++i) {
        const int ig = F.ign_gt[i];
        if (!FP) score_out[i] = __longlong_as_double(0x7ff8000000000000ll);
        if (ig == -1) continue;
        int det = -1;
        double valid = EV_NO_DETECTION, best = -100000.0;
        bool by_ignored = false;
        for (int j = 0; j < F.nd; ++j) {
            const int idt = F.ign_dt[j];
            if (idt == -1 || asg.test(j)) continue;
            const double sc = F.score[j];
            if (FP && sc < thresh) continue;
            const double o = O.at(j, i);
            if (!(o > min_overlap)) continue;
            if (!FP) {
                if (sc > valid) { det = j; valid = sc; }
            } else if (idt == 0) {
                if (o > best || by_ignored) { best = o; det = j; valid = 1.0; by_ignored = false; }
            } else if (idt == 1 && valid == EV_NO_DETECTION) {
                det = j; valid = 1.0; by_ignored = true;
            }
        }
        if (valid == EV_NO_DETECTION) {
            if (ig == 0) ++fn;
            continue;
        }
        asg.set(det);
        if (ig == 1 || F.ign_dt[det] == 1) continue;
        ++tp;
        if (!FP) {
            score_out[i] = F.score[det];
        } else {
            md += fabs(best);
            conf += -log(F.score[det]);
            if (angular) {
                yaw += fabs(ev_angle_diff(F.gt_yaw[i], F.dt_yaw[det]));
                sim += (1.0 + cos(F.gt_alpha[i] - F.dt_alpha[det])) / 2.0;
            }
        }
    }
    if (FP) {
        long long fp = 0;
        for (int j = 0; j < F.nd; ++j) {
            if (asg.test(j) || F.ign_dt[j] != 0 || F.score[j] < thresh) continue;
            ++fp;
            // the DontCare rule takes a false positive away once, whichever DontCare box covers it
            for (int q = 0; q < F.ndc; ++q)
                if (ev_dc_overlap(F.dt_bbox + 4 * j, F.dc + 4 * q) > min_overlap) { --fp; break; }
        }
        S.tp += tp; S.fp += fp; S.fn += fn;
        S.md += md; S.conf += conf; S.yaw += yaw; S.sim += sim;
    }
}

struct EvalArgs {
    const void* ov; int ov_f32; int64_t ov_len;
    const int64_t* ooff; const int32_t* doff; const int32_t* goff;
    int G, ND, NG;
    const double *dt_score, *dt_yaw, *dt_alpha, *gt_yaw, *gt_alpha, *dt_bbox;
    const int8_t *ign_dt, *ign_gt;
    const double* dc_boxes; int NDC; const int32_t* dc_off;
    int ML, K;
    const double* min_overlap;
    int words;                 // uint32 words of a lane's assigned-detection bit array (frames of more than 64 detections)
};

// frame f of the packed arrays; false when its offsets are out of range (such a frame contributes nothing)
__device__ __forceinline__ bool frame_bounds(const EvalArgs& A, int f, int& d0, int& nd, int& g0, int& ng, int64_t& o0) {
    d0 = A.doff[f]; const int d1 = A.doff[f + 1];
    g0 = A.goff[f]; const int g1 = A.goff[f + 1];
    o0 = A.ooff[f];
    if (d0 < 0 || d1 < d0 || d1 > A.ND || g0 < 0 || g1 < g0 || g1 > A.NG) return false;
    nd = d1 - d0; ng = g1 - g0;
    if (o0 < 0 || o0 + (int64_t)nd * ng > A.ov_len) return false;
    if (nd > 64 && (nd + 31) / 32 > A.words) return false;
    return true;
}

__device__ __forceinline__ void frame_view(const EvalArgs& A, int f, int ml, int d0, int nd, int g0, int ng, FrameView& F) {
    F.nd = nd; F.ng = ng;
    F.score = A.dt_score + d0;
    F.ign_dt = A.ign_dt + (int64_t)ml * A.ND + d0;
    F.ign_gt = A.ign_gt + (int64_t)ml * A.NG + g0;
    F.dt_yaw = A.dt_yaw ? A.dt_yaw + d0 : nullptr; F.dt_alpha = A.dt_alpha ? A.dt_alpha + d0 : nullptr;
    F.gt_yaw = A.gt_yaw ? A.gt_yaw + g0 : nullptr; F.gt_alpha = A.gt_alpha ? A.gt_alpha + g0 : nullptr;
    F.dt_bbox = nullptr; F.dc = nullptr; F.ndc = 0;
    if (A.dc_off) {
        const int32_t* off = A.dc_off + (int64_t)ml * (A.G + 1) + f;
        const int c0 = off[0], c1 = off[1];
        if (c0 >= 0 && c1 >= c0 && c1 <= A.NDC) {
            F.dt_bbox = A.dt_bbox + (int64_t)4 * d0;
            F.dc = A.dc_boxes + (int64_t)4 * c0;
            F.ndc = c1 - c0;
        }
    }
}

// (a) minus the planar centre distance, grouped per frame: one workgroup per frame
__global__ __launch_bounds__(64) void eval_dist_kernel(const double* __restrict__ dt_loc, int ND, const double* __restrict__ gt_loc, int NG,
                                                       int G, const int32_t* __restrict__ doff, const int32_t* __restrict__ goff,
                                                       const int64_t* __restrict__ ooff, int col, double* __restrict__ out, int64_t out_len) {
    const int f = blockIdx.x;
    if (f >= G) return;
    const int d0 = doff[f], d1 = doff[f + 1], g0 = goff[f], g1 = goff[f + 1];
    const int64_t o0 = ooff[f];
    if (d0 < 0 || d1 < d0 || d1 > ND || g0 < 0 || g1 < g0 || g1 > NG) return;
    const int nd = d1 - d0, ng = g1 - g0;
    if (o0 < 0 || o0 + (int64_t)nd * ng > out_len) return;
    for (int64_t p = threadIdx.x; p < (int64_t)nd * ng; p += blockDim.x) {
        const int j = (int)(p / ng), i = (int)(p - (int64_t)j * ng);
        const double* a = dt_loc + (int64_t)3 * (d0 + j);
        const double* b = gt_loc + (int64_t)3 * (g0 + i);
        const double dx = a[0] - b[0], dy = a[col] - b[col];
        double s = dx * dx;
        s += dy * dy;
        out[o0 + p] = -sqrt(s);
    }
}

// (b) pass A
__global__ __launch_bounds__(EV_TPB) void eval_scores_kernel(EvalArgs A, uint32_t* ws, double* __restrict__ out) {
    const int64_t lane = (int64_t)blockIdx.x * EV_TPB + threadIdx.x;
    const int C = A.ML * A.K;
    if (lane >= (int64_t)A.G * C) return;
    const int f = (int)(lane / C), c = (int)(lane - (int64_t)f * C), ml = c / A.K;
    int d0, nd, g0, ng;
    int64_t o0;
    double* so = out + (int64_t)c * A.NG;
    if (!frame_bounds(A, f, d0, nd, g0, ng, o0)) {      // (offsets out of range: if the ground truths' range is valid, mark them "no true positive")
        const int a = A.goff[f], b = A.goff[f + 1];
        if (a >= 0 && b >= a && b <= A.NG)
            for (int i = a; i < b; ++i) so[i] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    FrameView F;
    frame_view(A, f, ml, d0, nd, g0, ng, F);
    Overlap O{nullptr, A.ov_f32 ? (const float*)A.ov + o0 : nullptr, A.ov_f32 ? nullptr : (const double*)A.ov + o0, ng};
    Sums S;
    const double mo = A.min_overlap[c];
    if (nd <= 64) {
        Mask64 m;
        match_frame<false>(F, O, m, mo, 0.0, false, S, so + g0);
    } else {
        MaskMem m{ws + lane * A.words};
        for (int w = 0; w < (nd + 31) / 32; ++w) m.p[w] = 0u;
        match_frame<false>(F, O, m, mo, 0.0, false, S, so + g0);
    }
}

// (c) thresholds: one workgroup per combination compacts the pass-A scores of its row (NaN = none) into its workspace row, sorts them
// descending (bitonic, in global memory: the row stays in L2) and lane 0 walks the recall targets.  The walk keeps score i unless the
// running target is nearer to the next detection's recall than to this one's: `skip(i)` is true on a prefix of [i0, n - 1) (left and right
// recalls grow with i, rounding is monotone) and false at n - 1, so the first kept index is found by bisection with the walk's own
// float64 expressions -- the same thresholds as the reference's serial loop, in S * log2(n) steps instead of n.
constexpr int EV_SORT_TPB = 1024;

__global__ __launch_bounds__(EV_SORT_TPB) void eval_thresholds_kernel(const double* __restrict__ scores, int64_t NG, int64_t stride,
                                                                      const int64_t* __restrict__ num_gt, int C, int K, int S, double* rows,
                                                                      double* __restrict__ thr, int32_t* __restrict__ nthr,
                                                                      int32_t* __restrict__ count) {
    __shared__ unsigned long long s_n;
    const int c = blockIdx.x;
    if (c >= C) return;
    const double* src = scores + (int64_t)c * NG;
    double* a = rows + (int64_t)c * stride;
    if (threadIdx.x == 0) s_n = 0ull;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < NG; i += EV_SORT_TPB) {
        const double v = src[i];
        if (v == v) a[atomicAdd(&s_n, 1ull)] = v;          // (placement order is irrelevant: the row is sorted next)
    }
    __syncthreads();
    const int64_t n = (int64_t)s_n;
    int64_t P = 1;
    while (P < n) P <<= 1;
    for (int64_t i = n + threadIdx.x; i < P; i += EV_SORT_TPB) a[i] = -INFINITY;
    __syncthreads();
    for (int64_t k = 2; k <= P; k <<= 1) {
        for (int64_t j = k >> 1; j > 0; j >>= 1) {
            for (int64_t i = threadIdx.x; i < P; i += EV_SORT_TPB) {
                const int64_t o = i ^ j;
                if (o > i) {
                    const double x = a[i], y = a[o];
                    if (((i & k) == 0) ? (x < y) : (x > y)) { a[i] = y; a[o] = x; }
                }
            }
            __syncthreads();
        }
    }
    if (threadIdx.x != 0) return;
    if (count) count[c] = (int32_t)n;
    const double ngt = (double)num_gt[c / K];
    const double step = 1.0 / ((double)S - 1.0);
    double cur = 0.0;
    int t = 0;
    int64_t i = 0;
    while (i < n && t < S) {
        int64_t lo = i, hi = n - 1;
        while (lo < hi) {
            const int64_t m = lo + (hi - lo) / 2;              // m < n - 1: the walk's test for a detection that is not the last
            const double left = (double)(m + 1) / ngt, right = (double)(m + 2) / ngt;
            if ((right - cur) < (cur - left)) lo = m + 1; else hi = m;
        }
        thr[(int64_t)c * S + t] = a[lo];
        ++t;
        cur += step;
        i = lo + 1;
    }
    nthr[c] = t;
    for (; t < S; ++t) thr[(int64_t)c * S + t] = 0.0;
}

// (d) pass B.  grid.x: chunk of frames, grid.y: block of EV_TPB lanes (combination, threshold)
__global__ __launch_bounds__(EV_TPB) void eval_pr_kernel(EvalArgs A, const double* __restrict__ thr, const int32_t* __restrict__ nthr, int S,
                                                         int angular, int chunk, uint32_t* bits, double* __restrict__ partial) {
    __shared__ double s_ov[EV_OV_LDS];
    const int C = A.ML * A.K;
    const int lanes = C * S;
    const int lane = blockIdx.y * EV_TPB + threadIdx.x;
    const bool live_lane = lane < lanes;
    const int c = live_lane ? lane / S : 0, t = live_lane ? lane - c * S : 0, ml = c / A.K;
    const bool active = live_lane && t < nthr[c];
    const double mo = A.min_overlap[c];
    const double th = active ? thr[(int64_t)c * S + t] : 0.0;
    Sums sums;
    const int f0 = blockIdx.x * chunk, f1 = min(A.G, f0 + chunk);
    for (int f = f0; f < f1; ++f) {
        int d0, nd, g0, ng;
        int64_t o0;
        if (!frame_bounds(A, f, d0, nd, g0, ng, o0)) continue;          // uniform over the workgroup
        if (nd == 0 && ng == 0) continue;
        const int64_t cells = (int64_t)nd * ng;
        const bool staged = cells <= EV_OV_LDS;
        if (staged) {
            __syncthreads();                                            // the previous frame's readers are done
            for (int p = threadIdx.x; p < (int)cells; p += EV_TPB)
                s_ov[p] = A.ov_f32 ? (double)((const float*)A.ov)[o0 + p] : ((const double*)A.ov)[o0 + p];
            __syncthreads();
        }
        if (!active) continue;
        FrameView F;
        frame_view(A, f, ml, d0, nd, g0, ng, F);
        Overlap O{staged ? s_ov : nullptr, (!staged && A.ov_f32) ? (const float*)A.ov + o0 : nullptr,
                  (!staged && !A.ov_f32) ? (const double*)A.ov + o0 : nullptr, ng};
        if (nd <= 64) {
            Mask64 m;
            match_frame<true>(F, O, m, mo, th, angular != 0, sums, nullptr);
        } else {
            MaskMem m{bits + ((int64_t)blockIdx.x * lanes + lane) * A.words};
            for (int w = 0; w < (nd + 31) / 32; ++w) m.p[w] = 0u;
            match_frame<true>(F, O, m, mo, th, angular != 0, sums, nullptr);
        }
    }
    if (live_lane) {
        double* row = partial + ((int64_t)blockIdx.x * lanes + lane) * 7;
        row[0] = (double)sums.tp; row[1] = (double)sums.fp; row[2] = (double)sums.fn;
        row[3] = sums.yaw; row[4] = sums.sim; row[5] = sums.md; row[6] = sums.conf;
    }
}

// pr[lane][col] = sum over chunks, in chunk order
__global__ __launch_bounds__(EV_TPB) void eval_pr_reduce_kernel(const double* __restrict__ partial, int chunks, int64_t cells, double* __restrict__ pr) {
    const int64_t k = (int64_t)blockIdx.x * EV_TPB + threadIdx.x;
    if (k >= cells) return;
    double s = 0.0;
    for (int b = 0; b < chunks; ++b) s += partial[(int64_t)b * cells + k];
    pr[k] = s;
}

int ev_check_ptr(const void* p, int dev, const char* what, const char* name) {
    hipPointerAttribute_t a;
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        sdfr_set_error("%s: %s is not device memory (%s)", what, name, hipGetErrorString(e));
        return SDFR_E_INVALID;
    }
    if (a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged) {
        sdfr_set_error("%s: %s is not device memory", what, name);
        return SDFR_E_INVALID;
    }
    if (a.device != dev) {
        sdfr_set_error("%s: %s lives on device %d but the current device (the launch stream's) is %d", what, name, a.device, dev);
        return SDFR_E_INVALID;
    }
    return SDFR_OK;
}

#define EV_PTR(p)                                                         \
    do {                                                                  \
        if ((p) != nullptr) {                                             \
            const int rc_ = ev_check_ptr((p), dev, what, #p);             \
            if (rc_) return rc_;                                          \
        }                                                                 \
    } while (0)

int ev_words(int max_nd) { return max_nd > 64 ? (max_nd + 31) / 32 : 0; }
int ev_chunk(int frames_per_chunk) { return frames_per_chunk > 0 ? frames_per_chunk : EV_CHUNK; }
int64_t ev_pow2(int64_t n) { int64_t p = 1; while (p < n) p <<= 1; return p; }

}  // namespace

extern "C" int64_t sdfr_eval_ws_bytes(int G, int NG, int C, int S, int max_nd, int frames_per_chunk) {
    if (G < 0 || NG < 0 || C < 0 || S < 0 || max_nd < 0) return -1;
    const int64_t words = ev_words(max_nd);
    const int64_t chunks = sdfr_cdiv(G, ev_chunk(frames_per_chunk));
    const int64_t pass_a = (int64_t)G * C * words * 4;
    const int64_t sort = (int64_t)C * ev_pow2(NG) * 8;
    const int64_t pass_b = chunks * C * S * 7 * 8 + chunks * C * S * words * 4;
    return std::max<int64_t>(std::max(std::max(pass_a, sort), pass_b), 8);
}

extern "C" int sdfr_eval_center_dist(const double* dt_loc, int ND, const double* gt_loc, int NG, int G, const int32_t* doff, const int32_t* goff,
                                     const int64_t* ooff, int camera_frame, double* out, int64_t out_len, void* stream) {
    const char* what = "sdfr_eval_center_dist";
    SDFR_REQUIRE(ND >= 0 && NG >= 0 && G >= 0 && out_len >= 0, "%s: negative ND (%d), NG (%d), G (%d) or out_len", what, ND, NG, G);
    if (G == 0 || ND == 0 || NG == 0) return SDFR_OK;
    SDFR_REQUIRE(dt_loc && gt_loc && doff && goff && ooff && out, "%s: NULL argument", what);
    int dev = -1;
    SDFR_HIP_CHECK(hipGetDevice(&dev));
    EV_PTR(dt_loc); EV_PTR(gt_loc); EV_PTR(doff); EV_PTR(goff); EV_PTR(ooff); EV_PTR(out);
    hipLaunchKernelGGL(eval_dist_kernel, dim3((unsigned)G), dim3(64), 0, (hipStream_t)stream, dt_loc, ND, gt_loc, NG, G, doff, goff, ooff,
                       camera_frame ? 2 : 1, out, out_len);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_eval_match_scores(const void* overlaps, int ov_f32, int64_t ov_len, const int64_t* ooff, const int32_t* doff,
                                      const int32_t* goff, int G, int ND, int NG, const double* dt_score, const int8_t* ign_dt,
                                      const int8_t* ign_gt, int ML, int K, const double* min_overlap, int max_nd, void* ws, int64_t ws_bytes,
                                      double* out, void* stream) {
    const char* what = "sdfr_eval_match_scores";
    SDFR_REQUIRE(G >= 0 && ND >= 0 && NG >= 0 && ML >= 0 && K >= 0 && ov_len >= 0 && max_nd >= 0, "%s: negative size", what);
    const int64_t C = (int64_t)ML * K;
    if (G == 0 || C == 0 || NG == 0) return SDFR_OK;
    SDFR_REQUIRE((int64_t)G * C < ((int64_t)1 << 31) * EV_TPB && C < (1 << 24), "%s: too many frames x combinations", what);
    SDFR_REQUIRE(ooff && doff && goff && ign_gt && min_overlap && out, "%s: NULL argument", what);
    SDFR_REQUIRE(ND == 0 || (dt_score && ign_dt), "%s: NULL detection columns", what);
    SDFR_REQUIRE(ov_len == 0 || overlaps, "%s: NULL overlaps", what);
    const int words = ev_words(max_nd);
    SDFR_REQUIRE(words == 0 || (ws && ws_bytes >= (int64_t)G * C * words * 4), "%s: workspace too small (sdfr_eval_ws_bytes)", what);
    int dev = -1;
    SDFR_HIP_CHECK(hipGetDevice(&dev));
    EV_PTR(overlaps); EV_PTR(ooff); EV_PTR(doff); EV_PTR(goff); EV_PTR(dt_score); EV_PTR(ign_dt); EV_PTR(ign_gt); EV_PTR(min_overlap); EV_PTR(out);
    if (words) EV_PTR(ws);
    EvalArgs A{overlaps, ov_f32 ? 1 : 0, ov_len, ooff, doff, goff, G, ND, NG, dt_score, nullptr, nullptr, nullptr, nullptr, nullptr, ign_dt, ign_gt,
               nullptr, 0, nullptr, ML, K, min_overlap, words};
    const int64_t lanes = (int64_t)G * C;
    hipLaunchKernelGGL(eval_scores_kernel, dim3((unsigned)sdfr_cdiv(lanes, EV_TPB)), dim3(EV_TPB), 0, (hipStream_t)stream, A, (uint32_t*)ws, out);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_eval_thresholds(const double* scores, int NG, const int64_t* num_gt, int ML, int K, int S, void* ws, int64_t ws_bytes,
                                    double* thr, int32_t* nthr, int32_t* count, void* stream) {
    const char* what = "sdfr_eval_thresholds";
    SDFR_REQUIRE(ML >= 0 && K >= 1 && S >= 2 && NG >= 0, "%s: ML (%d) < 0, K (%d) < 1, sample points (%d) < 2 or NG (%d) < 0", what, ML, K, S, NG);
    const int64_t C = (int64_t)ML * K;
    if (C == 0) return SDFR_OK;
    SDFR_REQUIRE(C < (1 << 24), "%s: too many combinations", what);
    SDFR_REQUIRE(num_gt && thr && nthr && ws && (NG == 0 || scores), "%s: NULL argument", what);
    const int64_t stride = ev_pow2(NG);
    SDFR_REQUIRE(ws_bytes >= C * stride * 8, "%s: workspace too small (sdfr_eval_ws_bytes)", what);
    int dev = -1;
    SDFR_HIP_CHECK(hipGetDevice(&dev));
    EV_PTR(scores); EV_PTR(num_gt); EV_PTR(ws); EV_PTR(thr); EV_PTR(nthr); EV_PTR(count);
    hipLaunchKernelGGL(eval_thresholds_kernel, dim3((unsigned)C), dim3(EV_SORT_TPB), 0, (hipStream_t)stream, scores, (int64_t)NG, stride, num_gt,
                       (int)C, K, S, (double*)ws, thr, nthr, count);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_eval_pr(const void* overlaps, int ov_f32, int64_t ov_len, const int64_t* ooff, const int32_t* doff, const int32_t* goff, int G,
                            int ND, int NG, const double* dt_score, const double* dt_yaw, const double* dt_alpha, const double* gt_yaw,
                            const double* gt_alpha, const double* dt_bbox, const int8_t* ign_dt, const int8_t* ign_gt, const double* dc_boxes,
                            int NDC, const int32_t* dc_off, int ML, int K, const double* min_overlap, const double* thr, const int32_t* nthr,
                            int S, int angular, int max_nd, int frames_per_chunk, void* ws, int64_t ws_bytes, double* pr, void* stream) {
    const char* what = "sdfr_eval_pr";
    SDFR_REQUIRE(G >= 0 && ND >= 0 && NG >= 0 && NDC >= 0 && ML >= 0 && K >= 0 && ov_len >= 0 && max_nd >= 0 && S >= 1, "%s: negative size", what);
    const int64_t C = (int64_t)ML * K;
    if (C == 0) return SDFR_OK;
    SDFR_REQUIRE(C * S < (1 << 24), "%s: too many combinations x thresholds", what);
    SDFR_REQUIRE(min_overlap && thr && nthr && pr && ws, "%s: NULL argument", what);
    SDFR_REQUIRE(G == 0 || (ooff && doff && goff), "%s: NULL offsets", what);
    SDFR_REQUIRE(ND == 0 || (dt_score && ign_dt), "%s: NULL detection columns", what);
    SDFR_REQUIRE(NG == 0 || ign_gt, "%s: NULL ign_gt", what);
    SDFR_REQUIRE(ov_len == 0 || overlaps, "%s: NULL overlaps", what);
    SDFR_REQUIRE(!angular || ((ND == 0 || (dt_yaw && dt_alpha)) && (NG == 0 || (gt_yaw && gt_alpha))), "%s: angular sums need yaw and alpha", what);
    SDFR_REQUIRE(!dc_off || ((ND == 0 || dt_bbox) && (NDC == 0 || dc_boxes)), "%s: the DontCare rule needs dt_bbox and dc_boxes", what);
    SDFR_REQUIRE(ws_bytes >= sdfr_eval_ws_bytes(G, NG, (int)C, S, max_nd, frames_per_chunk), "%s: workspace too small (sdfr_eval_ws_bytes)", what);
    int dev = -1;
    SDFR_HIP_CHECK(hipGetDevice(&dev));
    EV_PTR(overlaps); EV_PTR(ooff); EV_PTR(doff); EV_PTR(goff); EV_PTR(dt_score); EV_PTR(dt_yaw); EV_PTR(dt_alpha); EV_PTR(gt_yaw); EV_PTR(gt_alpha);
    EV_PTR(dt_bbox); EV_PTR(ign_dt); EV_PTR(ign_gt); EV_PTR(dc_boxes); EV_PTR(dc_off); EV_PTR(min_overlap); EV_PTR(thr); EV_PTR(nthr); EV_PTR(ws);
    EV_PTR(pr);
    const int words = ev_words(max_nd);
    const int chunk = ev_chunk(frames_per_chunk);
    const int chunks = sdfr_cdiv(G, chunk);
    const int64_t cells = C * S * 7;
    double* partial = (double*)ws;
    uint32_t* bits = (uint32_t*)(partial + (int64_t)chunks * cells);
    EvalArgs A{overlaps, ov_f32 ? 1 : 0, ov_len, ooff, doff, goff, G, ND, NG, dt_score, angular ? dt_yaw : nullptr, angular ? dt_alpha : nullptr,
               angular ? gt_yaw : nullptr, angular ? gt_alpha : nullptr, dt_bbox, ign_dt, ign_gt, dc_boxes, NDC, dc_off, ML, K, min_overlap, words};
    if (chunks > 0) {
        hipLaunchKernelGGL(eval_pr_kernel, dim3((unsigned)chunks, (unsigned)sdfr_cdiv(C * S, EV_TPB)), dim3(EV_TPB), 0, (hipStream_t)stream, A, thr,
                           nthr, S, angular ? 1 : 0, chunk, bits, partial);
        SDFR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(eval_pr_reduce_kernel, dim3((unsigned)sdfr_cdiv(cells, EV_TPB)), dim3(EV_TPB), 0, (hipStream_t)stream, partial, chunks, cells,
                       pr);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
