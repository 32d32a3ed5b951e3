// Box overlaps of the reference's evaluator (pipelines/rotate_iou.py, the numba.cuda module that pipelines/detection_3d.py imports) on the
// device.  Built with -ffp-contract=off and without fast-math: every float32 / float64 expression rounds as written, division and sqrt are
// correctly rounded.
//
//   rotated BEV IoU   rotate_iou_kernel_eval + devRotateIoUEval (rotate_iou.py:22-286), float32, boxes [x, y, dx, dy, angle]
//   3-D IoU           rotate_iou_gpu_eval(criterion 2) on the BEV columns followed by d3_box_overlap_kernel (:328-355), one launch
//   image-box IoU     image_box_overlap (:358-379), float64 [x1, y1, x2, y2]
//
// One workgroup (256 threads) per 64 x 64 tile of (box, query box) pairs: the tile's boxes are staged in LDS with what every pair needs of
// them (corners, area, the vertical extent), each computed once per box; then one lane per pair.  Grouped mode: per-group offsets into
// boxes, qboxes and the packed output; only the pairs inside a group are evaluated and group g's n_g x k_g block is written row-major at
// ooff[g].  Dense mode is one group holding everything.
//
// The reference evaluates pair (n, k) as devRotateIoUEval(qboxes[k], boxes[n]) (:286): the query box is the FIRST polygon of the
// intersection and criterion 0 divides by the query box's area, criterion 1 by the box's area.  Its candidate-point array holds 8 points
// (16 floats, :230); a corner within eps of the other box's edge can count as "inside" and as an edge crossing, which can make more than 8
// candidates, and the reference then writes past its array.  Here the polygon holds IOU_CAP = 16 points.  The candidate loops bound the
// count at 8 + 16 = 24; candidates past the 16th are dropped, so every input gives a defined result.
#include "sdfr_common.h"
#include <algorithm>

#define IOU_TILE 64     // boxes and query boxes per tile
#define IOU_TPB 256     // threads per workgroup
#define IOU_CAP 16      // polygon capacity in points

namespace {

enum { KIND_BEV = 0, KIND_3D = 1, KIND_IMAGE = 2 };

// rbbox_to_corners (:202-223): clockwise corners, rotated clockwise.  cos / sin in double rounded to float (the reference's math.cos of a
// float32 angle, then float32 products).
__device__ __forceinline__ void rbox_corners(float x, float y, float dx, float dy, float angle, float* c) {
    const float cs = (float)cos((double)angle), sn = (float)sin((double)angle);
    const float hx = -dx / 2.0f, hy = -dy / 2.0f, gx = dx / 2.0f, gy = dy / 2.0f;
    const float cx[4] = {hx, hx, gx, gx};
    const float cy[4] = {hy, gy, gy, hy};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[2 * i] = cs * cx[i] + sn * cy[i] + x;
        c[2 * i + 1] = -sn * cx[i] + cs * cy[i] + y;
    }
}

// point_in_quadrilateral (:160-175), corners 0, 1, 3 of q
__device__ __forceinline__ bool in_quad(float px, float py, const float* q) {
    const float ab0 = q[2] - q[0], ab1 = q[3] - q[1];
    const float ad0 = q[6] - q[0], ad1 = q[7] - q[1];
    const float ap0 = px - q[0], ap1 = py - q[1];
    const float abab = ab0 * ab0 + ab1 * ab1, abap = ab0 * ap0 + ab1 * ap1;
    const float adad = ad0 * ad0 + ad1 * ad1, adap = ad0 * ap0 + ad1 * ap1;
    const float eps = 0.0001f;
    return abab >= abap - eps && abap >= 0.0f - eps && adad >= adap - eps && adap >= 0.0f - eps;
}

// line_segment_intersection (:76-117; the strict variant, not _v1): edge i of p1 against edge j of p2
__device__ __forceinline__ bool seg_cross(const float* p1, const float* p2, int i, int j, float& ox, float& oy) {
    const int i1 = (i + 1) & 3, j1 = (j + 1) & 3;
    const float A0 = p1[2 * i], A1 = p1[2 * i + 1], B0 = p1[2 * i1], B1 = p1[2 * i1 + 1];
    const float C0 = p2[2 * j], C1 = p2[2 * j + 1], D0 = p2[2 * j1], D1 = p2[2 * j1 + 1];
    const float BA0 = B0 - A0, BA1 = B1 - A1, DA0 = D0 - A0, CA0 = C0 - A0, DA1 = D1 - A1, CA1 = C1 - A1;
    const bool acd = DA1 * CA0 > CA1 * DA0;
    const bool bcd = (D1 - B1) * (C0 - B0) > (C1 - B1) * (D0 - B0);
    if (acd == bcd) return false;
    const bool abc = CA1 * BA0 > BA1 * CA0;
    const bool abd = DA1 * BA0 > BA1 * DA0;
    if (abc == abd) return false;
    const float DC0 = D0 - C0, DC1 = D1 - C1;
    const float ABBA = A0 * B1 - B0 * A1, CDDC = C0 * D1 - D0 * C1;
    const float DH = BA1 * DC0 - BA0 * DC1, Dx = ABBA * DC0 - BA0 * CDDC, Dy = ABBA * DC1 - BA1 * CDDC;
    ox = Dx / DH;
    oy = Dy / DH;
    return true;
}

// append (x, y) at position n.  `lim` (a constant once the caller's loops are unrolled) is the highest position this candidate can take,
// so the select chain stays short and every array index is static: the polygon lives in registers.
__device__ __forceinline__ void push(float (&px)[IOU_CAP], float (&py)[IOU_CAP], int& n, float x, float y, int lim) {
#pragma unroll
    for (int s = 0; s < IOU_CAP; ++s)
        if (s <= lim) {
            const bool hit = s == n;
            px[s] = hit ? x : px[s];
            py[s] = hit ? y : py[s];
        }
    n += n < IOU_CAP;
}

// inter (:226-239): quadrilateral_intersection (:178-198) + sort_vertex_in_convex_polygon (:36-72) + area (:28-32); float32
__device__ __forceinline__ float inter_area(const float* p1, const float* p2) {
    float px[IOU_CAP] = {}, py[IOU_CAP] = {};
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (in_quad(p1[2 * i], p1[2 * i + 1], p2)) push(px, py, n, p1[2 * i], p1[2 * i + 1], 2 * i);
        if (in_quad(p2[2 * i], p2[2 * i + 1], p1)) push(px, py, n, p2[2 * i], p2[2 * i + 1], 2 * i + 1);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x, y;
            if (seg_cross(p1, p2, i, j, x, y)) push(px, py, n, x, y, 8 + 4 * i + j);
        }
    if (n < 3) return 0.0f;     // the reference sorts, then sums no triangle
    // pseudo-angle keys about the mean of the points
    float c0 = 0.0f, c1 = 0.0f;
#pragma unroll
    for (int i = 0; i < IOU_CAP; ++i)
        if (i < n) { c0 += px[i]; c1 += py[i]; }
    c0 /= (float)n;
    c1 /= (float)n;
    float vs[IOU_CAP];
#pragma unroll
    for (int i = 0; i < IOU_CAP; ++i) {
        float v0 = px[i] - c0, v1 = py[i] - c1;
        const float d = sqrtf(v0 * v0 + v1 * v1);
        v0 = v0 / d;
        v1 = v1 / d;
        vs[i] = v1 < 0.0f ? -2.0f - v0 : v0;
    }
    // the reference's insertion sort as adjacent swaps: element i sinks while its left neighbour is greater (NaN keys stop it, as there)
#pragma unroll
    for (int i = 1; i < IOU_CAP; ++i) {
        bool act = i < n;
#pragma unroll
        for (int j = i; j > 0; --j) {
            act = act && vs[j - 1] > vs[j];
            const float t = vs[j - 1], tx = px[j - 1], ty = py[j - 1];
            vs[j - 1] = act ? vs[j] : t; px[j - 1] = act ? px[j] : tx; py[j - 1] = act ? py[j] : ty;
            vs[j] = act ? t : vs[j]; px[j] = act ? tx : px[j]; py[j] = act ? ty : py[j];
        }
    }
    // fan from point 0
    float a = 0.0f;
#pragma unroll
    for (int i = 0; i < IOU_CAP - 2; ++i)
        if (i < n - 2) a += fabsf(((px[0] - px[i + 2]) * (py[i + 1] - py[i + 2]) - (py[0] - py[i + 2]) * (px[i + 1] - px[i + 2])) / 2.0f);
    return a;
}

// devRotateIoUEval(rbox1 = query box, rbox2 = box) (:242-254)
__device__ __forceinline__ float rotate_eval(const float* qs, float qarea, const float* bs, float barea, int criterion) {
    float qc[8], bc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { qc[i] = qs[i]; bc[i] = bs[i]; }
    const float ai = inter_area(qc, bc);
    if (criterion == -1) return ai / (qarea + barea - ai);
    if (criterion == 0) return ai / qarea;
    if (criterion == 1) return ai / barea;
    return ai;
}

// Python's min / max of two floats (the first argument unless the second compares smaller / greater)
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }

struct Stage {
    float c[IOU_TILE][9];       // BEV: 8 corners + area
    double z[IOU_TILE][4];      // 3-D: top, bottom, volume; image: x1, y1, x2, y2
    double za[IOU_TILE];        // image: area
};

template <int KIND>
__device__ __forceinline__ void stage_box(const void* src, int64_t row, int camera, Stage& S, int t) {
    if (KIND == KIND_BEV) {
        const float* r = (const float*)src + row * 5;
        rbox_corners(r[0], r[1], r[2], r[3], r[4], S.c[t]);
        S.c[t][8] = r[2] * r[3];
    } else if (KIND == KIND_3D) {
        const double* r = (const double*)src + row * 7;
        // the reference's boxes[:, [0, 2, 3, 5, 6]] (camera frame) or [:, [0, 1, 3, 4, 6]], cast to float32 by rotate_iou_gpu_eval
        const float x = (float)r[0], y = (float)(camera ? r[2] : r[1]), dx = (float)r[3], dy = (float)(camera ? r[5] : r[4]);
        rbox_corners(x, y, dx, dy, (float)r[6], S.c[t]);
        S.c[t][8] = dx * dy;
        S.z[t][0] = camera ? r[1] : r[2] + r[5];            // top of the vertical extent
        S.z[t][1] = camera ? r[1] - r[4] : r[2];            // bottom
        S.z[t][2] = r[3] * r[4] * r[5];                     // volume
    } else {
        const double* r = (const double*)src + row * 4;
        S.z[t][0] = r[0]; S.z[t][1] = r[1]; S.z[t][2] = r[2]; S.z[t][3] = r[3];
        S.za[t] = (r[2] - r[0]) * (r[3] - r[1]);
    }
}

template <int KIND, typename OutT>
__global__ __launch_bounds__(IOU_TPB) void iou_kernel(const void* __restrict__ boxes, int N, const void* __restrict__ qboxes, int K, int G,
                                                      const int32_t* __restrict__ boff, const int32_t* __restrict__ qoff,
                                                      const int64_t* __restrict__ ooff, int per_group, int slices, int criterion, int camera,
                                                      const float* rinc_in, OutT* out, int64_t out_len) {
    __shared__ Stage SB, SQ;
    const int g = blockIdx.x / per_group;
    const int wg = blockIdx.x - g * per_group;
    if (g >= (G > 0 ? G : 1)) return;
    int b0 = 0, nb = N, q0 = 0, nq = K;
    int64_t o0 = 0;
    if (G > 0) {      // a group whose offsets are out of range or whose block does not fit in out writes nothing
        b0 = boff[g]; const int b1 = boff[g + 1];
        q0 = qoff[g]; const int q1 = qoff[g + 1];
        o0 = ooff[g];
        if (b0 < 0 || b1 < b0 || b1 > N || q0 < 0 || q1 < q0 || q1 > K) return;
        nb = b1 - b0;
        nq = q1 - q0;
        if (o0 < 0 || o0 + (int64_t)nb * nq > out_len) return;
    }
    const int tb = (nb + IOU_TILE - 1) / IOU_TILE, tq = (nq + IOU_TILE - 1) / IOU_TILE;
    const int tid = threadIdx.x;
    for (int w = wg; w < tb * tq * slices; w += per_group) {
        const int tile = w / slices, slice = w - tile * slices;
        const int rb = (tile / tq) * IOU_TILE, rq = (tile % tq) * IOU_TILE;
        const int mb = min(IOU_TILE, nb - rb), mq = min(IOU_TILE, nq - rq);
        __syncthreads();      // the previous tile's readers are done
        if (tid < mb) stage_box<KIND>(boxes, (int64_t)b0 + rb + tid, camera, SB, tid);
        else if (tid >= IOU_TILE && tid - IOU_TILE < mq) stage_box<KIND>(qboxes, (int64_t)q0 + rq + tid - IOU_TILE, camera, SQ, tid - IOU_TILE);
        __syncthreads();
        // pairs of the tile, query box fastest (coalesced rows of out)
        for (int p = slice * IOU_TPB + tid; p < mb * mq; p += IOU_TPB * slices) {
            const int r = p / mq, c = p - r * mq;
            const int64_t at = o0 + (int64_t)(rb + r) * nq + rq + c;
            OutT v;
            if (KIND == KIND_BEV) {
                v = rotate_eval(SQ.c[c], SQ.c[c][8], SB.c[r], SB.c[r][8], criterion);
            } else if (KIND == KIND_3D) {
                const float rinc = rinc_in ? rinc_in[at] : rotate_eval(SQ.c[c], SQ.c[c][8], SB.c[r], SB.c[r][8], 2);
                v = rinc;
                if (rinc > 0.0f) {
                    const double iw = py_min(SB.z[r][0], SQ.z[c][0]) - py_max(SB.z[r][1], SQ.z[c][1]);
                    if (iw > 0.0) {
                        const double a1 = SB.z[r][2], a2 = SQ.z[c][2];
                        const double inc = iw * (double)rinc;
                        const double ua = criterion == -1 ? a1 + a2 - inc : criterion == 0 ? a1 : criterion == 1 ? a2 : inc;
                        v = (float)(inc / ua);
                    } else {
                        v = 0.0f;
                    }
                }
            } else {
                const double* bb = SB.z[r];
                const double* qq = SQ.z[c];
                v = 0.0;
                const double iw = py_min(bb[2], qq[2]) - py_max(bb[0], qq[0]);
                if (iw > 0.0) {
                    const double ih = py_min(bb[3], qq[3]) - py_max(bb[1], qq[1]);
                    if (ih > 0.0) {
                        const double ua = criterion == -1 ? SB.za[r] + SQ.za[c] - iw * ih
                                          : criterion == 0 ? SB.za[r] : criterion == 1 ? SQ.za[c] : 1.0;
                        v = iw * ih / ua;
                    }
                }
            }
            out[at] = v;
        }
    }
}

// the current device must hold p (a library call never reads another device's memory over the fabric, and a host pointer would fault)
int check_ptr(const void* p, int dev, const char* what, const char* name) {
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

template <int KIND, typename InT, typename OutT>
int launch(const char* what, const InT* boxes, int N, const InT* qboxes, int K, int G, const int32_t* boff, const int32_t* qoff,
           const int64_t* ooff, int criterion, int camera, const float* rinc_in, OutT* out, int64_t out_len, void* stream) {
    SDFR_REQUIRE(N >= 0 && K >= 0 && G >= 0, "%s: negative N (%d), K (%d) or group count (%d)", what, N, K, G);
    SDFR_REQUIRE(G == 0 || (boff && qoff && ooff), "%s: grouped mode (G = %d) needs boff, qoff and ooff", what, G);
    SDFR_REQUIRE(out_len >= 0, "%s: negative out_len", what);
    SDFR_REQUIRE(G > 0 || out_len >= (int64_t)N * K, "%s: out_len %lld < N * K = %lld", what, (long long)out_len, (long long)N * K);
    if (N == 0 || K == 0) return SDFR_OK;
    SDFR_REQUIRE(boxes && qboxes && out, "%s: NULL argument", what);
    int dev = -1;
    SDFR_HIP_CHECK(hipGetDevice(&dev));
    int rc;
    if ((rc = check_ptr(boxes, dev, what, "boxes")) || (rc = check_ptr(qboxes, dev, what, "qboxes")) || (rc = check_ptr(out, dev, what, "out")))
        return rc;
    if (rinc_in && (rc = check_ptr(rinc_in, dev, what, "rinc"))) return rc;
    if (G > 0 && ((rc = check_ptr(boff, dev, what, "boff")) || (rc = check_ptr(qoff, dev, what, "qoff")) || (rc = check_ptr(ooff, dev, what, "ooff"))))
        return rc;
    const int64_t tiles = (int64_t)sdfr_cdiv(N, IOU_TILE) * sdfr_cdiv(K, IOU_TILE);
    int per_group, slices = 1;
    if (G == 0) {
        // enough workgroups to give every CU a few: split the pairs of a tile among `slices` workgroups when there are few tiles
        slices = (int)std::min<int64_t>(std::max<int64_t>(1, 2048 / tiles), 16);
        per_group = (int)std::min<int64_t>(tiles * slices, 1 << 20);
    } else {
        // workgroups striding over a group's tiles; small groups (an evaluator frame) take one each
        per_group = (int)std::max<int64_t>(1, std::min<int64_t>(tiles, 2048 / G));
    }
    const int64_t grid = (int64_t)per_group * (G > 0 ? G : 1);
    SDFR_REQUIRE(grid < ((int64_t)1 << 31), "%s: too many groups (%d)", what, G);
    hipLaunchKernelGGL((iou_kernel<KIND, OutT>), dim3((unsigned)grid), dim3(IOU_TPB), 0, (hipStream_t)stream, (const void*)boxes, N,
                       (const void*)qboxes, K, G, boff, qoff, ooff, per_group, slices, criterion, camera, rinc_in, out, out_len);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

}  // namespace

extern "C" int sdfr_rotate_iou(const float* boxes, int N, const float* qboxes, int K, int G, const int32_t* boff, const int32_t* qoff,
                               const int64_t* ooff, int criterion, float* out, int64_t out_len, void* stream) {
    return launch<KIND_BEV>("sdfr_rotate_iou", boxes, N, qboxes, K, G, boff, qoff, ooff, criterion, 0, nullptr, out, out_len, stream);
}

extern "C" int sdfr_box3d_iou(const double* boxes, int N, const double* qboxes, int K, int G, const int32_t* boff, const int32_t* qoff,
                              const int64_t* ooff, int criterion, int camera_frame, const float* rinc, float* out, int64_t out_len,
                              void* stream) {
    return launch<KIND_3D>("sdfr_box3d_iou", boxes, N, qboxes, K, G, boff, qoff, ooff, criterion, camera_frame ? 1 : 0, rinc, out, out_len,
                           stream);
}

extern "C" int sdfr_image_box_iou(const double* boxes, int N, const double* qboxes, int K, int G, const int32_t* boff, const int32_t* qoff,
                                  const int64_t* ooff, int criterion, double* out, int64_t out_len, void* stream) {
    return launch<KIND_IMAGE>("sdfr_image_box_iou", boxes, N, qboxes, K, G, boff, qoff, ooff, criterion, 0, nullptr, out, out_len, stream);
}
