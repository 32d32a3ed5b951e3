// Lidar normals on the device (gfx950): the road-plane removal of the reference's get_kitti_frame (utils/refinement.py:612-656), i.e. Open3D's
// estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) restated as our own semantics (include/sdfr.h; parity with Open3D is NOT tested).
//
// sdfr_lidar_normals   frustum test, fused with the key pass of the hash grid (hash_grid.h, shared with cluster.hip: cells a little wider
//                      than the radius, sorted by scan and scatter) -> one wave per frustum point: the 27 neighbouring cells' buckets are
//                      streamed 64 candidates at a time (the cells and the slot of a candidate are hash_grid.h's) and the running best max_nn
//                      by (d2, index) is kept across the lanes by rank counting -> mean, centred covariance and the Jacobi eigenvector in
//                      lane 0, in neighbour order.
// The order of a bucket's points depends on the scatter's integer atomics; the selection does not depend on the order candidates arrive in
// (ranks of a strict total order), so the results are the same bits on every run.  No float atomic.
// Compiled with -ffp-contract=off: hg_d2's d2 = (dx*dx + dy*dy) + dz*dz rounds as written.
#include "hash_grid.h"
#include "jacobi3.h"

#define NRM_MAX_POINTS (1 << 28)

struct NrmPlanes {
    float pl[12];                    // build_view_frustum's rows, float32
    int use;
};

// the workspace is the grid and nothing else: its taking points are the frustum points
static int64_t nrm_carve(void* base, int64_t N, HashGrid* ws) {
    char* p = (char*)base;
    int64_t at = 0;
    const HashGrid g = hg_carve(N, [&](int64_t bytes) { char* q = p ? p + at : nullptr; at += (bytes + 15) / 16 * 16; return q; });
    if (ws) *ws = g;
    return at;
}

__global__ __launch_bounds__(256) void sdfr_nrm_init_kernel(int32_t* __restrict__ count, int64_t T) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < T) count[i] = 0;
}

// Per input point: the frustum test, the cell key and the bucket's count.  A point outside the frustum gets its results here.
template <typename T>
__global__ __launch_bounds__(256) void sdfr_nrm_key_kernel(const T* __restrict__ pts, int N, NrmPlanes fr, double cell, int shift,
                                                          uint64_t* __restrict__ pkey, int32_t* __restrict__ count,
                                                          uint8_t* __restrict__ in_frustum, double* __restrict__ normals,
                                                          int32_t* __restrict__ nn_count, int32_t* __restrict__ nn_idx, int max_nn) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double X = (double)pts[3 * (int64_t)i], Y = (double)pts[3 * (int64_t)i + 1], Z = (double)pts[3 * (int64_t)i + 2];
    bool in = true;
    if (fr.use) {
#pragma unroll
        for (int k = 0; k < 4; ++k)                                      // as sdfr_depth_map tests it
            in = in && (((double)fr.pl[3 * k] * X + (double)fr.pl[3 * k + 1] * Y) + (double)fr.pl[3 * k + 2] * Z > 0.0);
    }
    in_frustum[i] = in ? 1 : 0;
    hg_key_point(in, X, Y, Z, cell, shift, i, pkey, count);
    if (!in) {
        normals[3 * (int64_t)i] = 0.0; normals[3 * (int64_t)i + 1] = 0.0; normals[3 * (int64_t)i + 2] = 1.0;
        nn_count[i] = 0;
        if (nn_idx)
            for (int k = 0; k < max_nn; ++k) nn_idx[(int64_t)i * max_nn + k] = -1;
    }
}

__device__ __forceinline__ bool nrm_less(double da, int ja, double db, int jb) { return da < db || (da == db && ja < jb); }

// One wave per slot of the sorted cloud.  B = the best neighbours so far, sorted by (d2, index), one per lane (and in LDS); C = the 64
// candidates of the round.  The rank of an element in the union is the number of elements before it in the strict order; the elements of
// rank < max_nn are the new B.  Invalid entries are never read as valid: only the first nb of B and the balloted lanes of C take part.
__global__ __launch_bounds__(64) void sdfr_nrm_query_kernel(const int32_t* __restrict__ start, int64_t T, int shift,
                                                           const int32_t* __restrict__ sidx, const uint64_t* __restrict__ skey,
                                                           const double* __restrict__ spts, double r2, int max_nn,
                                                           double* __restrict__ normals, int32_t* __restrict__ nn_count,
                                                           int32_t* __restrict__ nn_idx) {
    __shared__ double bd[64], cd[64], px[64], py[64], pz[64];
    __shared__ int bj[64], bp[64], cj[64], cp[64];
    __shared__ HgWalk cells;
    const int w = blockIdx.x, lane = threadIdx.x;
    if (w >= start[T]) return;                                           // (the same for the whole wave)
    const int i = sidx[w];
    const double q[3] = {spts[3 * (int64_t)w], spts[3 * (int64_t)w + 1], spts[3 * (int64_t)w + 2]};
    const int M = hg_walk_cells(cells, skey[w], start, shift, lane);
    int nb = 0;
    double md = INFINITY;
    int mj = 0x7fffffff, mp = 0;
    for (int base = 0; base < M; base += 64) {
        const int c = base + lane;
        bool v = c < M;
        double d = INFINITY;
        int j = 0x7fffffff, pos = 0;
        if (v) {
            v = hg_walk_slot(cells, skey, c, &pos);
            if (v) {
                const double p[3] = {spts[3 * (int64_t)pos], spts[3 * (int64_t)pos + 1], spts[3 * (int64_t)pos + 2]};
                d = hg_d2(p, q);
                j = sidx[pos];
                v = d < r2;
            }
        }
        if (v && nb == max_nn) v = nrm_less(d, j, bd[max_nn - 1], bj[max_nn - 1]);      // cannot enter a full B otherwise
        const unsigned long long mask = __ballot(v);
        if (!mask) continue;
        cd[lane] = d; cj[lane] = j; cp[lane] = pos;
        __syncthreads();
        int rb = lane, rc = 0;
        for (int k = 0; k < nb; ++k) rc += nrm_less(bd[k], bj[k], d, j) ? 1 : 0;
        for (unsigned long long m = mask; m; m &= m - 1) {
            const int k = __ffsll((long long)m) - 1;
            const double dk = cd[k];
            const int jk = cj[k];
            rb += nrm_less(dk, jk, md, mj) ? 1 : 0;
            rc += nrm_less(dk, jk, d, j) ? 1 : 0;
        }
        __syncthreads();
        if (lane < nb && rb < max_nn) { bd[rb] = md; bj[rb] = mj; bp[rb] = mp; }
        if (v && rc < max_nn) { bd[rc] = d; bj[rc] = j; bp[rc] = pos; }
        nb += __popcll(mask);
        if (nb > max_nn) nb = max_nn;
        __syncthreads();
        if (lane < nb) { md = bd[lane]; mj = bj[lane]; mp = bp[lane]; }
    }
    nn_count[i] = nb;
    if (nn_idx && lane < max_nn) nn_idx[(int64_t)i * max_nn + lane] = lane < nb ? mj : -1;
    if (lane < nb) { px[lane] = spts[3 * (int64_t)mp]; py[lane] = spts[3 * (int64_t)mp + 1]; pz[lane] = spts[3 * (int64_t)mp + 2]; }
    __syncthreads();
    if (lane != 0) return;
    double n[3] = {0.0, 0.0, 1.0};
    if (nb >= 3) {
        double m[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < nb; ++k) { m[0] += px[k]; m[1] += py[k]; m[2] += pz[k]; }
        for (int a = 0; a < 3; ++a) m[a] /= (double)nb;
        double S[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        for (int k = 0; k < nb; ++k) {
            const double e[3] = {px[k] - m[0], py[k] - m[1], pz[k] - m[2]};
            for (int a = 0; a < 3; ++a)
                for (int b = a; b < 3; ++b) S[a][b] += e[a] * e[b];
        }
        bool zero = true;
        for (int a = 0; a < 3; ++a)
            for (int b = a; b < 3; ++b) {
                S[a][b] /= (double)nb;
                S[b][a] = S[a][b];
                zero = zero && S[a][b] == 0.0;
            }
        if (!zero) {
            double lam[3], V[3][3];
            sdfr_jacobi3(S, lam, V);                                     // eigenvalues descending: column 2 belongs to the smallest
            const double len = sqrt((V[0][2] * V[0][2] + V[1][2] * V[1][2]) + V[2][2] * V[2][2]);
            if (len > 0.0 && len < INFINITY) {
                for (int a = 0; a < 3; ++a) n[a] = V[a][2] / len;
                if ((n[0] * q[0] + n[1] * q[1]) + n[2] * q[2] > 0.0)          // towards the camera; a product of exactly 0 keeps the solver's sign
                    for (int a = 0; a < 3; ++a) n[a] = -n[a];
            }
        }
    }
    for (int a = 0; a < 3; ++a) normals[3 * (int64_t)i + a] = n[a];
}

extern "C" int64_t sdfr_lidar_normals_ws_bytes(int N) {
    if (N < 0 || N > NRM_MAX_POINTS) return -1;
    return nrm_carve(nullptr, N, nullptr);
}

extern "C" int sdfr_lidar_normals(const void* points, int points_f64, int N, const float* planes, float radius32, int max_nn, double* normals,
                                  int32_t* nn_count, int32_t* nn_idx, uint8_t* in_frustum, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
    SDFR_REQUIRE(N >= 0 && N <= NRM_MAX_POINTS, "sdfr_lidar_normals: bad point count");
    const double radius = (double)radius32;
    SDFR_REQUIRE(radius > 0.0 && radius < INFINITY, "sdfr_lidar_normals: the radius must be positive and finite");
    SDFR_REQUIRE(max_nn >= 1 && max_nn <= 64, "sdfr_lidar_normals: max_nn must be 1 ... 64");
    if (N == 0) return SDFR_OK;
    SDFR_REQUIRE(points && normals && nn_count && in_frustum && workspace, "sdfr_lidar_normals: NULL argument");
    SDFR_REQUIRE(((uintptr_t)workspace & 15) == 0, "sdfr_lidar_normals: the workspace must be 16-byte aligned");
    HashGrid ws;
    SDFR_REQUIRE(workspace_bytes >= nrm_carve(workspace, N, &ws), "sdfr_lidar_normals: workspace too small (sdfr_lidar_normals_ws_bytes)");
    ws.cell = hg_cell_width(radius);
    hipStream_t s = (hipStream_t)stream;
    NrmPlanes fr;
    fr.use = planes ? 1 : 0;
    for (int i = 0; i < 12; ++i) fr.pl[i] = planes ? planes[i] : 0.f;
    hipLaunchKernelGGL(sdfr_nrm_init_kernel, dim3(sdfr_cdiv(ws.T, 256)), dim3(256), 0, s, ws.count, ws.T);
    SDFR_LAUNCH_CHECK();
    if (points_f64)
        hipLaunchKernelGGL(sdfr_nrm_key_kernel<double>, dim3(sdfr_cdiv(N, 256)), dim3(256), 0, s, (const double*)points, N, fr, ws.cell, ws.shift,
                           ws.pkey, ws.count, in_frustum, normals, nn_count, nn_idx, max_nn);
    else
        hipLaunchKernelGGL(sdfr_nrm_key_kernel<float>, dim3(sdfr_cdiv(N, 256)), dim3(256), 0, s, (const float*)points, N, fr, ws.cell, ws.shift,
                           ws.pkey, ws.count, in_frustum, normals, nn_count, nn_idx, max_nn);
    SDFR_LAUNCH_CHECK();
    const int sorted = hg_sort(ws, points, points_f64, N, s);
    if (sorted != SDFR_OK) return sorted;
    hipLaunchKernelGGL(sdfr_nrm_query_kernel, dim3(N), dim3(64), 0, s, ws.start, ws.T, ws.shift, ws.sidx, ws.skey, ws.spts, radius * radius, max_nn,
                       normals, nn_count, nn_idx);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
