// Lidar normals on the device (gfx950): the road-plane removal of the reference's get_kitti_frame (utils/refinement.py:612-656), i.e. Open3D's
// estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) restated as our own semantics (include/sdfr.h; parity with Open3D is NOT tested).
//
// sdfr_lidar_normals   frustum test -> a hash grid of cells a little wider than the radius, built by a counting sort (count, scan, scatter: no
//                      host sizing, no synchronisation) -> one wave per frustum point: the 27 neighbouring cells' buckets are streamed 64
//                      candidates at a time and the running best max_nn by (d2, index) is kept across the lanes by rank counting -> mean,
//                      centred covariance and the Jacobi eigenvector in lane 0, in neighbour order.
// The order of a bucket's points depends on the scatter's integer atomics; the selection does not depend on the order candidates arrive in
// (ranks of a strict total order), so the results are the same bits on every run.  No float atomic.
// Compiled with -ffp-contract=off: d2 = (dx*dx + dy*dy) + dz*dz rounds as written.
#include "sdfr_common.h"
#include "jacobi3.h"

#define NRM_HALF (1 << 20)           // cell coordinates are clamped to [-2^20, 2^20) and stored with this offset: 21 bits per axis
#define NRM_SCAN_TPB 1024
#define NRM_MAX_POINTS (1 << 28)

struct NrmPlanes {
    float pl[12];                    // build_view_frustum's rows, float32
    int use;
};

static int64_t nrm_table(int64_t N) {                                   // buckets of the hash grid: a power of two, at least 2 N
    int64_t T = 64;
    while (T < 2 * N) T <<= 1;
    return T;
}

static int nrm_log2(int64_t T) {
    int l = 0;
    while (((int64_t)1 << l) < T) ++l;
    return l;
}

struct NrmWs {
    double* spts;                    // [N][3] the frustum points in bucket order
    uint64_t* skey;                  // [N]    their cell keys
    uint64_t* pkey;                  // [N]    cell key per input point, ~0 outside the frustum
    int32_t* start;                  // [T + 4] first slot of every bucket; start[T] = the number of frustum points
    int32_t* count;                  // [T]
    int32_t* sidx;                   // [N]    input index of every slot
};

static int64_t nrm_carve(void* base, int64_t N, NrmWs* ws) {
    const int64_t T = nrm_table(N);
    char* p = (char*)base;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { char* q = p ? p + at : nullptr; at += (bytes + 15) / 16 * 16; return q; };
    char* a = take(N * 24); char* b = take(N * 8); char* c = take(N * 8); char* d = take((T + 4) * 4); char* e = take(T * 4); char* f = take(N * 4);
    if (ws) { ws->spts = (double*)a; ws->skey = (uint64_t*)b; ws->pkey = (uint64_t*)c; ws->start = (int32_t*)d; ws->count = (int32_t*)e; ws->sidx = (int32_t*)f; }
    return at;
}

__device__ __forceinline__ int nrm_cell(double p, double cell) {
    double c = floor(p / cell);
    if (!(c >= (double)-NRM_HALF)) c = (double)-NRM_HALF;               // (a NaN lands here too)
    if (c > (double)(NRM_HALF - 1)) c = (double)(NRM_HALF - 1);
    return (int)c + NRM_HALF;
}

__device__ __forceinline__ uint64_t nrm_pack(int cx, int cy, int cz) { return ((uint64_t)cx << 42) | ((uint64_t)cy << 21) | (uint64_t)cz; }

__device__ __forceinline__ int nrm_bucket(uint64_t key, int shift) { return (int)((key * 0x9E3779B97F4A7C15ull) >> shift); }

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
    if (in) {
        const uint64_t key = nrm_pack(nrm_cell(X, cell), nrm_cell(Y, cell), nrm_cell(Z, cell));
        pkey[i] = key;
        atomicAdd(&count[nrm_bucket(key, shift)], 1);
    } else {
        pkey[i] = ~0ull;
        normals[3 * (int64_t)i] = 0.0; normals[3 * (int64_t)i + 1] = 0.0; normals[3 * (int64_t)i + 2] = 1.0;
        nn_count[i] = 0;
        if (nn_idx)
            for (int k = 0; k < max_nn; ++k) nn_idx[(int64_t)i * max_nn + k] = -1;
    }
}

// Exclusive scan of count[T] into start[T + 1] by one workgroup, 4096 buckets per round; count is zeroed for the scatter.
__global__ __launch_bounds__(NRM_SCAN_TPB) void sdfr_nrm_scan_kernel(int32_t* __restrict__ count, int32_t* __restrict__ start, int64_t T) {
    __shared__ int wsum[NRM_SCAN_TPB / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int carry = 0;
    for (int64_t base = 0; base < T; base += 4 * NRM_SCAN_TPB) {
        const int64_t e = base + 4 * t;                                  // T is a multiple of 4: e < T covers e + 3
        int4 c = make_int4(0, 0, 0, 0);
        if (e < T) c = *(const int4*)(count + e);
        const int s = c.x + c.y + c.z + c.w;
        int v = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int n = __shfl_up(v, o);
            if (lane >= o) v += n;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < NRM_SCAN_TPB / 64; ++k) {
            const int x = wsum[k];
            if (k < wave) woff += x;
            tot += x;
        }
        const int ex = carry + woff + v - s;
        if (e < T) {
            *(int4*)(start + e) = make_int4(ex, ex + c.x, ex + c.x + c.y, ex + c.x + c.y + c.z);
            *(int4*)(count + e) = make_int4(0, 0, 0, 0);
        }
        carry += tot;
        __syncthreads();
    }
    if (t == 0) start[T] = carry;
}

template <typename T>
__global__ __launch_bounds__(256) void sdfr_nrm_scatter_kernel(const T* __restrict__ pts, int N, const uint64_t* __restrict__ pkey, int shift,
                                                              const int32_t* __restrict__ start, int32_t* __restrict__ count,
                                                              int32_t* __restrict__ sidx, uint64_t* __restrict__ skey, double* __restrict__ spts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint64_t key = pkey[i];
    if (key == ~0ull) return;
    const int b = nrm_bucket(key, shift);
    const int pos = start[b] + atomicAdd(&count[b], 1);                  // < start[b + 1] <= N: the counts are those of the key pass
    sidx[pos] = i;
    skey[pos] = key;
#pragma unroll
    for (int k = 0; k < 3; ++k) spts[3 * (int64_t)pos + k] = (double)pts[3 * (int64_t)i + k];
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
    __shared__ uint64_t ck[27];
    __shared__ int bj[64], bp[64], cj[64], cp[64], cs[27], cpre[28];
    const int w = blockIdx.x, lane = threadIdx.x;
    if (w >= start[T]) return;                                           // (the same for the whole wave)
    const int i = sidx[w];
    const double qx = spts[3 * (int64_t)w], qy = spts[3 * (int64_t)w + 1], qz = spts[3 * (int64_t)w + 2];
    const uint64_t qkey = skey[w];
    if (lane < 27) {
        const int nx = (int)((qkey >> 42) & 0x1FFFFF) + lane % 3 - 1, ny = (int)((qkey >> 21) & 0x1FFFFF) + (lane / 3) % 3 - 1,
                  nz = (int)(qkey & 0x1FFFFF) + lane / 9 - 1;
        int s = 0, len = 0;
        uint64_t k = 0;
        if (nx >= 0 && nx < 2 * NRM_HALF && ny >= 0 && ny < 2 * NRM_HALF && nz >= 0 && nz < 2 * NRM_HALF) {
            k = nrm_pack(nx, ny, nz);
            const int b = nrm_bucket(k, shift);
            s = start[b];
            len = start[b + 1] - s;
        }
        cs[lane] = s; ck[lane] = k; cpre[lane + 1] = len;
    }
    __syncthreads();
    if (lane == 0) {
        cpre[0] = 0;
        for (int k = 1; k <= 27; ++k) cpre[k] += cpre[k - 1];
    }
    __syncthreads();
    const int M = cpre[27];
    int nb = 0;
    double md = INFINITY;
    int mj = 0x7fffffff, mp = 0;
    for (int base = 0; base < M; base += 64) {
        const int c = base + lane;
        bool v = c < M;
        double d = INFINITY;
        int j = 0x7fffffff, pos = 0;
        if (v) {
            int s = 0;
            for (int k = 1; k < 27; ++k) s += cpre[k] <= c ? 1 : 0;      // the cell whose range holds candidate c
            pos = cs[s] + (c - cpre[s]);
            v = skey[pos] == ck[s];                                      // another cell of the same bucket: not this cell's point
            if (v) {
                const double dx = spts[3 * (int64_t)pos] - qx, dy = spts[3 * (int64_t)pos + 1] - qy, dz = spts[3 * (int64_t)pos + 2] - qz;
                d = (dx * dx + dy * dy) + dz * dz;
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
                if ((n[0] * qx + n[1] * qy) + n[2] * qz > 0.0)            // towards the camera; a product of exactly 0 keeps the solver's sign
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
    NrmWs ws;
    SDFR_REQUIRE(workspace_bytes >= nrm_carve(workspace, N, &ws), "sdfr_lidar_normals: workspace too small (sdfr_lidar_normals_ws_bytes)");
    hipStream_t s = (hipStream_t)stream;
    const int64_t T = nrm_table(N);
    const int shift = 64 - nrm_log2(T);
    const double cell = radius * (1.0 + 1.0 / 1048576.0);                // a little wider than the radius: rounding of p / cell cannot put a
    NrmPlanes fr;                                                        // neighbour two cells away
    fr.use = planes ? 1 : 0;
    for (int i = 0; i < 12; ++i) fr.pl[i] = planes ? planes[i] : 0.f;
    hipLaunchKernelGGL(sdfr_nrm_init_kernel, dim3(sdfr_cdiv(T, 256)), dim3(256), 0, s, ws.count, T);
    SDFR_LAUNCH_CHECK();
    if (points_f64)
        hipLaunchKernelGGL(sdfr_nrm_key_kernel<double>, dim3(sdfr_cdiv(N, 256)), dim3(256), 0, s, (const double*)points, N, fr, cell, shift, ws.pkey,
                           ws.count, in_frustum, normals, nn_count, nn_idx, max_nn);
    else
        hipLaunchKernelGGL(sdfr_nrm_key_kernel<float>, dim3(sdfr_cdiv(N, 256)), dim3(256), 0, s, (const float*)points, N, fr, cell, shift, ws.pkey,
                           ws.count, in_frustum, normals, nn_count, nn_idx, max_nn);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_nrm_scan_kernel, dim3(1), dim3(NRM_SCAN_TPB), 0, s, ws.count, ws.start, T);
    SDFR_LAUNCH_CHECK();
    if (points_f64)
        hipLaunchKernelGGL(sdfr_nrm_scatter_kernel<double>, dim3(sdfr_cdiv(N, 256)), dim3(256), 0, s, (const double*)points, N, ws.pkey, shift,
                           ws.start, ws.count, ws.sidx, ws.skey, ws.spts);
    else
        hipLaunchKernelGGL(sdfr_nrm_scatter_kernel<float>, dim3(sdfr_cdiv(N, 256)), dim3(256), 0, s, (const float*)points, N, ws.pkey, shift,
                           ws.start, ws.count, ws.sidx, ws.skey, ws.spts);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_nrm_query_kernel, dim3(N), dim3(64), 0, s, ws.start, T, shift, ws.sidx, ws.skey, ws.spts, radius * radius, max_nn,
                       normals, nn_count, nn_idx);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
