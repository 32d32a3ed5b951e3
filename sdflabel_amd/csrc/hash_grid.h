// The spatial hash grid of the lidar normals (normals.hip) and the lidar clusters (cluster.hip): points sorted by cell with a counting sort
// (count, scan, scatter: no host sizing, no synchronisation), so that the neighbours within a radius r of a point lie in the 27 cells around
// its own.  Cells are a little wider than r, cell coordinates take 21 bits per axis, a cell's key hashes multiplicatively into a power-of-two
// table of at least 2 N buckets; a bucket may hold several cells' points, so a walk compares the stored key.
// Two parts.  The cells part is plain functions of one point or one key, compiled for the device by the two units and for the host by
// tests/cluster_host/cluster_host.cpp.  The device part is the workspace, the kernels of the sort and the 27-cell prologue of a
// one-wave-per-slot walk.  Every user is compiled with -ffp-contract=off: every operation rounds separately.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HG_HD __host__ __device__ inline
#else
#define HG_HD static inline
#endif

#define HG_HALF (1 << 20)               // cell coordinates are clamped to [-2^20, 2^20) and stored with this offset: 21 bits per axis

HG_HD double hg_cell_width(double r) { return r * (1.0 + 1.0 / 1048576.0); }                    // a little wider than r: rounding of p / cell
                                                                                                // cannot put a neighbour two cells away
HG_HD int hg_cell(double p, double cell) {
    double c = floor(p / cell);
    if (!(c >= (double)-HG_HALF)) c = (double)-HG_HALF;                  // (a NaN lands here too)
    if (c > (double)(HG_HALF - 1)) c = (double)(HG_HALF - 1);
    return (int)c + HG_HALF;
}

HG_HD uint64_t hg_pack(int cx, int cy, int cz) { return ((uint64_t)cx << 42) | ((uint64_t)cy << 21) | (uint64_t)cz; }

HG_HD int hg_bucket(uint64_t key, int shift) { return (int)((key * 0x9E3779B97F4A7C15ull) >> shift); }

HG_HD int64_t hg_table(int64_t N) {                                      // buckets of the hash grid: a power of two, at least 2 N
    int64_t T = 64;
    while (T < 2 * N) T <<= 1;
    return T;
}

HG_HD int hg_log2(int64_t T) {
    int l = 0;
    while (((int64_t)1 << l) < T) ++l;
    return l;
}

// key of the k-th (0 ... 26) neighbouring cell of the cell `key`; false where it leaves the 21-bit range
HG_HD bool hg_neighbour_cell(uint64_t key, int k, uint64_t* out) {
    const int nx = (int)((key >> 42) & 0x1FFFFF) + k % 3 - 1, ny = (int)((key >> 21) & 0x1FFFFF) + (k / 3) % 3 - 1, nz = (int)(key & 0x1FFFFF) + k / 9 - 1;
    if (!(nx >= 0 && nx < 2 * HG_HALF && ny >= 0 && ny < 2 * HG_HALF && nz >= 0 && nz < 2 * HG_HALF)) return false;
    *out = hg_pack(nx, ny, nz);
    return true;
}

// THE distance of both users, in float64: the normals rank by it and keep d2 < r*r, the clusters keep d2 < eps*eps, both strictly
HG_HD double hg_d2(const double* a, const double* b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

#if defined(__HIPCC__)
#include "sdfr_common.h"

#define HG_SCAN_TPB 1024

struct HashGrid {
    double* spts;                    // [N][3] the taking points in bucket order
    uint64_t* skey;                  // [N]    their cell keys
    uint64_t* pkey;                  // [N]    cell key per input point, ~0 for a point that takes no part
    int32_t* start;                  // [T + 4] first slot of every bucket; start[T] = the number of taking points
    int32_t* count;                  // [T]
    int32_t* sidx;                   // [N]    input index of every slot
    int64_t T;
    int shift;                       // 64 - log2 T
    double cell;                     // the caller's hg_cell_width(radius)
};

// The six arrays, through the caller's take(bytes) -> char*, which may hand out nothing but NULL where only the sizes are wanted.
template <class Take>
static HashGrid hg_carve(int64_t N, Take take) {
    HashGrid g;
    g.T = hg_table(N);
    g.shift = 64 - hg_log2(g.T);
    g.cell = 0.0;
    g.spts = (double*)take(N * 24); g.skey = (uint64_t*)take(N * 8); g.pkey = (uint64_t*)take(N * 8);
    g.start = (int32_t*)take((g.T + 4) * 4); g.count = (int32_t*)take(g.T * 4); g.sidx = (int32_t*)take(N * 4);
    return g;
}

// The key pass of one input point, called from the user's own per-point kernel: a taking point gets its cell key and counts in its bucket
// (count[] zeroed before), any other point gets ~0.
__device__ __forceinline__ void hg_key_point(bool takes, double X, double Y, double Z, double cell, int shift, int i, uint64_t* pkey,
                                             int32_t* count) {
    if (takes) {
        const uint64_t key = hg_pack(hg_cell(X, cell), hg_cell(Y, cell), hg_cell(Z, cell));
        pkey[i] = key;
        atomicAdd(&count[hg_bucket(key, shift)], 1);
    } else {
        pkey[i] = ~0ull;
    }
}

// Exclusive scan of in[n] into out[n + 1] by one workgroup, 4096 elements per round; in and out may not overlap.  GRID: the counts of a
// HashGrid into its first slots -- T is a multiple of 4 and hg_carve's arrays are 16-byte aligned, so a thread's four elements move as one
// int4 (a table of 2^18 buckets is 64 rounds of one workgroup; with four guarded loads and stores remove_road took 0.55 ms instead of
// 0.41, profiles/hash_grid_notes.md), and the counts are zeroed once read, for the scatter to count up again.  Otherwise any n, tails guarded.
template <bool GRID>
__global__ __launch_bounds__(HG_SCAN_TPB) void sdfr_hg_scan_kernel(int32_t* __restrict__ in, int32_t* __restrict__ out, int64_t n) {
    __shared__ int wsum[HG_SCAN_TPB / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int carry = 0;
    for (int64_t base = 0; base < n; base += 4 * HG_SCAN_TPB) {
        const int64_t e = base + 4 * t;
        int c[4] = {0, 0, 0, 0};
        if (GRID) {
            if (e < n) {                                                 // (covers e + 3)
                const int4 q = *(const int4*)(in + e);
                c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] = e + k < n ? in[e + k] : 0;
        }
        const int s = (c[0] + c[1]) + (c[2] + c[3]);
        int v = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int m = __shfl_up(v, o);
            if (lane >= o) v += m;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < HG_SCAN_TPB / 64; ++k) {
            const int x = wsum[k];
            if (k < wave) woff += x;
            tot += x;
        }
        int ex = carry + woff + v - s;
        if (GRID) {
            if (e < n) {
                *(int4*)(out + e) = make_int4(ex, ex + c[0], ex + c[0] + c[1], ex + c[0] + c[1] + c[2]);
                *(int4*)(in + e) = make_int4(0, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e + k < n) out[e + k] = ex;
                ex += c[k];
            }
        }
        carry += tot;
        __syncthreads();
    }
    if (t == 0) out[n] = carry;
}

template <typename T>
__global__ __launch_bounds__(256) void sdfr_hg_scatter_kernel(const T* __restrict__ pts, int N, const uint64_t* __restrict__ pkey, int shift,
                                                             const int32_t* __restrict__ start, int32_t* __restrict__ count,
                                                             int32_t* __restrict__ sidx, uint64_t* __restrict__ skey, double* __restrict__ spts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint64_t key = pkey[i];
    if (key == ~0ull) return;
    const int b = hg_bucket(key, shift);
    const int pos = start[b] + atomicAdd(&count[b], 1);                  // < start[b + 1] <= N: the counts are those of the key pass
    sidx[pos] = i;
    skey[pos] = key;
#pragma unroll
    for (int k = 0; k < 3; ++k) spts[3 * (int64_t)pos + k] = (double)pts[3 * (int64_t)i + k];
}

// After the user's key pass: counts -> first slots (the counts zeroed again), then every taking point into its bucket.  Two launches.
static int hg_sort(const HashGrid& g, const void* points, int points_f64, int N, hipStream_t s) {
    hipLaunchKernelGGL(sdfr_hg_scan_kernel<true>, dim3(1), dim3(HG_SCAN_TPB), 0, s, g.count, g.start, g.T);
    SDFR_LAUNCH_CHECK();
    if (points_f64)
        hipLaunchKernelGGL(sdfr_hg_scatter_kernel<double>, dim3(sdfr_cdiv(N, 256)), dim3(256), 0, s, (const double*)points, N, g.pkey, g.shift, g.start,
                           g.count, g.sidx, g.skey, g.spts);
    else
        hipLaunchKernelGGL(sdfr_hg_scatter_kernel<float>, dim3(sdfr_cdiv(N, 256)), dim3(256), 0, s, (const float*)points, N, g.pkey, g.shift, g.start,
                           g.count, g.sidx, g.skey, g.spts);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

// The 27 cells around a slot's own, for a workgroup of ONE wave per slot of the sorted cloud: first slot, key and running candidate count
// per cell.  The candidates of the walk are numbered 0 ... M - 1 through the 27 bucket ranges one after the other.
struct HgWalk {
    uint64_t ck[27];
    alignas(16) int cpre[28];        // (read in wide words by the prefix and by every candidate)
    int cs[27];
};

// fills w (in LDS) for the cell qkey and returns M; every lane of the wave calls it (two barriers)
__device__ __forceinline__ int hg_walk_cells(HgWalk& w, uint64_t qkey, const int32_t* start, int shift, int lane) {
    if (lane < 27) {
        int s = 0, len = 0;
        uint64_t k = 0;
        if (hg_neighbour_cell(qkey, lane, &k)) {
            const int b = hg_bucket(k, shift);
            s = start[b];
            len = start[b + 1] - s;
        }
        w.cs[lane] = s; w.ck[lane] = k; w.cpre[lane + 1] = len;
    }
    __syncthreads();
    if (lane == 0) {
        w.cpre[0] = 0;
        for (int k = 1; k <= 27; ++k) w.cpre[k] += w.cpre[k - 1];
    }
    __syncthreads();
    return w.cpre[27];
}

// the slot of candidate c < M; false where that slot holds another cell of the same bucket: not this cell's point
__device__ __forceinline__ bool hg_walk_slot(const HgWalk& w, const uint64_t* skey, int c, int* pos) {
    int s = 0;
    for (int k = 1; k < 27; ++k) s += w.cpre[k] <= c ? 1 : 0;            // the cell whose range holds candidate c
    *pos = w.cs[s] + (c - w.cpre[s]);
    return skey[*pos] == w.ck[s];
}
#endif
