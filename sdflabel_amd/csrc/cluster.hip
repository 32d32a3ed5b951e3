// Lidar clusters and rough boxes on the device (gfx950): Euclidean clustering of a (road-free) cloud and a minimum-area rectangle per
// cluster.  The reference has no counterpart to this stage; the semantics are this library's own (include/sdfr.h) and are
// pinned by the numpy restatement tests/_cluster_ref.py.
//
// sdfr_lidar_clusters  participation, fused with the key pass of the hash grid (hash_grid.h, shared with normals.hip: counting sort; no host
//                      sizing, no synchronisation) -> one wave per sorted slot streams the 27 neighbouring cells' buckets 64 candidates at a time and
//                      unites the point with every neighbour of a lower index (union-find with parent[i] <= i, cluster_cells.h) -> flatten:
//                      root and component size per point -> cluster flags, an exclusive scan in index order (= ascending smallest member),
//                      labels -> offsets -> the stable partition into member lists (per-chunk counts, a scan over chunks per cluster, ranks
//                      inside a chunk wave by wave).
// sdfr_cluster_boxes   one workgroup per kept cluster, a direction per thread and loop, members staged through LDS; minima and maxima only.
// The order of a bucket's points depends on the scatter's integer atomics and the order of the unions on the schedule; neither reaches an
// output: the root of a component is its smallest index whatever the order (cluster_cells.h), and everything after the flatten pass is a
// function of the roots.  No float atomic, no sum of floats.  Compiled with -ffp-contract=off.
#include "cluster_cells.h"

struct CluWs {
    HashGrid grid;                   // of the participating points
    int32_t* parent;                 // [N]
    int32_t* root;                   // [N]    -1 for a point that takes no part
    int32_t* csize;                  // [N]    component size, at the root
    int32_t* isc;                    // [N]    1 at the root of a cluster
    int32_t* cid;                    // [N + 1] exclusive scan of isc; cid[N] = clusters found
    int32_t* csz;                    // [C]    size of every kept cluster, 0 beyond
    int32_t* hist;                   // [chunks][C]
};

static int64_t clu_chunks(int64_t N) { return (N + CLU_CHUNK - 1) / CLU_CHUNK; }

static int64_t clu_carve(void* base, int64_t N, int64_t C, CluWs* ws) {
    char* p = (char*)base;
    int64_t at = 0;
    auto take = [&](int64_t bytes) { char* q = p ? p + at : nullptr; at += (bytes + 15) / 16 * 16; return q; };
    CluWs w;
    w.grid = hg_carve(N, take);
    w.parent = (int32_t*)take(N * 4); w.root = (int32_t*)take(N * 4); w.csize = (int32_t*)take(N * 4); w.isc = (int32_t*)take(N * 4);
    w.cid = (int32_t*)take((N + 1) * 4); w.csz = (int32_t*)take(C * 4); w.hist = (int32_t*)take(clu_chunks(N) * C * 4);
    if (ws) *ws = w;
    return at;
}

static bool clu_sizes_ok(int64_t N, int64_t C) {
    return N >= 0 && N <= CLU_MAX_POINTS && C >= 1 && C <= CLU_MAX_CLUSTERS && clu_chunks(N) * C <= CLU_MAX_HIST;
}

__global__ __launch_bounds__(256) void sdfr_clu_init_kernel(int32_t* __restrict__ count, int64_t T, int32_t* __restrict__ csz, int C,
                                                           int32_t* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < T) count[i] = 0;
    if (i < C) csz[i] = 0;
    if (i < 4) counts[i] = 0;
}

// Per input point: participation, the cell key and the bucket's count; every point starts as its own root.
template <typename T>
__global__ __launch_bounds__(256) void sdfr_clu_key_kernel(const T* __restrict__ pts, const uint8_t* __restrict__ mask, int N, double cell, int shift,
                                                          uint64_t* __restrict__ pkey, int32_t* __restrict__ count, int32_t* __restrict__ parent,
                                                          int32_t* __restrict__ csize, int32_t* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double X = (double)pts[3 * (int64_t)i], Y = (double)pts[3 * (int64_t)i + 1], Z = (double)pts[3 * (int64_t)i + 2];
    const int part = clu_takes_part(mask ? mask[i] != 0 : 1, X, Y, Z);
    parent[i] = i;
    csize[i] = 0;
    hg_key_point(part == 1, X, Y, Z, cell, shift, i, pkey, count);
    if (part == 2) atomicOr(&counts[3], CLU_FLAG_NONFINITE);
}

// One wave per slot of the sorted cloud: unite the slot's point i with every neighbour j < i (every edge is seen from its larger end).
// TERMINATION AND RESULT: cluster_cells.h, at clu_find / clu_union.  parent[i] <= i always; every write lowers a value; clu_find descends
// strictly, clu_union retries from a strictly smaller index: no lane waits for another lane, wave or workgroup.  parent is read and written
// through agent-scope atomics only, so a stale cached line is never read; the algorithm would still be right with one (an old parent is an
// ancestor all the same, and the compare-and-swap decides).
__global__ __launch_bounds__(64) void sdfr_clu_union_kernel(const int32_t* __restrict__ start, int64_t T, int shift, const int32_t* __restrict__ sidx,
                                                           const uint64_t* __restrict__ skey, const double* __restrict__ spts, double e2,
                                                           int32_t* parent) {
    __shared__ HgWalk cells;
    const int w = blockIdx.x, lane = threadIdx.x;
    if (w >= start[T]) return;                                           // (the same for the whole wave)
    const int i = sidx[w];
    const double q[3] = {spts[3 * (int64_t)w], spts[3 * (int64_t)w + 1], spts[3 * (int64_t)w + 2]};
    const int M = hg_walk_cells(cells, skey[w], start, shift, lane);
    for (int base = 0; base < M; base += 64) {
        const int c = base + lane;
        if (c >= M) continue;
        int pos;
        if (!hg_walk_slot(cells, skey, c, &pos)) continue;
        const int j = sidx[pos];
        if (j >= i) continue;
        const double p[3] = {spts[3 * (int64_t)pos], spts[3 * (int64_t)pos + 1], spts[3 * (int64_t)pos + 2]};
        if (hg_d2(p, q) < e2) clu_union(parent, i, j);
    }
}

// Per input point: its root (the component's smallest index), the component's size at the root, the counts of points and components.
__global__ __launch_bounds__(256) void sdfr_clu_flatten_kernel(int N, const uint64_t* __restrict__ pkey, int32_t* parent, int32_t* __restrict__ root,
                                                              int32_t* __restrict__ csize, int32_t* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int r = -1;
    if (i < N && pkey[i] != ~0ull) {
        r = clu_find(parent, i);
        atomicAdd(&csize[r], 1);
    }
    if (i < N) root[i] = r;
    const unsigned long long part = __ballot(r >= 0), roots = __ballot(r >= 0 && r == i);
    if ((threadIdx.x & 63) == 0) {
        if (part) atomicAdd(&counts[0], (int)__popcll(part));
        if (roots) atomicAdd(&counts[1], (int)__popcll(roots));
    }
}

__global__ __launch_bounds__(256) void sdfr_clu_mark_kernel(int N, const int32_t* __restrict__ root, const int32_t* __restrict__ csize, int min_points,
                                                           int max_points, int32_t* __restrict__ isc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) isc[i] = root[i] == i && clu_is_cluster(csize[i], min_points, max_points) ? 1 : 0;
}

__global__ __launch_bounds__(256) void sdfr_clu_label_kernel(int N, const int32_t* __restrict__ root, const int32_t* __restrict__ csize,
                                                            const int32_t* __restrict__ isc, const int32_t* __restrict__ cid, int C,
                                                            int32_t* __restrict__ label, int32_t* __restrict__ csz, int32_t* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int r = root[i];
    const int32_t l = clu_label(r, isc, cid, C);
    label[i] = l;
    if (r == i && l >= 0) csz[l] = csize[i];                             // l < C
    if (i == 0) {
        const int found = cid[N];
        counts[2] = found;
        if (found > C) atomicOr(&counts[3], CLU_FLAG_CAPPED);
    }
}

// Per chunk of 1024 points: how many of them carry each kept label.
__global__ __launch_bounds__(CLU_CHUNK) void sdfr_clu_hist_kernel(int N, const int32_t* __restrict__ label, int C, int32_t* __restrict__ hist) {
    __shared__ int h[CLU_MAX_CLUSTERS];
    const int t = threadIdx.x, i = blockIdx.x * CLU_CHUNK + t;
    for (int c = t; c < C; c += CLU_CHUNK) h[c] = 0;
    __syncthreads();
    const int l = i < N ? label[i] : -1;
    if (l >= 0 && l < C) atomicAdd(&h[l], 1);
    __syncthreads();
    for (int c = t; c < C; c += CLU_CHUNK) hist[(int64_t)blockIdx.x * C + c] = h[c];
}

// Per cluster: its chunk counts become the first member slot of every chunk.
__global__ __launch_bounds__(256) void sdfr_clu_chunk_scan_kernel(int chunks, int C, const int32_t* __restrict__ off, int32_t* __restrict__ hist) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    int base = off[c];
    for (int ch = 0; ch < chunks; ++ch) {
        const int64_t at = (int64_t)ch * C + c;
        const int n = hist[at];
        hist[at] = base;
        base += n;
    }
}

// Per chunk: the members' slots.  A point's slot is its chunk's first slot for its label, plus the points of that label in the waves before
// its own (run[], wave after wave), plus those in the lanes before its own (a ballot per distinct label of the wave): ascending input index.
__global__ __launch_bounds__(CLU_CHUNK) void sdfr_clu_members_kernel(int N, const int32_t* __restrict__ label, int C, const int32_t* __restrict__ hist,
                                                                    int32_t* __restrict__ members) {
    __shared__ int run[CLU_MAX_CLUSTERS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, i = blockIdx.x * CLU_CHUNK + t;
    for (int c = t; c < C; c += CLU_CHUNK) run[c] = 0;
    int l = i < N ? label[i] : -1;
    if (l >= C) l = -1;
    int rank = 0, cnt = 0;
    bool last = false;
    unsigned long long todo = __ballot(l >= 0);
    while (todo) {                                                       // (uniform over the wave)
        const int leader = __ffsll((long long)todo) - 1;
        const int ll = __shfl(l, leader);
        const unsigned long long same = __ballot(l == ll);
        if (l == ll) {
            rank = (int)__popcll(same & ((1ull << lane) - 1ull));
            cnt = (int)__popcll(same);
            last = (same >> lane) == 1ull;
        }
        todo &= ~same;
    }
    __syncthreads();
    for (int w = 0; w < CLU_CHUNK / 64; ++w) {
        int before = 0;
        if (wave == w && l >= 0) {
            before = run[l];
            members[hist[(int64_t)blockIdx.x * C + l] + before + rank] = i;      // < off[kept] <= N: the counts are those of the labels
        }
        __syncthreads();
        if (wave == w && l >= 0 && last) run[l] = before + cnt;
        __syncthreads();
    }
}

// One workgroup per kept cluster: thread t holds the extents of the directions t, t + 256, ...; the members go through LDS 256 at a time.
template <typename T>
__global__ __launch_bounds__(CLU_BOX_TPB) void sdfr_clu_boxes_kernel(const T* __restrict__ pts, int N, const int32_t* __restrict__ members,
                                                                    const int32_t* __restrict__ off, const int32_t* __restrict__ counts, int C,
                                                                    const double* __restrict__ dirs, int K, double* __restrict__ rect) {
    __shared__ double sx[CLU_BOX_TPB], sy[CLU_BOX_TPB], sz[CLU_BOX_TPB], sarea[CLU_MAX_DIRS];
    __shared__ int swin;
    const int c = blockIdx.x, t = threadIdx.x;
    const int found = counts[2];
    if (c >= (found < C ? found : C)) return;                            // (the same for the whole workgroup)
    int m0 = off[c], m1 = off[c + 1];
    if (m0 < 0) m0 = 0;
    if (m1 > N) m1 = N;
    double dc[CLU_BOX_LOOPS], ds[CLU_BOX_LOOPS];
    CluExt eu[CLU_BOX_LOOPS], ev[CLU_BOX_LOOPS], ey;
    clu_ext_start(&ey);
#pragma unroll
    for (int q = 0; q < CLU_BOX_LOOPS; ++q) {
        const int k = t + q * CLU_BOX_TPB;
        dc[q] = k < K ? dirs[2 * k] : 0.0;
        ds[q] = k < K ? dirs[2 * k + 1] : 0.0;
        clu_ext_start(&eu[q]);
        clu_ext_start(&ev[q]);
    }
    for (int base = m0; base < m1; base += CLU_BOX_TPB) {
        const int n = m1 - base < CLU_BOX_TPB ? m1 - base : CLU_BOX_TPB;
        __syncthreads();
        if (t < n) {
            int j = members[base + t];
            if (j < 0 || j >= N) j = 0;                                  // (never with sdfr_lidar_clusters' members)
            sx[t] = (double)pts[3 * (int64_t)j]; sy[t] = (double)pts[3 * (int64_t)j + 1]; sz[t] = (double)pts[3 * (int64_t)j + 2];
        }
        __syncthreads();
        for (int p = 0; p < n; ++p) {
            const double x = sx[p], z = sz[p];
            clu_ext_add(&ey, sy[p]);
#pragma unroll
            for (int q = 0; q < CLU_BOX_LOOPS; ++q) {
                if (t + q * CLU_BOX_TPB < K) {
                    double u, v;
                    clu_uv(x, z, dc[q], ds[q], &u, &v);
                    clu_ext_add(&eu[q], u);
                    clu_ext_add(&ev[q], v);
                }
            }
        }
    }
    clu_ext_end(&ey);
#pragma unroll
    for (int q = 0; q < CLU_BOX_LOOPS; ++q) {
        const int k = t + q * CLU_BOX_TPB;
        clu_ext_end(&eu[q]);
        clu_ext_end(&ev[q]);
        if (k < K) sarea[k] = clu_area(&eu[q], &ev[q]);
    }
    __syncthreads();
    if (t == 0) {                                                        // the first k of the smallest area
        int win = 0;
        double best = sarea[0];
        for (int k = 1; k < K; ++k)
            if (sarea[k] < best) { best = sarea[k]; win = k; }
        swin = win;
    }
    __syncthreads();
    const int win = swin;
    if (win % CLU_BOX_TPB != t) return;
    double* o = rect + (int64_t)c * CLU_RECT;
#pragma unroll
    for (int q = 0; q < CLU_BOX_LOOPS; ++q)
        if (q == win / CLU_BOX_TPB) {
            o[0] = (double)win; o[1] = eu[q].lo; o[2] = eu[q].hi; o[3] = ev[q].lo; o[4] = ev[q].hi; o[5] = ey.lo; o[6] = ey.hi;
            o[7] = sarea[win];
        }
}

extern "C" int64_t sdfr_cluster_ws_bytes(int N, int max_clusters) {
    if (!clu_sizes_ok(N, max_clusters)) return -1;
    return clu_carve(nullptr, N, max_clusters, nullptr);
}

extern "C" int sdfr_lidar_clusters(const void* points, int points_f64, int N, const uint8_t* mask, float eps32, int min_points, int max_points,
                                   int max_clusters, int32_t* label, int32_t* members, int32_t* off, int32_t* counts, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    SDFR_REQUIRE(N >= 0 && N <= CLU_MAX_POINTS, "sdfr_lidar_clusters: bad point count");
    SDFR_REQUIRE(max_clusters >= 1 && max_clusters <= CLU_MAX_CLUSTERS, "sdfr_lidar_clusters: max_clusters must be 1 ... %d", CLU_MAX_CLUSTERS);
    SDFR_REQUIRE(clu_sizes_ok(N, max_clusters), "sdfr_lidar_clusters: too many points for this many clusters (sdfr_cluster_ws_bytes)");
    const double eps = (double)eps32;
    SDFR_REQUIRE(eps > 0.0 && eps < INFINITY, "sdfr_lidar_clusters: eps must be positive and finite");
    SDFR_REQUIRE(off && counts && workspace && (N == 0 || (points && label && members)), "sdfr_lidar_clusters: NULL argument");
    SDFR_REQUIRE(((uintptr_t)workspace & 15) == 0, "sdfr_lidar_clusters: the workspace must be 16-byte aligned");
    CluWs ws;
    SDFR_REQUIRE(workspace_bytes >= clu_carve(workspace, N, max_clusters, &ws), "sdfr_lidar_clusters: workspace too small (sdfr_cluster_ws_bytes)");
    HashGrid& g = ws.grid;
    g.cell = hg_cell_width(eps);
    hipStream_t s = (hipStream_t)stream;
    const int C = max_clusters, chunks = (int)clu_chunks(N);
    const int64_t ninit = g.T > C ? g.T : C;
    hipLaunchKernelGGL(sdfr_clu_init_kernel, dim3(sdfr_cdiv(ninit, 256)), dim3(256), 0, s, g.count, g.T, ws.csz, C, counts);
    SDFR_LAUNCH_CHECK();
    if (N > 0) {
        const dim3 per_point(sdfr_cdiv(N, 256));
        if (points_f64)
            hipLaunchKernelGGL(sdfr_clu_key_kernel<double>, per_point, dim3(256), 0, s, (const double*)points, mask, N, g.cell, g.shift, g.pkey, g.count,
                               ws.parent, ws.csize, counts);
        else
            hipLaunchKernelGGL(sdfr_clu_key_kernel<float>, per_point, dim3(256), 0, s, (const float*)points, mask, N, g.cell, g.shift, g.pkey, g.count,
                               ws.parent, ws.csize, counts);
        SDFR_LAUNCH_CHECK();
        const int sorted = hg_sort(g, points, points_f64, N, s);
        if (sorted != SDFR_OK) return sorted;
        hipLaunchKernelGGL(sdfr_clu_union_kernel, dim3(N), dim3(64), 0, s, g.start, g.T, g.shift, g.sidx, g.skey, g.spts, eps * eps, ws.parent);
        SDFR_LAUNCH_CHECK();
        hipLaunchKernelGGL(sdfr_clu_flatten_kernel, per_point, dim3(256), 0, s, N, g.pkey, ws.parent, ws.root, ws.csize, counts);
        SDFR_LAUNCH_CHECK();
        hipLaunchKernelGGL(sdfr_clu_mark_kernel, per_point, dim3(256), 0, s, N, ws.root, ws.csize, min_points, max_points, ws.isc);
        SDFR_LAUNCH_CHECK();
        hipLaunchKernelGGL(sdfr_hg_scan_kernel<false>, dim3(1), dim3(HG_SCAN_TPB), 0, s, ws.isc, ws.cid, (int64_t)N);
        SDFR_LAUNCH_CHECK();
        hipLaunchKernelGGL(sdfr_clu_label_kernel, per_point, dim3(256), 0, s, N, ws.root, ws.csize, ws.isc, ws.cid, C, label, ws.csz, counts);
        SDFR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sdfr_hg_scan_kernel<false>, dim3(1), dim3(HG_SCAN_TPB), 0, s, ws.csz, off, (int64_t)C);
    SDFR_LAUNCH_CHECK();
    if (N > 0) {
        hipLaunchKernelGGL(sdfr_clu_hist_kernel, dim3(chunks), dim3(CLU_CHUNK), 0, s, N, label, C, ws.hist);
        SDFR_LAUNCH_CHECK();
        hipLaunchKernelGGL(sdfr_clu_chunk_scan_kernel, dim3(sdfr_cdiv(C, 256)), dim3(256), 0, s, chunks, C, off, ws.hist);
        SDFR_LAUNCH_CHECK();
        hipLaunchKernelGGL(sdfr_clu_members_kernel, dim3(chunks), dim3(CLU_CHUNK), 0, s, N, label, C, ws.hist, members);
        SDFR_LAUNCH_CHECK();
    }
    return SDFR_OK;
}

extern "C" int sdfr_cluster_boxes(const void* points, int points_f64, int N, const int32_t* members, const int32_t* off, const int32_t* counts,
                                  int max_clusters, const double* dirs, int K, double* rect, void* stream) {
    SDFR_REQUIRE(N >= 0 && N <= CLU_MAX_POINTS, "sdfr_cluster_boxes: bad point count");
    SDFR_REQUIRE(max_clusters >= 1 && max_clusters <= CLU_MAX_CLUSTERS, "sdfr_cluster_boxes: max_clusters must be 1 ... %d", CLU_MAX_CLUSTERS);
    SDFR_REQUIRE(K >= 1 && K <= CLU_MAX_DIRS, "sdfr_cluster_boxes: the direction table must hold 1 ... %d directions", CLU_MAX_DIRS);
    if (N == 0) return SDFR_OK;                                          // no point, no cluster, no row to write
    SDFR_REQUIRE(points && members && off && counts && dirs && rect, "sdfr_cluster_boxes: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    if (points_f64)
        hipLaunchKernelGGL(sdfr_clu_boxes_kernel<double>, dim3(max_clusters), dim3(CLU_BOX_TPB), 0, s, (const double*)points, N, members, off, counts,
                           max_clusters, dirs, K, rect);
    else
        hipLaunchKernelGGL(sdfr_clu_boxes_kernel<float>, dim3(max_clusters), dim3(CLU_BOX_TPB), 0, s, (const float*)points, N, members, off, counts,
                           max_clusters, dirs, K, rect);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
