// Per-element rules of the lidar clusters and rough boxes (cluster.hip).  DESIGN.md 7n has the rules and the arguments.
// Everything here is a plain function of one point, one pair, one component or one (point, direction), compiled for the device by cluster.hip
// and for the host by tests/cluster_host/cluster_host.cpp, which runs the threads as loops and is compared with the numpy restatement
// (tests/_cluster_ref.py) bit for bit.  Both translation units are compiled with -ffp-contract=off: every operation rounds separately.
// The hash grid and the distance rule are hash_grid.h's (hg_*), shared with normals.hip and compiled for the host through this header.
#pragma once
#include "hash_grid.h"

#if defined(__HIPCC__)
#define CLU_HD __host__ __device__ inline
#else
#define CLU_HD static inline
#endif

#define CLU_CHUNK 1024                  // points per chunk of the stable partition
#define CLU_MAX_POINTS (1 << 24)
#define CLU_MAX_CLUSTERS 4096           // one LDS counter per kept cluster
#define CLU_MAX_HIST (1 << 26)          // chunks * max_clusters of the partition's table
#define CLU_FLAG_CAPPED 1               // counts[3] bit 1: more clusters than max_clusters
#define CLU_FLAG_NONFINITE 2            // counts[3] bit 2: a non-finite point under a set mask was left out
#define CLU_BOX_TPB 256                 // threads of a rectangle workgroup: one direction per thread and loop
#define CLU_BOX_LOOPS 4
#define CLU_MAX_DIRS (CLU_BOX_TPB * CLU_BOX_LOOPS)
#define CLU_RECT 8                      // k, u_min, u_max, v_min, v_max, y_min, y_max, area

CLU_HD bool clu_finite(double a) { return fabs(a) <= 1.7976931348623157e308; }                  // false for NaN and the infinities

// 1: the point takes part; 0: masked out; 2: its mask is set but a coordinate is not finite (left out, flag bit 2)
CLU_HD int clu_takes_part(int masked_in, double x, double y, double z) {
    if (!masked_in) return 0;
    return clu_finite(x) && clu_finite(y) && clu_finite(z) ? 1 : 2;
}

// ---- union-find over input indices ------------------------------------------------------------------------------------------------------
// INVARIANT: parent[i] <= i at all times.  Every write LOWERS a value: clu_find shortens a path by an integer atomic minimum with an ancestor
// (which is smaller), clu_union hooks a root a under a smaller index b by a compare-and-swap of parent[a] from a to b.  So (1) a walk
// x -> parent[x] strictly descends and ends after at most x steps, whatever other threads write meanwhile; (2) a failed compare-and-swap
// returns a value below a, the retry starts from it, and the larger of the two indices in hand strictly descends from retry to retry: no
// loop waits for another thread.  (3) Every tree has exactly one index with parent[i] == i, and the smallest index m of a tree has
// parent[m] <= m, hence == m: once all unions are done the root of every component is its smallest input index, whichever order they ran in.
// On the host (the test program) the same code runs with plain loads and stores, one thread after the other.
#if defined(__HIP_DEVICE_COMPILE__)
#define CLU_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define CLU_MIN(p, v) atomicMin((p), (v))
#define CLU_CAS(p, c, v) atomicCAS((p), (c), (v))
#else
#define CLU_LOAD(p) (*(p))
static inline int32_t clu_host_cas(int32_t* p, int32_t c, int32_t v) { const int32_t o = *p; if (o == c) *p = v; return o; }
static inline void clu_host_min(int32_t* p, int32_t v) { if (v < *p) *p = v; }
#define CLU_MIN(p, v) clu_host_min((p), (v))
#define CLU_CAS(p, c, v) clu_host_cas((p), (c), (v))
#endif

CLU_HD int32_t clu_find(int32_t* parent, int32_t x) {
    int32_t p = CLU_LOAD(parent + x);
    while (p != x) {                                                     // p < x
        const int32_t g = CLU_LOAD(parent + p);
        if (g != p) CLU_MIN(parent + x, g);                              // g < p < x: x now points at least as high up its own path
        x = p;
        p = g;
    }
    return x;
}

CLU_HD void clu_union(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = clu_find(parent, a);
        b = clu_find(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = CLU_CAS(parent + a, a, b);                   // hook the larger root under the smaller index
        if (old == a) return;
        a = old;                                                         // a was hooked by somebody else meanwhile: old < a, go on from there
    }
}

// ---- clusters ---------------------------------------------------------------------------------------------------------------------------
CLU_HD bool clu_is_cluster(int size, int min_points, int max_points) { return size >= min_points && (max_points <= 0 || size <= max_points); }

// the label of a point whose component has the root `root` (-1: the point takes no part), given the root's cluster flag and number
CLU_HD int32_t clu_label(int32_t root, const int32_t* is_cluster, const int32_t* cid, int max_clusters) {
    if (root < 0 || !is_cluster[root]) return -1;
    const int32_t c = cid[root];
    return c < max_clusters ? c : -1;
}

// ---- rectangles -------------------------------------------------------------------------------------------------------------------------
struct CluExt {
    double lo, hi;
};

CLU_HD void clu_ext_start(CluExt* e) { e->lo = INFINITY; e->hi = -INFINITY; }
CLU_HD void clu_ext_add(CluExt* e, double a) {
    if (a < e->lo) e->lo = a;
    if (a > e->hi) e->hi = a;
}
// a zero comes out as +0 whichever of -0 and +0 came first, so the extent is a function of the SET of values
CLU_HD void clu_ext_end(CluExt* e) { e->lo = e->lo + 0.0; e->hi = e->hi + 0.0; }

// u along (cos, sin), v along (-sin, cos) in the camera's (x, z); one rounding per statement
CLU_HD void clu_uv(double x, double z, double c, double s, double* u, double* v) {
    double a = x * c;
    double b = z * s;
    *u = a + b;
    a = z * c;
    b = x * s;
    *v = a - b;
}

CLU_HD double clu_area(const CluExt* u, const CluExt* v) {
    const double du = u->hi - u->lo;
    const double dv = v->hi - v->lo;
    return du * dv;
}
