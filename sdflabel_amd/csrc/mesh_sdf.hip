// Signed distances from query points to triangle meshes, and area-weighted points on their surfaces ("Signed distances to
// meshes").  The per-triangle, per-point arithmetic is mesh_sdf_cells.h; this file holds the launches.
//
//   sdfr_mesh_sdf             B ragged meshes, each with its own run of query points.  All pairs, float64.  One query point per thread, one
//                             workgroup per MSDF_BLOCK points of one mesh (a block table over qoff, built on the device); the mesh's triangles
//                             pass through LDS in tiles of MSDF_TILE, nine doubles each, converted and validated once per tile by the thread
//                             that stages them; every lane then reads the same LDS address (a broadcast).  Nearest triangle and winding sum
//                             are kept per chunk of MSDF_CHUNK triangles and folded in chunk order.  With few points and many triangles the
//                             grid gets a second dimension over the chunks: per-chunk partials go to the workspace and a second launch
//                             folds them in the same order, so both shapes give the same bits.
//   sdfr_mesh_surface_points  cumulative triangle areas in a fixed order (sequential inside chunks of MSDF_AREA_CHUNK, sequential over the chunk
//                             totals), then one thread per sample: binary search, barycentric point.
//
// No atomics and no floating-point reduction across lanes: the same bits on every run, and a mesh's results do not depend on the batch
// around it.  Compiled with -ffp-contract=off (build.sh).
#include "sdfr_common.h"
#include "mesh_sdf_cells.h"

#define MSDF_BLOCK 256               // threads per workgroup = query points per workgroup; equals MSDF_TILE: a thread stages one triangle
#define MSDF_SPLIT_POINTS 2048       // at most this many query points in all (and more than one chunk of triangles): the chunk-split shape
#define MSDF_MAX_GRID_Y 65535

static_assert(MSDF_BLOCK == MSDF_TILE && MSDF_CHUNK % MSDF_TILE == 0 && MSDF_BLOCK == MSDF_AREA_CHUNK, "tile geometry");

namespace {

struct MsdfArgs {
    const float* vertices;       // [V][3]
    const int32_t* faces;        // [T][3], indices local to the mesh
    const int64_t* voff;         // [B + 1]
    const int64_t* toff;         // [B + 1]
    const float* points;         // [N][3] query points, or [S][3] uniforms
    const int64_t* qoff;         // [B + 1]
    int64_t V, T, N;
    int B;
};

__device__ __forceinline__ bool msdf_mesh_ok(const MsdfArgs& a, int b) { return msdf_run_ok(a.voff + b, a.V) && msdf_run_ok(a.toff + b, a.T); }

// OR of one int per thread over the workgroup, in a fixed tree; valid in every thread
__device__ __forceinline__ int msdf_block_or(int v, int* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int o = MSDF_BLOCK / 2; o > 0; o >>= 1) {
        if (t < o) sh[t] |= sh[t + o];
        __syncthreads();
    }
    return sh[0];
}

// the flags of mesh b from a scan of its triangles (uniform over the workgroup)
__device__ __forceinline__ int msdf_mesh_flags(const MsdfArgs& a, int b, int* sh) {
    int f = 0;
    if (!msdf_mesh_ok(a, b)) {
        f = MSDF_FLAG_INVALID;
    } else {
        const int64_t t0 = a.toff[b], nt = a.toff[b + 1] - t0, v0 = a.voff[b], nv = a.voff[b + 1] - v0;
        double tri[9];
        for (int64_t t = threadIdx.x; t < nt; t += MSDF_BLOCK) f |= msdf_tri_load(a.vertices + 3 * v0, nv, a.faces + 3 * (t0 + t), tri);
    }
    return msdf_block_or(f, sh);
}

// Launch 1 of sdfr_mesh_sdf: defaults into every output row, the flags of every mesh, the block table.
//   boff[b + 1] - boff[b] = workgroups of mesh b: ceil(points / MSDF_BLOCK) for a mesh with usable offsets and at least one triangle, else 0
//   (its points keep the defaults).  The sum is at most ceil(N / MSDF_BLOCK) + B, the main launch's grid.
__global__ __launch_bounds__(MSDF_BLOCK) void sdfr_mesh_sdf_init_kernel(MsdfArgs a, int64_t* __restrict__ boff, float* __restrict__ sdf,
                                                                        float* __restrict__ dist, double* __restrict__ d2,
                                                                        int32_t* __restrict__ nearest, double* __restrict__ winding,
                                                                        int32_t* __restrict__ flags) {
    __shared__ int sh[MSDF_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * MSDF_BLOCK + threadIdx.x;
    if (i < a.N) {
        MsdfRun r;
        msdf_run_init(&r);
        msdf_finish(&r, false, &sdf[i], dist ? &dist[i] : nullptr, d2 ? &d2[i] : nullptr, nearest ? &nearest[i] : nullptr,
                    winding ? &winding[i] : nullptr);
    }
    if ((int)blockIdx.x < a.B) {
        const int f = msdf_mesh_flags(a, (int)blockIdx.x, sh);
        if (threadIdx.x == 0) flags[blockIdx.x] = f;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int64_t s = 0;
        boff[0] = 0;
        for (int b = 0; b < a.B; ++b) {
            const bool ok = msdf_mesh_ok(a, b) && msdf_run_ok(a.qoff + b, a.N) && a.toff[b + 1] > a.toff[b];
            if (ok) s += (a.qoff[b + 1] - a.qoff[b] + MSDF_BLOCK - 1) / MSDF_BLOCK;
            boff[b + 1] = s;
        }
    }
}

// the mesh and the query point of this thread; false for a workgroup beyond the table (uniform).  *q may lie beyond the mesh's run.
__device__ __forceinline__ bool msdf_locate(const MsdfArgs& a, const int64_t* boff, int* b, int64_t* q) {
    const int64_t bid = blockIdx.x;
    if (bid >= boff[a.B]) return false;
    *b = verify_owner(boff, a.B, bid);
    *q = a.qoff[*b] + (bid - boff[*b]) * MSDF_BLOCK + threadIdx.x;
    return true;
}

// SPLIT 0: the workgroup walks every chunk of its mesh and writes the outputs.  SPLIT 1: blockIdx.y is the chunk; the partial goes to
// pd2 / psum / pidx [chunk][N].
template <bool SIGN, bool SPLIT>
__global__ __launch_bounds__(MSDF_BLOCK) void sdfr_mesh_sdf_kernel(MsdfArgs a, const int64_t* __restrict__ boff, float* __restrict__ sdf,
                                                                   float* __restrict__ dist, double* __restrict__ d2,
                                                                   int32_t* __restrict__ nearest, double* __restrict__ winding,
                                                                   double* __restrict__ pd2, double* __restrict__ psum,
                                                                   int32_t* __restrict__ pidx) {
    __shared__ double tile[MSDF_TILE * 9];
    int b;
    int64_t q;
    if (!msdf_locate(a, boff, &b, &q)) return;
    const int64_t t0 = a.toff[b], nt = a.toff[b + 1] - t0, v0 = a.voff[b], nv = a.voff[b + 1] - v0;      // a mesh in the table has usable offsets
    int64_t lo = 0, hi = nt;
    if (SPLIT) {
        lo = (int64_t)blockIdx.y * MSDF_CHUNK;
        if (lo >= nt) return;                                              // uniform
        hi = lo + MSDF_CHUNK < nt ? lo + MSDF_CHUNK : nt;
    }
    const bool mine = q < a.qoff[b + 1];
    double p[3] = {0.0, 0.0, 0.0};
    bool live = mine;
    if (mine) {
        for (int k = 0; k < 3; ++k) p[k] = (double)a.points[3 * q + k];
        live = verify_finite(p[0]) && verify_finite(p[1]) && verify_finite(p[2]);
    }
    MsdfRun r, c;
    msdf_run_init(&r);
    msdf_run_init(&c);
    for (int64_t tile0 = lo; tile0 < hi; tile0 += MSDF_TILE) {
        __syncthreads();
        {
            double tri[9];
            const int64_t t = tile0 + threadIdx.x;
            const bool ok = t < hi && msdf_tri_load(a.vertices + 3 * v0, nv, a.faces + 3 * (t0 + t), tri) == 0;
            if (!ok) tri[0] = (double)NAN;                                 // the mark of a skipped triangle: a usable one is finite
            for (int i = 0; i < 9; ++i) tile[9 * threadIdx.x + i] = ok || i == 0 ? tri[i] : 0.0;
        }
        __syncthreads();
        const int n = hi - tile0 < MSDF_TILE ? (int)(hi - tile0) : MSDF_TILE;
        if (live) {
            for (int j = 0; j < n; ++j) {
                const double* tr = tile + 9 * j;                           // the same address in every lane
                if (tr[0] == tr[0]) msdf_run_tri(&c, p, tr, (int32_t)(tile0 + j), SIGN);
            }
        }
        if (!SPLIT && ((tile0 + MSDF_TILE) % MSDF_CHUNK == 0 || tile0 + MSDF_TILE >= hi)) {
            msdf_run_fold(&r, &c);
            msdf_run_init(&c);
        }
    }
    if (!mine) return;
    if (SPLIT) {
        const int64_t at = (int64_t)blockIdx.y * a.N + q;
        pd2[at] = c.d2, psum[at] = c.sum, pidx[at] = c.idx;
    } else {
        msdf_finish(&r, SIGN, &sdf[q], dist ? &dist[q] : nullptr, d2 ? &d2[q] : nullptr, nearest ? &nearest[q] : nullptr,
                    winding ? &winding[q] : nullptr);
    }
}

// the chunk partials of a point folded in chunk order
__global__ __launch_bounds__(MSDF_BLOCK) void sdfr_mesh_sdf_fold_kernel(MsdfArgs a, const int64_t* __restrict__ boff, int want_sign,
                                                                        const double* __restrict__ pd2, const double* __restrict__ psum,
                                                                        const int32_t* __restrict__ pidx, float* __restrict__ sdf,
                                                                        float* __restrict__ dist, double* __restrict__ d2,
                                                                        int32_t* __restrict__ nearest, double* __restrict__ winding) {
    int b;
    int64_t q;
    if (!msdf_locate(a, boff, &b, &q) || q >= a.qoff[b + 1]) return;
    const int64_t nt = a.toff[b + 1] - a.toff[b];
    const int64_t nch = (nt + MSDF_CHUNK - 1) / MSDF_CHUNK;
    MsdfRun r;
    msdf_run_init(&r);
    for (int64_t ch = 0; ch < nch; ++ch) {
        const int64_t at = ch * a.N + q;
        const MsdfRun c = {pd2[at], psum[at], pidx[at]};
        msdf_run_fold(&r, &c);
    }
    msdf_finish(&r, want_sign != 0, &sdf[q], dist ? &dist[q] : nullptr, d2 ? &d2[q] : nullptr, nearest ? &nearest[q] : nullptr,
                winding ? &winding[q] : nullptr);
}

// ---- surface sampler ---------------------------------------------------------------------------------------------------------------------

// coff[b + 1] - coff[b] = area chunks of mesh b (0 for unusable offsets); at most ceil(T / MSDF_AREA_CHUNK) + B in all
__global__ void sdfr_mesh_surface_table_kernel(MsdfArgs a, int64_t* __restrict__ coff) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t s = 0;
    coff[0] = 0;
    for (int b = 0; b < a.B; ++b) {
        if (msdf_mesh_ok(a, b)) s += (a.toff[b + 1] - a.toff[b] + MSDF_AREA_CHUNK - 1) / MSDF_AREA_CHUNK;
        coff[b + 1] = s;
    }
}

// one workgroup per area chunk: the areas in parallel, their running sum by one thread
__global__ __launch_bounds__(MSDF_BLOCK) void sdfr_mesh_surface_area_kernel(MsdfArgs a, const int64_t* __restrict__ coff,
                                                                            double* __restrict__ local, double* __restrict__ tot,
                                                                            int32_t* __restrict__ cflag) {
    __shared__ double sh[MSDF_AREA_CHUNK];
    __shared__ int shf[MSDF_AREA_CHUNK];
    const int64_t cb = blockIdx.x;
    if (cb >= coff[a.B]) return;
    const int b = verify_owner(coff, a.B, cb);
    const int64_t t0 = a.toff[b], nt = a.toff[b + 1] - t0, v0 = a.voff[b], nv = a.voff[b + 1] - v0;
    const int64_t t = (cb - coff[b]) * MSDF_AREA_CHUNK + threadIdx.x;
    double area = 0.0;
    int f = 0;
    if (t < nt) {
        double tri[9];
        f = msdf_tri_load(a.vertices + 3 * v0, nv, a.faces + 3 * (t0 + t), tri);
        if (f == 0) area = msdf_area(tri);
    }
    sh[threadIdx.x] = area, shf[threadIdx.x] = f;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        int g = 0;
        for (int i = 0; i < MSDF_AREA_CHUNK; ++i) {
            s += sh[i];
            sh[i] = s;
            g |= shf[i];
        }
        tot[cb] = s, cflag[cb] = g;
    }
    __syncthreads();
    if (t < nt) local[t0 + t] = sh[threadIdx.x];
}

// one thread per mesh: the exclusive running sum of its chunk totals, and its flags
__global__ __launch_bounds__(MSDF_BLOCK) void sdfr_mesh_surface_base_kernel(MsdfArgs a, const int64_t* __restrict__ coff,
                                                                            const double* __restrict__ tot, const int32_t* __restrict__ cflag,
                                                                            double* __restrict__ base, int32_t* __restrict__ flags) {
    const int b = blockIdx.x * MSDF_BLOCK + threadIdx.x;
    if (b >= a.B) return;
    double s = 0.0;
    int f = msdf_mesh_ok(a, b) ? 0 : MSDF_FLAG_INVALID;
    for (int64_t k = coff[b]; k < coff[b + 1]; ++k) {
        base[k] = s;
        s += tot[k];
        f |= cflag[k];
    }
    if (!(s > 0.0)) f |= MSDF_FLAG_INVALID;
    flags[b] = f;
}

__global__ __launch_bounds__(MSDF_BLOCK) void sdfr_mesh_surface_sample_kernel(MsdfArgs a, const int64_t* __restrict__ coff,
                                                                              const double* __restrict__ local, const double* __restrict__ base,
                                                                              float* __restrict__ points, int32_t* __restrict__ triangle) {
    const int64_t s = (int64_t)blockIdx.x * MSDF_BLOCK + threadIdx.x;
    if (s >= a.N) return;
    const int b = verify_owner(a.qoff, a.B, s);
    float x[3] = {0.0f, 0.0f, 0.0f};
    int64_t t = -1;
    if (msdf_mesh_ok(a, b)) {
        const int64_t t0 = a.toff[b], nt = a.toff[b + 1] - t0, v0 = a.voff[b], nv = a.voff[b + 1] - v0;
        t = msdf_pick(local + t0, base + coff[b], nt, a.points + 3 * s);
        double tri[9];
        if (t >= 0 && msdf_tri_load(a.vertices + 3 * v0, nv, a.faces + 3 * (t0 + t), tri) == 0)      // (a chosen triangle has area: it was loaded before)
            msdf_surface_point(tri, a.points[3 * s + 1], a.points[3 * s + 2], x);
        else
            t = -1;
    }
    points[3 * s] = x[0], points[3 * s + 1] = x[1], points[3 * s + 2] = x[2];
    triangle[s] = (int32_t)t;
}

inline int64_t up8(int64_t n) { return (n + 7) / 8 * 8; }
inline bool msdf_split(int64_t N, int64_t T) {
    return N <= MSDF_SPLIT_POINTS && T > MSDF_CHUNK && (T + MSDF_CHUNK - 1) / MSDF_CHUNK <= MSDF_MAX_GRID_Y;
}
inline bool msdf_sizes_ok(int B, int64_t V, int64_t T, int64_t N) {
    return B >= 0 && B < (1 << 24) && V >= 0 && T >= 0 && N >= 0 && V < ((int64_t)1 << 31) && T < ((int64_t)1 << 31) && N < ((int64_t)1 << 31);
}

}  // namespace

extern "C" int64_t sdfr_mesh_sdf_ws_bytes(int B, int64_t N, int64_t T) {
    if (!msdf_sizes_ok(B, 0, T, N)) return -1;
    int64_t n = 8 * ((int64_t)B + 1);
    if (msdf_split(N, T)) n += up8((T + MSDF_CHUNK - 1) / MSDF_CHUNK * N * 20);
    return n;
}

extern "C" int sdfr_mesh_sdf(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const int64_t* voff, const int64_t* toff,
                             const float* points, int64_t N, const int64_t* qoff, int B, int want_sign, void* ws, int64_t ws_bytes, float* sdf,
                             float* dist, double* d2, int32_t* nearest, double* winding, int32_t* flags, void* stream) {
    SDFR_REQUIRE(msdf_sizes_ok(B, V, T, N), "sdfr_mesh_sdf: B = %d, V = %lld, T = %lld, N = %lld out of range", B, (long long)V, (long long)T,
                 (long long)N);
    SDFR_REQUIRE(want_sign == 0 || want_sign == 1, "sdfr_mesh_sdf: want_sign must be 0 or 1");
    if (B == 0) return SDFR_OK;
    SDFR_REQUIRE(voff && toff && qoff && flags, "sdfr_mesh_sdf: NULL pointer");
    SDFR_REQUIRE((V == 0 || vertices) && (T == 0 || faces) && (N == 0 || (points && sdf)), "sdfr_mesh_sdf: NULL mesh, points or output");
    SDFR_REQUIRE(ws && ws_bytes >= sdfr_mesh_sdf_ws_bytes(B, N, T) && ((uintptr_t)ws & 7) == 0,
                 "sdfr_mesh_sdf: workspace of %lld bytes, sdfr_mesh_sdf_ws_bytes asks for %lld (8-byte aligned)", (long long)ws_bytes,
                 (long long)sdfr_mesh_sdf_ws_bytes(B, N, T));
    const MsdfArgs a = {vertices, faces, voff, toff, points, qoff, V, T, N, B};
    hipStream_t s = (hipStream_t)stream;
    int64_t* boff = (int64_t*)ws;
    const int64_t nblk = (N + MSDF_BLOCK - 1) / MSDF_BLOCK;
    const int64_t n_init = nblk > B ? nblk : B;
    hipLaunchKernelGGL(sdfr_mesh_sdf_init_kernel, dim3((unsigned)n_init), dim3(MSDF_BLOCK), 0, s, a, boff, sdf, dist, d2, nearest, winding, flags);
    SDFR_LAUNCH_CHECK();
    if (N == 0 || T == 0) return SDFR_OK;
    const unsigned gx = (unsigned)(nblk + B);
    if (!msdf_split(N, T)) {
        if (want_sign)
            hipLaunchKernelGGL((sdfr_mesh_sdf_kernel<true, false>), dim3(gx), dim3(MSDF_BLOCK), 0, s, a, boff, sdf, dist, d2, nearest, winding,
                               nullptr, nullptr, nullptr);
        else
            hipLaunchKernelGGL((sdfr_mesh_sdf_kernel<false, false>), dim3(gx), dim3(MSDF_BLOCK), 0, s, a, boff, sdf, dist, d2, nearest, winding,
                               nullptr, nullptr, nullptr);
        SDFR_LAUNCH_CHECK();
        return SDFR_OK;
    }
    const int64_t nch = (T + MSDF_CHUNK - 1) / MSDF_CHUNK;
    double* pd2 = (double*)((char*)ws + 8 * ((int64_t)B + 1));
    double* psum = pd2 + nch * N;
    int32_t* pidx = (int32_t*)(psum + nch * N);
    if (want_sign)
        hipLaunchKernelGGL((sdfr_mesh_sdf_kernel<true, true>), dim3(gx, (unsigned)nch), dim3(MSDF_BLOCK), 0, s, a, boff, sdf, dist, d2, nearest,
                           winding, pd2, psum, pidx);
    else
        hipLaunchKernelGGL((sdfr_mesh_sdf_kernel<false, true>), dim3(gx, (unsigned)nch), dim3(MSDF_BLOCK), 0, s, a, boff, sdf, dist, d2, nearest,
                           winding, pd2, psum, pidx);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_mesh_sdf_fold_kernel, dim3(gx), dim3(MSDF_BLOCK), 0, s, a, boff, want_sign, pd2, psum, pidx, sdf, dist, d2, nearest,
                       winding);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int64_t sdfr_mesh_surface_ws_bytes(int B, int64_t T) {
    if (!msdf_sizes_ok(B, 0, T, 0)) return -1;
    const int64_t nc = (T + MSDF_AREA_CHUNK - 1) / MSDF_AREA_CHUNK + B;
    return 8 * ((int64_t)B + 1) + 8 * T + 8 * nc + 8 * nc + up8(4 * nc);
}

extern "C" int sdfr_mesh_surface_points(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const int64_t* voff, const int64_t* toff,
                                        const float* uniforms, int64_t S, const int64_t* soff, int B, void* ws, int64_t ws_bytes, float* points,
                                        int32_t* triangle, int32_t* flags, void* stream) {
    SDFR_REQUIRE(msdf_sizes_ok(B, V, T, S), "sdfr_mesh_surface_points: B = %d, V = %lld, T = %lld, S = %lld out of range", B, (long long)V,
                 (long long)T, (long long)S);
    SDFR_REQUIRE(B >= 1 || S == 0, "sdfr_mesh_surface_points: %lld samples of no mesh", (long long)S);
    if (B == 0) return SDFR_OK;
    SDFR_REQUIRE(voff && toff && soff && flags, "sdfr_mesh_surface_points: NULL pointer");
    SDFR_REQUIRE((V == 0 || vertices) && (T == 0 || faces) && (S == 0 || (uniforms && points && triangle)),
                 "sdfr_mesh_surface_points: NULL mesh, uniforms or output");
    SDFR_REQUIRE(ws && ws_bytes >= sdfr_mesh_surface_ws_bytes(B, T) && ((uintptr_t)ws & 7) == 0,
                 "sdfr_mesh_surface_points: workspace of %lld bytes, sdfr_mesh_surface_ws_bytes asks for %lld (8-byte aligned)", (long long)ws_bytes,
                 (long long)sdfr_mesh_surface_ws_bytes(B, T));
    const MsdfArgs a = {vertices, faces, voff, toff, uniforms, soff, V, T, S, B};
    hipStream_t s = (hipStream_t)stream;
    const int64_t nc = (T + MSDF_AREA_CHUNK - 1) / MSDF_AREA_CHUNK + B;
    int64_t* coff = (int64_t*)ws;
    double* local = (double*)(coff + B + 1);
    double* tot = local + T;
    double* base = tot + nc;
    int32_t* cflag = (int32_t*)(base + nc);
    hipLaunchKernelGGL(sdfr_mesh_surface_table_kernel, dim3(1), dim3(64), 0, s, a, coff);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_mesh_surface_area_kernel, dim3((unsigned)nc), dim3(MSDF_BLOCK), 0, s, a, coff, local, tot, cflag);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_mesh_surface_base_kernel, dim3((unsigned)sdfr_cdiv(B, MSDF_BLOCK)), dim3(MSDF_BLOCK), 0, s, a, coff, tot, cflag, base,
                       flags);
    SDFR_LAUNCH_CHECK();
    if (S > 0) {
        hipLaunchKernelGGL(sdfr_mesh_surface_sample_kernel, dim3((unsigned)sdfr_cdiv(S, MSDF_BLOCK)), dim3(MSDF_BLOCK), 0, s, a, coff, local, base,
                           points, triangle);
        SDFR_LAUNCH_CHECK();
    }
    return SDFR_OK;
}
