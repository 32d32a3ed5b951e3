// Triangle meshes of SDF samples on a regular lattice: marching tetrahedra on the Kuhn subdivision, shared vertices welded (DESIGN.md,
// "Meshes").  The per-point code is mesh_cells.h; this file holds the launches.
//
//   sdfr_mesh_lattice_inputs   latent || xyz rows of a chunk of lattice rows of B shapes, for the decoder
//   sdfr_mesh_count            per point: crossing mask of the owned edges and triangle count of its cell; in-block prefixes; the exclusive
//                              scan of the block sums (any number of blocks); per-shape totals
//   sdfr_mesh_emit             vertices and shape-local triangle indices at the offsets the caller derived from the totals
//
// No atomics anywhere: vertex and triangle order are (owner row, class) and (cell row, tetrahedron, triangle), the same bits on every run,
// and a shape's output does not depend on what else is in the batch.  Compiled with -ffp-contract=off (build.sh).
#include "sdfr_common.h"
#include "mesh_cells.h"

namespace {

struct MeshWs {
    uint8_t* mask;        // [B][N] crossing mask of the point's owned edges
    uint16_t* pre_v;      // [B][N] vertices of the points before it in its block
    uint16_t* pre_t;      // [B][N] triangles likewise
    int32_t* block_v;     // [B][NB] vertices of the shape's blocks before this one (block sums until the scan ran)
    int32_t* block_t;     // [B][NB]
    int64_t* voff;        // [B + 1] the caller's offsets, copied by sdfr_mesh_emit
    int64_t* toff;        // [B + 1]
};

int64_t mesh_carve(void* base, int R, int B, MeshWs* ws) {
    const int64_t N = (int64_t)R * R * R, NB = (N + MESH_BLOCK - 1) / MESH_BLOCK;
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = off;
        off += (bytes + 255) / 256 * 256;
        return base ? (char*)base + at : (char*)nullptr;
    };
    char* p0 = take(B * N);
    char* p1 = take(B * N * 2);
    char* p2 = take(B * N * 2);
    char* p3 = take(B * NB * 4);
    char* p4 = take(B * NB * 4);
    char* p5 = take(((int64_t)B + 1) * 8);
    char* p6 = take(((int64_t)B + 1) * 8);
    if (ws) *ws = MeshWs{(uint8_t*)p0, (uint16_t*)p1, (uint16_t*)p2, (int32_t*)p3, (int32_t*)p4, (int64_t*)p5, (int64_t*)p6};
    return off;
}

bool mesh_shape_ok(int R, int B) {
    return R >= MESH_R_MIN && R <= MESH_R_MAX && B >= 1 && (int64_t)B * R * R * R < ((int64_t)1 << 31);
}

__global__ __launch_bounds__(256) void sdfr_mesh_inputs_kernel(const float* __restrict__ latents, int L, int R, int64_t row0, int64_t nrows,
                                                               int64_t total, float* __restrict__ inputs) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int NI = L + 3;
    const int64_t r = e / NI;
    const int c = (int)(e - r * NI);
    const int64_t b = r / nrows, row = row0 + (r - b * nrows);
    float v;
    if (c < L) {
        v = latents[b * L + c];
    } else {
        const int k = c - L;
        const int i = k == 0 ? (int)(row / ((int64_t)R * R)) : k == 1 ? (int)(row / R % R) : (int)(row % R);
        v = mesh_coord(i, R);
    }
    inputs[e] = v;
}

// inclusive scan of one packed word per thread over the workgroup (vertices in the low half, triangles in the high half: at most 7 and 12
// per point, 1792 and 3072 per block, so the halves never carry into each other)
__device__ __forceinline__ uint32_t mesh_block_scan(uint32_t v, uint32_t* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < MESH_BLOCK; o <<= 1) {
        const uint32_t x = t >= o ? sh[t - o] : 0u;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    return sh[t];
}

__global__ __launch_bounds__(MESH_BLOCK) void sdfr_mesh_count_kernel(const float* __restrict__ sdf, int R, int N, int NB, MeshWs ws) {
    __shared__ uint32_t sh[MESH_BLOCK];
    const int b = blockIdx.x / NB, blk = blockIdx.x - b * NB;
    const int row = blk * MESH_BLOCK + threadIdx.x;
    const int64_t at = (int64_t)b * N + row;
    unsigned m = 0;
    int nt = 0;
    if (row < N) m = mesh_point_record(sdf + (int64_t)b * N, R, row, &nt);
    const uint32_t v = (uint32_t)mesh_popc(m) | (uint32_t)nt << 16;
    const uint32_t incl = mesh_block_scan(v, sh);
    if (row < N) {
        ws.mask[at] = (uint8_t)m;
        ws.pre_v[at] = (uint16_t)((incl - v) & 0xffffu);
        ws.pre_t[at] = (uint16_t)((incl - v) >> 16);
    }
    if (threadIdx.x == MESH_BLOCK - 1) {
        ws.block_v[(int64_t)b * NB + blk] = (int32_t)(incl & 0xffffu);
        ws.block_t[(int64_t)b * NB + blk] = (int32_t)(incl >> 16);
    }
}

// second level: one workgroup per shape walks its block sums 256 at a time with a running carry, turning them into exclusive offsets
__global__ __launch_bounds__(MESH_BLOCK) void sdfr_mesh_scan_kernel(int NB, MeshWs ws, int32_t* __restrict__ nv, int32_t* __restrict__ nt) {
    __shared__ int32_t sv[MESH_BLOCK], st[MESH_BLOCK];
    const int b = blockIdx.x, t = threadIdx.x;
    int32_t* bv = ws.block_v + (int64_t)b * NB;
    int32_t* bt = ws.block_t + (int64_t)b * NB;
    int32_t carry_v = 0, carry_t = 0;
    for (int base = 0; base < NB; base += MESH_BLOCK) {
        const int i = base + t;
        const int32_t xv = i < NB ? bv[i] : 0, xt = i < NB ? bt[i] : 0;
        sv[t] = xv;
        st[t] = xt;
        __syncthreads();
        for (int o = 1; o < MESH_BLOCK; o <<= 1) {
            const int32_t av = t >= o ? sv[t - o] : 0, at = t >= o ? st[t - o] : 0;
            __syncthreads();
            sv[t] += av;
            st[t] += at;
            __syncthreads();
        }
        if (i < NB) {
            bv[i] = carry_v + sv[t] - xv;
            bt[i] = carry_t + st[t] - xt;
        }
        carry_v += sv[MESH_BLOCK - 1];
        carry_t += st[MESH_BLOCK - 1];
        __syncthreads();
    }
    if (t == 0) {
        nv[b] = carry_v;
        nt[b] = carry_t;
    }
}

__global__ __launch_bounds__(MESH_BLOCK) void sdfr_mesh_emit_kernel(const float* __restrict__ sdf, int R, int N, int NB, MeshWs ws,
                                                                    float* __restrict__ vertices, int32_t* __restrict__ faces) {
    const int b = blockIdx.x / NB, blk = blockIdx.x - b * NB;
    const int row = blk * MESH_BLOCK + threadIdx.x;
    if (row >= N) return;
    const int64_t at = (int64_t)b * N + row;
    const float* s = sdf + (int64_t)b * N;
    const int32_t* block_v = ws.block_v + (int64_t)b * NB;
    const int64_t v0 = ws.voff[b], t0 = ws.toff[b];
    const int64_t vid = (int64_t)block_v[blk] + ws.pre_v[at], tid = (int64_t)ws.block_t[(int64_t)b * NB + blk] + ws.pre_t[at];
    // never past the shape's own range, whatever offsets the caller passed (the host checked their end against the capacities)
    const int64_t room_v = ws.voff[b + 1] - v0 - vid, room_t = ws.toff[b + 1] - t0 - tid;
    const unsigned m = ws.mask[at];
    if (m != 0 && room_v > 0) mesh_point_vertices(s, R, row, m, vertices + 3 * (v0 + vid), (int)(room_v < 7 ? room_v : 7));
    if (room_t > 0)
        mesh_point_triangles(s, R, row, ws.mask + (int64_t)b * N, ws.pre_v + (int64_t)b * N, block_v, faces + 3 * (t0 + tid),
                             (int)(room_t < 12 ? room_t : 12));
}

}  // namespace

extern "C" int64_t sdfr_mesh_ws_bytes(int R, int B) {
    if (!mesh_shape_ok(R, B)) return -1;
    return mesh_carve(nullptr, R, B, nullptr);
}

extern "C" int sdfr_mesh_lattice_inputs(const float* latents, int L, int R, int B, int64_t row0, int64_t nrows, float* inputs, void* stream) {
    SDFR_REQUIRE(R >= MESH_R_MIN && R <= MESH_R_MAX, "sdfr_mesh_lattice_inputs: R = %d outside %d .. %d", R, MESH_R_MIN, MESH_R_MAX);
    SDFR_REQUIRE(B >= 1 && (int64_t)B * R * R * R < ((int64_t)1 << 31), "sdfr_mesh_lattice_inputs: B * R^3 must be below 2^31 (B = %d, R = %d)", B, R);
    SDFR_REQUIRE(L >= 0 && L <= 4096, "sdfr_mesh_lattice_inputs: latent size %d", L);
    SDFR_REQUIRE(row0 >= 0 && nrows >= 1 && row0 + nrows <= (int64_t)R * R * R, "sdfr_mesh_lattice_inputs: rows %lld + %lld outside the lattice",
                 (long long)row0, (long long)nrows);
    SDFR_REQUIRE((L == 0 || latents) && inputs, "sdfr_mesh_lattice_inputs: NULL pointer");
    const int64_t total = (int64_t)B * nrows * (L + 3);
    SDFR_REQUIRE((total + 255) / 256 < ((int64_t)1 << 31), "sdfr_mesh_lattice_inputs: chunk too large");
    hipLaunchKernelGGL(sdfr_mesh_inputs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, latents, L, R, row0, nrows,
                       total, inputs);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_mesh_count(const float* sdf, int R, int B, int32_t* nv, int32_t* nt, void* ws, int64_t ws_bytes, void* stream) {
    SDFR_REQUIRE(R >= MESH_R_MIN && R <= MESH_R_MAX, "sdfr_mesh_count: R = %d outside %d .. %d", R, MESH_R_MIN, MESH_R_MAX);
    SDFR_REQUIRE(B >= 1 && (int64_t)B * R * R * R < ((int64_t)1 << 31), "sdfr_mesh_count: B * R^3 must be below 2^31 (B = %d, R = %d)", B, R);
    SDFR_REQUIRE(sdf && nv && nt && ws, "sdfr_mesh_count: NULL pointer");
    MeshWs w;
    SDFR_REQUIRE(ws_bytes >= mesh_carve(ws, R, B, &w), "sdfr_mesh_count: workspace of %lld bytes, sdfr_mesh_ws_bytes asks for %lld",
                 (long long)ws_bytes, (long long)mesh_carve(nullptr, R, B, nullptr));
    const int N = R * R * R, NB = (N + MESH_BLOCK - 1) / MESH_BLOCK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sdfr_mesh_count_kernel, dim3((unsigned)((int64_t)B * NB)), dim3(MESH_BLOCK), 0, s, sdf, R, N, NB, w);
    SDFR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdfr_mesh_scan_kernel, dim3((unsigned)B), dim3(MESH_BLOCK), 0, s, NB, w, nv, nt);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}

extern "C" int sdfr_mesh_emit(const float* sdf, int R, int B, const int64_t* voff, const int64_t* toff, void* ws, int64_t ws_bytes,
                              float* vertices, int64_t cap_v, int32_t* faces, int64_t cap_t, void* stream) {
    SDFR_REQUIRE(R >= MESH_R_MIN && R <= MESH_R_MAX, "sdfr_mesh_emit: R = %d outside %d .. %d", R, MESH_R_MIN, MESH_R_MAX);
    SDFR_REQUIRE(B >= 1 && (int64_t)B * R * R * R < ((int64_t)1 << 31), "sdfr_mesh_emit: B * R^3 must be below 2^31 (B = %d, R = %d)", B, R);
    SDFR_REQUIRE(sdf && voff && toff && ws, "sdfr_mesh_emit: NULL pointer");
    SDFR_REQUIRE(cap_v >= 0 && cap_t >= 0 && voff[0] == 0 && toff[0] == 0, "sdfr_mesh_emit: offsets start at 0, capacities are not negative");
    for (int b = 0; b < B; ++b)
        SDFR_REQUIRE(voff[b + 1] >= voff[b] && toff[b + 1] >= toff[b], "sdfr_mesh_emit: offsets of shape %d decrease", b);
    SDFR_REQUIRE(voff[B] <= cap_v, "sdfr_mesh_emit: %lld vertices, room for %lld", (long long)voff[B], (long long)cap_v);
    SDFR_REQUIRE(toff[B] <= cap_t, "sdfr_mesh_emit: %lld triangles, room for %lld", (long long)toff[B], (long long)cap_t);
    SDFR_REQUIRE((voff[B] == 0 || vertices) && (toff[B] == 0 || faces), "sdfr_mesh_emit: NULL output");
    MeshWs w;
    SDFR_REQUIRE(ws_bytes >= mesh_carve(ws, R, B, &w), "sdfr_mesh_emit: workspace of %lld bytes, sdfr_mesh_ws_bytes asks for %lld",
                 (long long)ws_bytes, (long long)mesh_carve(nullptr, R, B, nullptr));
    if (voff[B] == 0 && toff[B] == 0) return SDFR_OK;
    const int N = R * R * R, NB = (N + MESH_BLOCK - 1) / MESH_BLOCK;
    hipStream_t s = (hipStream_t)stream;
    // the offsets are host values (the caller read the totals to allocate); the copies are ordered on the stream before the kernel
    SDFR_HIP_CHECK(hipMemcpyAsync(w.voff, voff, ((size_t)B + 1) * 8, hipMemcpyHostToDevice, s));
    SDFR_HIP_CHECK(hipMemcpyAsync(w.toff, toff, ((size_t)B + 1) * 8, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(sdfr_mesh_emit_kernel, dim3((unsigned)((int64_t)B * NB)), dim3(MESH_BLOCK), 0, s, sdf, R, N, NB, w, vertices, faces);
    SDFR_LAUNCH_CHECK();
    return SDFR_OK;
}
