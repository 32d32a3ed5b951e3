// Per-point code of the mesh extraction (mesh.hip): marching tetrahedra on the Kuhn subdivision of a regular lattice, welded.  DESIGN.md
// ("Meshes") has the rules.  Everything here is a plain function of one lattice point, compiled for the device by mesh.hip and for the host
// by tests/test_mesh_cpu.py, which loops over every thread index and compares with the numpy restatement bit for bit.
//
// Lattice: R points per axis, x_i = float32(-1 + 2 i / (R - 1)) evaluated in float64, row = (ix R + iy) R + iz.
// Codes: a cell corner and an edge class are 3-bit numbers with x the high bit; edge class d in 1..7 runs from p to p + d and belongs to p.
// A point's record: the 7-bit crossing mask of its owned edges (bit d - 1) and the triangle count of the cell whose low corner it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MESH_HD __host__ __device__ inline
#else
#define MESH_HD static inline
#endif

#define MESH_R_MIN 2
#define MESH_R_MAX 256
#define MESH_BLOCK 256          // lattice points per workgroup, the unit of the two-level scan

// corner codes of the six tetrahedra, 3 bits per corner, in the order of itertools.permutations((0, 1, 2)): 000 -> 111 one axis at a time
MESH_HD uint32_t mesh_tet_corners(int tet) {
    const uint32_t T[6] = {4000u, 3936u, 3984u, 3792u, 3912u, 3784u};
    return T[tet];
}
// triangles of a tetrahedron by inside mask (bit i: corner i inside).  Bits 0-1: the count; then per triangle vertex 4 bits, the edge's
// lower | higher << 2 corner position.  1 or 3 inside: one triangle; 2 inside: the quad [I0O0, I0O1, I1O1, I1O0] split (0,1,2), (0,2,3).
MESH_HD uint32_t mesh_tet_case(unsigned mask) {
    const uint32_t C[16] = {0x0u, 0x3211u, 0x3651u, 0x2763722u, 0x3a61u, 0x2793b12u, 0x2393b52u, 0x3b71u,
                            0x3b71u, 0x3793a12u, 0x3393a52u, 0x3a61u, 0x3363662u, 0x3651u, 0x3211u, 0x0u};
    return C[mask];
}
// winding: bit `mask` set = swap the last two vertices of the case's triangles so that the normal points from inside to outside.  Decided
// with every crossing at its edge's midpoint in integer arithmetic (never zero, whatever the sdf values); depends on the tetrahedron's
// parity only.
MESH_HD uint32_t mesh_tet_flip(int tet) {
    const uint32_t F[6] = {0x4d24u, 0x32dau, 0x32dau, 0x4d24u, 0x4d24u, 0x32dau};
    return F[tet];
}

MESH_HD float mesh_coord(int i, int R) { return (float)(-1.0 + 2.0 * (double)i / (double)(R - 1)); }
MESH_HD bool mesh_inside(float s) { return s < 0.0f; }                    // an exact 0 and a NaN are outside
MESH_HD int mesh_code_row(unsigned c, int R) { return ((int)(c >> 2 & 1u) * R + (int)(c >> 1 & 1u)) * R + (int)(c & 1u); }
MESH_HD int mesh_popc(unsigned v) {
    v = v - (v >> 1 & 0x55u);
    v = (v & 0x33u) + (v >> 2 & 0x33u);
    return (int)((v + (v >> 4)) & 0xfu);
}

// inside flags of the 8 corners of the cell at (ix, iy, iz), bit = corner code; corners outside the lattice read as outside (their bits are
// used by the owned-edge test only after a bounds check of their own)
MESH_HD unsigned mesh_corner_flags(const float* sdf, int R, int ix, int iy, int iz, int row) {
    unsigned fl = 0;
    for (unsigned c = 0; c < 8; ++c) {
        const bool in_lattice = ix + (int)(c >> 2 & 1u) < R && iy + (int)(c >> 1 & 1u) < R && iz + (int)(c & 1u) < R;
        if (in_lattice && mesh_inside(sdf[row + mesh_code_row(c, R)])) fl |= 1u << c;
    }
    return fl;
}

// the point's record: returns the crossing mask of the owned edges, *ntri = triangles of its cell (0 .. 12)
MESH_HD unsigned mesh_point_record(const float* sdf, int R, int row, int* ntri) {
    const int iz = row % R, iy = row / R % R, ix = row / (R * R);
    const unsigned fl = mesh_corner_flags(sdf, R, ix, iy, iz, row);
    unsigned mask = 0;
    for (unsigned d = 1; d < 8; ++d) {
        const bool in_lattice = ix + (int)(d >> 2 & 1u) < R && iy + (int)(d >> 1 & 1u) < R && iz + (int)(d & 1u) < R;
        if (in_lattice && ((fl ^ (fl >> d)) & 1u)) mask |= 1u << (d - 1);
    }
    int nt = 0;
    if (ix < R - 1 && iy < R - 1 && iz < R - 1) {
        for (int tet = 0; tet < 6; ++tet) {
            const uint32_t cc = mesh_tet_corners(tet);
            unsigned m = 0;
            for (int i = 0; i < 4; ++i) m |= (fl >> (cc >> (3 * i) & 7u) & 1u) << i;
            nt += (int)(mesh_tet_case(m) & 3u);
        }
    }
    *ntri = nt;
    return mask;
}

// the vertices of the point's crossing owned edges, in class order: t = sa / (sa - sb), p = pa + t (pb - pa) in float32 with separate
// multiply and add (the translation unit is compiled with -ffp-contract=off).  A t that is NaN (a NaN or infinite neighbour) becomes 1/2.
// Writes at most `room` vertices to out[][3]; returns the number written.
MESH_HD int mesh_point_vertices(const float* sdf, int R, int row, unsigned mask, float* out, int room) {
    const int iz = row % R, iy = row / R % R, ix = row / (R * R);
    const int ip[3] = {ix, iy, iz};
    const float sa = sdf[row];
    int n = 0;
    for (unsigned d = 1; d < 8 && n < room; ++d) {
        if (!(mask >> (d - 1) & 1u)) continue;
        const float sb = sdf[row + mesh_code_row(d, R)];
        float t = sa / (sa - sb);
        if (!(t == t)) t = 0.5f;
        for (int k = 0; k < 3; ++k) {
            const float pa = mesh_coord(ip[k], R), pb = mesh_coord(ip[k] + (int)(d >> (2 - k) & 1u), R);
            const float prod = t * (pb - pa);
            out[3 * n + k] = pa + prod;
        }
        ++n;
    }
    return n;
}

// shape-local id of the vertex on edge class d of owner point q: the owner's base plus the crossing lower classes in its mask
MESH_HD int32_t mesh_vertex_id(const uint8_t* mask, const uint16_t* pre_v, const int32_t* block_v, int q, unsigned d) {
    return block_v[q / MESH_BLOCK] + (int32_t)pre_v[q] + mesh_popc(mask[q] & ((1u << (d - 1)) - 1u));
}

// the triangles of the cell whose low corner is the point, in (tetrahedron, triangle) order, as shape-local vertex ids.  mask / pre_v /
// block_v: the shape's point records, in-block vertex prefixes and per-block vertex bases.  Writes at most `room` triangles to out[][3];
// returns the number written.
MESH_HD int mesh_point_triangles(const float* sdf, int R, int row, const uint8_t* mask, const uint16_t* pre_v, const int32_t* block_v,
                                 int32_t* out, int room) {
    const int iz = row % R, iy = row / R % R, ix = row / (R * R);
    if (!(ix < R - 1 && iy < R - 1 && iz < R - 1)) return 0;
    const unsigned fl = mesh_corner_flags(sdf, R, ix, iy, iz, row);
    int n = 0;
    for (int tet = 0; tet < 6; ++tet) {
        const uint32_t cc = mesh_tet_corners(tet);
        unsigned m = 0;
        for (int i = 0; i < 4; ++i) m |= (fl >> (cc >> (3 * i) & 7u) & 1u) << i;
        const uint32_t cs = mesh_tet_case(m);
        const int nt = (int)(cs & 3u);
        const bool flip = mesh_tet_flip(tet) >> m & 1u;
        for (int k = 0; k < nt && n < room; ++k, ++n) {
            int32_t v[3];
            for (int j = 0; j < 3; ++j) {
                const unsigned e = cs >> (2 + 4 * (3 * k + j)) & 15u;
                const unsigned lo = cc >> (3 * (e & 3u)) & 7u, hi = cc >> (3 * (e >> 2)) & 7u;
                v[j] = mesh_vertex_id(mask, pre_v, block_v, row + mesh_code_row(lo, R), hi ^ lo);
            }
            out[3 * n + 0] = v[0];
            out[3 * n + 1] = flip ? v[2] : v[1];
            out[3 * n + 2] = flip ? v[1] : v[2];
        }
    }
    return n;
}
