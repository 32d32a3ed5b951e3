// Host harness of sdflabel_amd/csrc/mesh_cells.h: runs the per-point code for every thread index of the count and emit launches, with the
// scans done sequentially, and writes what the kernels would write.  tests/test_mesh_cpu.py compares the output with the numpy restatement.
//   mesh_host IN OUT      IN: int32 R, float32 sdf[R^3]     OUT: int32 nv, nt, float32 v[nv][3], int32 f[nt][3], uint8 mask[R^3], uint8 tcount[R^3]
// Every buffer has exactly the size the kernels' caller would allocate, so a sanitizer build of this program checks the index arithmetic.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mesh_cells.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t R = 0;
    if (!f || fread(&R, 4, 1, f) != 1 || R < MESH_R_MIN || R > MESH_R_MAX) return 3;
    const int N = R * R * R, NB = (N + MESH_BLOCK - 1) / MESH_BLOCK;
    std::vector<float> sdf(N);
    if (fread(sdf.data(), 4, N, f) != (size_t)N) return 3;
    fclose(f);
    // count: one "thread" per slot of every block, the block's prefix taken in thread order
    std::vector<uint8_t> mask(N), tcount(N);
    std::vector<uint16_t> pre_v(N), pre_t(N);
    std::vector<int32_t> block_v(NB), block_t(NB);
    int32_t nv = 0, nt = 0;
    for (int blk = 0; blk < NB; ++blk) {
        int sv = 0, st = 0;
        for (int t = 0; t < MESH_BLOCK; ++t) {
            const int row = blk * MESH_BLOCK + t;
            if (row >= N) continue;
            int n = 0;
            const unsigned m = mesh_point_record(sdf.data(), R, row, &n);
            mask[row] = (uint8_t)m;
            tcount[row] = (uint8_t)n;
            pre_v[row] = (uint16_t)sv;
            pre_t[row] = (uint16_t)st;
            sv += mesh_popc(m);
            st += n;
        }
        block_v[blk] = nv;
        block_t[blk] = nt;
        nv += sv;
        nt += st;
    }
    // emit into exact-size buffers
    std::vector<float> verts((size_t)nv * 3);
    std::vector<int32_t> faces((size_t)nt * 3);
    for (int row = 0; row < N; ++row) {
        const int blk = row / MESH_BLOCK;
        const int64_t vid = (int64_t)block_v[blk] + pre_v[row], tid = (int64_t)block_t[blk] + pre_t[row];
        const int64_t room_v = nv - vid, room_t = nt - tid;
        if (mask[row] != 0 && room_v > 0)
            mesh_point_vertices(sdf.data(), R, row, mask[row], verts.data() + 3 * vid, (int)(room_v < 7 ? room_v : 7));
        if (room_t > 0)
            mesh_point_triangles(sdf.data(), R, row, mask.data(), pre_v.data(), block_v.data(), faces.data() + 3 * tid,
                                 (int)(room_t < 12 ? room_t : 12));
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 4;
    fwrite(&nv, 4, 1, o);
    fwrite(&nt, 4, 1, o);
    if (!verts.empty()) fwrite(verts.data(), 4, verts.size(), o);
    if (!faces.empty()) fwrite(faces.data(), 4, faces.size(), o);
    fwrite(mask.data(), 1, N, o);
    fwrite(tcount.data(), 1, N, o);
    fclose(o);
    return 0;
}
