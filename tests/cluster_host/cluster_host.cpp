// Host harness of sdflabel_amd/csrc/cluster_cells.h and, through it, of the cells part of hash_grid.h (the grid of normals.hip too): runs
// what the kernels of cluster.hip run, the threads as loops, and writes what they would write.  tests/test_cluster_cpu.py compares the
// output with the numpy restatement (tests/_cluster_ref.py) bit for bit; tests/test_normals_cpu.py runs the normals' radius through it.
//   cluster_host IN OUT
//   IN : int32 N, f64, has_mask, min_points, max_points, C, K, reverse; float32 eps; points [N][3] float32 or float64; uint8 mask[N] if
//        has_mask; float64 dirs[K][2]
//   OUT: int32 label[N], members[N], off[C + 1], counts[4]; float64 rect[C][8]
// members and rect start as the sentinel -7: what the kernels leave unwritten stays so.  `reverse` walks the scatter and the unions from
// the last point to the first: the bucket order and the order of the unions change, no output may.
// THE CONCURRENT UNION IS A DEVICE MATTER: one thread after the other, clu_union never sees a failed compare-and-swap here.  This program
// pins the per-element rules (participation, cells, neighbours, gates, labels, extents, areas) and the index arithmetic of every pass (the
// hash grid, the 27-cell walk, the scans, the chunk table and the ranks of the stable partition, the staging of the rectangles).
// Every buffer has exactly the size the kernels' caller allocates (sdfr_cluster_ws_bytes' parts), so a sanitizer build checks the indices.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "cluster_cells.h"

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

static void scan(const std::vector<int32_t>& in, size_t n, int32_t* out) {          // out[n + 1]
    int32_t s = 0;
    for (size_t i = 0; i < n; ++i) { out[i] = s; s += in[i]; }
    out[n] = s;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t h[8];
    float eps32;
    if (!f || fread(h, 4, 8, f) != 8 || fread(&eps32, 4, 1, f) != 1) return 3;
    const int N = h[0], f64 = h[1], has_mask = h[2], min_points = h[3], max_points = h[4], C = h[5], K = h[6], reverse = h[7];
    if (N < 0 || N > CLU_MAX_POINTS || C < 1 || C > CLU_MAX_CLUSTERS || K < 1 || K > CLU_MAX_DIRS) return 3;
    std::vector<float> p32;
    std::vector<double> p64, dirs;
    std::vector<uint8_t> mask;
    if (f64 ? !rd(f, p64, 3 * (size_t)N) : !rd(f, p32, 3 * (size_t)N)) return 3;
    if (has_mask && !rd(f, mask, (size_t)N)) return 3;
    if (!rd(f, dirs, 2 * (size_t)K)) return 3;
    fclose(f);
    auto coord = [&](int i, int k) { return f64 ? p64[3 * (size_t)i + k] : (double)p32[3 * (size_t)i + k]; };
    const double eps = (double)eps32, e2 = eps * eps, cell = hg_cell_width(eps);
    const int64_t T = hg_table(N);
    const int shift = 64 - hg_log2(T);
    const int chunks = (N + CLU_CHUNK - 1) / CLU_CHUNK;
    std::vector<double> spts(3 * (size_t)N);
    std::vector<uint64_t> skey((size_t)N), pkey((size_t)N);
    std::vector<int32_t> start((size_t)T + 1), count((size_t)T, 0), sidx((size_t)N), parent((size_t)N), root((size_t)N), csize((size_t)N), isc((size_t)N),
        cid((size_t)N + 1), csz((size_t)C, 0), hist((size_t)chunks * C);
    std::vector<int32_t> label((size_t)N), members((size_t)N, -7), off((size_t)C + 1), counts(4, 0);
    std::vector<double> rect((size_t)C * CLU_RECT, -7.0);
    // key
    for (int i = 0; i < N; ++i) {
        const double X = coord(i, 0), Y = coord(i, 1), Z = coord(i, 2);
        const int part = clu_takes_part(has_mask ? mask[i] != 0 : 1, X, Y, Z);
        parent[i] = i;
        csize[i] = 0;
        if (part == 1) {
            pkey[i] = hg_pack(hg_cell(X, cell), hg_cell(Y, cell), hg_cell(Z, cell));
            count[hg_bucket(pkey[i], shift)] += 1;
        } else {
            pkey[i] = ~0ull;
            if (part == 2) counts[3] |= CLU_FLAG_NONFINITE;
        }
    }
    scan(count, (size_t)T, start.data());
    for (int64_t b = 0; b < T; ++b) count[b] = 0;
    // scatter
    for (int n = 0; n < N; ++n) {
        const int i = reverse ? N - 1 - n : n;
        if (pkey[i] == ~0ull) continue;
        const int b = hg_bucket(pkey[i], shift);
        const int pos = start[b] + count[b]++;
        sidx[pos] = i;
        skey[pos] = pkey[i];
        for (int k = 0; k < 3; ++k) spts[3 * (size_t)pos + k] = coord(i, k);
    }
    // unions: one "wave" per slot, its candidates 64 at a time
    const int slots = start[T];
    for (int n = 0; n < slots; ++n) {
        const int w = reverse ? slots - 1 - n : n;
        const int i = sidx[w];
        const double* q = &spts[3 * (size_t)w];
        uint64_t ck[27];
        int cs[27], cpre[28];
        cpre[0] = 0;
        for (int k = 0; k < 27; ++k) {
            int s = 0, len = 0;
            uint64_t key = 0;
            if (hg_neighbour_cell(skey[w], k, &key)) {
                const int b = hg_bucket(key, shift);
                s = start[b];
                len = start[b + 1] - s;
            }
            cs[k] = s; ck[k] = key; cpre[k + 1] = cpre[k] + len;
        }
        const int M = cpre[27];
        for (int c = 0; c < M; ++c) {
            int s = 0;
            for (int k = 1; k < 27; ++k) s += cpre[k] <= c ? 1 : 0;
            const int pos = cs[s] + (c - cpre[s]);
            if (skey[pos] != ck[s]) continue;
            const int j = sidx[pos];
            if (j >= i) continue;
            if (hg_d2(&spts[3 * (size_t)pos], q) < e2) clu_union(parent.data(), i, j);
        }
    }
    // flatten, mark, number, label
    for (int i = 0; i < N; ++i) {
        int r = -1;
        if (pkey[i] != ~0ull) {
            r = clu_find(parent.data(), i);
            csize[r] += 1;
            counts[0] += 1;
            counts[1] += r == i;
        }
        root[i] = r;
    }
    for (int i = 0; i < N; ++i) isc[i] = root[i] == i && clu_is_cluster(csize[i], min_points, max_points) ? 1 : 0;
    scan(isc, (size_t)N, cid.data());
    for (int i = 0; i < N; ++i) {
        const int32_t l = clu_label(root[i], isc.data(), cid.data(), C);
        label[i] = l;
        if (root[i] == i && l >= 0) csz[l] = csize[i];
    }
    if (N > 0) {
        counts[2] = cid[N];
        if (cid[N] > C) counts[3] |= CLU_FLAG_CAPPED;
    }
    scan(csz, (size_t)C, off.data());
    // the stable partition: chunk counts, first slots, ranks wave by wave
    for (int ch = 0; ch < chunks; ++ch) {
        for (int c = 0; c < C; ++c) hist[(size_t)ch * C + c] = 0;
        for (int t = 0; t < CLU_CHUNK; ++t) {
            const int i = ch * CLU_CHUNK + t;
            const int l = i < N ? label[i] : -1;
            if (l >= 0 && l < C) hist[(size_t)ch * C + l] += 1;
        }
    }
    for (int c = 0; c < C; ++c) {
        int base = off[c];
        for (int ch = 0; ch < chunks; ++ch) {
            const size_t at = (size_t)ch * C + c;
            const int n = hist[at];
            hist[at] = base;
            base += n;
        }
    }
    std::vector<int32_t> run((size_t)C);
    for (int ch = 0; ch < chunks; ++ch) {
        for (int c = 0; c < C; ++c) run[c] = 0;
        for (int w = 0; w < CLU_CHUNK / 64; ++w) {
            int lab[64];
            for (int lane = 0; lane < 64; ++lane) {
                const int i = ch * CLU_CHUNK + w * 64 + lane;
                lab[lane] = i < N ? label[i] : -1;
            }
            for (int lane = 0; lane < 64; ++lane) {
                if (lab[lane] < 0) continue;
                int rank = 0;
                for (int k = 0; k < lane; ++k) rank += lab[k] == lab[lane];
                members[hist[(size_t)ch * C + lab[lane]] + run[lab[lane]] + rank] = ch * CLU_CHUNK + w * 64 + lane;
            }
            for (int lane = 0; lane < 64; ++lane)
                if (lab[lane] >= 0) run[lab[lane]] += 1;
        }
    }
    // rectangles: one "workgroup" per kept cluster, the members 256 at a time
    const int kept = counts[2] < C ? counts[2] : C;
    std::vector<CluExt> eu((size_t)K), ev((size_t)K);
    std::vector<double> area((size_t)K);
    for (int c = 0; c < kept; ++c) {
        CluExt ey;
        clu_ext_start(&ey);
        for (int k = 0; k < K; ++k) { clu_ext_start(&eu[k]); clu_ext_start(&ev[k]); }
        for (int base = off[c]; base < off[c + 1]; base += CLU_BOX_TPB) {
            const int n = off[c + 1] - base < CLU_BOX_TPB ? off[c + 1] - base : CLU_BOX_TPB;
            double sx[CLU_BOX_TPB], sy[CLU_BOX_TPB], sz[CLU_BOX_TPB];
            for (int t = 0; t < n; ++t) {
                const int j = members[base + t];
                sx[t] = coord(j, 0); sy[t] = coord(j, 1); sz[t] = coord(j, 2);
            }
            for (int p = 0; p < n; ++p) {
                clu_ext_add(&ey, sy[p]);
                for (int k = 0; k < K; ++k) {
                    double u, v;
                    clu_uv(sx[p], sz[p], dirs[2 * (size_t)k], dirs[2 * (size_t)k + 1], &u, &v);
                    clu_ext_add(&eu[k], u);
                    clu_ext_add(&ev[k], v);
                }
            }
        }
        clu_ext_end(&ey);
        for (int k = 0; k < K; ++k) {
            clu_ext_end(&eu[k]);
            clu_ext_end(&ev[k]);
            area[k] = clu_area(&eu[k], &ev[k]);
        }
        int win = 0;
        double best = area[0];
        for (int k = 1; k < K; ++k)
            if (area[k] < best) { best = area[k]; win = k; }
        double* o = &rect[(size_t)c * CLU_RECT];
        o[0] = (double)win; o[1] = eu[win].lo; o[2] = eu[win].hi; o[3] = ev[win].lo; o[4] = ev[win].hi; o[5] = ey.lo; o[6] = ey.hi; o[7] = area[win];
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 4;
    wr(o, label), wr(o, members), wr(o, off), wr(o, counts), wr(o, rect);
    fclose(o);
    return 0;
}
