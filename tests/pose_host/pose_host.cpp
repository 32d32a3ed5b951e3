// Host harness of sdflabel_amd/csrc/pose_cells.h (and, through it, of jacobi3.h): runs what the kernels of pose.hip run, the threads as
// loops, and writes what they would write, stage by stage.  tests/test_pose_refs_cpu.py compares the output with the numpy restatement
// (tests/_pose_ref.py) bit for bit.
//   pose_host IN OUT
//   IN : int32 B, ncap, mcap, T, type, f16, has_idx, reserved; int64 seed; float64 metric_thr, nocs_thr; float32 scale_model, reserved;
//        int32 mcnt[B], ncnt[B]; int64 keys[B]; float32 model[B][mcap][3], mcls[B][mcap][3], scene[B][ncap][3], scls[B][ncap][3];
//        int32 idx[B][T][4] if has_idx
//   OUT: int32 idx[B][T][4], cnn_idx[B][ncap]; float64 cnn_d[B][ncap]; int32 gate[B][T], counts[B][T]; float32 hyp[B][T][12];
//        int32 plist[B][T], pcount[B], best[B], n_inliers[B], mask[B][ncap], found[B]; float32 scale[B], rot[B][9], tra[B][3]
//   pose_host jacobi IN OUT: float64 S[n][9] -> float64 lam[n][3], V[n][9] (sdfr_jacobi3 alone; n from the file's size)
// cnn_idx, cnn_d, hyp, plist and mask start as the sentinel -7: what the kernels leave unwritten stays so.  Every buffer has exactly the size
// the kernels' caller allocates, so a sanitizer build checks the indices.
// The MUT_* switches are the mutants of the tests' mutation check: each changes ONE call site below, none touches pose_cells.h.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pose_cells.h"

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T>
static void wr(FILE* f, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
}

static bool sample_fit(const float fp[4][3], const float tp[4][3], bool f16, int type, float h[RS_TRANS], int* bits) {
#if defined(MUT_DROP_SV)
    double mf[3], mt[3], H[3][3], sig, R[3][3], c, tr[3], ratio, U[3][3], V[3][3], s1, s2, detV;
    bool pass = false;
    *bits = 0;
    rs_sample_moments(fp, tp, f16, mf, mt, H, &sig);
    rs_fit_basis(H, U, V, &s1, &s2, &detV);
    if (rs_fit_pose(H, U, V, s1, s2, 1.0, mf, mt, sig, type, R, &c, tr, &ratio) && !((float)c > 3.0f)) {
        *bits |= 2;
        pass = true;
        rs_hyp_row(R, c, tr, h);
    }
    if (ratio < 1e-3) *bits |= 4;
    return pass;
#else
    return pose_sample_fit(fp, tp, f16, type, h, bits);
#endif
}

static bool inlier(PoseV3 tp, int nn, const float* mp, const float* mc, float sx, float sy, float sz, double metric_thr, float nocs_thr32) {
#if defined(MUT_METRIC_LE)
    const double dx = (double)tp.x - (double)mp[(size_t)nn * 3], dy = (double)tp.y - (double)mp[(size_t)nn * 3 + 1],
                 dz = (double)tp.z - (double)mp[(size_t)nn * 3 + 2];
    const double d = sqrt(dx * dx + dy * dy + dz * dz);
    const float cx = sx - mc[(size_t)nn * 3], cy = sy - mc[(size_t)nn * 3 + 1], cz = sz - mc[(size_t)nn * 3 + 2];
    const float dc = sqrtf(cx * cx + cy * cy + cz * cz);
    return d <= metric_thr && dc < nocs_thr32;
#else
    return rs_inlier(tp, nn, mp, mc, sx, sy, sz, metric_thr, nocs_thr32);
#endif
}

// rs_nn_search for one transformed point: tiles of RS_TPB candidates in index order
static int nn_search(PoseV3 tp, const float* mp, int M) {
    float bd = INFINITY;
    int bi = 0;
    for (int base = 0; base < M; base += RS_TPB) {
        const int n = M - base < RS_TPB ? M - base : RS_TPB;
        for (int k = 0; k < n; ++k) rs_nn_step(tp, mp[(size_t)(base + k) * 3], mp[(size_t)(base + k) * 3 + 1], mp[(size_t)(base + k) * 3 + 2], base + k, &bd, &bi);
    }
    return bi;
}

// rs_block_sum: the 256 lanes' partials folded by the tree
static void block_sum(std::vector<double>& red, int K, double* out) {
    for (int o = RS_TPB / 2; o > 0; o >>= 1)
        for (int tid = 0; tid < o; ++tid)
            for (int k = 0; k < K; ++k) red[(size_t)k * RS_TPB + tid] += red[(size_t)k * RS_TPB + tid + o];
    for (int k = 0; k < K; ++k) out[k] = red[(size_t)k * RS_TPB];
}

static int jacobi_main(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    const size_t n = (size_t)bytes / 72;
    std::vector<double> S, lam(3 * n), V(9 * n);
    if (!rd(f, S, 9 * n)) return 3;
    fclose(f);
    for (size_t i = 0; i < n; ++i) {
        double s[3][3], l[3], v[3][3];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) s[a][b] = S[9 * i + 3 * a + b];
        sdfr_jacobi3(s, l, v);
        for (int a = 0; a < 3; ++a) {
            lam[3 * i + a] = l[a];
            for (int b = 0; b < 3; ++b) V[9 * i + 3 * a + b] = v[a][b];
        }
    }
    FILE* o = fopen(out, "wb");
    if (!o) return 4;
    wr(o, lam), wr(o, V);
    fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && argv[1][0] == 'j') return jacobi_main(argv[2], argv[3]);
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int32_t h[8];
    int64_t seed;
    double thr[2];
    float sm[2];
    if (!f || fread(h, 4, 8, f) != 8 || fread(&seed, 8, 1, f) != 1 || fread(thr, 8, 2, f) != 2 || fread(sm, 4, 2, f) != 2) return 3;
    const int B = h[0], ncap = h[1], mcap = h[2], T = h[3], type = h[4], has_idx = h[6];
    const bool f16 = h[5] != 0;
    if (B < 1 || ncap < 1 || mcap < 1 || T < 1 || (type != 0 && type != 1)) return 3;
    std::vector<int32_t> mcnt, ncnt, idx;
    std::vector<int64_t> keys;
    std::vector<float> model, mcls, scene, scls;
    if (!rd(f, mcnt, (size_t)B) || !rd(f, ncnt, (size_t)B) || !rd(f, keys, (size_t)B) || !rd(f, model, (size_t)B * mcap * 3) ||
        !rd(f, mcls, (size_t)B * mcap * 3) || !rd(f, scene, (size_t)B * ncap * 3) || !rd(f, scls, (size_t)B * ncap * 3))
        return 3;
    if (has_idx ? !rd(f, idx, (size_t)B * T * 4) : false) return 3;
    fclose(f);
    for (int b = 0; b < B; ++b)
        if (mcnt[b] < 0 || mcnt[b] > mcap || ncnt[b] < 0 || ncnt[b] > ncap) return 3;
    const double metric_thr = thr[0], nocs_thr = thr[1];
    const float nocs_thr32 = (float)nocs_thr, scale_model = sm[0];
    std::vector<int32_t> cnn_idx((size_t)B * ncap, -7), gate((size_t)B * T), counts((size_t)B * T), plist((size_t)B * T, -7), pcount((size_t)B),
        best((size_t)B), n_inliers((size_t)B), mask((size_t)B * ncap, -7), found((size_t)B);
    std::vector<double> cnn_d((size_t)B * ncap, -7.0);
    std::vector<float> hyp((size_t)B * T * RS_TRANS, -7.0f), scale((size_t)B), rot((size_t)B * 9), tra((size_t)B * 3);
    // sample
    if (!has_idx) {
        idx.resize((size_t)B * T * 4);
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < T; ++t) rs_sample_draw(rs_sample_key((uint64_t)seed, (uint64_t)keys[b]), t, ncnt[b], &idx[((size_t)b * T + t) * 4]);
    }
    for (int b = 0; b < B; ++b) {
        const int N = ncnt[b], M = mcnt[b];
        const float* mp = &model[(size_t)b * mcap * 3];
        const float* mc = &mcls[(size_t)b * mcap * 3];
        const float* sp = &scene[(size_t)b * ncap * 3];
        const float* sc = &scls[(size_t)b * ncap * 3];
        // cnn: tiles of RS_TPB colours in index order
        for (int p = 0; p < N; ++p) {
            const double qx = sc[(size_t)p * 3], qy = sc[(size_t)p * 3 + 1], qz = sc[(size_t)p * 3 + 2];
            double bst = INFINITY;
            int bi = 0;
            for (int base = 0; base < M; base += RS_TPB) {
                const int n = M - base < RS_TPB ? M - base : RS_TPB;
                for (int k = 0; k < n; ++k) {
                    const int j = base + k;
#if defined(MUT_CNN_TIE_LAST)
                    const double dx = qx - (double)mc[(size_t)j * 3], dy = qy - (double)mc[(size_t)j * 3 + 1], dz = qz - (double)mc[(size_t)j * 3 + 2];
                    const double d2 = dx * dx + dy * dy + dz * dz;
                    if (d2 <= bst) { bst = d2; bi = j; }
#else
                    rs_cnn_step(qx, qy, qz, mc[(size_t)j * 3], mc[(size_t)j * 3 + 1], mc[(size_t)j * 3 + 2], j, &bst, &bi);
#endif
                }
            }
            cnn_idx[(size_t)b * ncap + p] = bi;
            cnn_d[(size_t)b * ncap + p] = sqrt(bst);
        }
        // hyp: blocks of RS_TPB hypotheses, 4 waves of 64; a passing hypothesis lands at base + (waves before) + (lanes before)
        int base_s = 0;
        for (int t0 = 0; t0 < T; t0 += RS_TPB) {
            bool pass[RS_TPB];
            for (int tid = 0; tid < RS_TPB; ++tid) {
                const int t = t0 + tid;
                pass[tid] = false;
                if (t >= T) continue;
                int flag = 0, cnt = -1;
                if (N >= 5 && M >= 1) {
                    const int32_t* ii = &idx[((size_t)b * T + t) * 4];
                    bool ok = true;
                    for (int k = 0; k < 4; ++k) ok &= ii[k] >= 0 && ii[k] < N;
                    if (ok) {
                        bool g = true;
                        for (int k = 0; k < 4; ++k) g &= !(cnn_d[(size_t)b * ncap + ii[k]] > nocs_thr);
                        if (g) {
                            flag = 1;
                            float fp[4][3], tp[4][3], row[RS_TRANS];
                            for (int k = 0; k < 4; ++k)
                                for (int d = 0; d < 3; ++d) {
                                    fp[k][d] = sp[(size_t)ii[k] * 3 + d];
                                    tp[k][d] = mp[(size_t)cnn_idx[(size_t)b * ncap + ii[k]] * 3 + d];
                                }
                            int bits;
                            if (sample_fit(fp, tp, f16, type, row, &bits)) {
                                cnt = 0;
                                pass[tid] = true;
                                for (int k = 0; k < RS_TRANS; ++k) hyp[((size_t)b * T + t) * RS_TRANS + k] = row[k];
                            }
                            flag |= bits;
                        }
                    }
                }
                gate[(size_t)b * T + t] = flag;
                counts[(size_t)b * T + t] = cnt;
            }
            int wc[RS_TPB / 64], tot = 0;
            for (int w = 0; w < RS_TPB / 64; ++w) {
                wc[w] = 0;
                for (int l = 0; l < 64; ++l) wc[w] += pass[w * 64 + l];
                tot += wc[w];
            }
            for (int tid = 0; tid < RS_TPB; ++tid) {
                if (!pass[tid]) continue;
                const int wv = tid >> 6, lane = tid & 63;
                int woff = 0, before = 0;
                for (int k = 0; k < wv; ++k) woff += wc[k];
                for (int l = 0; l < lane; ++l) before += pass[wv * 64 + l];
                plist[(size_t)b * T + base_s + woff + before] = t0 + tid;
            }
            base_s += tot;
        }
        pcount[b] = base_s;
        // score: (chunk of RS_TPB points) x (group of RS_HG passing hypotheses)
        const int np = pcount[b];
        for (int g0 = 0; g0 < np; g0 += RS_HG) {
            const int nh = np - g0 < RS_HG ? np - g0 : RS_HG;
            for (int c0 = 0; c0 < N; c0 += RS_TPB) {
                int hc[RS_HG], hid[RS_HG];
                for (int hh = 0; hh < RS_HG; ++hh) {
                    hc[hh] = 0;
                    hid[hh] = plist[(size_t)b * T + g0 + (hh < nh ? hh : 0)];
                }
                for (int tid = 0; tid < RS_TPB; ++tid) {
                    const int p = c0 + tid;
                    if (p >= N) continue;
                    for (int hh = 0; hh < nh; ++hh) {
                        const PoseV3 tp = rs_transform(&hyp[((size_t)b * T + hid[hh]) * RS_TRANS], sp[(size_t)p * 3], sp[(size_t)p * 3 + 1], sp[(size_t)p * 3 + 2]);
                        const int nn = nn_search(tp, mp, M);
                        hc[hh] += inlier(tp, nn, mp, mc, sc[(size_t)p * 3], sc[(size_t)p * 3 + 1], sc[(size_t)p * 3 + 2], metric_thr, nocs_thr32) ? 1 : 0;
                    }
                }
                for (int tid = 0; tid < nh; ++tid)
                    if (hc[tid] > 0) counts[(size_t)b * T + hid[tid]] += hc[tid];
            }
        }
        // select: 256 lanes walk t = tid, tid + 256, ...; then the tree
        {
            int sc_[RS_TPB], st_[RS_TPB];
            for (int tid = 0; tid < RS_TPB; ++tid) {
                int bc = 0, bt = -1;
                for (int t = tid; t < T; t += RS_TPB) {
                    const int c = counts[(size_t)b * T + t];
#if defined(MUT_SELECT_GE)
                    if (c >= bc) { bc = c; bt = t; }
#else
                    if (rs_select_takes(c, bc)) { bc = c; bt = t; }
#endif
                }
                sc_[tid] = bc;
                st_[tid] = bt;
            }
            for (int o = RS_TPB / 2; o > 0; o >>= 1)
                for (int tid = 0; tid < o; ++tid)
                    if (rs_select_folds(sc_[tid + o], st_[tid + o], sc_[tid], st_[tid])) { sc_[tid] = sc_[tid + o]; st_[tid] = st_[tid + o]; }
            best[b] = st_[0];
            n_inliers[b] = sc_[0];
        }
        // mask
        const int bt = best[b];
        for (int p = 0; p < N; ++p) {
            if (bt < 0) { mask[(size_t)b * ncap + p] = 0; continue; }
            const PoseV3 tp = rs_transform(&hyp[((size_t)b * T + bt) * RS_TRANS], sp[(size_t)p * 3], sp[(size_t)p * 3 + 1], sp[(size_t)p * 3 + 2]);
            const int nn = nn_search(tp, mp, M);
            mask[(size_t)b * ncap + p] = inlier(tp, nn, mp, mc, sc[(size_t)p * 3], sc[(size_t)p * 3 + 1], sc[(size_t)p * 3 + 2], metric_thr, nocs_thr32) ? 1 : 0;
        }
        // final
        const int ni = n_inliers[b];
        bool ok = N >= 5 && ni >= 5;
        double R[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, c = 0.0, t[3] = {0.0, 0.0, 0.0};
        if (ok) {
            const int32_t* mk = &mask[(size_t)b * ncap];
            std::vector<double> red((size_t)10 * RS_TPB, 0.0);
            double v6[7], v10[10], mf[3], mt[3];
            for (int tid = 0; tid < RS_TPB; ++tid) {
                double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (int p = tid; p < N; p += RS_TPB)
                    if (mk[p]) rs_final_sums(mp + (size_t)cnn_idx[(size_t)b * ncap + p] * 3, sp + (size_t)p * 3, v);
                for (int k = 0; k < 7; ++k) red[(size_t)k * RS_TPB + tid] = v[k];
            }
            block_sum(red, 7, v6);
            rs_final_means(v6, f16, mf, mt);
#if defined(MUT_NO_F16_MEAN_ROUND)
            if (f16)
                for (int d = 0; d < 3; ++d) mf[d] = v6[d] / v6[6];
#endif
            for (int tid = 0; tid < RS_TPB; ++tid) {
                double v[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (int p = tid; p < N; p += RS_TPB)
                    if (mk[p]) rs_final_cov(mp + (size_t)cnn_idx[(size_t)b * ncap + p] * 3, sp + (size_t)p * 3, mf, mt, f16, v);
                for (int k = 0; k < 10; ++k) red[(size_t)k * RS_TPB + tid] = v[k];
            }
            block_sum(red, 10, v10);
            double H[3][3], ratio;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) H[i][j] = v10[i * 3 + j];
            ok = rs_fit(H, mf, mt, v10[9], type, R, &c, t, &ratio);
        }
        found[b] = ok ? 1 : 0;
        if (!ok) n_inliers[b] = ni > 0 ? ni : 0;
        scale[b] = ok ? (type == 1 ? (float)c : scale_model) : 0.0f;
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) rot[(size_t)b * 9 + i * 3 + j] = ok ? (float)R[i][j] : 0.0f;
            tra[(size_t)b * 3 + i] = ok ? (float)t[i] : 0.0f;
        }
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 4;
    wr(o, idx), wr(o, cnn_idx), wr(o, cnn_d), wr(o, gate), wr(o, counts), wr(o, hyp), wr(o, plist), wr(o, pcount), wr(o, best), wr(o, n_inliers),
        wr(o, mask), wr(o, found), wr(o, scale), wr(o, rot), wr(o, tra);
    fclose(o);
    return 0;
}
