// The kernels of csrc/encode_kernels.h on the host, ONCE, for the three harnesses (tests/{encode,complete,align}_host): the workgroups and
// threads of the samples, rows, chunk, fold and step kernels as loops, over the SAME policy structs the kernels are instantiated with
// (csrc/encode_cells.h, complete_cells.h, align_cells.h).  Every buffer is a vector of its exact size and the policies point into such
// vectors, so a sanitizer build sees any step outside them; what a thread reads of the samples goes through .at() first.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "align_cells.h"

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_exact(FILE* f, const void* p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }
template <class... V>
static bool read_all(FILE* f, V&... v) { return (read_exact(f, v.data(), v.size() * sizeof(v[0])) && ...); }
template <class... V>
static bool write_all(FILE* f, const V&... v) { return (write_exact(f, v.data(), v.size() * sizeof(v[0])) && ...); }
static inline float bits_float(int64_t w) {
    const uint32_t u = (uint32_t)w;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static inline double bits_double(int64_t w) {
    double d;
    std::memcpy(&d, &w, 8);
    return d;
}

// enc_samples_kernel<POSED>, thread g.  rows [N (3 + F)][5], flags [B]; pose [B][6] with POSED.
template <bool POSED>
static void host_samples(const std::vector<float>& points, const std::vector<double>& normals, bool has_normals, int64_t N, const std::vector<int64_t>& ptoff,
                         int B, const std::vector<float>& pose, const std::vector<float>& origin, int shape0, int F, double eta, double s_max, uint64_t seed,
                         std::vector<float>& rows, std::vector<int32_t>& flags) {
    const int P = 3 + F;
    const int64_t threads = N > B ? N : (int64_t)B;
    for (int64_t g = 0; g < threads; ++g) {
        if (g < B) flags[g] = POSED ? cpl_view_flags(ptoff.data(), pose.data(), (int)g, N) : (cpl_table_ok(ptoff.data(), (int)g, N) ? 0 : CPL_BAD_TABLE);
        if (g >= N) continue;
        const int b = cpl_owner(ptoff.data(), B, N, g), bb = b < 0 ? 0 : b;
        const int64_t i = b < 0 ? 0 : g - ptoff[b];
        // exact-size copies of what the thread may read: the sanitizer build sees a step outside the point's own words
        std::vector<float> p(points.begin() + 3 * g, points.begin() + 3 * g + 3), ps, o((size_t)P * CPL_ROW);
        std::vector<double> n;
        if (has_normals) n.assign(normals.begin() + 3 * g, normals.begin() + 3 * g + 3);
        if (POSED) {
            ps.assign(pose.begin() + VERIFY_POSE * bb, pose.begin() + VERIFY_POSE * (bb + 1));
            cpl_view_row(p.data(), has_normals ? n.data() : nullptr, ps.data(), origin.data(), b >= 0 && cpl_pose_ok(ps.data()), seed, shape0 + bb, i, F, eta,
                         s_max, o.data());
        } else {
            aln_sample_row(p.data(), has_normals ? n.data() : nullptr, origin.data(), b >= 0, seed, shape0 + bb, i, F, eta, s_max, o.data());
        }
        std::memcpy(rows.data() + (size_t)g * P * CPL_ROW, o.data(), o.size() * 4);
    }
}

// enc_rows_kernel<Rows>, workgroup (bx, b).  inputs [B k][L + 3], zn [B][L], flags [B]; the side arrays are the policy's.
template <class Rows>
static void host_rows(const std::vector<float>& samples, int64_t S, const std::vector<int64_t>& soff, int B, int shape0, int64_t k, int draw, uint64_t seed,
                      int64_t iter, const std::vector<float>& z, int L, int unit, const Rows& rows, std::vector<float>& inputs, std::vector<float>& zn,
                      std::vector<int32_t>& flags) {
    const int NI = L + 3;
    const int64_t blocks = (k + ENC_THREADS - 1) / ENC_THREADS;
    for (int b = 0; b < B; ++b)
        for (int64_t bx = 0; bx < blocks; ++bx) {
            std::vector<float> s_zn(L);
            std::vector<typename Rows::Staged> s_row(ENC_THREADS);
            const int64_t count = enc_count(soff.data(), b, S);
            const bool bad = count < 0 || (!draw && count > 0 && k > count);
            const bool zero = bad || count == 0;
            const typename Rows::Shape shape = rows.shape(b);
            const float nrm = unit ? latent_norm(z.data() + (size_t)b * L, L) : 1.f;
            for (int tid = 0; tid < L; ++tid) {
                const float v = unit ? z[(size_t)b * L + tid] / nrm : z[(size_t)b * L + tid];
                s_zn[tid] = v;
                if (bx == 0) zn[(size_t)b * L + tid] = v;
            }
            if (bx == 0) flags[b] = rows.flags(shape, bad, count);
            const int64_t s0 = bx * ENC_THREADS;
            const int n = (int)((k - s0) < ENC_THREADS ? (k - s0) : ENC_THREADS);
            for (int tid = 0; tid < n; ++tid) {
                const int64_t s = s0 + tid;
                const int64_t src = zero ? -1 : soff[b] + (draw ? enc_draw(seed, iter, shape0 + b, s, count) : s);
                if (src >= 0) (void)samples.at((size_t)src * Rows::W + Rows::W - 1);
                s_row[tid] = rows.stage(shape, samples.data(), src, (int64_t)b * k + s);
            }
            float* o = inputs.data() + ((size_t)b * k + s0) * NI;
            for (int e = 0; e < n * NI; ++e) {
                const int r = e / NI, c = e - r * NI;
                o[e] = zero ? 0.f : (c < L ? s_zn[c] : rows.xyz(samples.data(), s_row.at(r), c - L));
            }
        }
}

// enc_chunk_kernel<Rule, Cols>, workgroup (ch, b), then enc_fold_kernel, workgroup b: THE chunk and fold loops of the host.
// part [B][chunks][G + 2], loss [B], g [B][G]; flags [B] on entry and exit.
template <class Rule, class Cols>
static void host_reduce(const std::vector<float>& pred, const Rule& rule, const Cols& cols, int G, int B, int64_t k, float clamp, std::vector<double>& part,
                        std::vector<double>& loss, std::vector<double>& g, std::vector<int32_t>& flags) {
    const int64_t chunks = enc_chunks(k);
    const int NC = G + 2;
    for (int b = 0; b < B; ++b)
        for (int64_t ch = 0; ch < chunks; ++ch) {
            const int64_t row0 = ch * ENC_CHUNK;
            const int n = (int)((k - row0) < ENC_CHUNK ? (k - row0) : ENC_CHUNK);
            const int64_t base = (int64_t)b * k + row0;
            std::vector<double> s_e(n), s_acc((size_t)ENC_SLOTS * (ENC_COLS + 1)), s_x((size_t)n * Cols::EXTRA);
            std::vector<float> s_w(n);
            std::vector<unsigned char> s_ok(n);
            for (int r = 0; r < n; ++r) {
                const EncRow q = rule(pred.at(base + r), base + r, b, clamp);
                s_e[r] = q.e; s_w[r] = q.w; s_ok[r] = (unsigned char)q.ok;
                cols.prepare(s_x.data() + (size_t)r * Cols::EXTRA, q.w, base + r, b);
            }
            for (int c0 = 0; c0 < NC; c0 += ENC_COLS) {
                const int nc = (NC - c0) < ENC_COLS ? (NC - c0) : ENC_COLS;
                for (int e = 0; e < ENC_SLOTS * nc; ++e) {
                    const int j = e / nc, c = c0 + (e - j * nc);
                    double a = 0.0;
                    ENC_SLOT_ROWS(r, j, n) a += cols(c, G, s_w[r], s_e[r], s_ok[r], base + r, b, s_x.data() + (size_t)r * Cols::EXTRA);
                    s_acc[(size_t)j * (ENC_COLS + 1) + (c - c0)] = a;
                }
                for (int o = ENC_SLOTS / 2; o > 0; o >>= 1)
                    for (int e = 0; e < o * nc; ++e) {
                        const int j = e / nc, cc = e - j * nc;
                        enc_tree_step(s_acc.data() + cc, ENC_COLS + 1, j, o);
                    }
                for (int c = 0; c < nc; ++c) part[((size_t)b * chunks + ch) * NC + c0 + c] = s_acc[c];
            }
        }
    for (int b = 0; b < B; ++b) {
        std::vector<double> tot(NC);
        for (int c = 0; c < NC; ++c) {
            double a = 0.0;
            for (int64_t ch = 0; ch < chunks; ++ch) a += part[((size_t)b * chunks + ch) * NC + c];
            tot[c] = a;
        }
        const double n_ok = tot[G + 1];
        for (int c = 0; c < G; ++c) g[(size_t)b * G + c] = enc_mean(tot[c], n_ok);
        loss[b] = enc_mean(tot[G], n_ok);
        if (!(n_ok > 0.0)) flags[b] |= ENC_NO_ROWS;
    }
}

// enc_step_kernel<Pose>, workgroup b.  z, m, v [B][L]; g [B][L + Pose::EXTRA]; the pose's own state is the policy's.
template <class Pose>
static void host_step(std::vector<float>& z, std::vector<float>& m, std::vector<float>& v, int L, int B, int unit, const Pose& pose,
                      const std::vector<double>& g, std::vector<int32_t>& flags, float code_reg, float lr, int t) {
    float bc1, bc2;
    enc_bias(t, &bc1, &bc2);
    for (int b = 0; b < B; ++b) {
        float* zb = z.data() + (size_t)b * L;
        const double* gb = g.data() + (size_t)b * (L + Pose::EXTRA);
        std::vector<float> s_g(L);
        for (int i = 0; i < L; ++i) s_g[i] = (float)gb[i];
        const int fl = flags[b];
        const float nrm = unit ? latent_norm(zb, L) : 1.f;
        const float dot = unit ? latent_unit_dot(zb, s_g.data(), L, nrm) : 0.f;
        const float nz = unit ? 0.f : enc_raw_norm(zb, L);
        int skip = (fl & Pose::SKIP) ? 1 : 0;
        for (int i = 0; i < L; ++i)
            if (!isfinite(enc_step_grad(zb[i], s_g[i], unit, nrm, dot, nz, code_reg))) skip = 1;
        if (!pose.ok(b, gb, L, bc1, bc2)) skip = 1;
        if (skip) {
            flags[b] = fl | ENC_SKIPPED;
            continue;
        }
        for (int tid = 0; tid < L && pose.steps_latent(lr); ++tid) {                  // (element tid's gradient reads element tid of z alone)
            const float gi = enc_step_grad(zb[tid], s_g[tid], unit, nrm, dot, nz, code_reg);
            latent_adam(&zb[tid], &m[(size_t)b * L + tid], &v[(size_t)b * L + tid], gi, lr, bc1, bc2);
        }
        pose.step(b, gb, L, bc1, bc2);
    }
}

// the sizes every mode refuses
static inline bool host_sizes_ok(int B, int64_t k, int L) { return B >= 0 && B <= ENC_MAX_B && k >= 1 && k <= ENC_MAX_K && L >= 1 && L <= ENC_MAX_L; }

// `prog MODE IN OUT`: reads int64 head[head_words] and hands the rest to run(mode, in, out, head); its return value is the exit status
static int host_main(int argc, char** argv, int head_words, int (*run)(const char*, FILE*, FILE*, const int64_t*)) {
    if (argc != 4) return 2;
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    std::vector<int64_t> head(head_words);
    const int rc = read_all(in, head) ? run(argv[1], in, out, head.data()) : 3;
    std::fclose(in);
    return std::fclose(out) == 0 ? rc : 4;
}
