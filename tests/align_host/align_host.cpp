// Host harness of csrc/align_cells.h (tests/test_align_cpu.py): the kernels of csrc/align.hip with their workgroups and threads as loops,
// every per-element rule taken from the headers.  Reads one binary file, writes one; all buffers have their exact sizes, so a sanitizer
// build sees any step outside them.  int64 head[10] first.
//   align_host samples IN: head = N B F shape0 seed eta_bits s_max_bits has_normals | int64 ptoff[B + 1] | float origin[3] | float points[N][3] |
//                          double normals[N][3] (with has_normals)
//                      OUT: float rows[N (3 + F)][5] | int32 flags[B]
//   align_host rows    IN: head = S B k draw seed iter L unit shape0 | int64 soff[B + 1] | float samples[S][5] | float z[B][L] | float pose[B][6]
//                      OUT: float inputs[B k][L + 3] | float cam[B k][3] | float lo[B k] | float hi[B k] | float zn[B][L] | int32 flags[B]
//   align_host reduce  IN: head = B k L Jstride clamp_bits | float pred[B k] | float lo[B k] | float hi[B k] | float J[B k][Jstride] |
//                          float cam[B k][3] | float pose[B][6] | int32 flags[B]
//                      OUT: double loss[B] | double g[B][L + 5] | double part[B][chunks][L + 7] | int32 flags[B]
//   align_host step    IN: head = B L unit t code_reg_bits lr_bits | float lr_pose[5] | float z, m, v [B][L] | float theta, tm, tv [B][5] |
//                          float pose[B][6] | double g[B][L + 5] | int32 flags[B]
//                      OUT: float z, m, v [B][L] | float theta, tm, tv [B][5] | float pose[B][6] | int32 flags[B]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "align_cells.h"

#define THREADS 256

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_exact(FILE* f, const void* p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }
static float bits_float(int64_t w) {
    const uint32_t u = (uint32_t)w;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static double bits_double(int64_t w) {
    double d;
    std::memcpy(&d, &w, 8);
    return d;
}

static int run_samples(FILE* in, FILE* out, const int64_t* head) {
    const int64_t N = head[0];
    const int B = (int)head[1], F = (int)head[2], shape0 = (int)head[3];
    const uint64_t seed = (uint64_t)head[4];
    const double eta = bits_double(head[5]), s_max = bits_double(head[6]);
    const bool has_normals = head[7] != 0;
    if (N < 0 || B < 1 || F < 0 || F > CPL_MAX_FREE) return 2;
    std::vector<int64_t> ptoff(B + 1);
    std::vector<float> origin(3), points((size_t)N * 3);
    std::vector<double> normals(has_normals ? (size_t)N * 3 : 0);
    if (!read_exact(in, ptoff.data(), ptoff.size() * 8) || !read_exact(in, origin.data(), 12) || !read_exact(in, points.data(), points.size() * 4) ||
        !read_exact(in, normals.data(), normals.size() * 8))
        return 3;
    const int P = 3 + F;
    std::vector<float> rows((size_t)N * P * ALN_ROW);
    std::vector<int32_t> flags(B);
    const int64_t threads = N > B ? N : (int64_t)B;
    for (int64_t g = 0; g < threads; ++g) {                                          // sdfr_align_samples_kernel, thread g
        if (g < B) flags[g] = cpl_table_ok(ptoff.data(), (int)g, N) ? 0 : CPL_BAD_TABLE;
        if (g >= N) continue;
        const int b = cpl_owner(ptoff.data(), B, N, g);
        // exact-size copies of what the thread may read: the sanitizer build sees a step outside the point's own words
        std::vector<float> p(points.begin() + 3 * g, points.begin() + 3 * g + 3);
        std::vector<double> n;
        if (has_normals) n.assign(normals.begin() + 3 * g, normals.begin() + 3 * g + 3);
        std::vector<float> o((size_t)P * ALN_ROW);
        aln_sample_row(p.data(), has_normals ? n.data() : nullptr, origin.data(), b >= 0, seed, shape0 + (b < 0 ? 0 : b), b < 0 ? 0 : g - ptoff[b], F, eta,
                       s_max, o.data());
        std::memcpy(rows.data() + (size_t)g * P * ALN_ROW, o.data(), o.size() * 4);
    }
    return write_exact(out, rows.data(), rows.size() * 4) && write_exact(out, flags.data(), flags.size() * 4) ? 0 : 4;
}

static int run_rows(FILE* in, FILE* out, const int64_t* head) {
    const int W = ALN_ROW;
    const int64_t S = head[0], k = head[2], iter = head[5];
    const int B = (int)head[1], draw = (int)head[3], L = (int)head[6], unit = (int)head[7], shape0 = (int)head[8];
    const uint64_t seed = (uint64_t)head[4];
    if (S < 0 || B < 0 || B > ENC_MAX_B || k < 1 || k > ENC_MAX_K || L < 1 || L > ENC_MAX_L) return 2;
    const int NI = L + 3;
    std::vector<int64_t> soff(B + 1);
    std::vector<float> samples(S * W), z((size_t)B * L), pose((size_t)B * VERIFY_POSE);
    if (!read_exact(in, soff.data(), soff.size() * 8) || !read_exact(in, samples.data(), samples.size() * 4) || !read_exact(in, z.data(), z.size() * 4) ||
        !read_exact(in, pose.data(), pose.size() * 4))
        return 3;
    std::vector<float> inputs((size_t)B * k * NI), cam((size_t)B * k * 3), lo((size_t)B * k), hi((size_t)B * k), zn((size_t)B * L);
    std::vector<int32_t> flags(B);
    const int64_t blocks = (k + THREADS - 1) / THREADS;
    for (int b = 0; b < B; ++b)
        for (int64_t bx = 0; bx < blocks; ++bx) {                                    // sdfr_align_rows_kernel, workgroup (bx, b)
            std::vector<float> s_zn(L), s_x((size_t)THREADS * 3);
            const int64_t count = enc_count(soff.data(), b, S);
            const bool bad = count < 0 || (!draw && count > 0 && k > count);
            const bool zero = bad || count == 0;
            const std::vector<float> ps(pose.begin() + VERIFY_POSE * b, pose.begin() + VERIFY_POSE * (b + 1));
            const bool ok = cpl_pose_ok(ps.data());
            const float nrm = unit ? latent_norm(z.data() + (size_t)b * L, L) : 1.f;
            for (int tid = 0; tid < L; ++tid) {
                const float v = unit ? z[(size_t)b * L + tid] / nrm : z[(size_t)b * L + tid];
                s_zn[tid] = v;
                if (bx == 0) zn[(size_t)b * L + tid] = v;
            }
            if (bx == 0) flags[b] = aln_rows_flags(bad, count, ok);
            const int64_t s0 = bx * THREADS;
            const int rows = (int)((k - s0) < THREADS ? (k - s0) : THREADS);
            for (int tid = 0; tid < rows; ++tid) {
                const int64_t s = s0 + tid;
                const size_t i = (size_t)b * k + s;
                float q[3] = {0.f, 0.f, 0.f}, x[3] = {0.f, 0.f, 0.f}, l = 0.f, h = 0.f;
                if (!zero) {
                    const int64_t src = soff[b] + (draw ? enc_draw(seed, iter, shape0 + b, s, count) : s);
                    for (int a = 0; a < 3; ++a) q[a] = samples.at((size_t)src * W + a);
                    l = samples.at((size_t)src * W + 3), h = samples.at((size_t)src * W + 4);
                    aln_row(q, ps.data(), ok, x, &l, &h);
                }
                for (int a = 0; a < 3; ++a) cam[3 * i + a] = q[a], s_x[3 * tid + a] = x[a];
                lo[i] = l, hi[i] = h;
            }
            float* o = inputs.data() + ((size_t)b * k + s0) * NI;
            for (int e = 0; e < rows * NI; ++e) {
                const int r = e / NI, c = e - r * NI;
                o[e] = zero ? 0.f : (c < L ? s_zn[c] : s_x[3 * r + (c - L)]);
            }
        }
    return write_exact(out, inputs.data(), inputs.size() * 4) && write_exact(out, cam.data(), cam.size() * 4) && write_exact(out, lo.data(), lo.size() * 4) &&
                   write_exact(out, hi.data(), hi.size() * 4) && write_exact(out, zn.data(), zn.size() * 4) && write_exact(out, flags.data(), flags.size() * 4)
               ? 0 : 4;
}

static int run_reduce(FILE* in, FILE* out, const int64_t* head) {
    const int B = (int)head[0], L = (int)head[2], Jstride = (int)head[3];
    const int64_t k = head[1];
    const float clamp = bits_float(head[4]);
    if (B < 0 || B > ENC_MAX_B || k < 1 || k > ENC_MAX_K || L < 1 || L > ENC_MAX_L || Jstride < L + 3) return 2;
    const size_t n_all = (size_t)B * k;
    std::vector<float> pred(n_all), lo(n_all), hi(n_all), J(n_all * Jstride), cam(n_all * 3), pose((size_t)B * VERIFY_POSE);
    std::vector<int32_t> flags(B);
    if (!read_exact(in, pred.data(), n_all * 4) || !read_exact(in, lo.data(), n_all * 4) || !read_exact(in, hi.data(), n_all * 4) ||
        !read_exact(in, J.data(), J.size() * 4) || !read_exact(in, cam.data(), cam.size() * 4) || !read_exact(in, pose.data(), pose.size() * 4) ||
        !read_exact(in, flags.data(), flags.size() * 4))
        return 3;
    const int64_t chunks = enc_chunks(k);
    const int G = L + ALN_POSE, NC = G + 2;
    std::vector<double> part((size_t)B * chunks * NC), loss(B), g((size_t)B * G);
    for (int b = 0; b < B; ++b)
        for (int64_t ch = 0; ch < chunks; ++ch) {                                  // enc_chunk_kernel<AlnRowRule, AlnCols>, workgroup (ch, b)
            const int64_t row0 = ch * ENC_CHUNK;
            const int n = (int)((k - row0) < ENC_CHUNK ? (k - row0) : ENC_CHUNK);
            const size_t base = (size_t)b * k + row0;
            const float* ps = pose.data() + (size_t)VERIFY_POSE * b;
            std::vector<double> s_e(n), s_acc((size_t)ENC_SLOTS * (ENC_COLS + 1));
            std::vector<float> s_w(n);
            std::vector<unsigned char> s_ok(n);
            for (int r = 0; r < n; ++r) {
                const EncRow q = cpl_row(aln_metric(pred[base + r], ps), lo[base + r], hi[base + r], clamp);
                s_e[r] = q.e; s_w[r] = q.w; s_ok[r] = (unsigned char)q.ok;
            }
            for (int c0 = 0; c0 < NC; c0 += ENC_COLS) {
                const int nc = (NC - c0) < ENC_COLS ? (NC - c0) : ENC_COLS;
                for (int e = 0; e < ENC_SLOTS * nc; ++e) {
                    const int j = e / nc, c = c0 + (e - j * nc);
                    double a = 0.0;
                    ENC_SLOT_ROWS(r, j, n)
                        a += aln_value(c, L, s_w[r], s_e[r], s_ok[r], pred[base + r], J.data() + (base + r) * Jstride, cam.data() + 3 * (base + r), ps);
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
    for (int b = 0; b < B; ++b) {                                                    // enc_fold_kernel, workgroup b
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
    return write_exact(out, loss.data(), loss.size() * 8) && write_exact(out, g.data(), g.size() * 8) && write_exact(out, part.data(), part.size() * 8) &&
                   write_exact(out, flags.data(), flags.size() * 4) ? 0 : 4;
}

static int run_step(FILE* in, FILE* out, const int64_t* head) {
    const int B = (int)head[0], L = (int)head[1], unit = (int)head[2], t = (int)head[3];
    const float code_reg = bits_float(head[4]), lr = bits_float(head[5]);
    if (B < 0 || B > ENC_MAX_B || L < 1 || L > ENC_MAX_L || t < 1) return 2;
    const int G = L + ALN_POSE;
    std::vector<float> rates(ALN_POSE), z((size_t)B * L), m((size_t)B * L), v((size_t)B * L), theta((size_t)B * ALN_POSE), tm((size_t)B * ALN_POSE),
        tv((size_t)B * ALN_POSE), pose((size_t)B * VERIFY_POSE);
    std::vector<double> g((size_t)B * G);
    std::vector<int32_t> flags(B);
    if (!read_exact(in, rates.data(), rates.size() * 4) || !read_exact(in, z.data(), z.size() * 4) || !read_exact(in, m.data(), m.size() * 4) ||
        !read_exact(in, v.data(), v.size() * 4) || !read_exact(in, theta.data(), theta.size() * 4) || !read_exact(in, tm.data(), tm.size() * 4) ||
        !read_exact(in, tv.data(), tv.size() * 4) || !read_exact(in, pose.data(), pose.size() * 4) || !read_exact(in, g.data(), g.size() * 8) ||
        !read_exact(in, flags.data(), flags.size() * 4))
        return 3;
    float bc1, bc2;
    enc_bias(t, &bc1, &bc2);
    for (int b = 0; b < B; ++b) {                                                    // sdfr_align_step_kernel, workgroup b
        float* zb = z.data() + (size_t)b * L;
        const double* gb = g.data() + (size_t)b * G;
        float *th = theta.data() + (size_t)ALN_POSE * b, *mb = tm.data() + (size_t)ALN_POSE * b, *vb = tv.data() + (size_t)ALN_POSE * b;
        std::vector<float> s_g(L);
        for (int i = 0; i < L; ++i) s_g[i] = (float)gb[i];
        const int fl = flags[b];
        const float nrm = unit ? latent_norm(zb, L) : 1.f;
        const float dot = unit ? latent_unit_dot(zb, s_g.data(), L, nrm) : 0.f;
        const float nz = unit ? 0.f : enc_raw_norm(zb, L);
        int skip = (fl & (ENC_EMPTY | ENC_NO_ROWS | ENC_BAD_TABLE | ALN_BAD_POSE)) ? 1 : 0;
        for (int i = 0; i < L; ++i)
            if (!isfinite(enc_step_grad(zb[i], s_g[i], unit, nrm, dot, nz, code_reg))) skip = 1;
        if (!aln_pose_grad_ok(gb, L)) skip = 1;
        const float sc = aln_scale_after(th, mb, vb, gb, L, rates[4], bc1, bc2);
        if (!(isfinite(sc) && sc > 0.f)) skip = 1;
        if (skip) {
            flags[b] = fl | ENC_SKIPPED;
            continue;
        }
        std::vector<float> gi(L);
        for (int i = 0; i < L; ++i) gi[i] = enc_step_grad(zb[i], s_g[i], unit, nrm, dot, nz, code_reg);      // every thread reads z before any update
        if (lr != 0.f)
            for (int i = 0; i < L; ++i) latent_adam(&zb[i], &m[(size_t)b * L + i], &v[(size_t)b * L + i], gi[i], lr, bc1, bc2);
        aln_pose_step(th, mb, vb, gb, L, rates.data(), bc1, bc2, pose.data() + (size_t)VERIFY_POSE * b);
    }
    return write_exact(out, z.data(), z.size() * 4) && write_exact(out, m.data(), m.size() * 4) && write_exact(out, v.data(), v.size() * 4) &&
                   write_exact(out, theta.data(), theta.size() * 4) && write_exact(out, tm.data(), tm.size() * 4) && write_exact(out, tv.data(), tv.size() * 4) &&
                   write_exact(out, pose.data(), pose.size() * 4) && write_exact(out, flags.data(), flags.size() * 4) ? 0 : 4;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    int64_t head[10];
    int rc = 3;
    if (read_exact(in, head, sizeof(head))) {
        if (std::strcmp(argv[1], "samples") == 0) rc = run_samples(in, out, head);
        else if (std::strcmp(argv[1], "rows") == 0) rc = run_rows(in, out, head);
        else if (std::strcmp(argv[1], "reduce") == 0) rc = run_reduce(in, out, head);
        else if (std::strcmp(argv[1], "step") == 0) rc = run_step(in, out, head);
        else rc = 2;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? rc : 4;
}
