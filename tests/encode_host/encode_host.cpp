// Host harness of csrc/encode_cells.h (tests/test_encode_cpu.py): the three kernels of csrc/encode.hip with their workgroups and threads as
// loops, every per-element rule and the summation order taken from the header.  Reads one binary file, writes one; all buffers have their
// exact sizes, so a sanitizer build sees any step outside them.
//   encode_host rows   IN OUT   IN: int64 head[9] = S B k draw seed iter L unit shape0 | int64 soff[B + 1] | float samples[S][4] | float z[B][L]
//                               OUT: float inputs[B k][L + 3] | float target[B k] | float zn[B][L] | int32 flags[B]
//   encode_host reduce IN OUT   IN: int64 head[9] = B k L Jstride clamp_bits 0 0 0 0 | float pred[B k] | float target[B k] | float J[B k][Jstride] | int32 flags[B]
//                               OUT: double loss[B] | double g_zn[B][L] | double part[B][chunks][L + 2] | int32 flags[B]
//   encode_host step   IN OUT   IN: int64 head[9] = B L unit t code_reg_bits lr_bits 0 0 0 | float z, m, v [B][L] | double g_zn[B][L] | int32 flags[B]
//                               OUT: float z, m, v [B][L] | int32 flags[B]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "encode_cells.h"

#define THREADS 256

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }
static bool write_exact(FILE* f, const void* p, size_t bytes) { return bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes; }
static float bits_float(int64_t w) {
    const uint32_t u = (uint32_t)w;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static int run_rows(FILE* in, FILE* out, const int64_t* head) {
    const int64_t S = head[0], k = head[2], iter = head[5];
    const int B = (int)head[1], draw = (int)head[3], L = (int)head[6], unit = (int)head[7], shape0 = (int)head[8];
    const uint64_t seed = (uint64_t)head[4];
    if (S < 0 || B < 0 || B > ENC_MAX_B || k < 1 || k > ENC_MAX_K || L < 1 || L > ENC_MAX_L) return 2;
    const int NI = L + 3;
    std::vector<int64_t> soff(B + 1);
    std::vector<float> samples(S * 4), z((size_t)B * L);
    if (!read_exact(in, soff.data(), soff.size() * 8) || !read_exact(in, samples.data(), samples.size() * 4) || !read_exact(in, z.data(), z.size() * 4))
        return 3;
    std::vector<float> inputs((size_t)B * k * NI), target((size_t)B * k), zn((size_t)B * L);
    std::vector<int32_t> flags(B);
    const int64_t blocks = (k + THREADS - 1) / THREADS;
    for (int b = 0; b < B; ++b)
        for (int64_t bx = 0; bx < blocks; ++bx) {
            std::vector<float> s_zn(L);
            std::vector<int64_t> s_src(THREADS);
            const int64_t count = enc_count(soff.data(), b, S);
            const bool bad = count < 0 || (!draw && count > 0 && k > count);
            const bool zero = bad || count == 0;
            const float nrm = unit ? latent_norm(z.data() + (size_t)b * L, L) : 1.f;
            for (int tid = 0; tid < L; ++tid) {
                const float v = unit ? z[(size_t)b * L + tid] / nrm : z[(size_t)b * L + tid];
                s_zn[tid] = v;
                if (bx == 0) zn[(size_t)b * L + tid] = v;
            }
            if (bx == 0) flags[b] = bad ? ENC_BAD_TABLE : (count == 0 ? ENC_EMPTY : 0);
            const int64_t s0 = bx * THREADS;
            const int rows = (int)((k - s0) < THREADS ? (k - s0) : THREADS);
            for (int tid = 0; tid < rows; ++tid) {
                const int64_t s = s0 + tid;
                const int64_t src = zero ? -1 : soff[b] + (draw ? enc_draw(seed, iter, shape0 + b, s, count) : s);
                s_src[tid] = src;
                target[(size_t)b * k + s] = zero ? 0.f : samples.at((size_t)src * 4 + 3);
            }
            float* o = inputs.data() + ((size_t)b * k + s0) * NI;
            for (int e = 0; e < rows * NI; ++e) {
                const int r = e / NI, c = e - r * NI;
                o[e] = zero ? 0.f : (c < L ? s_zn[c] : samples.at((size_t)s_src[r] * 4 + (c - L)));
            }
        }
    return write_exact(out, inputs.data(), inputs.size() * 4) && write_exact(out, target.data(), target.size() * 4) &&
                   write_exact(out, zn.data(), zn.size() * 4) && write_exact(out, flags.data(), flags.size() * 4) ? 0 : 4;
}

static int run_reduce(FILE* in, FILE* out, const int64_t* head) {
    const int B = (int)head[0], L = (int)head[2], Jstride = (int)head[3];
    const int64_t k = head[1];
    const float clamp = bits_float(head[4]);
    if (B < 0 || B > ENC_MAX_B || k < 1 || k > ENC_MAX_K || L < 1 || L > ENC_MAX_L || Jstride < L) return 2;
    const size_t n_all = (size_t)B * k;
    std::vector<float> pred(n_all), target(n_all), J(n_all * Jstride);
    std::vector<int32_t> flags(B);
    if (!read_exact(in, pred.data(), n_all * 4) || !read_exact(in, target.data(), n_all * 4) || !read_exact(in, J.data(), J.size() * 4) ||
        !read_exact(in, flags.data(), flags.size() * 4))
        return 3;
    const int64_t chunks = enc_chunks(k);
    const int NC = L + 2;
    std::vector<double> part((size_t)B * chunks * NC), loss(B), g_zn((size_t)B * L);
    for (int b = 0; b < B; ++b)
        for (int64_t ch = 0; ch < chunks; ++ch) {                                  // sdfr_encode_chunk_kernel, workgroup (ch, b)
            const int64_t row0 = ch * ENC_CHUNK;
            const int n = (int)((k - row0) < ENC_CHUNK ? (k - row0) : ENC_CHUNK);
            const size_t base = (size_t)b * k + row0;
            std::vector<double> s_e(n), s_acc((size_t)ENC_SLOTS * (ENC_COLS + 1));
            std::vector<float> s_w(n);
            std::vector<unsigned char> s_ok(n);
            for (int r = 0; r < n; ++r) {
                const EncRow q = enc_row(pred[base + r], target[base + r], clamp);
                s_e[r] = q.e; s_w[r] = q.w; s_ok[r] = (unsigned char)q.ok;
            }
            for (int c0 = 0; c0 < NC; c0 += ENC_COLS) {
                const int nc = (NC - c0) < ENC_COLS ? (NC - c0) : ENC_COLS;
                for (int e = 0; e < ENC_SLOTS * nc; ++e) {
                    const int j = e / nc, c = c0 + (e - j * nc);
                    double a = 0.0;
                    ENC_SLOT_ROWS(r, j, n) a += enc_value(c, L, s_w[r], s_e[r], s_ok[r], J.data() + (base + r) * Jstride);
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
    for (int b = 0; b < B; ++b) {                                                    // sdfr_encode_fold_kernel, workgroup b
        std::vector<double> tot(NC);
        for (int c = 0; c < NC; ++c) {
            double a = 0.0;
            for (int64_t ch = 0; ch < chunks; ++ch) a += part[((size_t)b * chunks + ch) * NC + c];
            tot[c] = a;
        }
        const double n_ok = tot[L + 1];
        for (int c = 0; c < L; ++c) g_zn[(size_t)b * L + c] = enc_mean(tot[c], n_ok);
        loss[b] = enc_mean(tot[L], n_ok);
        if (!(n_ok > 0.0)) flags[b] |= ENC_NO_ROWS;
    }
    return write_exact(out, loss.data(), loss.size() * 8) && write_exact(out, g_zn.data(), g_zn.size() * 8) &&
                   write_exact(out, part.data(), part.size() * 8) && write_exact(out, flags.data(), flags.size() * 4) ? 0 : 4;
}

static int run_step(FILE* in, FILE* out, const int64_t* head) {
    const int B = (int)head[0], L = (int)head[1], unit = (int)head[2], t = (int)head[3];
    const float code_reg = bits_float(head[4]), lr = bits_float(head[5]);
    if (B < 0 || B > ENC_MAX_B || L < 1 || L > ENC_MAX_L || t < 1) return 2;
    const size_t n = (size_t)B * L;
    std::vector<float> z(n), m(n), v(n);
    std::vector<double> g_zn(n);
    std::vector<int32_t> flags(B);
    if (!read_exact(in, z.data(), n * 4) || !read_exact(in, m.data(), n * 4) || !read_exact(in, v.data(), n * 4) || !read_exact(in, g_zn.data(), n * 8) ||
        !read_exact(in, flags.data(), flags.size() * 4))
        return 3;
    float bc1, bc2;
    enc_bias(t, &bc1, &bc2);
    for (int b = 0; b < B; ++b) {
        std::vector<float> s_g(L);
        float* zb = z.data() + (size_t)b * L;
        for (int i = 0; i < L; ++i) s_g[i] = (float)g_zn[(size_t)b * L + i];
        const int fl = flags[b];
        const float nrm = unit ? latent_norm(zb, L) : 1.f;
        const float dot = unit ? latent_unit_dot(zb, s_g.data(), L, nrm) : 0.f;
        const float nz = unit ? 0.f : enc_raw_norm(zb, L);
        int skip = (fl & (ENC_EMPTY | ENC_NO_ROWS | ENC_BAD_TABLE)) ? 1 : 0;
        for (int i = 0; i < L; ++i)
            if (!isfinite(enc_step_grad(zb[i], s_g[i], unit, nrm, dot, nz, code_reg))) skip = 1;
        if (skip) {
            flags[b] = fl | ENC_SKIPPED;
            continue;
        }
        for (int tid = 0; tid < L; ++tid) {
            const float gi = enc_step_grad(zb[tid], s_g[tid], unit, nrm, dot, nz, code_reg);
            latent_adam(&zb[tid], &m[(size_t)b * L + tid], &v[(size_t)b * L + tid], gi, lr, bc1, bc2);
        }
    }
    return write_exact(out, z.data(), n * 4) && write_exact(out, m.data(), n * 4) && write_exact(out, v.data(), n * 4) &&
                   write_exact(out, flags.data(), flags.size() * 4) ? 0 : 4;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    int64_t head[9];                                    // (reduce and step use eight words and leave the ninth 0)
    int rc = 3;
    if (read_exact(in, head, sizeof(head))) {
        if (std::strcmp(argv[1], "rows") == 0) rc = run_rows(in, out, head);
        else if (std::strcmp(argv[1], "reduce") == 0) rc = run_reduce(in, out, head);
        else if (std::strcmp(argv[1], "step") == 0) rc = run_step(in, out, head);
        else rc = 2;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? rc : 4;
}
