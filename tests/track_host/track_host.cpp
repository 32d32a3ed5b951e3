// Host harness of csrc/track_cells.h (tests/test_track_cpu.py): the workgroups and threads of trk_step_kernel (csrc/track.hip) as loops over
// the same functions.  Reads one binary file, writes one; all buffers have their exact sizes, so a sanitizer build sees any step outside
// them.  int64 head[10] first.
//   track_host step IN: head = T L unit t code_reg_bits lr_bits share_scale V has_weight | float lr_pose[5] | int64 voff[T + 1] |
//                        float weight[V] (with has_weight) | float z, m, v [T][L] | float scale, sm, sv [T] | float theta, tm, tv [V][5] |
//                        float pose[V][6] | float z_view[V][L] | double g[V][L + 5] | double view_loss[V] | int32 vflags[V] | double loss[T] |
//                        int32 tflags[T] | float history[T]
//                   OUT: float z, m, v [T][L] | float scale, sm, sv [T] | float theta, tm, tv [V][5] | float pose[V][6] | float z_view[V][L] |
//                        int32 vflags[V] | double loss[T] | int32 tflags[T] | float history[T]
#include "../fit_host.h"
#include "track_cells.h"

// trk_step_kernel, workgroup t
static void host_track(std::vector<float>& z, std::vector<float>& m, std::vector<float>& v, int L, int T, int unit, std::vector<float>& scale,
                       std::vector<float>& sm, std::vector<float>& sv, bool share, const std::vector<int64_t>& voff, int V, const std::vector<float>& weight,
                       bool has_weight, std::vector<float>& theta, std::vector<float>& tm, std::vector<float>& tv, std::vector<float>& pose,
                       std::vector<float>& z_view, const std::vector<double>& g, const std::vector<double>& view_loss, std::vector<int32_t>& vflags,
                       std::vector<double>& loss, std::vector<int32_t>& tflags, float code_reg, float lr, const std::vector<float>& rates, int step,
                       std::vector<float>& history) {
    float bc1, bc2;
    enc_bias(step, &bc1, &bc2);
    const int G = L + ALN_POSE;
    for (int t = 0; t < T; ++t) {
        const int64_t count = trk_count(voff.data(), t, V);
        if (count < 0) {
            tflags[t] = TRK_BAD_TABLE;
            continue;
        }
        const int n = (int)count;
        const int64_t v0 = voff[t];
        std::vector<unsigned char> s_ok(n);
        std::vector<float> s_w(n), s_g(L);
        for (int i = 0; i < n; ++i) {
            const size_t vi = (size_t)(v0 + i);
            const float w = has_weight ? weight.at(vi) : 1.f;
            const int32_t fl = vflags.at(vi);
            // exact-size copies of what the thread may read
            std::vector<double> gv(g.begin() + vi * G, g.begin() + (vi + 1) * G);
            std::vector<float> th(theta.begin() + vi * ALN_POSE, theta.begin() + (vi + 1) * ALN_POSE), am(tm.begin() + vi * ALN_POSE, tm.begin() + (vi + 1) * ALN_POSE),
                av(tv.begin() + vi * ALN_POSE, tv.begin() + (vi + 1) * ALN_POSE);
            const bool ok = trk_view_usable(fl, w, gv.data(), L, !share, th.data(), am.data(), av.data(), rates[4], bc1, bc2);
            s_ok[i] = ok ? 1 : 0;
            s_w[i] = w;
            if (!ok) vflags[vi] = fl | ENC_SKIPPED;
        }
        int used;
        const double W = trk_weight_sum(s_w.data(), s_ok.data(), n, &used);
        float s_gs = 0.f;
        double s_loss = 0.0;
        if (used)
            for (int c = 0; c < L + 2; ++c) {
                if (c < L) {
                    s_g[c] = (float)(trk_fold(g.data() + v0 * G + c, G, s_w.data(), s_ok.data(), n) / W);
                } else if (c == L) {
                    s_gs = share ? (float)(trk_fold(g.data() + v0 * G + L + 4, G, s_w.data(), s_ok.data(), n) / W) : 0.f;
                } else {
                    s_loss = trk_fold(view_loss.data() + v0, 1, s_w.data(), s_ok.data(), n) / W;
                }
            }
        float* zb = z.data() + (size_t)t * L;
        int skip = 1, fl = (n == 0 ? TRK_NO_VIEWS : 0) | TRK_NO_USABLE | TRK_SKIPPED;
        double ls = 0.0;
        float nrm = 1.f, dot = 0.f, nz = 0.f, sc = 0.f;
        if (used) {
            nrm = unit ? latent_norm(zb, L) : 1.f;
            dot = unit ? latent_unit_dot(zb, s_g.data(), L, nrm) : 0.f;
            nz = unit ? 0.f : enc_raw_norm(zb, L);
            skip = 0;
            for (int i = 0; i < L; ++i)
                if (!isfinite(enc_step_grad(zb[i], s_g[i], unit, nrm, dot, nz, code_reg))) skip = 1;
            float scm = 0.f, scv = 0.f;
            if (share) {
                trk_scale_step(scale.at(t), sm.at(t), sv.at(t), s_gs, rates[4], bc1, bc2, &sc, &scm, &scv);
                if (!(isfinite(sc) && sc > 0.f)) skip = 1;
                if (!skip && rates[4] != 0.f) scale[t] = sc, sm[t] = scm, sv[t] = scv;
            }
            fl = skip ? TRK_SKIPPED : 0;
            ls = s_loss;
        }
        tflags[t] = fl;
        loss[t] = ls;
        history[t] = (float)ls;
        if (skip) {
            for (int i = 0; i < n; ++i)
                if (s_ok[i]) vflags[(size_t)(v0 + i)] |= ENC_SKIPPED;
            continue;
        }
        for (int tid = 0; tid < L; ++tid) {
            if (lr != 0.f) {
                const float gi = enc_step_grad(zb[tid], s_g[tid], unit, nrm, dot, nz, code_reg);
                latent_adam(&zb[tid], &m[(size_t)t * L + tid], &v[(size_t)t * L + tid], gi, lr, bc1, bc2);
            }
            for (int i = 0; i < n; ++i) z_view.at((size_t)(v0 + i) * L + tid) = zb[tid];
        }
        for (int i = 0; i < n; ++i) {
            const size_t vi = (size_t)(v0 + i);
            std::vector<double> gv(g.begin() + vi * G, g.begin() + (vi + 1) * G);
            std::vector<float> th(theta.begin() + vi * ALN_POSE, theta.begin() + (vi + 1) * ALN_POSE), am(tm.begin() + vi * ALN_POSE, tm.begin() + (vi + 1) * ALN_POSE),
                av(tv.begin() + vi * ALN_POSE, tv.begin() + (vi + 1) * ALN_POSE), ps(pose.begin() + vi * VERIFY_POSE, pose.begin() + (vi + 1) * VERIFY_POSE);
            trk_view_step(s_ok[i] != 0, share, sc, th.data(), am.data(), av.data(), gv.data(), L, rates.data(), bc1, bc2, ps.data());
            std::copy(th.begin(), th.end(), theta.begin() + vi * ALN_POSE);
            std::copy(am.begin(), am.end(), tm.begin() + vi * ALN_POSE);
            std::copy(av.begin(), av.end(), tv.begin() + vi * ALN_POSE);
            std::copy(ps.begin(), ps.end(), pose.begin() + vi * VERIFY_POSE);
        }
    }
}

static int run(const char* mode, FILE* in, FILE* out, const int64_t* head) {
    if (std::strcmp(mode, "step") != 0) return 2;
    const int T = (int)head[0], L = (int)head[1], unit = (int)head[2], t = (int)head[3], V = (int)head[7];
    const bool share = head[6] != 0, has_weight = head[8] != 0;
    if (!host_sizes_ok(T, 1, L) || V < 0 || V > ENC_MAX_B || t < 1) return 2;
    std::vector<float> rates(ALN_POSE), weight(has_weight ? V : 0), z((size_t)T * L), m((size_t)T * L), v((size_t)T * L), scale(T), sm(T), sv(T),
        theta((size_t)V * ALN_POSE), tm((size_t)V * ALN_POSE), tv((size_t)V * ALN_POSE), pose((size_t)V * VERIFY_POSE), z_view((size_t)V * L), history(T);
    std::vector<int64_t> voff(T + 1);
    std::vector<double> g((size_t)V * (L + ALN_POSE)), view_loss(V), loss(T);
    std::vector<int32_t> vflags(V), tflags(T);
    if (!read_all(in, rates, voff, weight, z, m, v, scale, sm, sv, theta, tm, tv, pose, z_view, g, view_loss, vflags, loss, tflags, history)) return 3;
    host_track(z, m, v, L, T, unit, scale, sm, sv, share, voff, V, weight, has_weight, theta, tm, tv, pose, z_view, g, view_loss, vflags, loss, tflags,
               bits_float(head[4]), bits_float(head[5]), rates, t, history);
    return write_all(out, z, m, v, scale, sm, sv, theta, tm, tv, pose, z_view, vflags, loss, tflags, history) ? 0 : 4;
}

int main(int argc, char** argv) { return host_main(argc, argv, 10, run); }
