// Per-element rules of the joint fit of ONE shape to SEVERAL views (track.hip): which views of a track are usable on an iteration, the order
// in which their losses and gradients are folded into the track's, the step of the track's scale, and what a view of a stepped track
// receives.  A view is one cloud of one object with its own yaw and trans; a track is an ordered list of views with one latent and (with
// share_scale) one scale.  Plain functions, compiled for the device by track.hip and for the host by tests/track_host/track_host.cpp, which
// is compared with the numpy restatement (tests/_track_ref.py) bit for bit.  Every operation rounds on its own (-ffp-contract=off).
// DESIGN.md 7o has the rules.
#pragma once
#include <math.h>
#include <stdint.h>

#include "align_cells.h"

#define TRK_MAX_VIEWS 1024       // views of one track at the most: the workgroup keeps a byte and a weight per view in LDS
#define TRK_NO_VIEWS 1           // tflags, bit 0: the track has no views
#define TRK_NO_USABLE 2          //         bit 1: no view of the track is usable on this iteration; its loss is 0
#define TRK_SKIPPED 4            //         bit 2: the track was not stepped (ENC_SKIPPED, which its usable views then carry too)
#define TRK_BAD_TABLE 8          //         (the whole word) voff is broken at this track, or it has more than TRK_MAX_VIEWS views

// views of track t, or -1 when the table is broken there or the track is too long (V: views of the call)
ENC_HD int64_t trk_count(const int64_t* voff, int t, int64_t V) {
    const int64_t a = voff[t], e = voff[t + 1];
    return (a < 0 || e < a || e > V || e - a > TRK_MAX_VIEWS) ? -1 : e - a;
}

// A view takes part in its track's fold and is stepped: no flag that keeps sdfr_align_step from stepping a shape, a finite positive weight,
// float32 of each of its L + 5 gradient entries finite, and -- where the view owns its scale -- a scale its own update leaves finite and
// positive.  gv: the view's row of g; theta, tm, tv: the view's five words each; lr4: the scale's rate (read with own_scale alone).
ENC_HD bool trk_view_usable(int32_t vflag, float w, const double* gv, int L, bool own_scale, const float* theta, const float* tm, const float* tv,
                            float lr4, float bc1, float bc2) {
    if (vflag & (ENC_EMPTY | ENC_NO_ROWS | ENC_BAD_TABLE | ALN_BAD_POSE)) return false;
    if (!(isfinite(w) && w > 0.f)) return false;
    for (int c = 0; c < L + ALN_POSE; ++c)
        if (!isfinite((float)gv[c])) return false;
    if (own_scale) {
        const float sc = aln_scale_after(theta, tm, tv, gv, L, lr4, bc1, bc2);
        if (!(isfinite(sc) && sc > 0.f)) return false;
    }
    return true;
}

// THE FOLD ORDER.  sum of w_i x[i stride] over the usable views i < n of a track in ascending order, in float64, one product and one
// addition a view; the sum STARTS FROM ITS FIRST TERM, so a lone -0.0 survives.  0.0 without a usable view.
ENC_HD double trk_fold(const double* x, int64_t stride, const float* w, const unsigned char* ok, int n) {
    double a = 0.0;
    bool first = true;
    for (int i = 0; i < n; ++i) {
        if (!ok[i]) continue;
        const double term = (double)w[i] * x[(int64_t)i * stride];
        a = first ? term : a + term;
        first = false;
    }
    return a;
}

// W = sum of the usable views' weights in the same order, from its first term; *count receives the number of usable views
ENC_HD double trk_weight_sum(const float* w, const unsigned char* ok, int n, int* count) {
    double a = 0.0;
    int c = 0;
    for (int i = 0; i < n; ++i) {
        if (!ok[i]) continue;
        a = c ? a + (double)w[i] : (double)w[i];
        ++c;
    }
    *count = c;
    return a;
}

// the track's scale and its Adam state after one update with the gradient gs at the rate lr4 (nothing is stored; lr4 == 0: as they are)
ENC_HD void trk_scale_step(float scale, float sm, float sv, float gs, float lr4, float bc1, float bc2, float* s, float* m, float* v) {
    *s = scale, *m = sm, *v = sv;
    if (lr4 != 0.f) latent_adam(s, m, v, gs, lr4, bc1, bc2);
}

// What view v of a STEPPED track receives beside the track's latent.  A usable view: aln_pose_step on its own state with ITS OWN gradient
// row gv (not scaled by its weight: Adam divides a constant factor out again), rate 4 taken as 0 when the scale is shared.  With a shared
// scale every view, usable or not, then takes the track's scale into theta[4] and its pose row; an unusable view keeps everything else.
ENC_HD void trk_view_step(bool usable, bool share_scale, float scale, float* theta, float* tm, float* tv, const double* gv, int L, const float* lr_pose,
                          float bc1, float bc2, float* pose) {
    if (usable) {
        const float lr[ALN_POSE] = {lr_pose[0], lr_pose[1], lr_pose[2], lr_pose[3], share_scale ? 0.f : lr_pose[4]};
        aln_pose_step(theta, tm, tv, gv, L, lr, bc1, bc2, pose);
    }
    if (share_scale) {
        theta[4] = scale;
        pose[5] = scale;
    }
}
