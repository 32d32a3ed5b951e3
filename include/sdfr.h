/*
 * sdfr.h -- C ABI of libsdfr_hip.so: the MI355X (gfx950) differentiable SDF renderer hot path.
 *
 * The upstream reference (TRI-ML/sdflabel) exposes this path only as Python/PyTorch objects
 * (SURVEY.md 8b); there is no upstream FFI.  Each entry point below therefore names the reference
 * Python interface whose arithmetic it replaces (file:line relative to the reference root).  The
 * host-side mirror of those Python interfaces lives in sdflabel_amd/ and binds this library with
 * ctypes.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless the name starts with h_.
 *   - all floating-point data is float32, row-major, densely packed.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All work is enqueued on it;
 *     no entry point synchronises except sdfr_decoder_create/destroy.
 *   - ragged per-crop data uses the layout [B][cap][...] with a device-side count per crop (`cnt`, int32[B]).
 *     cnt == NULL means "every crop holds exactly cap items".
 *   - return value: 0 on success, negative SDFR_E_* on error; sdfr_last_error() gives a message.
 */
#ifndef SDFR_H
#define SDFR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDFR_OK 0
#define SDFR_E_INVALID (-1)   /* bad argument (shape, NULL pointer, unsupported architecture spec) */
#define SDFR_E_HIP (-2)       /* a HIP runtime call failed */
#define SDFR_E_UNSUPPORTED (-3)

#define SDFR_MAX_LAYERS 16
#define SDFR_TRACE_LEVELS 6     /* most speculation levels of a sphere-tracing march schedule (sdfr_trace_march) */
#define SDFR_TRACE_COUNTERS 32  /* int32 device counters of a march / a cone march (zeroed by sdfr_trace_setup / sdfr_trace_cone) */

#define SDFR_VERSION 424       /* what sdfr_version() of the library this header belongs to returns; a binding compares the two */

/* ABI version: bumped whenever an exported signature or a buffer size changes (300: the r04 argument lists of sdfr_trace_march /
 * sdfr_trace_cone and the 32-word SDFR_TRACE_COUNTERS; 400: the r06 fused entry points below -- sdfr_params_plan, sdfr_band_select_ex,
 * sdfr_mlp_forward_candidates, sdfr_candidate_band, sdfr_losses_fused, sdfr_splat_backward_x, sdfr_pose_latent_solver; 401: the RANSAC pose initialisation sdfr_ransac_*; 402: the evaluator's box overlaps sdfr_rotate_iou, sdfr_box3d_iou,
 * sdfr_image_box_iou; 403: the evaluator's statistics sdfr_eval_*; 404: frame labelling, sdfr_reproject and
 * sdfr_point_extents; 405: frame ingest, sdfr_depth_map, sdfr_match_boxes and sdfr_css_input; 406: the CSS output head, sdfr_css_head and
 * sdfr_css_latent; 407: its training losses and gradients, sdfr_css_head_loss and sdfr_css_latent_loss; 408: the road-plane removal, sdfr_lidar_normals_ws_bytes,
 * sdfr_lidar_normals and sdfr_depth_map_masked; 409: the training-crop augmentation, sdfr_augment; 410: the grid forward with the caller's tile order,
 * sdfr_grid_tile_order and sdfr_mlp_forward_ordered; 411: triangle meshes, sdfr_mesh_*; 412: verification of
 * refined labels, sdfr_mesh_raster and sdfr_verify_*; 413: the export of training crops, sdfr_crop_*; 414: synthetic
 * bootstrap crops, sdfr_synth_*; 415: signed distances to meshes and surface samples, sdfr_mesh_sdf* and sdfr_mesh_surface_*; 416: the
 * grid forward's launch order from the last pass, sdfr_mlp_balance_* and sdfr_mlp_forward_balanced, and the per-workgroup tile trace of trace
 * builds, sdfr_debug_set_tile_trace; 417: training the decoder, sdfr_decoder_train_*; 418: encoding shapes under a
 * frozen decoder, sdfr_encode_*; 419: shape completion from one view, sdfr_view_samples and
 * sdfr_bound_*; 420: pose and shape fitted to one view, sdfr_align_*;
 * 421: lidar clusters and rough boxes, sdfr_cluster_* and sdfr_lidar_clusters; 422: band selection and tile ranking in one launch,
 * sdfr_mlp_forward_balanced_deferred and sdfr_band_select_rank;
 * 423: one shape fitted to several views, sdfr_track_step; 424: choosing a fit's start, sdfr_search_*).  A caller built
 * against another header must refuse the library. */
int sdfr_version(void);
/* 0 for the product library.  Bit 0: built with SDFR_EXPERIMENT (kernel geometry / option A/B build of tools/ab_variant.sh);
 * bit 1: a timing-only ablation is compiled in and results are wrong by construction.  Bindings refuse a non-zero value. */
int sdfr_build_flags(void);
const char* sdfr_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * DeepSDF decoder  --  replaces Decoder.forward (sdfrenderer/deepsdf/networks/deep_sdf_decoder_scale.py:78-107)
 * and the autograd backward of it w.r.t. its input (the normals hook of sdfrenderer/grid.py:11-12,55-56 and
 * the latent gradient of pipelines/optimizer.py:156).
 *
 * The decoder is described by its EFFECTIVE linear layers (weight-norm g*v/||v|| already folded, as
 * nn.utils.weight_norm recomputes on every call, deep_sdf_decoder_scale.py:51-52):
 *   n_lin         number of nn.Linear layers (9 for the 8x512 DeepSDF decoder); the last one must have out_dim 1
 *   in_dim[l]     input width of layer l INCLUDING any re-injected input columns
 *   out_dim[l]    output width of layer l
 *   inj_n[l]      number of input columns concatenated to the activations BEFORE layer l
 *                 (L+3 when l is in latent_in, :90-91; 3 when xyz_in_all, :92-93; else 0); inj_n[0] must be 0
 *   inj_off[l]    first input column that is concatenated (0 for latent_in, L for xyz_in_all)
 *   h_W[l]        HOST pointer, float32 [out_dim[l]][in_dim[l]] row-major (torch nn.Linear.weight layout)
 *   h_b[l]        HOST pointer, float32 [out_dim[l]]
 *   n_inputs      width of an input row (L+3)
 *   use_tanh      apply tanh to the last linear before the final tanh (:96-97); the final tanh (:106-107) is always applied
 *   h_ln_w[l], h_ln_b[l]   HOST pointers to the nn.LayerNorm weight / bias [out_dim[l]] applied between layer l's linear and its ReLU
 *                 (the weight_norm=False decoder variant, :56-57,:99-101), or NULL; the arrays themselves may be NULL.  LayerNorm decoders
 *                 run in float32 without mask saving (their Jacobian recomputes the forward).
 * Hidden widths up to 512 are supported.
 */
typedef struct sdfr_decoder sdfr_decoder;

int sdfr_decoder_create(sdfr_decoder** out, int n_lin, const int* in_dim, const int* out_dim,
                        const int* inj_n, const int* inj_off, const float* const* h_W, const float* const* h_b,
                        const float* const* h_ln_w, const float* const* h_ln_b, int n_inputs, int use_tanh, int device);
int sdfr_decoder_destroy(sdfr_decoder* dec);
/* algorithmic multiply-accumulates per evaluated point (sum of in_dim*out_dim) */
int64_t sdfr_decoder_macs(const sdfr_decoder* dec);

/* sdf[i] = Decoder(inputs[i,:]) for i < n.   inputs [n][n_inputs], sdf [n].
 * Reference: pred_sdf_grid, _ = dsdf(inputs)  (pipelines/optimizer.py:99-101). */
int sdfr_mlp_forward(const sdfr_decoder* dec, const float* inputs, int64_t n, float* sdf,
                     uint32_t* mask_ws /* optional: sdfr_decoder_mask_words(dec, n) uint32 words; receives the ReLU masks
                                          (1 bit per hidden feature, point and layer) for a later sdfr_mlp_jacobian */,
                     void* stream);
/* Tile order of the exact-f32 grid forward for a D^3 grid (row = x D D + y D + z), computed on the host: out[D^3] receives the rows block by
 * block -- 4x4x4 blocks in lexicographic (bx, by, bz) order, a block's rows in (x, y, z) order, blocks at the border clipped.  A permutation
 * of 0 .. D^3 - 1; for D divisible by 4 every run of 64 entries is one block.  1 <= D <= 1024. */
int sdfr_grid_tile_order(int D, int32_t* out);
/* sdfr_mlp_forward with the rows that share a tile chosen by the caller: slot j of the launch evaluates row
 * (j / order_rows) * order_rows + order[j % order_rows] and stores value and masks AT THAT ROW, so sdf and mask_ws receive what
 * sdfr_mlp_forward writes, bit for bit.  What changes is what the per-tile K compaction can leave out (spatially compact tiles keep fewer
 * hidden features alive).  order: DEVICE int32 [order_rows], a permutation of 0 .. order_rows - 1 (an entry outside that range makes its
 * slot evaluate nothing: the row it should have named is left unwritten); n must be a multiple of order_rows (n / order_rows crops of
 * order_rows rows each; order_rows need not be a multiple of the tile).  Float32 decoders of padded width 512 without LayerNorm. */
int sdfr_mlp_forward_ordered(const sdfr_decoder* dec, const float* inputs, int64_t n, float* sdf, uint32_t* mask_ws, const int32_t* order,
                             int64_t order_rows, void* stream);
/* sdfr_mlp_forward_ordered with the launch order of the 64-entry chunks of `order` taken from the last pass (SDFR_VERSION 416).  Since the
 * K compaction a tile's time follows the K extent its products walk, and the one-crop launch is under four tiles per CU: launched in
 * the static order the heavy late tiles make a tail.  Every tile of a balanced launch adds that K extent (an integer) to its chunk's word of
 * `state`, and a small kernel behind the launch ranks the full chunks by (cost descending, static index ascending) and writes the
 * order of the NEXT call; a partial last chunk keeps the last place.  sdf and mask_ws receive what sdfr_mlp_forward writes, bit for bit,
 * whatever the state holds: chunks stay whole, and the next order is always written from the state's own copy of the static order.
 *   state   DEVICE memory of sdfr_mlp_balance_bytes(order_rows) bytes, 4-byte aligned, int32 words, T = (order_rows + 63) / 64:
 *           [0, T) costs added since the last ranking; [T, 2 T) the costs the last ranking read; [2 T, 3 T) the chunk of the static order at each
 *           place of the next launch; 4 control words; order_rows words, the order the next call launches with; order_rows words, the
 *           static order.  One state per order and stream of calls.
 *   sdfr_mlp_balance_init   order: DEVICE int32 [order_rows]; writes it to both order fields and zeroes the costs (one kernel); the state
 *           must be memory of the current device (checked).
 *   sdfr_mlp_forward_balanced   arguments and checks of sdfr_mlp_forward_ordered.  Two launches, no host read, no synchronisation, no
 *           pointer that changes from call to call: a captured graph replays it.  Orders of more than 4096 chunks (tens of rounds of tiles:
 *           no tail) are launched in the static order and not ranked. */
int64_t sdfr_mlp_balance_bytes(int64_t order_rows);
int sdfr_mlp_balance_init(void* state, const int32_t* order, int64_t order_rows, void* stream);
int sdfr_mlp_forward_balanced(const sdfr_decoder* dec, const float* inputs, int64_t n, float* sdf, uint32_t* mask_ws, void* state,
                              int64_t order_rows, void* stream);
/* sdfr_mlp_forward_balanced without its ranking launch (SDFR_VERSION 422): same arguments, same checks, the tiles still add their costs to
 * `state`; the ranking is left to the sdfr_band_select_rank that follows.  One launch.  A forward that runs twice without a ranking between
 * adds the costs of both passes: the next order is then ranked by the sums and is still a permutation (every entry of it is written from the
 * state's static order). */
int sdfr_mlp_forward_balanced_deferred(const sdfr_decoder* dec, const float* inputs, int64_t n, float* sdf, uint32_t* mask_ws, void* state,
                                       int64_t order_rows, void* stream);
/* sdfr_mlp_forward with float16 operands on the matrix cores (weights and hidden activations rounded to half, float32 accumulation, bias,
 * ReLU and tanh) -- the decoder precision of the reference's default config (configs/config_refine.ini:19); inputs/outputs stay float32. */
int sdfr_mlp_forward_f16(const sdfr_decoder* dec, const float* inputs, int64_t n, float* sdf, uint32_t* mask_ws, void* stream);

/* sdfr_mlp_forward_f16 over the first *n_dev rows only (n_dev: device int32, clamped to n_max; no host read) -- the sphere tracer's hit pass
 * in the decoder's own half precision; mask_ws sized for n_max rows. */
int sdfr_mlp_forward_f16_counted(const sdfr_decoder* dec, const float* inputs, int64_t n_max, const int32_t* n_dev, float* sdf, uint32_t* mask_ws,
                                 void* stream);

/* the same with error-compensated float16 operands: each float32 weight and hidden activation x is carried as hi = half(x),
 * lo = half((x - hi) * 2^11) and every product as hi*hi + 2^-11 (hi*lo + lo*hi) on the f16 matrix cores, float32 accumulation
 * (~22 significand bits per product; the output differs from sdfr_mlp_forward by float32 summation-order noise, not by half
 * rounding).  Same replaced interface as sdfr_mlp_forward (deep_sdf_decoder_scale.py:78-107); mask_ws has the layout
 * sdfr_mlp_forward writes (pass mask_from_f16 = 0 to sdfr_mlp_jacobian).  Requires |hidden activation| < 65504. */
int sdfr_mlp_forward_split(const sdfr_decoder* dec, const float* inputs, int64_t n, float* sdf, uint32_t* mask_ws, void* stream);
/* ... over the first *n_dev rows (device int32, clamped to n_max; rows beyond are not touched): the audit rows of the two-stage evaluation */
int sdfr_mlp_forward_split_counted(const sdfr_decoder* dec, const float* inputs, int64_t n_max, const int32_t* n_dev, float* sdf, void* stream);
/* size (in uint32 words) of the mask workspace for n rows */
int64_t sdfr_decoder_mask_words(const sdfr_decoder* dec, int64_t n);

/* Input Jacobian of the decoder at selected rows:
 *   for crop b < B, slot s < cnt[b]:  r = row_base + b*rows_per_crop + idx[b*cap+s]
 *     J[b][s][:]      = d sdf(inputs[r,:]) / d inputs[r,:]      (n_inputs values)
 *     sdf_sel[b][s]   = sdf(inputs[r,:])                         (may be NULL)
 * Rows s < cnt[b] are fully written by the call (no prior initialisation needed); rows s >= cnt[b] are left untouched.
 * Reference: the xyz columns are what grid.py:55-56 captures through its hook for the band points; the latent
 * columns give d sdf/d latent, which autograd recomputes at optimizer.py:156. */
int sdfr_mlp_jacobian(const sdfr_decoder* dec, const float* inputs, int64_t rows_per_crop, int B,
                      const int32_t* idx, int cap, const int32_t* cnt, float* J, float* sdf_sel,
                      const float* sdf_full /* optional: output of the sdfr_mlp_forward call over the same rows */,
                      const uint32_t* mask_ws /* optional: masks that call saved; with both, no forward recomputation */,
                      int mask_from_f16 /* 0: mask_ws from sdfr_mlp_forward(_split); 1: from sdfr_mlp_forward_f16, float32 backward;
                                            2: from sdfr_mlp_forward_f16 and the backward also runs with half operands;
                                            | SDFR_JAC_MANY_ROWS: hint for the recomputing kernel (no masks) that the launch holds many
                                            thousands of rows (32-row tiles; results equal to float rounding, not bit for bit) */,
                      void* stream);

/* ------------------------------------------------------------------------------------------------
 * Zero-isosurface projection  --  replaces Grid3D.get_surface_points (sdfrenderer/grid.py:43-71)
 */

/* Order-preserving selection of the band |sdf| < thr (grid.py:64-66), per crop:
 *   idx[b][0..cnt[b])  = ascending local row indices g in [0,G) with |sdf[b*G+g]| < thr
 *   slot[b*G+g]        = position of g in idx[b] or -1          (may be NULL)
 * If a crop holds more than cap band points the surplus is dropped and cnt[b] is set to the TRUE count
 * (callers compare against cap).  scratch: int32[B * ceil(G/256)]. */
int sdfr_band_select(const float* sdf, int64_t G, int B, float thr, int32_t* idx, int cap, int32_t* cnt,
                     int32_t* slot, int32_t* scratch, void* stream);

/* points[b][s] = x - sdf * n_hat, n_hat = J_xyz/||J_xyz||, nocs = (points+1)/2   (grid.py:57-67)
 *   inputs [B*G][n_inputs] (xyz = last 3 columns), J [B][cap][n_inputs] from sdfr_mlp_jacobian, or
 *   (when Jstride == 3) raw normals d sum(sdf)/d xyz gathered by the caller.
 *   outputs points, nocs, normals: [B][cap][3]. */
int sdfr_surface_project(const float* xyz, int xyz_stride, const float* sdf, int64_t G, int B,
                         const int32_t* idx, int cap, const int32_t* cnt, const float* J, int Jstride, int Joff,
                         float* points, float* nocs, float* normals, void* stream);

/* Backward of the projection (n_hat is a constant, grid.py:56-58):
 *   g_sdf[b*G + idx] = -(g_points + g_nocs/2) . n_hat ; g_xyz[b*G+idx][:] = g_points + g_nocs/2   (others 0; buffers are
 *   fully overwritten).  g_nocs, g_xyz may be NULL. */
int sdfr_surface_project_bwd(const float* g_points, const float* g_nocs, const float* normals, int64_t G, int B,
                             const int32_t* idx, int cap, const int32_t* cnt, float* g_sdf, float* g_xyz, void* stream);

/* Two-stage band selection (optional): a half-operand decoder pass over the grid + sdfr_band_select with a safety margin gives
 * candidate rows; sdfr_mlp_jacobian without masks evaluates them exactly (float32 sdf + Jacobian).  sdfr_scatter_values writes the exact
 * values back, dst[b*G + idx[b][s]] = src[b][s] for s < cnt[b], so that the ordinary sdfr_band_select on dst yields the exact band of
 * grid.py:64; sdfr_gather_rows re-orders rows of ncol floats, out[b][e] = src[b][slot[b*G + idx[b][e]]] for e < cnt[b] (slot = the
 * grid-row -> candidate-slot map sdfr_band_select wrote; src has src_cap rows per crop). */
int sdfr_scatter_values(float* dst, const float* src, const int32_t* idx, int64_t G, int B, int cap, const int32_t* cnt, void* stream);
/* sdfr_band_select with a per-crop addition to the threshold (thr + thr_extra[b]): the candidate selection with a device-resident margin. */
int sdfr_band_select_margin(const float* sdf, int64_t G, int B, float thr, const float* thr_extra, int32_t* idx, int cap, int32_t* cnt,
                            int32_t* slot, int32_t* scratch, void* stream);
/* sdfr_scatter_values plus the run-time guard of the two-stage evaluation: max_dev[b] = max over the crop's candidates of
 * |sdf_grid (half pass) - sdf_exact|, measured while the exact values are patched in.  max_dev > margin[b]/2: violations[2b] += 1 and
 * margin[b] = max(margin[b], 4 max_dev) for the following selections; max_dev >= margin[b]: violations[2b+1] += 1 as well (a band row may
 * have been excluded in this step).  margin float[B] in/out, violations int32[B][2] in/out; no host synchronisation. */
int sdfr_prefilter_guard(float* sdf_grid, const float* sdf_exact, const int32_t* idx, int64_t G, int B, int cap, const int32_t* cnt,
                         float* margin, float* max_dev, int32_t* violations, void* stream);
/* Candidate-set reuse of the two-stage evaluation.  sdfr_prefilter_plan decides per crop, on the device, whether the candidates of the last
 * half pass still cover the band: reuse[b] = 1 while lip * |latent - latent of that pass| <= margin[b]/4, max_dev[b] <= margin[b]/2 and at
 * most max_reuse steps in a row (lip: Lipschitz constant of the decoder in the normalised latent; inputs: the decoder input rows, whose
 * first L columns hold it; lat_ref float[B][L], age int32[B]: state, zero-initialised).  The half pass, the candidate selection and the
 * guard then take the flags: flagged crops are skipped (sdfr_mlp_forward_f16_skip, sdfr_band_select_skip) / patched but not judged
 * (sdfr_prefilter_guard2).  n_full int32[B] (may be NULL; r05): += 1 for every crop that is NOT flagged, i.e. runs its full-grid pass. */
int sdfr_prefilter_plan(const float* inputs, int64_t G, int n_inputs, int L, int B, float lip, const float* margin, const float* max_dev,
                        float* lat_ref, int32_t* age, int max_reuse, int32_t* reuse, int32_t* n_full, void* stream);
int sdfr_mlp_forward_f16_skip(const sdfr_decoder* dec, const float* inputs, int64_t n, float* sdf, const int32_t* skip, int64_t rows_per_crop,
                              void* stream);
int sdfr_band_select_skip(const float* sdf, int64_t G, int B, float thr, const float* thr_extra, const int32_t* skip, int32_t* idx, int cap,
                          int32_t* cnt, int32_t* slot, int32_t* scratch, void* stream);
int sdfr_prefilter_guard2(float* sdf_grid, const float* sdf_exact, const int32_t* idx, int64_t G, int B, int cap, const int32_t* cnt,
                          float* margin, float* max_dev, int32_t* violations, const int32_t* reused, void* stream);
int sdfr_gather_rows(float* out, const float* src, int ncol, const int32_t* idx, const int32_t* slot, int64_t G, int B, int cap,
                     int src_cap, const int32_t* cnt, void* stream);
/* Audit of the two-stage evaluation (r04): the guard above observes the half pass only at the candidates; a row outside them that the half
 * pass misplaced by more than the margin is invisible to it.  Every step the NON-candidate rows of one slice of the grid -- the contiguous
 * rows [ph * ceil(G / stride), (ph + 1) * ceil(G / stride)), ph = *phase mod stride: every row once per `stride` steps -- are listed by
 * sdfr_prefilter_audit_select (rows
 * float[cap_rows][n_inputs] = their decoder input rows, src int32[cap_rows] = b * G + g, *n_audit = how many; cslot: the grid-row ->
 * candidate-slot map of the candidate selection), evaluated exactly by the caller (sdfr_mlp_forward_counted(dec, rows, cap_rows, n_audit,
 * sdf_exact, 0)) and judged by sdfr_prefilter_audit_check: |exact| < thr on such a row = a band row was excluded in this step ->
 * violations[2b+1] += 1 (a hard violation, like the guard's); audit_dev[b] = the largest |half - exact| seen on crops that ran the half pass
 * (reused[b] == 0; reused may be NULL); then *phase += 1.  phase, n_audit: device int32; no host synchronisation. */
int sdfr_prefilter_audit_select(const float* inputs, const int32_t* cslot, int64_t G, int n_inputs, int B, int stride, const int32_t* phase,
                                float* rows, int32_t* src, int32_t* n_audit, int cap_rows, void* stream);
int sdfr_prefilter_audit_check(const float* sdf_grid, const float* sdf_exact, const int32_t* src, const int32_t* n_audit, int cap_rows,
                               int64_t G, int B, float thr, const int32_t* reused, float* audit_dev, int32_t* violations, int32_t* phase,
                               void* stream);

/* Candidate reuse of the float16 decoder mode (r05; the reference's shipped precision, configs/config_refine.ini:19, re-evaluates all G grid
 * rows every iteration of pipelines/optimizer.py:96-104 although the latent moves by ~1e-6 per iteration).  The band is taken from the
 * candidate rows (|half sdf| < thr + margin at the crop's last full-grid pass) alone:
 *   sdfr_candidate_rows      rows[b][s][:] = inputs[b*G + cidx[b][s]][:] for s < ccnt[b] (ragged [B][stride] array, stride a multiple of 128;
 *                            the rows up to the next multiple of 128 are filled with a finite row)
 *   sdfr_mlp_forward_f16_ragged   the half decoder on crop b's first cnt[b] rows of such an array (whole 128-row tiles), masks saved: every
 *                            row gets the bits sdfr_mlp_forward_f16 gives it in a full-grid launch
 *   sdfr_scatter_values      writes them into the grid array; sdfr_band_select there returns the band (rows outside the candidates keep
 *                            their values of the last full pass, >= thr + margin in magnitude)
 *   sdfr_candidate_band_map  pos[b][e] = cslot[b*G + idx[b][e]]: the band rows' positions in the candidate array, for the mask-fed half
 *                            Jacobian (sdfr_mlp_jacobian(dec, rows, stride, B, pos, ...)); a band row that is no candidate counts a hard
 *                            violation (violations[2b+1], may be NULL)
 * sdfr_prefilter_plan (with a proven Lipschitz bound as `lip`) decides per crop when a full pass is due; the audit re-evaluates a rotating
 * slice of the other rows with the same kernel. */
int sdfr_candidate_rows(const float* inputs, int64_t G, int n_inputs, int B, const int32_t* cidx, int stride, const int32_t* ccnt, float* rows,
                        void* stream);
int sdfr_mlp_forward_f16_ragged(const sdfr_decoder* dec, const float* inputs, int B, int64_t rows_per_crop, const int32_t* cnt, float* sdf,
                                uint32_t* mask_ws, int half_tiles, void* stream);
int sdfr_candidate_band_map(const int32_t* idx, int cap, const int32_t* cnt, const int32_t* cslot, int64_t G, int B, int stride, int32_t* pos,
                            int32_t* violations, void* stream);
/* The same scheme with the EXACT float32 decoder (the parity path): sdfr_mlp_forward with per-crop skip flags (full-grid pass of the crops
 * whose candidate set is due; no masks) and over a ragged [B][rows_per_crop] array (rows_per_crop a multiple of 64; masks saved for the
 * float32 mask-fed Jacobian).  Every row gets the bits sdfr_mlp_forward gives it in a full-grid launch. */
int sdfr_mlp_forward_skip(const sdfr_decoder* dec, const float* inputs, int64_t n, float* sdf, const int32_t* skip, int64_t rows_per_crop,
                          void* stream);
int sdfr_mlp_forward_ragged(const sdfr_decoder* dec, const float* inputs, int B, int64_t rows_per_crop, const int32_t* cnt, float* sdf,
                            uint32_t* mask_ws, int half_tiles, void* stream);
/* half_tiles = 1 (float16 only; sdfr_mlp_forward_ragged returns SDFR_E_UNSUPPORTED): 64-row tiles instead of 128 -- the candidates of one or
 * two crops are a few dozen full-size tiles on 256 CUs, and a tile pass is pure latency; the same bits per row.  The mask-fed Jacobian then
 * needs SDFR_JAC_HALF_TILES in its mask_from_f16 argument. */

/* g_inputs[r][:] = g_sdf[r] * J[slot[r]][:]  for rows with slot[r] >= 0, else 0   (DeepSDF backward through the
 * cached band Jacobian).  n_uncached (device int32, may be NULL) receives the number of rows with g_sdf != 0 and
 * slot < 0, i.e. rows the cache does not cover. */
int sdfr_sdf_input_grad(const float* g_sdf, const int32_t* slot, const float* J, int n_inputs, int64_t G, int B, int cap,
                        float* g_inputs, int32_t* n_uncached, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Projection to the camera frame  --  replaces project_in_2D (sdfrenderer/renderer/projection.py:7-101), rot='dcm'
 *   pose [B][16] row-major 4x4 (only the top 3 rows are used, :34); K [B][9]
 *   in : points, normals, colors [B][cap][3]  (colors ignored when output_nocs != 0: 1 -> c = p*(-1,1,1), :53-55; 2 -> c = p, :147-149;
 *        5 / 6 = 1 / 2 with the compositing map (c+1)/2 of rasterer.py:113-114 already applied, so that col feeds sdfr_splat_* directly)
 *   out: p_cam, n_cam, col [B][cap][3]; uv [B][cap][2] (clamped, :88-93; may be NULL)
 *        front-facing filter n_cam.p_cam < 0 (:61-70): fidx [B][cap] ascending slots, fcnt [B]  (fidx/fcnt may be NULL);
 *        optional with fidx: xyzf [B][cap][3] = p_cam rows of the front-facing surfels in fidx order (points['xyzf'], rasterer.py:151)
 *        and fslot [B][cap] = position of each surfel in fidx or -1 (what the backward needs to route g_xyzf).
 */
int sdfr_project_dcm(const float* pose, const float* K, const float* points, const float* normals, const float* colors,
                     int B, int cap, const int32_t* cnt, int output_nocs, int res_x, int res_y,
                     float* p_cam, float* n_cam, float* col, float* uv, int32_t* fidx, int32_t* fcnt, float* xyzf, int32_t* fslot,
                     void* stream);

/* Batched path, one launch: sdfr_surface_project (band rows -> points, unit normals; grid.py:57-67) + sdfr_project_dcm in a NOCS colour
 * mode (projection.py:34-70) + the conservative disc screen boxes and their 8x8-pixel tile lists that sdfr_splat_forward would otherwise
 * build (bbox = its workspace; pass primitive | SDFR_PRIM_BOXES_READY to it; bbox may be NULL).  output_nocs | 8: bbox is the large
 * workspace of sdfr_splat_ws_words(B, cap, res_x, res_y) words and the tile lists are built too (then also pass SDFR_PRIM_BINS to
 * sdfr_splat_forward; building the lists costs one workgroup per crop ~13 us, which pays from about four crops per launch); without it
 * bbox is int32[B][cap][4].  Same arithmetic and outputs as the separate calls. */
int sdfr_surfels_forward(const float* xyz, int xyz_stride, const float* sdf, int64_t G, const int32_t* idx, const float* J, int Jstride,
                         int Joff, const float* pose, const float* K, int B, int cap, const int32_t* cnt, int output_nocs, int res_x,
                         int res_y, float diam, float* points, float* normals, float* p_cam, float* n_cam, float* col, int32_t* fidx,
                         int32_t* fcnt, float* xyzf, int32_t* fslot, int32_t* bbox, void* stream);

/* Backward: g_points, g_normals, g_colors [B][cap][3] (g_colors NULL when output_nocs), g_pose [B][16].  g_xyzf [B][cap][3] (may be
 * NULL): gradient w.r.t. the xyzf rows, added to g_p_cam through fslot. */
int sdfr_project_dcm_bwd(const float* pose, const float* points, const float* normals,
                         const float* g_p_cam, const float* g_n_cam, const float* g_col,
                         int B, int cap, const int32_t* cnt, int output_nocs,
                         float* g_points, float* g_normals, float* g_colors, float* g_pose, const float* g_xyzf, const int32_t* fslot,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * Surfel splat + depth-softmax composite  --  replaces the primitives of sdfrenderer/renderer/primitives.py and the compositing of
 * Rasterer.forward (sdfrenderer/renderer/rasterer.py:92-144) without ever forming the N x P tensors.
 *   primitive 0 'disc'        inside_surfel(diam=0.04, softclamp=False, depth_constant=150)   primitives.py:165-242  (the optimizer's)
 *   primitive 1 'circle'      inside_circle(diam=0.02, softclamp=True, depth_constant=100)     primitives.py:4-71
 *   primitive 2 'circle_opt'  inside_circle_opt(diam=0.025, depth_constant=10000)              primitives.py:74-162
 *   Kinv [B][9] = inverse(K.float()) (primitives.py:204), K [B][9]
 *   p_cam, n_cam, attr [B][cap][3]   attr is the composited colour attribute AFTER the (c+1)/2 mapping
 *   uv [B][cap][2], znorm [B]        primitives 1,2 only: clamped pixel projections (sdfr_project_dcm) and ||depths||_2 per crop
 *   bg [B][3][H][W], bg_logit [B]    optional background row (add_bg): its colour and its logit (min over the surfels' logits - 1,
 *                                    primitives.py:65,147,235); both NULL for bg=None
 *   images: color [B][3][H][W], mask [B][H][W], depth [B][H][W], normals [B][3][H][W] (any may be NULL)
 *   aux [B][H*W][4]: per-pixel state for the backward (nu, max logit, softmax denominator, clamp gates)
 */
#define SDFR_JAC_MANY_ROWS 16
/* Since SDFR_VERSION 400 the mask workspace has ONE layout whatever launch saved it (64 bytes per row and layer, rows in blocks of 128:
 * csrc/mlp_kernel.h sdfr_mask_dword), so the two flags below no longer select anything; they are accepted and ignored. */
#define SDFR_JAC_HALF_TILES 32  /* (until version 300) the masks were saved by a forward on half-size tiles (sdfr_mlp_forward_ragged / _f16_ragged with half_tiles = 1) */
#define SDFR_JAC_QUARTER_TILES 64  /* (until version 300) ... on quarter-size tiles (sdfr_mlp_forward_candidates with half_tiles = 2: 32-row tiles, float16) */
#define SDFR_PRIM_BOXES_READY 256   /* OR into `primitive` of sdfr_splat_forward: bbox_ws already holds the surfels' screen boxes and tile lists */
#define SDFR_PRIM_BINS 512          /* OR into `primitive`: bbox_ws is the LARGE workspace of sdfr_splat_ws_words() and per-tile surfel lists are
                                       built in it and used; without the flag bbox_ws only needs int32[B][cap][4] (boxes) and every 8x8 tile
                                       scans all boxes -- same bits either way */
/* words of the large splat workspace: the conservative screen boxes int32[B][cap][4] followed, per crop, by the 8x8-pixel tile lists built
 * from them (count -> scan -> fill): tile_off[T+2] | tile_list[32*cap], T = ceil(W/8)*ceil(H/8) */
int64_t sdfr_splat_ws_words(int B, int cap, int W, int H);
int sdfr_splat_forward(int primitive, const float* K, const float* Kinv, const float* p_cam, const float* n_cam, const float* attr,
                       const float* uv, const float* znorm, const float* bg, const float* bg_logit,
                       int B, int cap, const int32_t* cnt, int W, int H, float diam, float depth_constant,
                       int32_t* bbox_ws /* workspace: int32[B][cap][4], or sdfr_splat_ws_words(B, cap, W, H) words with SDFR_PRIM_BINS */,
                       float* color, float* mask, float* depth, float* normals, float* aux, void* stream);

/* Backward w.r.t. p_cam, n_cam, attr given the gradients of the four images (any may be NULL; a non-NULL gradient
 * needs the corresponding forward image, which carries the softmax-backward sum <grad, output>).  The background logit is a
 * constant here. */
int sdfr_splat_backward(int primitive, const float* K, const float* Kinv, const float* p_cam, const float* n_cam, const float* attr,
                        const float* uv, const float* znorm, const float* bg, const float* bg_logit,
                        int B, int cap, const int32_t* cnt, int W, int H, float diam, float depth_constant,
                        const float* aux, const float* color, const float* mask, const float* depth, const float* normals,
                        const float* g_color, const float* g_mask, const float* g_depth, const float* g_normals,
                        float* g_p_cam, float* g_n_cam, float* g_attr, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ragged extents (r04): every crop of a batch its OWN image size and intrinsics, as the crops of the reference pipeline have
 * (utils/refinement.py:586-609 adjust_intrinsics_crop: area-normalised, aspect kept; pipelines/refine_css.py:117-129,203-223 builds a
 * Rasterer per crop).  The `_r` entry points take the extents as DATA -- wh int32[B][2] = (W_b, H_b) on the device, next to the per-crop
 * K / Kinv [B][9] -- instead of launch constants, so one captured launch sequence serves any crop sizes within the caps:
 *   images / aux / gradients live in slots of pix_stride pixels per channel: color [B][3][pix_stride], mask / depth [B][pix_stride],
 *   aux [B][pix_stride][4]; crop b uses the first W_b H_b entries of each channel, rows of W_b pixels;
 *   tiles_cap >= ceil(W_b / 8) ceil(H_b / 8) for every crop (launch bound and tile-list layout of the splat workspace,
 *   sdfr_splat_ws_words_r words); tiles16_cap likewise for the 16 x 16 tiles of the 2-D loss.
 * Arithmetic per crop exactly as the fixed-extent calls: a crop's results are bit-identical to rendering it alone at its own size.
 * Disc primitive (the optimizer's), no background.
 * CALLER'S CONTRACT (the extents live on the device, the entry points cannot check them): for every crop  1 <= W_b, 1 <= H_b,
 * W_b * H_b <= pix_stride,  ceil(W_b/8) * ceil(H_b/8) <= tiles_cap,  ceil(W_b/16) * ceil(H_b/16) <= tiles16_cap,  and for the tracer
 * ceil(W_b/block) * ceil(H_b/block) <= cone_cap.  The Python layer validates them in set_extents() (sdflabel_amd/batch.py,
 * renderer/sphere_tracer.py) before they reach the device.  Defence in depth (r05): the kernels treat a crop with W_b < 1, H_b < 1,
 * W_b * H_b > pix_stride or more 8x8 tiles than tiles_cap as EMPTY (nothing rendered, zero loss and gradients, its slot untouched) instead
 * of writing out of bounds (tests/test_gpu_ragged.py); cone_cap and tiles16_cap remain the caller's to guarantee. */
int64_t sdfr_splat_ws_words_r(int B, int cap, int tiles_cap);
int sdfr_surfels_forward_r(const float* xyz, int xyz_stride, const float* sdf, int64_t G, const int32_t* idx, const float* J, int Jstride,
                           int Joff, const float* pose, const float* K, int B, int cap, const int32_t* cnt, int output_nocs,
                           const int32_t* wh, int tiles_cap, float diam, float* points, float* normals, float* p_cam, float* n_cam, float* col,
                           int32_t* fidx, int32_t* fcnt, float* xyzf, int32_t* fslot, int32_t* bbox, void* stream);
int sdfr_splat_forward_r(int flags /* SDFR_PRIM_BOXES_READY | SDFR_PRIM_BINS */, const float* K, const float* Kinv, const float* p_cam,
                         const float* n_cam, const float* attr, int B, int cap, const int32_t* cnt, const int32_t* wh, int pix_stride,
                         int tiles_cap, float diam, float depth_constant, int32_t* bbox_ws, float* color, float* mask, float* depth,
                         float* normals, float* aux, void* stream);
int sdfr_splat_backward_r(const float* K, const float* Kinv, const float* p_cam, const float* n_cam, const float* attr, int B, int cap,
                          const int32_t* cnt, const int32_t* wh, int pix_stride, float diam, float depth_constant, const float* aux,
                          const float* color, const float* mask, const float* depth, const float* normals, const float* g_color,
                          const float* g_mask, const float* g_depth, const float* g_normals, float* g_p_cam, float* g_n_cam, float* g_attr,
                          void* stream);
/* sdfr_loss_2d on ragged extents; scratch float[3 * B * tiles16_cap] */
int sdfr_loss_2d_r(const float* rend, const float* target, int B, const int32_t* wh, int pix_stride, int tiles16_cap, float diam,
                   float threshold_nocs, float weight, float* loss, float* g_rend, int32_t* nvalid, float* scratch, void* stream);

/* The dense weight matrix the reference's standalone primitives return (prob_color[:, 0, :] of inside_surfel / inside_circle /
 * inside_circle_opt, primitives.py:71,162,243): weights [B][rows][W*H], rows = cap (+1 background row when bg_logit != NULL), from the
 * per-pixel state `aux` of a sdfr_splat_forward call over the same surfels (with the same bg_logit).  `weights` must be zero-filled; only
 * covered (surfel, pixel) pairs are written.  Not used by the renderer itself. */
int sdfr_splat_weights(int primitive, const float* K, const float* Kinv, const float* p_cam, const float* n_cam, const float* uv,
                       const float* znorm, const float* bg_logit, int B, int cap, const int32_t* cnt, int W, int H, float diam,
                       float depth_constant, const float* aux, float* weights, void* stream);
/* Its backward w.r.t. p_cam / n_cam given g_weights [B][rows][W*H] and wsum[b][pix] = sum_j weights_j * g_weights_j (the softmax-backward
 * sum over ALL rows of the pixel, background row included).  Coverage masks, the per-pixel norm and the background logit are constants, as
 * in the reference's autograd (primitives.py:55,59,226,228). */
int sdfr_splat_weights_backward(int primitive, const float* K, const float* Kinv, const float* p_cam, const float* n_cam, const float* uv,
                                const float* znorm, int has_bg_row, int B, int cap, const int32_t* cnt, int W, int H, float diam,
                                float depth_constant, const float* aux, const float* g_weights, const float* wsum, float* g_p_cam,
                                float* g_n_cam, void* stream);

/* The same three calls with the primitive's clamp configuration spelled out (r05) -- what the reference's standalone functions accept
 * beyond the calls Rasterer.forward makes (rasterer.py:92-104):
 *   clamp_alt = 0   the renderer's clamp: disc hard (softclamp=False), circle / circle_opt sigmoid (softclamp=True)
 *   clamp_alt = 1   the other one: disc softclamp=True -- inside_surfel's OWN default, primitives.py:174,217-218: the mask
 *                   sigmoid((diam - d) * c) > 0 holds until exp overflows, so practically every surfel covers every pixel (dense work,
 *                   whole-image screen boxes); circle / circle_opt softclamp=False -- a hard edge (:51-53,:120)
 *   clamp_constant  softclamp_constant of the sigmoid clamps (> 0; 3 / 5 / 5 are the functions' defaults, :13,:83,:175); ignored by hard clamps
 * sdfr_splat_forward / _weights / _weights_backward are these with (0, default constant).  clamp_alt = 1 computes its own screen boxes
 * (no SDFR_PRIM_BOXES_READY / SDFR_PRIM_BINS). */
int sdfr_splat_forward_clamp(int primitive, const float* K, const float* Kinv, const float* p_cam, const float* n_cam, const float* attr,
                             const float* uv, const float* znorm, const float* bg, const float* bg_logit, int B, int cap, const int32_t* cnt,
                             int W, int H, float diam, float depth_constant, int clamp_alt, float clamp_constant, int32_t* bbox_ws,
                             float* color, float* mask, float* depth, float* normals, float* aux, void* stream);
int sdfr_splat_weights_clamp(int primitive, const float* K, const float* Kinv, const float* p_cam, const float* n_cam, const float* uv,
                             const float* znorm, const float* bg_logit, int B, int cap, const int32_t* cnt, int W, int H, float diam,
                             float depth_constant, int clamp_alt, float clamp_constant, const float* aux, float* weights, void* stream);
int sdfr_splat_weights_backward_clamp(int primitive, const float* K, const float* Kinv, const float* p_cam, const float* n_cam, const float* uv,
                                      const float* znorm, int has_bg_row, int B, int cap, const int32_t* cnt, int W, int H, float diam,
                                      float depth_constant, int clamp_alt, float clamp_constant, const float* aux, const float* g_weights,
                                      const float* wsum, float* g_p_cam, float* g_n_cam, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Batched refinement step glue  --  the per-iteration host tensor algebra of pipelines/optimizer.py:86-100, for B crops
 * at once and entirely on the device (no host synchronisation anywhere in a step).
 */

/* pose[b] = [R_y(yaw_b) | t_b] with the rotation's row 1 negated (optimizer.py:87-90, utils/refinement.py:108-125);
 * inputs[b*G+g] = [latent_b / max(||latent_b||, 1e-12), grid[g]]  (optimizer.py:96-100);  latnorm[b] = the norm used.
 * inputs == NULL: pose and latnorm only (pose-only refinement of a frozen shape; grid may then be NULL too). */
int sdfr_params_forward(const float* yaw, const float* trans, const float* latent, int L, const float* grid, int64_t G, int B,
                        float* inputs, float* pose, float* latnorm, void* stream);

/* g_latn[b][:] = sum_s -( (g_points + g_nocs/2)_s . n_hat_s ) * J[b][s][0:L]   -- backward of grid.py:61,67 chained with the
 * decoder's input gradient summed over the expanded latent rows (what autograd does at optimizer.py:156).  g_nocs may be NULL. */
int sdfr_surface_latent_grad(const float* g_points, const float* g_nocs, const float* normals, const float* J, int n_inputs, int L,
                             int B, int cap, const int32_t* cnt, float* g_latn, void* stream);

/* g_yaw[B], g_trans[B][3] from g_pose[B][16]; g_latent[B][L] from g_latn through F.normalize. */
int sdfr_params_backward(const float* yaw, const float* latent, int L, const float* latnorm, const float* g_pose, const float* g_latn,
                         int B, float* g_yaw, float* g_trans, float* g_latent, void* stream);

/* The backward tail of the batched step in one launch (latent sizes 1..8): sdfr_project_dcm_bwd (with its optional g_xyzf / fslot and
 * colour-map handling), sdfr_surface_latent_grad (g_latn[b][c] = sum_s -(g_points_s . normals_s) J[b][s][c]) and sdfr_params_backward,
 * with the same fixed-order reductions -- the results are bit-identical to calling the three.  g_points may be NULL (not stored).
 * J == NULL: pose gradients only (the latent is not a variable: pose-only refinement); g_latn and g_latent are zero-filled.
 * Replaces the autograd of pipelines/optimizer.py:86-100 + sdfrenderer/renderer/projection.py:34-70 + sdfrenderer/grid.py:61. */
int sdfr_pose_latent_backward(const float* pose, const float* points, const float* normals, const float* g_p_cam, const float* g_n_cam,
                              const float* g_col, int B, int cap, const int32_t* cnt, int output_nocs, const float* g_xyzf,
                              const int32_t* fslot, const float* J, int n_inputs, int L, const float* yaw, const float* latent,
                              const float* latnorm, float* g_points, float* g_pose, float* g_latn, float* g_yaw, float* g_trans,
                              float* g_latent, void* stream);

/* padded front-facing selection (points['xyzf'], rasterer.py:151): out[b][j] = src[b][idx[b][j]] for j < cnt[b], 0 beyond;
 * and its backward dst[b][idx[b][j]] += src[b][j]. */
int sdfr_gather_rows3(float* out, const float* src, const int32_t* idx, int B, int cap, const int32_t* cnt, void* stream);
int sdfr_scatter_add_rows3(float* dst, const float* src, const int32_t* idx, int B, int cap, const int32_t* cnt, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Losses and solver step of the refinement loop (pipelines/optimizer.py:144-157, 166-237), B crops at once, device resident.
 */

/* compute_loss_3d (optimizer.py:166-198): exact nearest lidar point (lidar/scale, :84) of every estimated point est[b][j], j < ecnt[b];
 * pairs with distance < threshold/scale[b]; loss[b] = mean pair distance (0 without pairs).  g_est [B][ecap][3] and g_scale [B] receive
 * weight * d loss / d(est, scale).  npairs[b] = number of pairs, or -1 when either cloud is empty (the loop skips the crop, :127-129).
 * scratch: 3 * B * ceil(ecap / 64) floats (partial sums of the two-pass reduction). */
int sdfr_loss_3d(const float* est, const int32_t* ecnt, int ecap, const float* lidar, const int32_t* lcnt, int lcap, const float* scale,
                 float threshold, float weight, int B, float* loss, float* g_est, float* g_scale, int32_t* npairs, float* scratch,
                 void* stream);

/* compute_loss_2d (optimizer.py:200-237) on rend, target [B][3][H][W]: per rendered non-zero pixel the smallest distance to the target
 * weighted by clamp(diam - pixel distance, 0); loss[b] = mean of the minima below threshold_nocs (NaN if none, 0 without rendered pixels,
 * exactly as the reference); g_rend = weight * d loss / d rend; nvalid[b] = number of pixels in the mean. */
int sdfr_loss_2d(const float* rend, const float* target, int B, int H, int W, float diam, float threshold_nocs, float weight,
                 float* loss, float* g_rend, int32_t* nvalid, float* scratch /* float[3 * B * ceil(W/16) * ceil(H/16)] */, void* stream);

/* MultipleOptimizer.step (optimizer.py:13-23,34-52): Adam(lr_adam, betas .9/.999, eps 1e-8) on yaw and trans, SGD on scale (lr_scale) and
 * latent (lr_latent).  params / grads are ONE flat structure-of-arrays buffer [ yaw(B) | trans(B,3) | scale(B) | latent(B,L) ].
 * total[b] = w3*loss3d + w2*loss2d; a crop is skipped (stepped[b] = 0, no state change) when npairs[b] < 0, total is NaN or total == 0
 * (optimizer.py:127-129,149-151). */
int sdfr_solver_step(float* params, const float* grads, int L, const float* loss2d, const float* loss3d, const int32_t* npairs,
                     float w2, float w3, float* adam_m, float* adam_v, int32_t* adam_t, float lr_adam, float lr_scale, float lr_latent,
                     int B, float* total, int32_t* stepped, void* stream);

/* ------------------------------------------------------------------------------------------------
 * r06: the refinement iteration in 12 launches instead of 21 (the per-annotation call of pipelines/refine_css.py:203-223 is a chain of
 * latency-bound launches: every one removed is ~5 us of a 0.3 ms iteration).  Each entry point below is the fusion of entry points above and
 * returns THEIR bits (GPU tests compare the two launch sequences array by array).
 */
/* sdfr_params_forward + sdfr_prefilter_plan (optimizer.py:86-100 + the candidate-reuse plan). */
int sdfr_params_plan(const float* yaw, const float* trans, const float* latent, int L, const float* grid, int64_t G, int B, float* inputs,
                     float* pose, float* latnorm, float lip, const float* margin, const float* max_dev, float* lat_ref, int32_t* age,
                     int max_reuse, int32_t* reuse, int32_t* n_full, void* stream);
/* sdfr_band_select_skip with a STICKY truncation flag: over[b] |= over_bit whenever crop b's selection holds more than cap rows (cnt[b] is
 * overwritten by every selection; the reference has no capacity, grid.py:64-66, so a truncated band must never pass silently).  thr_extra,
 * skip, slot and over may be NULL.  Launches of up to 8 crops with a flag array take one workgroup per crop (one launch instead of two). */
int sdfr_band_select_ex(const float* sdf, int64_t G, int B, float thr, const float* thr_extra, const int32_t* skip, int32_t* idx, int cap,
                        int32_t* cnt, int32_t* slot, int32_t* scratch, int32_t* over, int over_bit, void* stream);
/* sdfr_band_select_ex and the ranking of sdfr_mlp_forward_balanced in ONE launch (SDFR_VERSION 422), for the serial stretch between a
 * one-crop grid forward and the band's Jacobian.  Selection: idx / cnt / slot / over receive what sdfr_band_select_ex writes (ascending grid
 * order, cap, thr_extra, skip, the sticky bit); there is no scratch -- a workgroup of 1024 rows counts the band rows of its crop in front of
 * its own straight from sdf, redundant reads that grow with B G^2, instead of a counting launch.  No workgroup waits for another.
 * balance_state / order_rows: the state of sdfr_mlp_forward_balanced_deferred, ranked by further workgroups of the same launch exactly as
 * sdfr_mlp_forward_balanced ranks it (orders of more than 4096 chunks: not ranked); NULL: the selection alone.  One kernel, no memset or copy
 * node.  sdfr_band_select_rank_max_rows(): the B G up to which this launch is the faster form (measured, profiles/chain_notes.md); callers keep
 * sdfr_mlp_forward_balanced + sdfr_band_select_ex above it. */
int sdfr_band_select_rank(const float* sdf, int64_t G, int B, float thr, const float* thr_extra, const int32_t* skip, int32_t* idx, int cap,
                          int32_t* cnt, int32_t* slot, int32_t* over, int over_bit, void* balance_state, int64_t order_rows, void* stream);
int64_t sdfr_band_select_rank_max_rows(void);
/* sdfr_candidate_rows + sdfr_mlp_forward(_f16)_ragged without the gathered copy: row s < cnt[b] of crop b is
 * inputs[b * rows_per_crop_in + cidx[b][s]]; values -> sdf [B][stride], masks -> mask_ws.  half: the float16 kernel (half_tiles: 64-row
 * tiles); else the exact-float32 kernel.  stride a multiple of the tile (128 / 64).  (deep_sdf_decoder_scale.py:78-107 on the candidate rows) */
int sdfr_mlp_forward_candidates(const sdfr_decoder* d, const float* inputs, int64_t rows_per_crop_in, int B, const int32_t* cidx, int64_t stride,
                                const int32_t* cnt, float* sdf, uint32_t* mask_ws, int half, int half_tiles, void* stream);
/* sdfr_scatter_values + sdfr_band_select + sdfr_candidate_band_map: the band of a crop whose candidate set is valid lies inside the candidates,
 * which are listed in ascending grid-row order -- idx[b][e] = grid row of the e-th candidate with |csdf| < thr, pos[b][e] = its position in the
 * candidate array, cnt[b] their number; the candidate values are also written into sdf_grid.  over (may be NULL): sticky flags, |= 1 band > cap,
 * |= 2 candidates > stride.  (grid.py:64-66 on the candidate rows) */
int sdfr_candidate_band(float* sdf_grid, const float* csdf, const int32_t* cidx, int64_t G, int B, int stride, const int32_t* ccnt, float thr,
                        int32_t* idx, int cap, int32_t* cnt, int32_t* pos, int32_t* over, void* stream);
/* sdfr_loss_2d(_r) + sdfr_loss_3d in one launch (optimizer.py:166-237).  wh == NULL: dense H x W images; else ragged extents (pix_stride,
 * tiles16_cap as sdfr_loss_2d_r).  g_rend / g_est receive the UN-normalised gradients and kscale float[B][2] the per-crop factors
 * (weight / count, or 0) the consumers multiply on load: sdfr_splat_backward_x (kscale[2b]) and sdfr_pose_latent_solver (kscale[2b+1]).
 * Two launches (pixel + pairs passes together; one tiny finalize pass) where sdfr_loss_2d + sdfr_loss_3d take four. */
int sdfr_losses_fused(const float* rend, const float* target, int B, int H, int W, const int32_t* wh, int pix_stride, int tiles16_cap, float diam,
                      float threshold_nocs, float weight2d, float* loss2d, float* g_rend, int32_t* nvalid, float* scratch2, const float* est,
                      const int32_t* ecnt, int ecap, const float* lidar, const int32_t* lcnt, int lcap, const float* scale, float threshold3d,
                      float weight3d, float* loss3d, float* g_est, float* g_scale, int32_t* npairs, float* scratch3, float* kscale,
                      void* stream);
/* sdfr_splat_backward(_r) of the disc primitive for a colour gradient alone, scaled by kscale[2 b] on load (primitives.py:209-242 backward).
 * bbox_ws (may be NULL): the splat workspace this step's sdfr_surfels_forward(_r) / sdfr_splat_forward(_r) filled -- the surfels' screen boxes at
 * its head are then read instead of recomputed (same boxes, same results). */
int sdfr_splat_backward_x(const float* K, const float* Kinv, const float* p_cam, const float* n_cam, const float* attr, int B, int cap,
                          const int32_t* cnt, int W, int H, const int32_t* wh, int pix_stride, float diam, float depth_constant, const float* aux,
                          const float* color, const float* g_color, const float* kscale, float* g_p_cam, float* g_n_cam, float* g_attr,
                          const int32_t* bbox_ws, void* stream);
/* sdfr_pose_latent_backward (g_xyzf scaled by kscale[2 b + 1] on load) + sdfr_solver_step.  g_yaw / g_trans / g_latent are the sections of
 * `grads`, whose scale section the loss launch has written (optimizer.py:156 backward, :13-23 step). */
int sdfr_pose_latent_solver(const float* pose, const float* points, const float* normals, const float* g_p_cam, const float* g_n_cam,
                            const float* g_col, int B, int cap, const int32_t* cnt, int output_nocs, const float* g_xyzf, const int32_t* fslot,
                            const float* kscale, const float* J, int n_inputs, int L, const float* yaw, const float* latent, const float* latnorm,
                            float* g_pose, float* g_latn, float* params, float* grads, const float* loss2d, const float* loss3d,
                            const int32_t* npairs, float w2, float w3, float* adam_m, float* adam_v, int32_t* adam_t, float lr_adam,
                            float lr_scale, float lr_latent, float* total, int32_t* stepped, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sphere-tracing render mode  --  NOT in the reference (its renderer splats surfels of a grid band); the mode BASELINE.json's north_star words
 * literally: per-ray march with a decoder evaluation per step and ballot compaction of terminated rays.  No parity claim.
 *   rays in object space: p_cam = R p + t (pose [B][16]), pixel ray K^-1 [x, y, 1] (Kinv [B][9]); lam = camera-frame depth along the ray.
 *   state: counters int32[3] (rotating active-ray counts, on the device), pix int32[n_max] (crop*W*H + pixel), lam float[n_max], two of each
 *   (ping-pong), far float[B*W*H], inputs float[n_max][L+3] decoder input rows of the active rays (latn [B][L] = normalised latent),
 *   hit_lam / hit_sdf float[B*W*H] (zero-filled by the caller; lam and decoder value of the rays that reached |sdf| < eps).
 */
/* decoder forward over the first *n_dev rows (device int32, clamped to n_max); half != 0: half operands on the matrix cores.
 * float32, 512-wide decoders: two launches per call, 64-row and 16-row tiles; the one that does not fit the count exits at once
 * (a thin step is one decoder pass of latency per workgroup: 0.12 ms on 16-row tiles, 0.44 ms on 64-row tiles).
 * half | 2 (half operands only): one product shape whatever the count -- 128-row tiles while they fill the chip, 64-row tiles of the same
 * 32x32x16 products below -- so that a row's value has the same bits in every launch (a crop then marches identically alone and in a batch;
 * the 16-row tiles of plain `half` use 16x16x32 products, whose summation order differs). */
int sdfr_mlp_forward_counted(const sdfr_decoder* dec, const float* inputs, int64_t n_max, const int32_t* n_dev, float* sdf, int half,
                             void* stream);
/* all pixels of all crops: slab test against the cube [-bound, bound]^3; hits enter the active list (counters[0]) at lam = max(entry, near).
 * cone (optional, from sdfr_trace_cone with the same cone_block): per pixel block the parameter its rays start from instead, or -1: the
 * block's rays are misses. */
int sdfr_trace_setup(const float* pose, const float* Kinv, const float* latn, int L, int B, int W, int H, float bound, float near,
                     int32_t* counters, int32_t* pix,
                     float* lam /* ray state float[n][4]: lam = next sample, rho = |sdf| of the previous sample, q = ratio of the last two radii, - */,
                     float* far, float* inputs, const float* cone, int cone_block, void* stream);
/* ... which also zero-fills hit_lam / hit_sdf (float[B*W*H], both or neither NULL): no separate fills before a march */
int sdfr_trace_setup2(const float* pose, const float* Kinv, const float* latn, int L, int B, int W, int H, float bound, float near,
                      int32_t* counters, int32_t* pix, float* lam, float* far, float* inputs, const float* cone, int cone_block, float* hit_lam,
                      float* hit_sdf, void* stream);
/* Cone marching ahead of the per-ray march (optional): ONE ray through the centre of every block x block pixel tile stands for its pixels --
 * all pixel rays share origin and parametrisation, so the tile's rays at parameter lam lie within lam * delta of the centre ray's point
 * (delta = max |d_corner - d_centre|).  v = decoder(centre point): v - lam delta > eps -> nothing within the cone's cross-section, advance by
 * (v - lam delta) / (|d_c| + delta); <= eps -> the tile's rays start their own march there; past the cube's far side for all of them ->
 * culled; after cone_steps passes the cones stop where they are.  cone float[B][ceil(W/block) * ceil(H/block)]: start parameter or -1.
 * A centre point outside the cube is evaluated clamped into it, v = sqrt(clamp distance^2 + max(f, 0)^2): no extrapolated decoder value is trusted.
 * spec_k (1 ... 8; r04): speculative cone passes -- a pass evaluates spec_k samples of a cone, p_0 = lam, p_j = p_{j-1} + sigma q^j a_prev
 * (a_prev = the cone's previous advance, q = ratio of its last two advances in [0.5, 1.5]); sample j counts only inside the range its
 * predecessor proved free, so the accepted prefix is a valid, shorter-stepped cone march (4 samples x 4 passes cull what 10 plain passes cull).
 * counters: device int32[SDFR_TRACE_COUNTERS] (zeroed here; [0..2] rotating ROW counts, [4..5] one uint64 = decoder evaluations); ids0/st0/aux0, ids1/st1/aux1:
 * ping-pong cone lists (int32[n], float[n][4], float[n][2], n = B * tiles); inputs float[n * spec_k][L+3], sdf float[n * spec_k] scratch.
 * half | 2: see sdfr_mlp_forward_counted.  No host synchronisation. */
int sdfr_trace_cone(const sdfr_decoder* dec, const float* pose, const float* Kinv, const float* latn, int L, int B, int W, int H, float bound,
                    float near, float eps, int block, int cone_steps, int spec_k, float sigma, int half, int32_t* counters, int32_t* ids0,
                    float* st0, float* aux0, int32_t* ids1, float* st1, float* aux1, float* inputs, float* sdf, float* cone, void* stream);
/* march step `step` (0, 1, ...): sdf = decoder values of the active rays (counters[step % 3] of them); lam += sdf / |d|; rays with
 * |sdf| < eps are recorded in hit_lam / hit_sdf and retired, rays past `far` are retired, the rest are compacted into pix_out / lam_out /
 * inputs (count in counters[(step + 1) % 3]) */
int sdfr_trace_step(const float* pose, const float* Kinv, const float* latn, int L, int W, int H, float eps, const float* sdf,
                    int32_t* counters, int step, int64_t n_max, const int32_t* pix_in, const float* lam_in, int32_t* pix_out, float* lam_out,
                    const float* far, float* inputs, float* hit_lam, float* hit_sdf, void* stream);

/* The whole march in ONE call, no host synchronisation (counters: device int32[SDFR_TRACE_COUNTERS], zeroed by sdfr_trace_setup -- [0..2]
 * rotating active counts, [3] rays unresolved when the step budget ran out, [4..5] one uint64 = decoder evaluations of the march, [6] hits,
 * [7 + i] rays handed from stage i of the looping kernel to stage i + 1, [16 + i] tile counter of stage i).  While the device-side count is
 * >= tail_rows a step is the decoder on the active rows + the step kernel; below it ONE launch of the decoder kernel in its looping mode takes
 * the remaining rays on (ray state in registers, no per-step launch, no compaction); the gate is evaluated on the device in each of the first
 * head_steps steps, then an unconditional launch takes what is left (tail_rows = 0: the hand-over happens at pass index head_steps, whatever
 * the count -- a crop then marches the same alone and inside a batch).
 * levels: HOST array int32[n_levels][2] = (first pass index, samples per ray and pass), both ascending, samples 4 / 8 / 16 / 32 / 64,
 * n_levels <= SDFR_TRACE_LEVELS: from pass index levels[i][0] on a pass evaluates levels[i][1] samples per ray (p_0 = lam, p_j = p_{j-1} +
 * sigma q^j rho / |d|; q = ratio of the ray's last two radii clamped to [0.5, q_max], q_max >= 1) and accepts the prefix in which every sample
 * lies inside the previous one's safe sphere -- a valid sphere-tracing sequence, nothing skipped; the pass index alone decides (head_steps is
 * clamped to levels[0][0]), so a ray's samples do not depend on the launch schedule.  n_levels = 0: plain tracing.  Each level is one launch of
 * the looping kernel: 64 / samples rays per 64-row tile, a pool of sdfr_trace_pool() persistent workgroups fetching tiles from a device counter,
 * survivors appended to the next level's list -- fewer, equally long passes for the grazing rays that end a march.
 * Decoders with LayerNorm or a hidden width below 257 march with per-step launches of their own float32 forward kernels (plain tracing, no
 * looping kernel; half must be 0).
 * pix0/lam0 (filled by sdfr_trace_setup) and pix1/lam1 are the ping-pong active lists (lam: ray state float[n][4]), pix2/lam2 the hand-over
 * list between levels (same sizes; may be NULL with fewer than two levels; pix0/lam0 is the other one), sdf float[B*W*H] scratch, tail_rows_buf
 * float[sdfr_trace_pool()][64][L + 3] scratch of the looping kernel. */
int sdfr_trace_pool(void);
int sdfr_trace_march(const sdfr_decoder* dec, const float* pose, const float* Kinv, const float* latn, int L, int B, int W, int H, float eps,
                     int steps, int head_steps, int tail_rows, const int32_t* levels, int n_levels, float q_max, float sigma, int half,
                     int32_t* counters, int32_t* pix0, float* lam0, int32_t* pix1, float* lam1, int32_t* pix2, float* lam2, const float* far,
                     float* inputs, float* sdf, float* tail_rows_buf, float* hit_lam, float* hit_sdf, void* stream);
/* hit pixels (hit_lam > 0) -> compact list: rows float[n][L+3] = [latn, o + lam d] for sdfr_mlp_jacobian (rows_per_crop = B*W*H, B = 1,
 * idx = the identity written here, cnt = n_hits), hit_slot int32[B*W*H] = list position of the pixel's hit or -1.  n_hits: device int32,
 * zero on entry (counters + 6 after sdfr_trace_setup). */
int sdfr_trace_hits(const float* pose, const float* Kinv, const float* latn, int L, int B, int W, int H, const float* hit_lam, int32_t* n_hits,
                    int32_t* hit_slot, int32_t* idx, float* rows, void* stream);
/* images of the hits after one Newton step along the ray with the exact-f32 decoder value f0 [slot] and input Jacobian J [slot][L+3]
 * (non-grazing rays only): depth [B][1][H][W] = lam_s r_z, color [B][3][H][W] = NOCS of the hit point, normals [B][3][H][W] = (R n + 1) / 2,
 * mask [B][1][H][W] = 1; zero at the other pixels.  lam_s (optional) float[B*W*H]: the polished ray parameter. */
int sdfr_trace_composite(const float* pose, const float* Kinv, int L, int B, int W, int H, const float* hit_lam, const int32_t* hit_slot,
                         const float* J, const float* f0, float* color, float* mask, float* depth, float* normals, float* lam_s, void* stream);
/* backward at a fixed hit set through the implicit function f(o + lam d, z) = 0: image gradients (each may be NULL) -> g_pose [B][16]
 * (gradient w.r.t. the entries of the row-major 4x4 pose) and g_latn [B][L] (w.r.t. the normalised latent); fixed-order sums per crop.
 * ws: sdfr_trace_backward_ws_floats(B, W, H) floats.  sdfr_params_backward maps the result to yaw / trans / latent. */
int64_t sdfr_trace_backward_ws_floats(int B, int W, int H);
int sdfr_trace_backward(const float* pose, const float* Kinv, int L, int B, int W, int H, const float* hit_lam, const int32_t* hit_slot,
                        const float* J, const float* f0, const float* g_color, const float* g_depth, const float* g_normals, float* ws,
                        float* g_pose, float* g_latn, void* stream);

/* Ragged extents for the sphere tracer (r04): every crop of the batch its own image size and intrinsics, as for the splat path's `_r` entry points.
 * ext->wh: DEVICE int32[B][2] = (W_b, H_b); ext->pix_stride: pixels of a crop's slot in every per-pixel array (far, hit_lam, hit_sdf, hit_slot,
 * pt_slot, lam_s: [B * pix_stride]; images [B][C][pix_stride]; global pixel id = b * pix_stride + y * W_b + x); ext->cone_cap: cone slots per crop
 * (>= ceil(W_b / block) * ceil(H_b / block); cone float[B * cone_cap], the cone lists n = B * cone_cap).  The struct itself is read on the HOST at
 * the call.  Same arithmetic per crop as the fixed-extent entry points: a crop traces bit-identically alone at its own size. */
typedef struct sdfr_extents { const int32_t* wh; int pix_stride; int cone_cap; } sdfr_extents;
int sdfr_trace_setup_r(const float* pose, const float* Kinv, const float* latn, int L, int B, const sdfr_extents* ext, float bound, float near,
                       int32_t* counters, int32_t* pix, float* lam, float* far, float* inputs, const float* cone, int cone_block, float* hit_lam,
                       float* hit_sdf, void* stream);
int sdfr_trace_cone_r(const sdfr_decoder* dec, const float* pose, const float* Kinv, const float* latn, int L, int B, const sdfr_extents* ext,
                      float bound, float near, float eps, int block, int cone_steps, int spec_k, float sigma, int half, int32_t* counters,
                      int32_t* ids0, float* st0, float* aux0, int32_t* ids1, float* st1, float* aux1, float* inputs, float* sdf, float* cone,
                      void* stream);
int sdfr_trace_march_r(const sdfr_decoder* dec, const float* pose, const float* Kinv, const float* latn, int L, int B, const sdfr_extents* ext, float eps,
                       int steps, int head_steps, int tail_rows, const int32_t* levels, int n_levels, float q_max, float sigma, int half,
                       int32_t* counters, int32_t* pix0, float* lam0, int32_t* pix1, float* lam1, int32_t* pix2, float* lam2, const float* far,
                       float* inputs, float* sdf, float* tail_rows_buf, float* hit_lam, float* hit_sdf, void* stream);
int sdfr_trace_hits_r(const float* pose, const float* Kinv, const float* latn, int L, int B, const sdfr_extents* ext, const float* hit_lam,
                      int32_t* n_hits, int32_t* hit_slot, int32_t* idx, float* rows, void* stream);
int sdfr_trace_composite_r(const float* pose, const float* Kinv, int L, int B, const sdfr_extents* ext, const float* hit_lam, const int32_t* hit_slot,
                           const float* J, const float* f0, float* color, float* mask, float* depth, float* normals, float* lam_s, void* stream);
int sdfr_trace_points_r(const float* Kinv, int B, const sdfr_extents* ext, const int32_t* hit_slot, const float* lam_s, float* xyzf, int ecap,
                        int32_t* ecnt, int32_t* pt_slot, void* stream);
int sdfr_trace_refine_backward_r(const float* pose, const float* Kinv, int L, int B, const sdfr_extents* ext, const float* hit_lam,
                                 const int32_t* hit_slot, const float* J, const float* f0, const float* g_color, const float* g_depth,
                                 const float* g_normals, const float* g_xyzf, const int32_t* pt_slot, int ecap, int surfel, float* ws /* sdfr_trace_backward_ws_floats(B, pix_stride, 1) */,
                                 float* g_pose, float* g_latn, void* stream);

/* The sphere tracer as a backend of the refinement loop (pipelines/optimizer.py:110-146 reads rendering['color'] and points['xyzf'] from its
 * renderer).  sdfr_trace_points gives points['xyzf'] of a traced render: the camera-frame hit points p_cam = lam_s K^-1 [x, y, 1] of each crop's
 * hit pixels, compacted in pixel (row-major) order into xyzf [B][ecap][3]; ecnt [B] = the crop's TRUE hit count (surplus beyond ecap dropped:
 * callers compare), pt_slot int32[B*W*H] = a pixel's row or -1.  hit_slot / lam_s: from sdfr_trace_hits / sdfr_trace_composite. */
int sdfr_trace_points(const float* Kinv, int B, int W, int H, const int32_t* hit_slot, const float* lam_s, float* xyzf, int ecap,
                      int32_t* ecnt, int32_t* pt_slot, void* stream);
/* sdfr_trace_backward with the gradient arriving through those points (g_xyzf [B][ecap][3] + pt_slot, both may be NULL) and a choice of
 * derivative semantics:
 *   surfel = 0  image-space derivative at the fixed pixels through the implicit function f(o + lam d, z) = 0 (what sdfr_trace_backward computes;
 *               a hit point then moves along its fixed pixel ray only: g_lam += g_xyzf . r);
 *   surfel = 1  the autograd semantics of the reference's surface points (sdfrenderer/grid.py:61 p = x - sdf n_hat with n_hat constant;
 *               sdfrenderer/renderer/projection.py:53-58 colour = the point's own object coordinates, p_cam = R p + t): every hit is a MATERIAL
 *               point x_s that moves rigidly with the pose and along its normal with the latent, d x_s = -n_hat (d f/d z . dz) / |grad f|; its
 *               NOCS colour does not depend on the pose; depth = (R x_s + t)_z; normals = (R n_hat + 1) / 2 with n_hat constant.
 *               This is the mode the refinement loop converges with (the loop's one-directional nearest-neighbour 3-D loss needs points that
 *               can move laterally). */
int sdfr_trace_refine_backward(const float* pose, const float* Kinv, int L, int B, int W, int H, const float* hit_lam, const int32_t* hit_slot,
                               const float* J, const float* f0, const float* g_color, const float* g_depth, const float* g_normals,
                               const float* g_xyzf, const int32_t* pt_slot, int ecap, int surfel, float* ws, float* g_pose, float* g_latn,
                               void* stream);

/* The decoder's scale head on one latent row (deep_sdf_decoder_scale.py:68-75,110-112): out[0] = W3 relu(W2 relu(W1 lat + b1) + b2) + b3 with
 * W1 [3][L], W2 [3][3], W3 [1][3] row-major as nn.Linear stores them.  Returned by Decoder.forward next to the SDF values; unused by the loop. */
int sdfr_scale_net(const float* latent_row, int L, const float* W1, const float* b1, const float* W2, const float* b2, const float* W3,
                   const float* b3, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RANSAC pose initialisation  --  replaces PoseEstimator.init_pose_3d (utils/pose.py:85-233, type 'kabsch' / 'procrustes') for B crops.
 *
 * Model (the decoder's surface points and their NOCS colours) and scene (reprojected NOCS points and colours) are ragged:
 * model / model_cls [B][mcap][3] with mcnt[b] >= 1 rows, scene / scene_cls [B][ncap][3] with ncnt[b] rows, all float32.  A float16 model
 * is passed widened to float32 (exact) with model_f16 = 1: the fits then round the model's means and centred values to float16 as numpy
 * does.  For 'kabsch' the caller has already scaled the model by scale_model in its own dtype (utils/pose.py:126-127).
 * T hypotheses (the reference: 567), 4 distinct scene indices each.
 */
/* bytes of the workspace of sdfr_ransac_pose (colour-NN distances, hypothesis transforms, pass lists, inlier mask) */
int64_t sdfr_ransac_ws_bytes(int B, int ncap, int T);
/* device sampler: idx [B][T][4] int32 = 4 distinct indices in [0, ncnt[b]) per hypothesis (all zero when ncnt[b] < 4), from a
 * counter-based hash of (seed, keys[b], t, draw, attempt); keys (DEVICE pointer, int64[B]) == NULL means key b.  A crop's draws depend on
 * its own key only.  idx must be 16-byte aligned (written as int4). */
int sdfr_ransac_sample(int64_t seed, const int64_t* keys, const int32_t* ncnt, int B, int T, int32_t* idx, void* stream);
/* The whole estimate: colour-NN table, gate + fit of every hypothesis, inlier counts, first best, final fit model -> scene.
 *   idx        [B][T][4] the sampled scene indices (e.g. the reference's np.random.choice draws), or NULL: the device sampler with
 *              (seed, keys) writes them to idx_out first (keys: DEVICE pointer, int64[B], or NULL = key b); idx and idx_out must be
 *              16-byte aligned (read / written as int4)
 *   type       0 kabsch (final scale = scale_model), 1 procrustes (final scale from the fit)
 *   h_thr      HOST pointer, double[2] = metric_distance_threshold, nocs_distance_threshold (the reference's Python floats)
 *   ws         sdfr_ransac_ws_bytes(B, ncap, T) bytes
 * outputs:  found[b] (0 = the reference returns None: ncnt < 5, fewer than 5 best inliers, or a rank-deficient final procrustes),
 *   best[b] (winning hypothesis, -1 if none), n_inliers[b], scale[b], rot [B][3][3], tra [B][3];
 *   cnn_idx [B][ncap] nearest model colour per scene point; gate [B][T] bit 0 colour gate passed, bit 1 fit accepted (scored),
 *   bit 2 rank-deficient sample (s2/s1 < 1e-3); counts [B][T] inlier count per scored hypothesis, -1 otherwise.
 * A scene point with a NaN or infinite coordinate (the reference's SVD would raise on a sample that holds one) is nobody's inlier, and a
 * hypothesis that samples it is scored with 0 inliers (gate 7, count 0) or, type 1 only, rejected by the rank rule (gate 5, count -1);
 * every other hypothesis, and with it the winner and the pose, is what it would be with that point far from the model. */
int sdfr_ransac_pose(const float* model, const float* model_cls, const int32_t* mcnt, int mcap, int model_f16, const float* scene,
                     const float* scene_cls, const int32_t* ncnt, int ncap, int B, const int32_t* idx, int64_t seed, const int64_t* keys,
                     int T, int type, float scale_model, const double* h_thr, void* ws, int32_t* found, int32_t* best, int32_t* n_inliers,
                     float* scale, float* rot, float* tra, int32_t* cnn_idx, int32_t* gate, int32_t* counts, int32_t* idx_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Box overlaps of the evaluator  --  replace pipelines/rotate_iou.py (numba.cuda) of the reference.
 *
 * Pair (n, k) of boxes [N] x query boxes [K] goes to out[n][k] (row-major, K fastest).  All pointers are DEVICE pointers of the current
 * device.  Dense mode: G == 0, boff / qoff / ooff NULL, out holds out_len >= N * K elements.  Grouped mode (G > 0): group g holds boxes
 * [boff[g], boff[g+1]) and query boxes [qoff[g], qoff[g+1]) (int32[G + 1] each, non-decreasing, within N and K); only pairs inside a group
 * are evaluated and group g's block is written row-major at out + ooff[g] (int64[G + 1], out_len elements in all).  A group whose offsets
 * are out of range or whose block does not fit in out_len writes nothing.  N == 0 or K == 0 launches nothing.  No synchronisation.
 *
 * criterion: -1 IoU; 0 intersection / area of the QUERY box (BEV) -- the reference evaluates devRotateIoUEval(qboxes[k], boxes[n]);
 * 1 intersection / area of the box; any other value: the intersection itself.
 */
/* rotated BEV IoU, float32 boxes [x, y, dx, dy, angle] (rotate_iou.py:22-286); out float32 */
int sdfr_rotate_iou(const float* boxes, int N, const float* qboxes, int K, int G, const int32_t* boff, const int32_t* qoff,
                    const int64_t* ooff, int criterion, float* out, int64_t out_len, void* stream);
/* 3-D IoU, float64 boxes [x, y, z, d0, d1, d2, ry]: the BEV intersection (criterion 2) of columns [0, 2, 3, 5, 6] (camera_frame != 0) or
 * [0, 1, 3, 4, 6] in float32, then d3_box_overlap_kernel (rotate_iou.py:328-355) in float64 rounded to float32; here criterion 0 divides
 * by the BOX's volume and 1 by the query box's, as that kernel does.  rinc: NULL (the BEV intersection is computed), or the caller's
 * float32 BEV intersections laid out as out (d3_box_overlap_kernel on given rinc; may be out itself).  out float32 */
int sdfr_box3d_iou(const double* boxes, int N, const double* qboxes, int K, int G, const int32_t* boff, const int32_t* qoff,
                   const int64_t* ooff, int criterion, int camera_frame, const float* rinc, float* out, int64_t out_len, void* stream);
/* axis-aligned image-box IoU, float64 [x1, y1, x2, y2] (image_box_overlap, rotate_iou.py:358-379; no +1 pixel convention); criterion 0
 * divides by the box's area, 1 by the query box's; out float64 */
int sdfr_image_box_iou(const double* boxes, int N, const double* qboxes, int K, int G, const int32_t* boff, const int32_t* qoff,
                       const int64_t* ooff, int criterion, double* out, int64_t out_len, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluator statistics  --  replace compute_statistics_jit, get_thresholds, fused_compute_statistics (numba CPU JIT) and scipy's cdist of
 * the reference's pipelines/detection_3d.py.  All pointers are DEVICE pointers of the current device; nothing synchronises.
 *
 * Packed dataset of G frames: frame f holds detections [doff[f], doff[f+1]) of ND and ground truths [goff[f], goff[f+1]) of NG (int32[G + 1]
 * each) and its match degrees as a row-major block [nd][ng] (detection major, like out[n][k] of the box overlaps with boxes = detections)
 * at overlaps + ooff[f] (int64[G + 1], ov_len elements in all); ov_f32 != 0: float32 values (BEV, 3-D), converted to float64 before they
 * are compared, else float64 (image boxes, distances).  A frame whose offsets are out of range contributes nothing.
 * Columns: dt_score, dt_yaw, dt_alpha [ND], gt_yaw, gt_alpha [NG], dt_bbox [ND][4], all float64.
 * Combination c = ml * K + k of ML (class, difficulty) pairs and K overlap levels: flags ign_dt int8[ML][ND] and ign_gt int8[ML][NG]
 * (-1 other class, 0 valid, 1 ignored), min_overlap float64[ML * K] (for the distance metric minus the distance threshold; every test
 * is a strict >).  max_nd: the largest detection count of a frame, frames_per_chunk: 0 for the default; both size the workspace.
 */
/* bytes of the workspace `ws` of sdfr_eval_match_scores, sdfr_eval_thresholds and sdfr_eval_pr (one buffer serves the three calls in
 * turn) for C = ML * K combinations and S sample points; -1 on bad sizes */
int64_t sdfr_eval_ws_bytes(int G, int NG, int C, int S, int max_nd, int frames_per_chunk);
/* out[ooff[f] + j * ng + i] = -sqrt(dx * dx + dy * dy) (float64; squares summed in this order, one square root) of detection j and ground
 * truth i of frame f; loc float64 [n][3], columns (0, 2) if camera_frame != 0, else (0, 1) */
int sdfr_eval_center_dist(const double* dt_loc, int ND, const double* gt_loc, int NG, int G, const int32_t* doff, const int32_t* goff,
                          const int64_t* ooff, int camera_frame, double* out, int64_t out_len, void* stream);
/* pass A: the greedy matching without score threshold (highest score above min_overlap wins, the first on a tie).  out float64[ML * K][NG]:
 * the matched detection's score at every true positive's ground truth, NaN elsewhere; every element of a frame in range is written */
int sdfr_eval_match_scores(const void* overlaps, int ov_f32, int64_t ov_len, const int64_t* ooff, const int32_t* doff, const int32_t* goff,
                           int G, int ND, int NG, const double* dt_score, const int8_t* ign_dt, const int8_t* ign_gt, int ML, int K,
                           const double* min_overlap, int max_nd, void* ws, int64_t ws_bytes, double* out, void* stream);
/* get_thresholds per combination: row c of scores (float64[ML * K][NG], NaN = no score: the output of sdfr_eval_match_scores) is
 * compacted and sorted descending in ws, then walked against num_gt[c / K] valid ground truths (int64[ML]) with the reference's float64
 * recall arithmetic -> thr float64[ML * K][S] (zero past the count), nthr int32[ML * K] <= S, count int32[ML * K] (scores per row; may
 * be NULL).  One launch whatever NG is */
int sdfr_eval_thresholds(const double* scores, int NG, const int64_t* num_gt, int ML, int K, int S, void* ws, int64_t ws_bytes, double* thr,
                         int32_t* nthr, int32_t* count, void* stream);
/* pass B: for every combination c and threshold t < nthr[c] the matching of every frame among the detections with score >= thr[c][t]
 * (highest overlap wins), summed over the frames: pr float64[ML * K][S][7] = tp, fp, fn, yaw error, orientation similarity, match degree,
 * -log(score); rows t >= nthr[c] are zero.  angular == 0: columns 3 and 4 stay zero (the yaw / alpha pointers may be NULL).  dc_off
 * int32[ML][G + 1] into dc_boxes float64[NDC][4]: the DontCare boxes of (ml, frame) for the 2-D metric's rule (an unassigned detection
 * whose intersection with one of them over its OWN area exceeds min_overlap is no false positive); NULL: no such rule.  Frames are summed
 * in chunks of frames_per_chunk and the chunks in order: the same inputs give the same bits on every device */
int sdfr_eval_pr(const void* overlaps, int ov_f32, int64_t ov_len, const int64_t* ooff, const int32_t* doff, const int32_t* goff, int G,
                 int ND, int NG, const double* dt_score, const double* dt_yaw, const double* dt_alpha, const double* gt_yaw,
                 const double* gt_alpha, const double* dt_bbox, const int8_t* ign_dt, const int8_t* ign_gt, const double* dc_boxes,
                 int NDC, const int32_t* dc_off, int ML, int K, const double* min_overlap, const double* thr, const int32_t* nthr,
                 int S, int angular, int max_nd, int frames_per_chunk, void* ws, int64_t ws_bytes, double* pr, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Frame labelling (csrc/frame.hip): the per-annotation glue of pipelines/refine_css.py:130-196 and utils/refinement.py:501-562 for a
 * frame's annotations at once.
 */
/* reproject (utils/refinement.py:360-410, torch branch) of B depth crops packed one behind the other:
 *   meta int32[B][4] = (W, H, index of the crop's first pixel in depth, colour layout: 1 = [3][H][W], 0 = [H][W][3]); the crop's colours start
 *   at color + 3 * that index.  max_pix >= every W * H.  kinv [B][9] = inverse(K) of the crop, inverted by the caller.
 *   Kept: the pixels with depth != 0 and, if filter != 0, some colour channel > 0, in row-major order (y outer, x inner):
 *     points[b][s] = (kinv [x, y, 1]) * depth, colors[b][s] = the pixel's colour      ([B][cap][3] each)
 *   cnt[b] = the TRUE number of kept pixels; beyond cap nothing is written and over[b] |= over_bit (sticky; over may be NULL).
 *   scratch: int32[B * ceil(max_pix / 256)]. */
int sdfr_reproject(const float* depth, const float* color, const int32_t* meta, const float* kinv, int B, int max_pix, int filter, int cap,
                   float* points, float* colors, int32_t* cnt, int32_t* scratch, int32_t* over, int over_bit, void* stream);
/* Segmented extents: for list b < B of n_b points, p' = A_b (s_b p) + t_b in float32 (each product and sum rounded separately),
 *   ext[b][0..6)  = min x, max x, min y, max y, min z, max z of p'
 *   ext[b][6..10) = min u, max u, min v, max v of u = fx x'/z' + cx, v = fy y'/z' + cy (K_b [9], no distortion); NaN when K == NULL
 *   n_out[b] = n_b; an empty list reports NaN extents.
 * List b starts at pts + 3 * off[b] (off int64[B]) and holds cnt[b] points, or (off == NULL) is row b of a [B][cap][3] array holding
 * min(cnt[b], cap) points (cnt == NULL: cap).  With off given, cap bounds every count.  A [B][9], scale [B], t [B][3], K [B][9]: each may be
 * NULL (identity, 1, 0, no projection).  flags & 1: the points and the scale are float16 values and s p is rounded to float16
 * (a float16 cloud times a float16 scale, utils/refinement.py:541). */
int sdfr_point_extents(const float* pts, const int64_t* off, const int32_t* cnt, int cap, int B, const float* A, const float* scale,
                       const float* t, const float* K, int flags, float* ext, int32_t* n_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Frame ingest (csrc/ingest.hip): what pipelines/refine_css.py:101-138 does on the host before a crop exists.
 */
/* compute_depth_map (utils/refinement.py:87-105).  lidar [N][3] in the camera frame, device memory, float64 (lidar_f64 != 0) or float32.
 *   planes: HOST float[4][3], the rows of build_view_frustum(K, 0, 0, w, h); cam: HOST double[4] = fx, fy, cx, cy.  Both are read at the call.
 *   A point is kept when all four plane . p > 0 (float64); its pixel is x = (int)(float)(fx (X / Z) + cx), y likewise (float64 pinhole
 *   rounded to float32, truncated toward zero).  A kept point outside [0, w) x [0, h) is dropped and counted.
 *   winner int32[h][w] = the largest index of the kept points on the pixel, -1 without one (an integer atomic maximum: the LAST point in
 *   input order wins, as the reference's loop overwrites); depth float[h][w] = (float)Z of the winner, 0 without one.
 *   info int32[2] = { points that landed on a pixel, kept points dropped for lying outside the image }.  Three launches. */
int sdfr_depth_map(const void* lidar, int lidar_f64, int N, const float* planes, const double* cam, int w, int h, float* depth,
                   int32_t* winner, int32_t* info, void* stream);
/* sdfr_depth_map over the points with mask[i] != 0 (uint8 [N], device memory): the depth map of the cloud without the others.  winner holds
 * indices into the WHOLE cloud and the last kept point in input order wins, so the image equals sdfr_depth_map of the compacted cloud.
 * This is how get_kitti_frame's road-removed map is rasterised without a compaction (and without a host synchronisation).  Three launches. */
int sdfr_depth_map_masked(const void* lidar, int lidar_f64, int N, const uint8_t* mask, const float* planes, const double* cam, int w, int h,
                          float* depth, int32_t* winner, int32_t* info, void* stream);
/* The box matching of refine_css.py:101-114: anno double[A][4], det double[M][4] as [x1, y1, x2, y2].  Per annotation a:
 *   iou[a] = the largest get_iou(det[m], anno[a]) (utils/refinement.py:128-165: 0 when width < 0 or height < 0, divisor + 1e-5), float64;
 *   best[a] = the FIRST m that attains it (np.argmax), -1 when M == 0; keep[a] = (iou[a] >= 0.5).  One launch. */
int sdfr_match_boxes(const double* anno, int A, const double* det, int M, int32_t* best, double* iou, int32_t* keep, void* stream);
/* transform_bgr_crop (utils/refinement.py:60-84) for A boxes of one frame image [H][W][3] (float32 BGR, 0 ... 1, device memory).
 *   meta int32[A][8] = { l, t, crop width, crop height, index of the crop's first mask element in masks or -1, first row of the crop in
 *   tmp, first workgroup of the crop in the horizontal pass, 0 }: rows are counted one crop behind the other (sum of the heights so far),
 *   workgroups likewise with ceil(height / 8) per crop; n_hblocks is their total.  Boxes must lie inside the image.
 *   masks: float [height][width] per masked crop, multiplied into the crop in float32 first (refine_css.py:135); may be NULL.
 *   Per pixel: uint8(trunc(v * 255.0f)), BGR -> RGB, Pillow's 8-bit bilinear resample to 128 x 128 (horizontal pass over all rows, vertical
 *   pass over its uint8 result, coefficients in double rounded to 22-bit integers), then
 *     im_orig [A][3][128][128] = float(u8) / 255.0f          im [A][3][128][128] = (im_orig - mean) / std      u8 [A][128][128][3]
 *   each of the three may be NULL.  ksize >= 2 * ceil(max(largest crop extent / 128, 1)) + 1 (Pillow's ksize).
 *   Workspaces: coef int32[A][2][128][2 + ksize], tmp uint8[total rows][128][3].  Three launches. */
int sdfr_css_input(const float* image, int H, int W, const int32_t* meta, int A, const float* masks, int ksize, int n_hblocks,
                   int32_t* coef, uint8_t* tmp, float* im, float* im_orig, uint8_t* u8, void* stream);

/* Augmentation of a ragged batch of B training crops (csrc/augment.hip): what datasets/crops.py asks of Pillow through torchvision's PIL
 * backend -- ColorJitter in a given order, rotate(angle, expand=True), resize to 128 x 128, crop((j, i, j + w, i + h)), resize to 128 x 128,
 * ToTensor / Normalize; bilinear for the RGB image, nearest for the UVW label image -- byte for byte for the given parameters.
 *   rgb_src, uvw_src: the uint8 [h_b][w_b][3] images of all samples, one behind the other (device memory, the same layout for both).
 *   meta int32[B][8] = { h, w, index of the sample's first pixel in the packed sources, width and height of the rotated image
 *   (Image.rotate's expanded size), 1 when angle % 360 == 0 (Pillow copies), 0, 0 }.
 *   params float64[B][SDFR_AUG_PARAMS]: the factors Image.blend receives for brightness, contrast and saturation; the hue factor (0 skips
 *   the step); the four operation ids (0 brightness, 1 contrast, 2 saturation, 3 hue) in the order applied; the six entries of
 *   Image.rotate's re-centred affine matrix (host float64 arithmetic); the crop box i (top), j (left), h, w inside the intermediate.
 *   ksize >= 2 * ceil(max(largest rotated extent / 128, 1)) + 1.
 *   Workspaces: tab int32[B][4][128][3 + ksize], jit uint8[source pixels][3], mid_rgb and mid_uvw uint8[B][128][128][3].
 *   Outputs: rgb float[B][3][128][128], uvw uint8[B][3][128][128], mask uint8[B][128][128] = (u + v + w > 0); rgb_u8 uint8[B][128][128][3],
 *   the image before ToTensor, may be NULL.  After the call jit holds the images after the colour jitter.
 *   Four launches whatever B; no atomics; a sample's results depend on its own rows alone. */
#define SDFR_AUG_PARAMS 20
#define SDFR_AUG_BRIGHTNESS 0
#define SDFR_AUG_CONTRAST 1
#define SDFR_AUG_SATURATION 2
#define SDFR_AUG_HUE 3
#define SDFR_AUG_ORDER 4
#define SDFR_AUG_MATRIX 8
#define SDFR_AUG_BOX_I 14
#define SDFR_AUG_BOX_J 15
#define SDFR_AUG_BOX_H 16
#define SDFR_AUG_BOX_W 17
int sdfr_augment(const uint8_t* rgb_src, const uint8_t* uvw_src, const int32_t* meta, const double* params, int B, int ksize, int32_t* tab,
                 uint8_t* jit, uint8_t* mid_rgb, uint8_t* mid_uvw, float* rgb, uint8_t* uvw, uint8_t* mask, uint8_t* rgb_u8, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Lidar normals (csrc/normals.hip): the normal estimation behind get_kitti_frame's road-plane removal (utils/refinement.py:628-644).
 * The semantics are this library's own, written from Open3D's EstimateNormals / KDTreeFlann::SearchHybrid; Open3D is not installed where
 * this was developed, so parity with it is NOT tested.
 */
/* points [N][3] in the camera frame, device memory, float64 (points_f64 != 0) or float32 (widened first).  planes: HOST float[4][3], the rows
 * of build_view_frustum(K, 0, 0, W, H), read at the call; NULL: every point is in the frustum.
 *   in_frustum uint8[N]: all four planes . p > 0 (float32 planes, float64 products, as sdfr_depth_map).  Only frustum points are queries and
 *     only frustum points can be neighbours.
 *   neighbours of i: the frustum points j (i itself included) with d2 = (dx*dx + dy*dy) + dz*dz < radius*radius, strictly, in float64 (the
 *     radius is a float32 value, widened: 1.0 and 0.5 are exact);
 *     ordered by (d2, j) ascending, the first max_nn (1 ... 64) kept -- a tie at the cut goes to the lower index.  No cap on candidates.
 *   nn_count int32[N]; nn_idx int32[N][max_nn] in that order, padded with -1 (NULL: not written).
 *   normals double[N][3]: with fewer than 3 neighbours (0, 0, 1); else mean and centred covariance C = (1 / k) sum (q - m)(q - m)^T in float64,
 *     summed in neighbour order, and the unit eigenvector of C's smallest eigenvalue (cyclic Jacobi); C == 0: (0, 0, 1).  Sign: n . p <= 0
 *     (towards the camera); a product of exactly 0 keeps the solver's sign.  Outside the frustum: (0, 0, 1), count 0.
 * The same bits on every run; a point's result does not depend on its place in the array apart from the tie rule; no float atomic.
 * workspace: sdfr_lidar_normals_ws_bytes(N) bytes of device memory, 16-byte aligned (-1: N out of range; N <= 2^28).  N == 0: success,
 * nothing written.  Five launches, no host synchronisation. */
int64_t sdfr_lidar_normals_ws_bytes(int N);
int sdfr_lidar_normals(const void* points, int points_f64, int N, const float* planes, float radius, int max_nn, double* normals,
                       int32_t* nn_count, int32_t* nn_idx, uint8_t* in_frustum, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The CSS network's output head (csrc/css_head.hip): networks/resnet_css.py:194-196 and :203-249 of the reference, inference only.
 */
/* Features x_u, x_v, x_w, x_mask: contiguous float32 NCHW [B][C][H][W] with C == 64 (anything else is refused).  Weights w_* [256][64] with
 * biases b_* [256] of out_u / out_v / out_w, w_mask [2][64] with b_mask [2] of out_mask.  Per pixel, with logit = W x + b (exact-f32 MFMA,
 * k = 0 ... 63 in order, the bias last):
 *   uvw_sm        [B][3][H][W]  sum_k k softmax_k(100 logit) per colour head (the maximum is subtracted before exp)
 *   mask          [B][2][H][W]  the raw mask logits
 *   mask_sm       [B][1][H][W]  softmax(100 mask)[1]
 *   uvw_sm_masked [B][3][H][W]  uvw_sm where mask[1] > mask[0], else 0 (a tie is background, as argmax returns the first index)
 *   u, v, w       [B][256][H][W] log_softmax(logit); all three NULL: not computed
 * A pixel's result does not depend on B, on its neighbours or on the launch.  B == 0 or H * W == 0: success, nothing written.  One launch
 * on `stream`; the tensors must live on the current device. */
int sdfr_css_head(const float* x_u, const float* x_v, const float* x_w, const float* x_mask, int B, int C, int H, int W, const float* w_u,
                  const float* b_u, const float* w_v, const float* b_v, const float* w_w, const float* b_w, const float* w_mask,
                  const float* b_mask, float* uvw_sm, float* uvw_sm_masked, float* mask, float* mask_sm, float* u, float* v, float* w,
                  void* stream);
/* out_lat on x4 [B][C][h][w] (C == 256): the 1x1 convolution w_lat [3][256], b_lat [3] per pixel, the mean over the h * w pixels, then
 * latent[b] = v * (1 / (|v| + 1e-8)) (project_vecs_onto_sphere, radius 1).  One workgroup per crop, fixed-order sums.  latent [B][3]. */
int sdfr_css_latent(const float* x4, int B, int C, int h, int w, const float* w_lat, const float* b_lat, float* latent, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training the CSS head (csrc/css_train.hip): the losses of pipelines/train_css.py:71-80 of the reference and their gradients for UNIT
 * upstream gradient.  Nothing 256 channels wide is written to global memory, no atomics: the same bits in every run.
 */
#define SDFR_CSS_LOSS_WS_FIXED 16045824ll   /* bytes of the head loss's workspace that do not depend on the input: the workgroups' partials */
/* Inputs as sdfr_css_head, plus uvw_gt uint8 [B][3][H][W] and mask_gt uint8 [B][H][W] (nonzero: foreground).  With N = B H W, m = mask_gt != 0,
 * t_h = uvw_gt[:, h] m and z_h the logits of head h:
 *   loss[0..2] = (1/N) [ sum_{m=1} (logsumexp(z_h) - z_h[t_h]) + (N - n_fg) ln 256 ]     (CrossEntropyLoss(log_softmax(z_h) * m, t_h))
 *   loss[3]    = 2 CrossEntropyLoss(z_mask, m)
 *   dx_* [B][64][H][W], dw_u/v/w [256][64], db_u/v/w [256], dw_mask [2][64], db_mask [2]: the gradients of the head's own loss; dx_u/v/w are
 *   exactly 0 at background pixels.
 * workspace: device memory of at least SDFR_CSS_LOSS_WS_FIXED + 12 N bytes (8-byte aligned); the call fails with -1 and names the size otherwise.
 * B == 0 or H * W == 0: success, nothing written.  Four launches on `stream`. */
int sdfr_css_head_loss(const float* x_u, const float* x_v, const float* x_w, const float* x_mask, int B, int C, int H, int W, const float* w_u,
                       const float* b_u, const float* w_v, const float* b_v, const float* w_w, const float* b_w, const float* w_mask,
                       const float* b_mask, const uint8_t* uvw_gt, const uint8_t* mask_gt, float* loss, float* dx_u, float* dx_v, float* dx_w,
                       float* dx_mask, float* dw_u, float* db_u, float* dw_v, float* db_v, float* dw_w, float* db_w, float* dw_mask,
                       float* db_mask, void* workspace, int64_t workspace_bytes, void* stream);
/* loss[0] = mean over B * 3 of (lat - latent_gt)^2 with lat = v / (|v| + 1e-8), v = w_lat mean_p(x4) + b_lat; the length is a constant of the
 * backward, as in the reference (project_vecs_onto_sphere detaches it): dv = 2 (lat - gt) / (3 B) / (|v| + 1e-8), dx4[b][c][p] =
 * (w_lat^T dv_b)[c] / (h w), dw_lat [3][256] = sum_b dv_b (x) mean_p x4_b, db_lat [3] = sum_b dv_b, crops summed in order.  latent_gt float32
 * [B][3].  workspace: at least B * 3092 bytes of device memory (8-byte aligned).  Two launches. */
int sdfr_css_latent_loss(const float* x4, int B, int C, int h, int w, const float* w_lat, const float* b_lat, const float* latent_gt,
                         float* loss, float* dx4, float* dw_lat, float* db_lat, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * Triangle meshes of SDF samples on a regular lattice (csrc/mesh.hip; no counterpart in the reference, which never leaves the shape as
 * geometry).  Marching tetrahedra on the Kuhn subdivision -- six tetrahedra per cell walking from corner 000 to 111 one axis at a time, in
 * the order of the permutations of (x, y, z) --, the vertices shared between triangles welded.  DESIGN.md ("Meshes") states the rules.
 *   lattice   R points per axis, 2 <= R <= 256, x_i = float32(-1 + 2 i / (R - 1)) evaluated in float64, row = (ix R + iy) R + iz;
 *             B * R^3 < 2^31
 *   inside    sdf < 0; an exact 0 and a NaN are outside
 *   vertices  one per lattice edge p -> p + d (d in {0,1}^3 \ 0, the class: d as a binary number with x the high bit) whose ends differ,
 *             at p_a + t (p_b - p_a) with t = s_a / (s_a - s_b), float32, multiply and add rounded separately (a NaN t becomes 1/2); ordered
 *             by (row of p, class)
 *   triangles ordered by (row of the cell's low corner, tetrahedron, triangle), wound so that the normal points from inside to outside;
 *             indices are local to the shape.  Triangles of zero area (exact zeros at lattice points) are kept; a surface that leaves the
 *             cube stays open there.
 * No atomics: the same bits on every run, and a shape's output does not depend on the batch around it.
 */
/* bytes of the workspace of the count / emit pair for B shapes (-1: R or B out of range) */
int64_t sdfr_mesh_ws_bytes(int R, int B);
/* inputs[b][j][:] = latents[b][0..L) || xyz of lattice row row0 + j, for b < B, j < nrows: the decoder's input rows of a chunk of the lattice.
 * latents [B][L], inputs [B][nrows][L + 3]. */
int sdfr_mesh_lattice_inputs(const float* latents, int L, int R, int B, int64_t row0, int64_t nrows, float* inputs, void* stream);
/* sdf [B][R^3] -> nv[b], nt[b] (device int32): shape b's vertex and triangle counts.  The workspace keeps the per-point records and the
 * scanned block offsets for the emit call.  Two launches, no host synchronisation. */
int sdfr_mesh_count(const float* sdf, int R, int B, int32_t* nv, int32_t* nt, void* workspace, int64_t workspace_bytes, void* stream);
/* vertices [cap_v][3] float32 (lattice frame) and faces [cap_t][3] int32 of all shapes: shape b's at voff[b] .. voff[b + 1] and
 * toff[b] .. toff[b + 1].  voff, toff: HOST int64 [B + 1], the exclusive sums of the counts the caller read after the count call over the
 * same sdf and workspace.  Fails before any launch if voff[B] > cap_v or toff[B] > cap_t, and never writes outside a shape's own range.  The
 * offsets travel to the device in two small copies, so the call cannot be captured in a graph. */
int sdfr_mesh_emit(const float* sdf, int R, int B, const int64_t* voff, const int64_t* toff, void* workspace, int64_t workspace_bytes,
                   float* vertices, int64_t cap_v, int32_t* faces, int64_t cap_t, void* stream);

/*
 * Verification of refined autolabels (csrc/verify.hip; the reference's published code stops before this stage).  DESIGN.md ("Verification")
 * states the rules; csrc/verify_cells.h is the arithmetic, which also compiles for the host.  All pointers are device pointers except K.
 *
 * sdfr_mesh_raster: B ragged camera-frame meshes, each rendered into its own window of a W x H image.
 *   vertices float32 [V][3], faces int32 [T][3] with indices local to the mesh, voff / toff int64 [B + 1] the meshes' vertex and triangle
 *   offsets, windows int32 [B][4] the half-open integer windows l, t, r, b inside the image (an empty one is legal), poff int64 [B + 1] the
 *   windows' pixel offsets: poff[b + 1] - poff[b] = (r - l)(b - t), pixel (x, y) of window b at poff[b] + (y - t)(r - l) + (x - l).
 *   K: HOST double[4] = fx, fy, cx, cy.  z_min >= 0.
 *   projection   float64 from the float32 vertex: u = fx (X / Z) + cx, v = fy (Y / Z) + cy, every operation rounded separately
 *   sample       pixel (x, y) is sampled at the point (x, y)
 *   coverage     E_i = (a.u - x)(b.v - y) - (a.v - y)(b.u - x) for the edge (a, b) opposite vertex i, A2 = (u1 - u0)(v2 - v0) - (v1 - v0)(u2 - u0);
 *                covered when A2 != 0 and all E_i sign(A2) >= 0: inclusive edges, both windings
 *   depth        S = (E0 + E1) + E2, depth = (float)(S / ((E0 / Z0 + E1 / Z1) + E2 / Z2)); a depth that is not a positive finite float is no cover
 *   winner       the minimum of (bits(depth) << 32) | triangle index: nearest, and on an exact tie the lowest index
 *   skipped      a triangle with a non-finite vertex or projection; one with a vertex at Z <= z_min (flag bit 0); one with a face index outside
 *                its mesh (flag bit 1).  A mesh whose window leaves the image or does not match its pixel offsets is skipped whole (flag bit 1).
 *   outputs      per window pixel mask uint8 (0 / 1), depth float32 (0 where uncovered), triangle int32 (-1 where uncovered), each [P];
 *                flags int32 [B].  keys: workspace of 8 P bytes (8-byte aligned).
 * The pixel box of a triangle is clamped to the window in floating point before it becomes integers: no vertex value gives a write or a loop
 * outside the window.  Integer atomic minimum on the keys, then a resolve launch: the same bits on every run.  Three launches, no memset.
 */
int sdfr_mesh_raster(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const int64_t* voff, const int64_t* toff,
                     const int32_t* windows, const int64_t* poff, int64_t P, int B, int W, int H, const double* K, float z_min, void* keys,
                     uint8_t* mask, float* depth, int32_t* triangle, int32_t* flags, void* stream);
/* counts int32 [B][8] per window: covered area; the tight half-open box l, t, r, b of the covered pixels (zeros for none); the label's area and
 * the intersection area (zeros when label_mask, uint8 [P] laid out like mask, is NULL); flag bit 1 if the window is unusable (then all zeros).
 * One workgroup per window, integer sums. */
int sdfr_verify_mask_counts(const uint8_t* mask, const uint8_t* label_mask, const int32_t* windows, const int64_t* poff, int64_t P, int B, int W,
                            int H, int32_t* counts, void* stream);
/* The decoder's input rows of camera-frame lidar points: rows[j] = latents[a] || x for point row0 + j, a its annotation, j < nrows.
 * points float32 [N][3], ptoff int64 [B + 1] the annotations' point offsets (ptoff[0] = 0, ptoff[B] = N), pose float32 [B][6] = cos(yaw),
 * sin(yaw), trans x y z, scale (the label's own float32 values), latents [B][L] (raw).  x = diag(1, -1, 1) rot_yaw^T (p / scale - trans) in
 * float64, rounded once to float32: the inverse of Mesh.to_camera / assemble_labels.  in_cube uint8 [N]: 1 when x lies in [-1, 1]^3. */
int sdfr_verify_point_rows(const float* points, int64_t N, const int64_t* ptoff, int B, const float* pose, const float* latents, int L,
                           int64_t row0, int64_t nrows, float* rows, uint8_t* in_cube, void* stream);
/* counts int32 [B][3] = n_pts, n_cube, n_band per annotation from the decoder's values sdf [N] at those rows: a point is in the band when it
 * is in the cube and fabsf(sdf) * scale < band in float32.  One workgroup per annotation, integer sums. */
int sdfr_verify_band_counts(const float* sdf, const uint8_t* in_cube, int64_t N, const int64_t* ptoff, int B, const float* pose, float band,
                            int32_t* counts, void* stream);

/*
 * Export of CSS training crops from rasterised autolabels (csrc/crops.hip; DESIGN.md "Training crops").  csrc/crop_cells.h is the
 * arithmetic, which also compiles for the host.  All pointers are device pointers except K.  windows / poff / P, voff / toff, K and z_min are
 * sdfr_mesh_raster's, and mask / depth / triangle its packed outputs.
 *
 * sdfr_crop_owner: owner int32 [P] per window pixel of a frame's B rasters: -1 where the annotation's own mask does not cover, its own index
 *   where it is the nearest there, otherwise the index of the nearest occluder.  The key of annotation b at a pixel is
 *   (bits(depth) << 32) | b and the minimum wins: the nearest, and on an exact tie the lowest index.  An annotation counts at a pixel only if
 *   its window contains the pixel and its mask covers it there: AN OCCLUDER IS SEEN ONLY INSIDE ITS OWN WINDOW.  A window that leaves the
 *   image or does not match its offsets is ignored and its pixels get -1.  One launch.
 */
int sdfr_crop_owner(const uint8_t* mask, const float* depth, const int32_t* windows, const int64_t* poff, int64_t P, int B, int W, int H,
                    int32_t* owner, void* stream);
/* Per annotation a half-open box l, t, r, b (boxes int32 [B][4]) inside its window; outputs packed by qoff int64 [B + 1], the exclusive sum of
 * the box areas (Q = qoff[B]): box pixel (x, y) of annotation b at qoff[b] + (y - t)(r - l) + (x - l).
 *   uvw uint8 [Q][3]   where the pixel's winning triangle is not -1 and (owner is NULL or owner == b): with E_i the rasteriser's edge values of
 *                      the winning triangle at the pixel, q_i = E_i / Z_i, D = (q0 + q1) + q2, n_k = (q0 a0[k] + q1 a1[k]) + q2 a2[k] (float64,
 *                      every operation rounded separately), val = (n_k / D + 1) 127.5 -> 0 for val <= 0 or NaN, 255 for val >= 255, else
 *                      rint(val); three zero bytes become (0, 0, 1).  a_i: attributes float32 [V][3] at the triangle's vertices (the
 *                      lattice-frame positions: NOCS).  Zeros elsewhere.  owner == NULL: occlusion off.
 *   rgb uint8 [Q][3]   optional (rgb and colors both or neither): colors float32 [Q][3] is the annotation's BGR colour crop packed the same
 *                      way; the bytes are rintf(255 v) in float32 clamped to 0 ... 255 (NaN: 0), written in RGB order.
 *   flags int32 [B]    VERIFY_FLAG_INVALID (2) for an annotation whose window leaves the image, whose box leaves its window, whose offsets do
 *                      not fit the arrays, or whose triangle image holds an index outside the mesh other than -1 (or a triangle the
 *                      rasteriser would have skipped); all pixels of such an annotation are zeroed.
 * Nothing is read or written out of bounds for any values in the arrays.  Three launches, no memset, no host synchronisation. */
int sdfr_crop_export(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const float* attributes, const int64_t* voff,
                     const int64_t* toff, const int32_t* windows, const int64_t* poff, int64_t P, const int32_t* triangle, const int32_t* owner,
                     const int32_t* boxes, const int64_t* qoff, int64_t Q, const float* colors, int B, int W, int H, const double* K, float z_min,
                     uint8_t* uvw, uint8_t* rgb, int32_t* flags, void* stream);
/* counts int32 [B][4] per annotation: box pixels, covered (mask != 0 inside the box), visible (covered and owner == b; owner NULL: all covered),
 * and the flag word: flags[b] (sdfr_crop_export's, may be NULL) or-ed with bit 1 if window and box do not fit, in which case the three
 * counts are 0.  One workgroup per annotation, integer sums in a fixed tree. */
int sdfr_crop_counts(const uint8_t* mask, const int32_t* owner, const int32_t* windows, const int64_t* poff, int64_t P, const int32_t* boxes,
                     const int64_t* qoff, int64_t Q, const int32_t* flags, int B, int W, int H, int32_t* counts, void* stream);

/*
 * Synthetic bootstrap crops: colour images of posed shapes of the prior (csrc/synth.hip; DESIGN.md "Synthetic crops").  csrc/synth_cells.h is
 * the arithmetic, which also compiles for the host.  All pointers are device pointers except K.  The NOCS image of such a crop is
 * sdfr_crop_export's (colors NULL) and its counts are sdfr_crop_counts', both fed sdfr_synth_owner's owner image.
 *
 * sdfr_synth_owner: sdfr_crop_owner with scene int32 [B]: annotation c can own a pixel of annotation b only when scene[c] == scene[b], so
 *   that several scenes -- different images sharing K and the image size -- go through one launch.  scene == NULL: sdfr_crop_owner's bits.
 */
int sdfr_synth_owner(const uint8_t* mask, const float* depth, const int32_t* windows, const int64_t* poff, int64_t P, const int32_t* scene, int B,
                     int W, int H, int32_t* owner, void* stream);
/* rgb uint8 [Q][3], packed as sdfr_crop_export packs uvw.  Box pixel (x, y) of annotation b in scene s = scene[b] (0 for scene == NULL): with
 * c = owner[b's window pixel], if c is an annotation of scene s whose window holds (x, y) and whose winning triangle there is not -1, the
 * pixel is that triangle shaded, in float64 with every operation rounded separately and dot products summed left to right:
 *   weights q_i = E_i / Z_i, D = (q0 + q1) + q2 as sdfr_crop_export; n_k = ((q0 n0k + q1 n1k) + q2 n2k) / D over normals float32 [V][3] (camera
 *   frame); len2 = (n0^2 + n1^2) + n2^2; n = 0 if !(len2 > 0) else n / sqrt(len2); p = ((x - cx) / fx, (y - cy) / fy, 1), v = -(p / sqrt(|p|^2));
 *   light[s] = l x, y, z, ambient, kd (double [S][5], l taken as given); d = max(0, n.l); h = (l + v) / |l + v| (0 if the length is not positive);
 *   s = max(0, n.h) squared shin times; paint[c] = albedo r, g, b, ks, shin (double [B][5]; shin truncated to 0 .. 7);
 *   val_k = albedo_k (ambient + kd d) + ks s; byte = 0 for 255 val <= 0 or NaN, 255 for >= 255, else rint(255 val).
 * Every other box pixel takes the scene's background: the byte of bg uint8 [NBG][H][W][3] (RGB) number bg_index[s] (int32 [S]) if that is in
 * 0 .. NBG - 1, else the procedural one from ramp[s] = top r, g, b, bottom r, g, b, amp, seed (int32 [S][8], colours and amp clamped to 0 .. 255):
 *   clamp(top_k + ((bottom_k - top_k) y) / max(H - 1, 1) + ((hash32(seed, x, y, k) >> 24) amp >> 8) - (amp >> 1), 0, 255), integers only, C
 *   division; hash32 = high half of mix64(seed ^ mix64((x << 33 | y << 2 | k) 0x9E3779B97F4A7C15 + 1)), mix64 the splitmix64 finaliser.
 * flags int32 [B]: VERIFY_FLAG_INVALID (2) for an annotation whose window, box, offsets or scene (outside 0 .. S - 1) do not fit, or one of
 *   whose pixels met a triangle index outside the owner's mesh other than -1 (or a triangle the rasteriser would have skipped); all pixels of
 *   such an annotation are zeroed.  Nothing is read or written out of bounds for any values in the arrays; nothing outside qoff[b] ..
 *   qoff[b + 1] is written for annotation b.  Three launches, no memset, no host synchronisation. */
int sdfr_synth_shade(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const float* normals, const int64_t* voff, const int64_t* toff,
                     const int32_t* windows, const int64_t* poff, int64_t P, const int32_t* triangle, const int32_t* owner, const int32_t* scene,
                     const int32_t* boxes, const int64_t* qoff, int64_t Q, const double* paint, const double* light, int S, const int32_t* bg_index,
                     const uint8_t* bg, int NBG, const int32_t* ramp, int B, int W, int H, const double* K, float z_min, uint8_t* rgb, int32_t* flags,
                     void* stream);

/*
 * Signed distances from query points to triangle meshes, and area-weighted points on their surfaces (csrc/mesh_sdf.hip; DESIGN.md "Signed
 * distances to meshes").  csrc/mesh_sdf_cells.h is the arithmetic -- its comment fixes the component order of every dot and cross product --
 * and also compiles for the host.  All pointers are device pointers.  Meshes are packed as sdfr_mesh_raster takes them: vertices float32
 * [V][3], faces int32 [T][3] with indices local to the mesh, voff / toff int64 [B + 1].
 *
 * sdfr_mesh_sdf: points float32 [N][3] with qoff int64 [B + 1], the run of query points of each mesh.  All pairs of a mesh's points and
 *   triangles, float64 on the float32 values, every operation rounded separately.
 *   distance   d2(p, tri) = min over the three edges of the squared distance to the segment (t = l2 > 0 ? ap.ab / l2 : 0 clamped to [0, 1]) and,
 *              when the triangle has area (nn = n.n > 0, n = (b - a) x (c - a)) and p projects into it (the three edge tests >= 0),
 *              ((p - a).n)^2 / nn.  Zero-area triangles act as segments or points.
 *   nearest    the minimum of d2 over the mesh's triangles, on equal d2 the lowest index; dist = (float) sqrt(d2)
 *   winding    the sum of omega = det == 0 ? 0 : atan2(det, den) / (2 pi) (van Oosterom and Strackee) over the triangles
 *   order      triangles are cut into chunks of 4096 in index order; minimum and sum are taken sequentially inside a chunk (from +inf and
 *              0) and the chunk results are folded in chunk order.  A function of T alone: the launch shape does not change a bit.
 *   sign       inside when want_sign and |winding| >= 0.5; sdf = inside ? -dist : dist.  want_sign = 0 skips the winding pass: the unsigned
 *              distance, for open meshes; winding is then 0.
 *   skipped    a triangle with a non-finite vertex (flag bit 0) or a face index outside its mesh (flag bit 1); a mesh whose vertex or
 *              triangle offsets do not fit the arrays (flag bit 1).  A point of a mesh with no usable triangle, a non-finite point, and a
 *              point outside every usable run of qoff get dist = sdf = +inf, d2 = +inf, nearest = -1, winding = 0.
 *   outputs    sdf float32 [N]; dist float32 [N], d2 float64 [N], nearest int32 [N] (index within the mesh), winding float64 [N]: each of
 *              these four may be NULL; flags int32 [B].
 *   ws         sdfr_mesh_sdf_ws_bytes(B, N, T) bytes, 8-byte aligned (-1: sizes out of range; all of B < 2^24, V, T, N < 2^31).
 * No atomics, no floating-point reduction across lanes: the same bits on every run, and a mesh's results do not depend on B or on its
 * position in the batch.  Two launches (three in the chunk-split shape for few points and many triangles), no memset.
 */
int64_t sdfr_mesh_sdf_ws_bytes(int B, int64_t N, int64_t T);
int sdfr_mesh_sdf(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const int64_t* voff, const int64_t* toff,
                  const float* points, int64_t N, const int64_t* qoff, int B, int want_sign, void* ws, int64_t ws_bytes, float* sdf, float* dist,
                  double* d2, int32_t* nearest, double* winding, int32_t* flags, void* stream);
/* Area-weighted surface points from uniforms the caller drew: uniforms float32 [S][3] in [0, 1) with soff int64 [B + 1] the meshes' sample
 * runs (soff[0] = 0, soff[B] = S, non-decreasing).
 *   area       area_t = sqrt(nn) / 2 in float64, 0 for a skipped triangle.  local = the sequential running sum inside chunks of 256 triangles,
 *              base = the sequential exclusive running sum of the chunk totals, cum[t] = base[t / 256] + local[t].
 *   sample     the triangle is the first t with cum[t] > u0 cum[T - 1] (never one of zero area); s = sqrt(u1), w0 = 1 - s, w1 = s (1 - u2),
 *              w2 = s u2, x_k = (float)((w0 a_k + w1 b_k) + w2 c_k).
 *   outputs    points float32 [S][3], triangle int32 [S] (index within the mesh), flags int32 [B]: the bits of sdfr_mesh_sdf, and bit 1 for a
 *              mesh of zero total area.  Samples of such a mesh, and samples whose uniforms are not all in [0, 1), get triangle = -1 and
 *              zero points.
 *   ws         sdfr_mesh_surface_ws_bytes(B, T) bytes, 8-byte aligned.
 * Four launches, no atomics, no memset. */
int64_t sdfr_mesh_surface_ws_bytes(int B, int64_t T);
int sdfr_mesh_surface_points(const float* vertices, int64_t V, const int32_t* faces, int64_t T, const int64_t* voff, const int64_t* toff,
                             const float* uniforms, int64_t S, const int64_t* soff, int B, void* ws, int64_t ws_bytes, float* points,
                             int32_t* triangle, int32_t* flags, void* stream);

/*
 * Training the DeepSDF decoder (csrc/mlp_train.hip): the forward of Decoder.forward in train() mode
 * (sdfrenderer/deepsdf/networks/deep_sdf_decoder_scale.py:78-107, dropout included) with its activations kept, and the gradient of a scalar
 * loss with respect to the input rows AND the weights.  Exact float32 (v_mfma_f32_32x32x2_f32, k in order, bias last); no half path, no
 * LayerNorm decoders.
 *
 * The weights change every step, so W[l] / b[l] are DEVICE pointers to plain float32 [out_dim[l]][in_dim[l]] / [out_dim[l]] (the arrays W, b,
 * dW, db themselves are host arrays of n_lin device pointers).  The decoder is described as for sdfr_decoder_create: n_lin, in_dim, out_dim,
 * inj_n, inj_off, n_inputs, use_tanh; out_dim up to 512, in_dim up to 1024, n up to 2^26.
 *
 *   forward    a_l = drop(relu(xin_l W_l^T + b_l)); xin_0 = inputs, xin_{l+1} = cat(a_l, inputs[:, inj_off[l+1] : + inj_n[l+1]]).
 *              sdf[n] = tanh(y1), y1 = use_tanh ? tanh(y) : y, y the last linear.
 *   dropout    stateless: unit (l, row, j) of a layer whose bit l is set in drop_layers is kept when the top 24 bits of
 *              mix64(seed ^ mix64((row << 14 | l << 10 | j) * 0x9E3779B97F4A7C15 + 1)) are >= rint(drop_p 2^24) (mix64: the splitmix64 finaliser,
 *              csrc/train_cells.h); a kept unit is multiplied by the float32 value 1 / (1 - drop_p).  drop_p = 0 takes no hash.  This is the
 *              library's own random stream, not torch's.
 *   backward   d of the last linear = g_sdf (1 - out^2) (1 - y1^2 with use_tanh); d_{l-1} = (d_l W_l) * (a_{l-1} > 0 ? 1 / (1 - drop_p) : 0) -- the
 *              stored activation is the mask; g_inputs[n][n_inputs] = layer 0's term plus the re-injected columns' terms of the injection
 *              layers in ascending l; dW_l = d_l^T xin_l and db_l = the column sums of d_l: the rows are cut into chunks of 1024 in order, a
 *              chunk is summed in row order, and the chunk sums are added in chunk order.  No atomics: dW / db are functions of n and the shapes
 *              and have the same bits on every run; sdf[i] and g_inputs[i] do not depend on the batch or (with drop_p = 0) on i.
 *   workspace  sdfr_decoder_train_bytes(...) bytes (-1: a description the kernels refuse), float32 words, with chunks = ceil(n / 1024) and
 *              nh = n_lin - 1:
 *                header   16 words: [0] float 1 / (1 - drop_p) of the forward that filled the workspace, [1] int32 the drop_layers it applied
 *                x0       [n][in_dim[0]]                the input rows
 *                act[l]   [n][in_dim[l + 1]], l < nh    a_l (after ReLU, dropout and its scale) in columns 0 .. out_dim[l] - 1, the re-injected
 *                                                       input columns of layer l + 1 behind them; act[l] starts at word
 *                                                       16 + n (in_dim[0] + in_dim[1] + ... + in_dim[l])
 *                tail     [n][2]                        y1 and out
 *                delta    2 x [n][max out_dim]          d_l in half l & 1
 *                ginj[l]  [n][inj_n[l]], l >= 1
 *                part     [chunks][out][in] then [chunks][out]: the partials of the layer the backward handled last (layer 0); the section is
 *                         sized chunks * max_l (out_dim[l] in_dim[l] + out_dim[l])
 *              sdfr_decoder_train_backward reads what the forward of the same n left there.  A workspace that is too small is an error.
 * Launches: 1 + n_lin (forward), 1 + 3 n_lin (backward); no host synchronisation, no host read, no memset.
 */
int64_t sdfr_decoder_train_bytes(int n_lin, const int* in_dim, const int* out_dim, const int* inj_n, const int* inj_off, int n_inputs, int64_t n);
int sdfr_decoder_train_forward(int n_lin, const int* in_dim, const int* out_dim, const int* inj_n, const int* inj_off, int n_inputs,
                               int use_tanh, const float* const* W, const float* const* b, const float* inputs, int64_t n, float drop_p,
                               int drop_layers, int64_t seed, float* sdf, void* ws, int64_t ws_bytes, void* stream);
int sdfr_decoder_train_backward(int n_lin, const int* in_dim, const int* out_dim, const int* inj_n, const int* inj_off, int n_inputs,
                                int use_tanh, const float* const* W, const float* g_sdf, int64_t n, void* ws, int64_t ws_bytes,
                                float* const* dW, float* const* db, float* g_inputs, void* stream);

/* ---- encoding shapes under a frozen decoder (csrc/encode.hip, SDFR_VERSION 418) ----
 *
 * DeepSDF's "reconstruct": the latent of a shape the decoder was not trained on, fitted to the shape's SDF samples with the decoder frozen.  One
 * iteration is  sdfr_encode_rows -> a decoder forward that saves its masks -> sdfr_mlp_jacobian with an identity index list ->
 * sdfr_encode_reduce -> sdfr_encode_step, for B shapes at once.  All pointers are device pointers; no atomics, no memset, no host
 * synchronisation, the same bits on every run, and a shape's results do not depend on B or on its position in the batch.  Float64 and float32
 * operations are rounded one by one (no contraction).  csrc/encode_cells.h holds the per-element rules; DESIGN.md 7k.
 *
 *   flags[b]   bit 0 (1) the shape has no samples; bit 1 (2) no row with a finite prediction and target; bit 2 (4) the latent was not stepped;
 *              bit 3 (8) soff is broken at this shape (soff[b] < 0, soff[b + 1] < soff[b] or soff[b + 1] > S), or draw = 0 with k > count_b.
 *              sdfr_encode_rows stores bits 0 and 3 and clears the others; the reduce and the step add theirs.  The table lives on the device,
 *              so a broken entry cannot be a return code: the shape's rows are zero, nothing is read through it, and it is never stepped.
 *
 * sdfr_encode_rows: samples [S][4] = x y z sdf, soff int64 [B + 1] (shape b owns samples soff[b] .. soff[b + 1] - 1, count_b of them), z [B][L]
 *   the raw latents.  Row s < k of shape b takes sample soff[b] + s with draw = 0 and soff[b] + mulhi64(mix64(seed ^ mix64((iter << 40 | (shape0 + b)
 *   << 24 | s) * 0x9E3779B97F4A7C15 + 1)), count_b) with draw = 1 (with replacement; mix64: the splitmix64 finaliser of csrc/train_cells.h; mulhi64:
 *   the upper 64 bits of the 128-bit product; the library's own random stream).  Writes inputs [B k][L + 3] = (zn[b], x y z), target [B k] and
 *   zn [B][L]: z / max(||z||, 1e-12) in float32 with unit != 0 (the rule of sdfr_params_forward), z otherwise.  A shape with flag bit 0 or 3
 *   gets zero rows and zero targets.  inputs == NULL: zn and flags only.  shape0: the index the first
 *   shape has in the caller's whole batch, for the hash alone (a caller that stages its shapes in groups draws the same rows whatever the groups).
 *   1 <= L <= 256, 1 <= k <= 2^20, shape0 + B <= 65535, 0 <= iter < 2^24.
 *
 * sdfr_encode_reduce: pred [B k] (the decoder's values), target [B k], J [B k][Jstride] whose latent columns are columns 0 .. L - 1.  With
 *   cp = clamp(p, -clamp, clamp), ct likewise, over the rows whose p and t are both finite (n_ok of them), in float64:
 *   loss[b] = mean |cp - ct|;  g_zn[b][c] = mean sgn(cp - ct) [-clamp <= p <= clamp] J[i][c]  (sgn(0) = 0; a row whose factor is 0 adds nothing,
 *   whatever its J holds); both are 0 and bit 1 of flags[b] is set when n_ok = 0.  The rows of a shape are cut into chunks of 1024 in order; in a
 *   chunk, accumulator j < 64 sums rows j, j + 64, ... in ascending order and the accumulators are folded by halves (j takes j + 32, then
 *   j + 16, ... j + 1); the chunk sums are added in chunk order.  ws: sdfr_encode_ws_bytes(B, k, L) bytes (-1: sizes the kernels refuse),
 *   aligned to 8.  Two launches.
 *
 * sdfr_encode_step: Adam (betas 0.9 / 0.999, eps 1e-8, the update of sdfr_solver_step) on z [B][L] with state m, v [B][L], step count t >= 1
 *   and learning rate lr per call; 1 - beta^t is formed in double on the host.  The gradient is float32(g_zn) taken through the normalisation
 *   with unit != 0 (the formula of sdfr_params_backward) and float32(g_zn) + code_reg z / ||z|| (nothing added at z = 0) otherwise.  A shape
 *   whose flags hold bit 0, 1 or 3, or whose gradient has a non-finite element, keeps z, m and v and gets bit 2.  history != NULL:
 *   history[(t - 1) history_stride + b] = float32(loss[b]).
 */
int64_t sdfr_encode_ws_bytes(int B, int64_t k, int L);
int sdfr_encode_rows(const float* samples, int64_t S, const int64_t* soff, int B, int shape0, int64_t k, int draw, int64_t seed, int64_t iter, const float* z,
                     int L, int unit, float* inputs, float* target, float* zn, int32_t* flags, void* stream);
int sdfr_encode_reduce(const float* pred, const float* target, const float* J, int Jstride, int L, int B, int64_t k, float clamp, void* ws,
                       int64_t ws_bytes, double* loss, double* g_zn, int32_t* flags, void* stream);
int sdfr_encode_step(float* z, float* m, float* v, int L, int B, int unit, const double* g_zn, const double* loss, int32_t* flags, float code_reg,
                     float lr, int t, float* history, int64_t history_stride, void* stream);

/* ---- shape completion from one view (csrc/complete.hip, SDFR_VERSION 419) ----
 *
 * A latent fitted to what one sensor position sees of a shape, the decoder frozen.  Every sample row carries an interval [lo, hi] the true
 * signed distance lies in: lo == hi for an exact sample, [0, s] for a free-space point s in front of its ray's hit.  One iteration is
 * sdfr_bound_rows -> a decoder forward that saves its masks -> sdfr_mlp_jacobian -> sdfr_bound_reduce -> sdfr_encode_step.  All pointers are
 * device pointers; no atomics, no memset, no host synchronisation, the same bits on every run.  csrc/complete_cells.h holds the per-element
 * rules; DESIGN.md 7l.
 *
 * sdfr_view_samples: points [N][3] float32 (camera frame), normals [N][3] float64 (camera frame) or NULL, ptoff int64 [B + 1] (shape b owns
 *   points ptoff[b] .. ptoff[b + 1] - 1), pose [B][6] = cos(yaw), sin(yaw), trans, scale as sdfr_verify_point_rows takes it, origin [3] the
 *   sensor's position (camera frame, float32).  Point g gives P = 3 + F rows, rows [N P][5] = x y z lo hi, row P g + j for slot j.  With
 *   x = diag(1, -1, 1) rot_yaw^T (p / scale - trans) in float64 (every operation rounded on its own, the rule of sdfr_verify_point_rows), o the
 *   origin through the same map and n^ the normal through diag(1, -1, 1) rot_yaw^T divided by its length:
 *     slot 0      x                       [0, 0]
 *     slot 1      x + eta n^              [eta, eta]         slots 1 and 2 are invalid without normals, or with a non-finite or zero normal
 *     slot 2      x - eta n^              [-eta, -eta]
 *     slot 3 + f  x - s d^                [0, float32(s)]    d^ = (x - o) / r, r = |x - o| = sqrt((dx dx + dy dy) + dz dz),
 *                                                            s = ((f + u) / F) min(s_max, r); invalid when r is zero or not finite
 *   u = (mix64(seed ^ mix64(((shape0 + b) << 40 | i << 8 | f) * 0x9E3779B97F4A7C15 + 1)) >> 11) 2^-53 with i = g - ptoff[b] and the mix64 of
 *   csrc/train_cells.h.  Positions are rounded once to float32; a slot is valid only if its float32 position is finite and in [-1, 1]^3.  An
 *   invalid slot holds position 0 and lo = hi = NaN, which the reduce leaves out.  eta and s_max are in lattice units (float32, widened to float64 for the
 *   arithmetic above).  0 <= F <= 64,
 *   N <= 2^32.  flags int32 [B]: bit 3 (8) ptoff is broken at this shape (ptoff[b] < 0, ptoff[b + 1] < ptoff[b] or ptoff[b + 1] > N) --
 *   nothing is read through it; bit 2 (4) a non-finite pose word or a scale <= 0.  Every slot of such a shape, and of a point no usable entry
 *   holds, is invalid.  One point per thread; one launch.
 *
 * sdfr_bound_rows: sdfr_encode_rows for samples [S][5] = x y z lo hi: the same table rules, the same draw, the same zn; writes inputs
 *   [B k][L + 3], lo [B k] and hi [B k].
 *
 * sdfr_bound_reduce: sdfr_encode_reduce with the interval rule.  With cp, cl, ch the float32 clamps of p, lo and hi to [-clamp, clamp], over the
 *   rows with a finite p, lo <= hi and at least one finite bound (n_ok of them; any NaN leaves a row out), in float64:
 *   d = cp - cl where cp < cl, cp - ch where cp > ch, else 0;  loss[b] = mean |d|;  g_zn[b][c] = mean sgn(d) [-clamp <= p <= clamp] J[i][c].
 *   A row inside its interval adds nothing but counts in n_ok.  With lo == hi the results are sdfr_encode_reduce's in every bit.  The
 *   summation order and the workspace (sdfr_encode_ws_bytes) are sdfr_encode_reduce's.  Two launches. */
int sdfr_view_samples(const float* points, const double* normals, int64_t N, const int64_t* ptoff, int B, const float* pose, const float* origin,
                      int shape0, int F, float eta, float s_max, int64_t seed, float* rows, int32_t* flags, void* stream);
int sdfr_bound_rows(const float* samples, int64_t S, const int64_t* soff, int B, int shape0, int64_t k, int draw, int64_t seed, int64_t iter, const float* z,
                    int L, int unit, float* inputs, float* lo, float* hi, float* zn, int32_t* flags, void* stream);
int sdfr_bound_reduce(const float* pred, const float* lo, const float* hi, const float* J, int Jstride, int L, int B, int64_t k, float clamp, void* ws,
                      int64_t ws_bytes, double* loss, double* g_zn, int32_t* flags, void* stream);

/* ---- pose and shape fitted to one view (csrc/align.hip, SDFR_VERSION 420) ----
 *
 * The interval fit of the completion with the pose free: yaw, trans and scale move with the latent, the decoder frozen.  The observation rows
 * are made once, in the CAMERA frame and in METRES, so they hold whatever the pose becomes.  One iteration is  sdfr_align_rows -> a decoder
 * forward that saves its masks -> sdfr_mlp_jacobian (its last three columns are d sdf / d xyz) -> sdfr_align_reduce -> sdfr_align_step.  All
 * pointers are device pointers (but lr_pose, five floats of the host read before the launch, like lr); no atomics, no memset, no host
 * synchronisation, the same bits on every run, and a shape's results do not depend on B or on its position in the batch.  Float64 and
 * float32 operations are rounded one by one.  csrc/align_cells.h holds the per-element rules; DESIGN.md 7m.
 *
 *   pose [B][6] = cos(yaw), sin(yaw), trans, scale (the row of sdfr_verify_point_rows); theta [B][5] = yaw, trans, scale, the variables.
 *   flags[b]    the bits of sdfr_encode_rows / _reduce / _step, and bit 4 (16): pose[b] holds a non-finite word or a scale <= 0.
 *
 * sdfr_align_samples: sdfr_view_samples without a pose.  Point g (float32, camera frame) with normal n (float64, camera frame, or NULL) gives
 *   P = 3 + F rows [N P][5] = q lo hi, q the float64 position rounded once, [lo, hi] an interval the true METRIC signed distance at q lies in:
 *     slot 0      p                [0, 0]
 *     slot 1      p + eta n^       [eta, eta]          n^ = n / sqrt((n0 n0 + n1 n1) + n2 n2); invalid without a finite non-zero normal
 *     slot 2      p - eta n^       [-eta, -eta]
 *     slot 3 + f  p - s d^         [0, float32(s)]     d^ = (p - o) / r, s = ((f + u) / F) min(s_max, r); invalid when r is zero or not finite
 *   u: the hash of sdfr_view_samples.  eta and s_max are in metres.  A slot is valid only if its point is finite; an invalid slot holds position
 *   0 and NaN bounds; there is no cube test.  flags int32 [B]: bit 3 (8) ptoff is broken at this shape; nothing is read through it.
 *
 * sdfr_align_rows: sdfr_bound_rows (the same table rules, draw and zn) on those rows, with pose [B][6]: for the drawn sample (q, lo, hi) it
 *   writes inputs [B k][L + 3] = (zn[b], float32(x)) with x = diag(1, -1, 1) rot_yaw^T (q / scale - trans) in float64 (the operations of
 *   sdfr_verify_point_rows), cam [B k][3] = q, lo and hi [B k].  A row whose float32 x leaves [-1, 1]^3 gets x = 0 and NaN bounds for this
 *   iteration.  An unusable pose makes every row of its shape so and raises bit 4.  inputs == NULL: zn and flags only.
 *
 * sdfr_align_reduce: with pm = float32(scale p) the row rule is sdfr_bound_reduce's on (pm, lo, hi, clamp), clamp in metres.  Per shape over
 *   the ok rows, in float64: loss[b] = mean e;  g[b][0 .. L + 4] = mean w d pm / d (zn, yaw, tx, ty, tz, scale), with (gx, gy, gz) =
 *   J[L .. L + 2], c, sn = pose[0], pose[1], x recomputed in float64 from cam and pose:
 *     zn_i   scale J[i]                          yaw    scale (gz x0 - gx x2)
 *     tx     -(scale (gx c + gz sn))             ty     scale gy                 tz    scale (gx sn - gz c)
 *     scale  p + scale ((gx (c u0 - sn u2) - gy u1) + gz (sn u0 + c u2)),  u = -(q / (scale scale))
 *   each operation as written, one rounding each.  The summation order is sdfr_encode_reduce's (the same kernels).  J has Jstride >= L + 3
 *   words a row.  ws: sdfr_align_ws_bytes(B, k, L) bytes, aligned to 8.  At scale == 1 loss and the L latent columns are sdfr_bound_reduce's
 *   in every bit.  Two launches.
 *
 * sdfr_align_step: the latent by sdfr_encode_step's rule with rate lr, and the same Adam on theta with state tm, tv [B][5] and rates
 *   lr_pose[5]; a rate of 0 (lr included) leaves its parameter and state untouched.  A shape whose flags hold bit 0, 1, 3 or 4, whose
 *   gradient has a non-finite element (all L + 5, as float32), or whose stepped scale would not be finite and positive keeps everything and
 *   gets bit 2.  A stepped shape gets its next pose row: float32(cos(double(yaw))), float32(sin(double(yaw))), trans, scale.  history as
 *   sdfr_encode_step's. */
int sdfr_align_samples(const float* points, const double* normals, int64_t N, const int64_t* ptoff, int B, const float* origin, int shape0, int F,
                       float eta, float s_max, int64_t seed, float* rows, int32_t* flags, void* stream);
int sdfr_align_rows(const float* samples, int64_t S, const int64_t* soff, int B, int shape0, int64_t k, int draw, int64_t seed, int64_t iter, const float* z,
                    int L, int unit, const float* pose, float* inputs, float* cam, float* lo, float* hi, float* zn, int32_t* flags, void* stream);
int64_t sdfr_align_ws_bytes(int B, int64_t k, int L);
int sdfr_align_reduce(const float* pred, const float* lo, const float* hi, const float* J, int Jstride, const float* cam, const float* pose, int L, int B,
                      int64_t k, float clamp, void* ws, int64_t ws_bytes, double* loss, double* g, int32_t* flags, void* stream);
int sdfr_align_step(float* z, float* m, float* v, int L, int B, int unit, float* theta, float* tm, float* tv, float* pose, const double* g,
                    const double* loss, int32_t* flags, float code_reg, float lr, const float* lr_pose, int t, float* history, int64_t history_stride,
                    void* stream);

/* ---- one shape fitted to several views (csrc/track.hip, SDFR_VERSION 423) ----
 *
 * A VIEW is one cloud of one object in one camera frame, with its own yaw and trans; a TRACK is an object: an ordered list of views with ONE
 * latent and (with share_scale) ONE scale.  Views are numbered 0 .. V - 1; track t owns views voff[t] .. voff[t + 1] - 1.  One iteration of
 * the joint fit is  sdfr_align_rows over the V views with z = z_view [V][L] -> the decoder forward with its masks saved -> sdfr_mlp_jacobian
 * -> sdfr_align_reduce over the V views (loss [V], g [V][L + 5], vflags [V]) -> sdfr_track_step.  The first four are unchanged.
 *
 * sdfr_track_step: ONE launch, grid (T), one workgroup a track.  All pointers are device pointers (but lr_pose, five floats of the host read
 * before the launch); no atomics, no memset, no host synchronisation, the same bits on every run, and a track's results do not depend on T
 * or on its position in the batch.  Float64 and float32 operations round one by one.  The rules (csrc/track_cells.h):
 *   table   voff[t] < 0, voff[t + 1] < voff[t], voff[t + 1] > V or more than 1024 views: tflags[t] = 8; nothing is read or written through
 *           such an entry, loss[t] and the history word included, and the track is not stepped.  tflags[t] is stored, not OR-ed.
 *   usable  a view is usable when vflags[v] holds none of bit 0, 1, 3, 4 (what keeps sdfr_align_step from stepping a shape), its weight
 *           (weight[v]; 1 with weight == NULL) is finite and > 0, float32 of each of its L + 5 gradient entries is finite, and -- without
 *           share_scale -- the scale its own Adam update would leave is finite and positive.  An unusable view gets bit 2 in vflags[v] and
 *           keeps theta, tm, tv and the yaw / trans words of its pose row.
 *   fold    over the usable views of the track in ASCENDING view order, in float64: W = sum w_v, S_c = sum w_v g[v][c] for the latent
 *           columns c < L and, with share_scale, column L + 4, E = sum w_v view_loss[v]; every sum STARTS FROM ITS FIRST TERM (a lone -0.0
 *           survives).  G_c = S_c / W, loss[t] = E / W.  A track without views gets bit 0 of tflags; a track with no usable view loss[t] = 0
 *           and bits 1 and 2, and nothing of it moves.
 *   track   the latent z[t] is stepped by sdfr_encode_step's rule (through the unit normalisation with unit, the regulariser code_reg ||z||
 *           without; the finite check in index order) with float32(G_c) at the rate lr; lr == 0 leaves z, m, v untouched.  With share_scale
 *           the same Adam on scale[t] (state sm, sv) with float32(G_{L + 4}) at lr_pose[4]; a rate of 0 leaves it untouched.  If the
 *           latent's gradient is not finite, or the stepped scale would not be finite and positive, the WHOLE track keeps everything --
 *           latent, scale and every view's pose --; tflags[t] and the vflags of its usable views get bit 2.
 *   views   of a stepped track: each usable view steps its own theta, tm, tv by sdfr_align_step's rule with ITS OWN gradient columns
 *           g[v][L .. L + 4] (not scaled by w_v / W: Adam divides a constant factor out again, and a track of one view is then
 *           sdfr_align_step in every bit) at the rates lr_pose, rate 4 taken as 0 when the scale is shared, and its pose row is rewritten.
 *           EVERY view of a stepped track, usable or not, receives z_view[v] = z[t] (the raw latent; sdfr_align_rows normalises it) and, with
 *           share_scale, theta[v][4] = scale[t] and the scale word of its pose row.
 *   history[(t - 1) history_stride + track] = float32(loss[track]) (history may be NULL).  1 - beta^t as in sdfr_encode_step.
 * scale, sm, sv are read with share_scale alone.  Refused: NULL arguments, L outside 1 .. 256, T or V outside 0 .. 65535, t < 1, a rate that is
 * not finite, history_stride < T. */
int sdfr_track_step(float* z, float* m, float* v, int L, int T, int unit, float* scale, float* sm, float* sv, int share_scale, const int64_t* voff, int V,
                    const float* weight, float* theta, float* tm, float* tv, float* pose, float* z_view, const double* g, const double* view_loss,
                    int32_t* vflags, double* loss, int32_t* tflags, float code_reg, float lr, const float* lr_pose, int t, float* history,
                    int64_t history_stride, void* stream);

/* ---- choosing a fit's start: scored candidates (csrc/search.hip, SDFR_VERSION 424) ----
 *
 * The frozen-decoder fits are local: from a far start they end in another minimum.  A START is a candidate (latent, pose) for one shape; many
 * starts share one shape's samples.  The three entry points score all starts of all shapes on the SAME drawn rows per shape, by the loss
 * alone, and rank them per shape:  sdfr_search_rows -> a decoder forward (no Jacobian) -> sdfr_search_reduce -> sdfr_search_select.  All
 * pointers are device pointers; no atomics, no memset, no host synchronisation, the same bits on every run, and a start's results depend
 * neither on N nor on its position in the batch.  Float64 and float32 operations round one by one.  csrc/search_cells.h holds the
 * per-element rules; DESIGN.md 7p.
 *
 * sdfr_search_rows: the rows kernel of the fits with one indirection.  Start s < N reads the samples of shape own[s] (int32 [N]; samples
 *   [S][5] and soff int64 [B + 1] as sdfr_bound_rows / sdfr_align_rows take them), with its own latent z[s] and, with pose != NULL, its own
 *   pose row pose[s][6].  The draw's hash takes shape0 + own[s], not s: every start of a shape sees the same drawn samples in the same
 *   order.  pose == NULL: lattice-frame interval rows, the rule of sdfr_bound_rows.  pose != NULL: camera-frame rows through the start's
 *   pose, the rule of sdfr_align_rows -- NaN bounds for a row that leaves the cube, bit 4 for an unusable pose --; cam [N k][3] may be NULL,
 *   then nothing is written for it.  own[s] outside [0, B): flags[s] = 8 and zero rows; nothing is read through it.  The other flags are
 *   those of sdfr_bound_rows / sdfr_align_rows, per start.  Writes inputs [N k][L + 3], lo, hi [N k], zn [N][L], flags [N]; inputs == NULL:
 *   zn and flags only.  With own = 0 .. B - 1 every output equals that of sdfr_bound_rows / sdfr_align_rows bit for bit.  N <= 65535,
 *   shape0 + B <= 65535.  One launch.
 *
 * sdfr_search_reduce: the loss alone, per start: loss[s] = the mean of e over the ok rows of start s, by the row rule of sdfr_bound_reduce
 *   on p (pose == NULL) or of sdfr_align_reduce on float32(pose[s][5] p), summed in sdfr_encode_reduce's order (the same kernels with no
 *   gradient columns) -- the loss word of those calls on the same pred, lo, hi, pose in every bit.  No J is read.  A start without an ok row
 *   gets loss 0 and bit 1 of flags[s] (flags [N] on entry and exit).  ws: sdfr_search_ws_bytes(N, k) = N chunks 2 float64 words, aligned
 *   to 8 (-1 for sizes the kernels refuse).  Two launches.
 *
 * sdfr_search_select: grid (B), one workgroup a shape.  Shape b owns starts coff[b] .. coff[b + 1] - 1 (int64 [B + 1]).  A start is USABLE if
 *   its flags hold none of bit 0, 1, 3, 4 and its loss is finite.  The usable starts are ranked by (loss as float64, start index) ascending;
 *   equal losses, -0.0 == 0.0 included, go to the lower index.  order [B][keep] int32: the global start index of rank r for
 *   r < min(keep, usable), -1 beyond; count [B] int32: that minimum.  coff[b] < 0, coff[b + 1] < coff[b], coff[b + 1] > N or more than 4096
 *   starts: count[b] = -1 and a row of -1; nothing is read through such an entry.  A shape without starts gets count 0.  1 <= keep <= 64.
 *   One launch. */
int sdfr_search_rows(const float* samples, int64_t S, const int64_t* soff, int B, const int32_t* own, int N, int shape0, int64_t k, int draw,
                     int64_t seed, int64_t iter, const float* z, int L, int unit, const float* pose, float* inputs, float* cam, float* lo, float* hi,
                     float* zn, int32_t* flags, void* stream);
int64_t sdfr_search_ws_bytes(int N, int64_t k);
int sdfr_search_reduce(const float* pred, const float* lo, const float* hi, const float* pose, int N, int64_t k, float clamp, void* ws,
                       int64_t ws_bytes, double* loss, int32_t* flags, void* stream);
int sdfr_search_select(const double* loss, const int32_t* flags, const int64_t* coff, int B, int64_t N, int keep, int32_t* order, int32_t* count,
                       void* stream);

/* ---- lidar clusters and rough boxes (csrc/cluster.hip, SDFR_VERSION 421) ----
 * Object proposals from a raw scan: Euclidean clusters of the (road-free) cloud and a minimum-area rectangle per cluster.  The reference
 * has no counterpart to this stage; the semantics are this library's own.  Every output is a function of the input alone -- the same bits
 * on every run, whatever the schedule --: integer atomics only, no float atomic, no sum of floats.
 *
 * sdfr_lidar_clusters.  points [N][3], device memory, float64 (points_f64 != 0) or float32 (widened first), as sdfr_lidar_normals takes
 * them.  mask uint8[N] or NULL (every point).  A point TAKES PART if its mask is non-zero and its three coordinates are finite.  Two such
 * points are NEIGHBOURS if d2 = (dx*dx + dy*dy) + dz*dz < eps*eps, strictly, in float64 (eps is a float32 value, widened).  A COMPONENT
 * is a connected component of that graph.  A component is a CLUSTER if min_points <= size and (max_points <= 0 or size <= max_points).
 * Clusters are numbered 0, 1, ... in ascending order of their smallest member index; only the first max_clusters (1 ... 4096) are kept.
 *   counts int32[4] = participating points, components, clusters found (the true number, capped or not), flags: bit 1 (value 1) the cap
 *     cut something, bit 2 (value 2) a non-finite point under a set mask was left out.
 *   label int32[N]: the cluster's number; -1 for a point that takes no part, whose component is no cluster, or whose cluster is beyond the cap.
 *   off int32[max_clusters + 1]: first member slot of every kept cluster; the entries beyond the kept count equal the total.
 *   members int32[N]: the input indices cluster by cluster, ascending within a cluster (a stable partition); entries from off[kept] on are
 *     NOT written.
 * The components come from a union-find over input indices with parent[i] <= i (every write lowers a value; no loop waits for another
 * thread; a component's root is its smallest index whatever the order of the unions), over the hash grid of sdfr_lidar_normals.
 * workspace: sdfr_cluster_ws_bytes(N, max_clusters) bytes of device memory, 16-byte aligned (-1 beyond the limits: N <= 2^24,
 * max_clusters <= 4096, ceil(N / 1024) * max_clusters <= 2^26).  N == 0: counts and off are zeroed.  No host read, nothing for the caller
 * to clear, no host synchronisation.
 *
 * sdfr_cluster_boxes.  members, off, counts: sdfr_lidar_clusters' (of the same points).  dirs double[K][2] = (cos, sin) of K directions
 * (1 ... 1024), device memory, made by the caller: no cosine or sine is evaluated on the device.  Per member point and direction, in float64
 * of the stored coordinates, one rounding per statement: a = x*c; b = z*s; u = a + b; a = z*c; b = x*s; v = a - b.  Per cluster and
 * direction: the minima and maxima of u and v (a zero is +0), area = (u_max - u_min) * (v_max - v_min); the winner is the first
 * direction of the smallest area.  rect double[max_clusters][8] = k, u_min, u_max, v_min, v_max, y_min, y_max, area of the winner; rows
 * beyond the kept count are NOT written.  One launch, no host synchronisation. */
int64_t sdfr_cluster_ws_bytes(int N, int max_clusters);
int sdfr_lidar_clusters(const void* points, int points_f64, int N, const uint8_t* mask, float eps, int min_points, int max_points,
                        int max_clusters, int32_t* label, int32_t* members, int32_t* off, int32_t* counts, void* workspace,
                        int64_t workspace_bytes, void* stream);
int sdfr_cluster_boxes(const void* points, int points_f64, int N, const int32_t* members, const int32_t* off, const int32_t* counts,
                       int max_clusters, const double* dirs, int K, double* rect, void* stream);

/* Debug only: forward kernels of a library built with -DSDFR_MLP_TRACE write cycle stamps of their workgroup 0 into this device buffer
 * (8 waves * SDFR_MAX_LAYERS * 5 uint64; see tools/cycle_trace.py); pass NULL to disable.  Production builds ignore it. */
int sdfr_debug_set_trace(void* device_buffer);
/* Debug only: sdfr_mlp_forward and sdfr_mlp_forward_ordered of a library built with -DSDFR_MLP_TRACE write one record of 6 uint64 per
 * workgroup into this device buffer of `tiles` records: shader clock at the workgroup's start, 100 MHz constant clock at its start, the same
 * two at its end (behind the tile's sdf store), XCC_ID << 32 | HW_ID of the CU it ran on, blockIdx.x (see tools/tile_gantt.py).  Workgroups
 * beyond `tiles` write nothing; NULL or tiles <= 0 disables it.  Production builds ignore it. */
int sdfr_debug_set_tile_trace(void* device_buffer, int64_t tiles);

#ifdef __cplusplus
}
#endif
#endif /* SDFR_H */
