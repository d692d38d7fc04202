/* hmme_test.h -- entry points of libhmme.so that exist for tests and measurements only.  NOT part of the drop-in boundary
 * (include/hmme.h): nothing a host application needs, no stability promise, not counted in HMME_ABI_VERSION. */
#ifndef HMME_TEST_H
#define HMME_TEST_H

#include "hmme.h"

#ifdef __cplusplus
extern "C" {
#endif

/* device address of a plane's sample (0,0) (plane != NULL) or of the context's per-CTU current-block staging area: lets a test
 * prove that a launch ran on addresses whose low dword has bit 31 set (tests/test_gpu_parity.py, high-address case) */
uint64_t hmme_test_device_address(const hmme_ctx* ctx, const hmme_plane* plane);
/* average device time in ms of the search kernel(s) alone over `reps` back-to-back launches on `stream` (job tables prepared once,
 * outside the timed region), measured with hipEvents recorded on that stream */
int hmme_test_time_search_kernel(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp,
                                 const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream, int reps,
                                 float* avg_ms);

/* how an 8-bit whole-picture search of n_pairs pictures of width x height at `search_range` (<= 64) is dealt to a chip of `slots` workgroup slots
 * (hmme.hip plan_search; host arithmetic, needs no device): out[0] = jobs, out[1] = jobs searched whole (the head; == jobs: no tail plan),
 * out[2] = workgroups (segments) of the tail, out[3] = 1 if head and tail are one launch */
int hmme_test_tail_plan(int width, int height, int search_range, int n_pairs, int slots, int* out);

/* whether an 8-bit search launch at this lambda runs the packed-minimum twin of the search kernel (me_pk_gate, me_kernels.hpp; host
 * arithmetic, needs no device): 1 while the largest MV cost the launch can meet + the largest sum of an 8x8 CU stays below the packed
 * marker of an invalid candidate, 0 where the 32-bit tree runs */
int hmme_test_pk_gate(uint32_t lambda_q16);

/* which body an 8-bit search launch at this lambda and FEN runs (me_pk_body; host arithmetic): 0 the 32-bit tree, 1 the packed-minimum
 * twin, 2 the kernel that also holds the full-task body (FEN 1, the largest MV cost + the largest 16x12 sum within 16 bits) */
int hmme_test_pk_body(uint32_t lambda_q16, int fen);

/* whether a task of that kernel -- part k (2^k quads per lane row), lane-iterations it0 .. it0 + n_it - 1 of a wx x wy window -- runs the
 * marker-free body: 1 where every lane of every one of its lane-iterations is wholly valid or wholly invalid (me_task_marker_free) */
int hmme_test_pk_task_marker_free(int wx, int wy, int k, int it0, int n_it);

/* whether that task runs the full-task twin, the body whose first two butterfly levels work on packed 16-bit minima (me_task_full): 1 where
 * k >= 2, the part does not hold the row's cut quad and every lane of every one of its lane-iterations lies inside the part's rows (which
 * excludes the folded iteration).  Every other task of the kernel runs the packed-minimum twin */
int hmme_test_pk_task_full(int wx, int wy, int k, int it0, int n_it);

/* The packed running minima a wave of a whole-picture launch carries across the full tasks of one part (me_kernels.hpp, above
 * me_task_carry_fits; host arithmetic, needs no device).  Their keys hold the absolute lane-iteration (6 bits) above the 16-candidate group
 * inside it (4 bits):
 *   hmme_test_task_carry_fits   1 unless the task is full and one of its lane-iterations lies beyond the six bits (me_task_carry_fits)
 *   hmme_test_carry_index       the ten-bit index of the group at window row `row`, `group` groups into part k (2..5) (me_carry_index);
 *                               -1 for a k or a group the part does not have
 *   hmme_test_carry_position    out[0], out[1] = the row and group of an index (me_carry_position: what the flush decodes); -1 for a bad argument */
int hmme_test_task_carry_fits(int wx, int wy, int k, int it0, int n_it);
int hmme_test_carry_index(int k, int row, int group);
int hmme_test_carry_position(int k, int index, int* out);

/* where the staging arena of a synchronous, host-array call puts n items of bytes[i] bytes (hmme.hip stage_layout: what every hmme_*_frame*
 * entry point lays its arrays out with; host arithmetic, needs no device): offsets[i] and *total, the arena's size.  Returns the alignment of
 * every item, or a negative value for a null argument */
int hmme_test_stage_layout(const size_t* bytes, int n, size_t* offsets, size_t* total);

/* which job the k-th workgroup of a refinement launch over `n_pairs` whole pictures of width x height takes (me_frac_deal, me_kernels.hpp:
 * edge CTUs of every pair first, then the interiors); host code, needs no device.  -1 for k outside the launch */
int hmme_test_frac_deal(int k, int n_pairs, int width, int height);

/* the MeJob of job `job` of a launch over CTUs [ctu_first, ctu_first + ctu_count) of a pic_w x pic_h picture at search range `sr`
 * (me_picture_job, me_kernels.hpp: what every job table and the table-less refinement launch derive on the device; host code, needs no
 * device): reference job / ctu_count, CTU ctu_first + job % ctu_count.  pred_q / center_q: [references][CTUs of the picture][2] quarter
 * pels, covering every reference `job` reaches; null = zero predictors / windows centred on the predictors.
 * out[8] = ctu_x | reference, ctu_y, lt_x, lt_y, rb_x, rb_y, pred_x, pred_y */
int hmme_test_picture_job(int job, int ctu_first, int ctu_count, int pic_w, int pic_h, int sr, const int16_t* pred_q, const int16_t* center_q,
                          int16_t* out);

/* The plan of a per-CTU call (hmme_search_ctu, hmme_search_refine_ctu, hmme_refine_ctu and their _w forms) on a context created with sr_max
 * (hmme.hip ctu_arg_check, ctu_plan_block, ctu_plan_window: the functions the call itself runs; host arithmetic, no device, no context).
 * mode: HMME_TEST_CTU_SEARCH and / or HMME_TEST_CTU_REFINE, the latter with or without HMME_TEST_CTU_HADAMARD; wp: the weight of a _w
 * entry, or null; range[4] = the smallest and largest sample of the 64 x 64 block, then of the staged window (what the call scans).
 * Returns what the call would return for these numbers -- its refusals, in the call's order, with the message in msg (may be null) -- and
 * for HMME_OK:
 *   out[17]   = wide (the 16-bit kernels), bias added to the staged samples, 1 for a bi-prediction origin, shift_bd (the sums are shifted by
 *               shift_bd - 8), halo, rows and columns of the staged window, workgroups n_wg of the search (0: a refinement alone), LDS pitch
 *               pdw and largest strip smax (16-bit deal; 0 otherwise), the refinement build's (u16 samples, Hadamard, weighted), and the
 *               task counts of window tiles (0,0), (1,0), (0,1), (1,1) (8-bit deal; 0 otherwise)
 *   out_fw[3] = the refinement's FracWp (scale, round, what is taken off the current samples); zeros without a weight
 *   out_wg    = per workgroup 8 values: the window lt_x, lt_y, rb_x, rb_y it searches, its tile's x and y, and its range [y0, y1) -- of
 *               tasks of that tile (8-bit deal) or of candidate rows (16-bit deal); room for 64 workgroups
 * HMME_ERR_ARG also for a null p / range / out / out_fw / out_wg, sr_max outside 1..128 or a mode that is none of the six entries'. */
#define HMME_TEST_CTU_SEARCH 1
#define HMME_TEST_CTU_REFINE 2
#define HMME_TEST_CTU_HADAMARD 4
int hmme_test_ctu_plan(int sr_max, const hmme_search_params* p, int mode, const hmme_weight* wp, const int* range, int* out, float* out_fw,
                       int16_t* out_wg, char* msg, int msg_len);

/* average device time in ms of the two plane passes of a weighted whole-picture search on their own, `reps` back-to-back launches each on
 * `stream`: *ref_ms = weighting the padded reference plane (me_weight_plane_kernel), *cur_ms = the u16 CTU-blocked copy of the current picture */
int hmme_test_time_weight_passes(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_weight* wp, void* stream, int reps,
                                 float* ref_ms, float* cur_ms);

/* average device time in ms of the origin pass of a bi-prediction search on its own (me_predict_kernel, OUT = 1: the prediction of
 * `other` from the motion field folded into the CTU blocks of `cur`), `reps` back-to-back launches over the whole picture on `stream` */
int hmme_test_time_bipred_origin(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* other, const void* d_other_mv, int mv_per_ctu, void* stream,
                                 int reps, float* avg_ms);

/* average device time in ms of the estimator's passes on their own, `reps` back-to-back launches each on `stream`, through the launchers every
 * estimator call uses: *stats_ms = the two statistics launches over a set of one plane, `cur` (me_plane_stats_kernel); *sad_ms = me_wp_sad_set_kernel
 * over n_refs pairs, `cur` against each reference, every one with weight wp->w0, offset wp->offset (8-bit units) and denominator wp->shift (<= 7) */
int hmme_test_time_wp_estimate_passes(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_weight* wp, void* stream,
                                      int reps, float* stats_ms, float* sad_ms);

/* The estimator's arithmetic on its own, comps = 1 what hmme_wp_estimate runs and comps = 3 what hmme_wp_estimate_420 runs (hmme.hip wp_parameters /
 * wp_select; host arithmetic, needs no device).  Plane i of a call is component i % comps of the current picture (i < comps) or of reference
 * i / comps - 1: stats[2 i], stats[2 i + 1] = its (dc_sum, ac) as hmme_plane_stats gives them, n_samples[c] = the sample count of component c;
 * entry comps * r + c belongs to component c of reference r.  HMME_ERR_ARG: a null argument (out_info may be null), comps other than 1 or 3,
 * n_refs outside 1..16, bit_depth outside 8..12, a denominator outside 3..7, a sample count below 1.
 * hmme_test_wp_parameters: steps 1 and 2 of the rule in include/hmme.h -> *log2_denom = d and (weight, clipped offset) of every entry. */
int hmme_test_wp_parameters(const int64_t* stats, const int64_t* n_samples, int comps, int n_refs, int bit_depth, int log2_denom_start, int* log2_denom,
                            int* weight, int* offset);
/* hmme_test_wp_select: steps 3 and 4 on those parameters and the two sums per entry as me_wp_sad_set_kernel leaves them -- sums[2 i] = the sum of
 * |(org << d) - (ref * weight + (offset << (d + bit_depth - 8)))|, sums[2 i + 1] = the sum of |org - ref| -> out_wp[i] and, where given,
 * out_info[i] of every entry */
int hmme_test_wp_select(const int64_t* stats, const int64_t* n_samples, int comps, int n_refs, int bit_depth, int log2_denom, const int* weight,
                        const int* offset, const uint64_t* sums, hmme_weight* out_wp, hmme_wp_info* out_info);

#ifdef __cplusplus
}
#endif
#endif
