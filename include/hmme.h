/*
 * hmme.h -- C ABI of the MI355X-native integer motion-estimation engine for HM 16.4.
 *
 * This is the drop-in boundary: plain C types, no exceptions, no torch/HIP types in the
 * signatures (streams and device buffers travel as void*).  It replaces what the reference's
 * OpenCL add-on does behind TEncOpenCL (all citations relative to /root/reference/):
 *
 *   hmme_create            <- TEncOpenCL::findDevice + compileKernelSource + createBuffers
 *                             (source/Lib/TLibEncoder/TEncOpenCL.cpp:69, :139, :195; called from
 *                             TEncTop::xInitOpenCL, TEncTop.cpp:1116-1162)
 *   hmme_set_lambda*       <- TEncOpenCL::setLambda (TEncOpenCL.h:121; TEncSlice.cpp:150)
 *   hmme_search_ctu        <- TEncOpenCL::calcMotionVectors + getX/getY/getRuiCost
 *                             (TEncOpenCL.cpp:240-362, TEncOpenCL.h:117-119; caller
 *                             TEncSearch::xMotionEstimation, TEncSearch.cpp:3743-3765)
 *   hmme_refine_ctu,       <- TEncSearch::xPatternSearchFracDIF (TEncSearch.cpp:4294-4331) for the 593 slots of that CTU,
 *   hmme_search_refine_ctu    the per-PU call at TEncSearch.cpp:3798 turned into a table lookup like the integer search
 *   hmme_search_frame*     <- the same search batched over every CTU of a picture (the
 *                             reference has no batched form: it launches 2*(2SR+1)^2 kernels per
 *                             CTU from the host, TEncOpenCL.cpp:312-333)
 *   hmme_search_pairs_device, <- the same for up to 16 (current, reference) picture pairs of a GOP in one launch
 *   hmme_refine_pairs_device     (cfg/encoder_randomaccess_main.cfg:28-31, cfg/encoder_lowdelay_P_main.cfg:24-27)
 *   hmme_search_pairs_w_device, <- the same in a slice with explicit weighted prediction (TEncSearch::setWpScalingDistParam,
 *   hmme_refine_pairs_w_device,    TEncSearch.cpp:5594-5635; TComRdCostWeightPrediction.cpp:55-90, :407-470), one weight per pair
 *   hmme_search_frame_w, hmme_refine_frame_w
 *   hmme_plane_stats, hmme_wp_estimate <- WeightPredAnalysis::xCalcACDCParamSlice / xEstimateWPParamSlice (WeightPredAnalysis.cpp:67-120, :172-351):
 *                                the weights those calls take, estimated from the planes
 *   hmme_predict_pairs_device,    <- motion compensation (TComPrediction::xPredInterBlk, TComPrediction.cpp:590-594, :669) and the bi-prediction
 *   hmme_search_pairs_bi_device,     pass of xMotionEstimation (origin 2*org - pred_other, TEncSearch.cpp:3702-3712; window around the list's
 *   hmme_refine_pairs_bi_device, ... MV, TEncSearch.cpp:3726-3737) on whole pictures and picture pairs
 *   hmme_predict_pairs_w_device,  <- the same in a slice with explicit weighted prediction (TComPrediction::motionCompensation,
 *   hmme_search_pairs_bi_w_device,   TComPrediction.cpp:527-541 + addWeightUni for the other list, bApplyWeight with the searched list's
 *   hmme_refine_pairs_bi_w_device    weight)
 *   hmme_plane_*           <- the padded reference plane calcMotionVectors reads
 *                             (TComPicYuv, TLibCommon/TComPicYuv.cpp:91-92, 214-262); hmme_plane_upload_* take what
 *                             TVideoIOYuv::read delivers (TVideoIOYuv.cpp:247, :680: 8-bit or 16-bit little-endian samples)
 *   hmme_last_error        <- TEncOpenCL::checkError (TEncOpenCL.h:93-101)
 *   hmme_destroy           <- TEncOpenCL::~TEncOpenCL (TEncOpenCL.cpp:38-66)
 *
 * Results use the reference's slot order (TComDataCU::getIndexBlock, TComDataCU.cpp:3379-3391):
 * out_mv is laid out exactly like TComMv[NUM_CTU_PARTS] ({Short hor, Short ver}, integer pels)
 * and out_sad like Distortion[NUM_CTU_PARTS], so one memcpy fills
 * TEncSearch::allMotionVectors[list][refIdx] / allRuiCost[list][refIdx] (TEncSearch.h:114-115).
 *
 * Arithmetic is HM's CPU arithmetic (TEncSearch::xPatternSearch, TEncSearch.cpp:3835-3897):
 * predictor-relative MV cost, window LT..RB, strict '<' in raster order, optional FEN row
 * sub-sampling.  hmme_params_ocl_compat() selects what cl/sad.cl does instead (pred (0,0),
 * window LT..LT+2*SR, all rows).
 *
 * Threading: a context is not thread-safe; use one per host thread / per GPU.
 * Streams: a context owns scratch (job tables, merge tables, staging) that every frame call reuses, and planes are filled
 * asynchronously by hmme_plane_set_device_u8.  The library orders these itself: a *_device call issued on another stream than the
 * context's previous frame call first waits -- on the device, with hipStreamWaitEvent, never blocking the host -- for that call's
 * last use of the scratch, every search / refinement waits for the last fill of each plane it reads if that fill ran on
 * another stream, and every fill / upload of a plane waits for the last search / refinement that read it on another stream (so a
 * ring of planes can be refilled on a copy stream while the compute stream is still searching older contents: tools/me_sequence.py
 * --stream).  So calls of one context may be spread over streams; they serialise where they share scratch.  Output buffers
 * are the caller's: reading d_out_* on another stream than the one passed in needs the caller's own event.  The synchronous
 * host-facing calls run on a private non-blocking stream of the context and return when done.
 * Every function returns HMME_OK (0) or a negative HMME_ERR_* code; nothing ever falls back
 * to a CPU implementation.
 */
#ifndef HMME_H
#define HMME_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct of this header changes layout or an entry point changes meaning; hmme_abi_version() returns the value the
 * library was built with.  TEncOpenCL::findDevice and hmme/api.py refuse a library whose version differs from the header they were
 * written against (hmme_search_params grew by `shift_free` in version 2: a caller built against version 1 would have the library
 * read 4 bytes past its struct).  3: hmme_search_pairs_device / hmme_refine_pairs_device, asynchronous uploads, bi-prediction
 * origins in the refinement calls.  4: hmme_search_ctu_w (explicit weighted prediction); hmme_time_search_kernel and
 * hmme_debug_device_address left this header (include/hmme_test.h).  5: hmme_set_error_printing.  6: hmme_set_error_printing returns the
 * previous setting; frame calls refuse planes of another context. */
#define HMME_ABI_VERSION 6
int hmme_abi_version(void);
/* identifies the kernel sources + build flags the library was compiled from (bench.py ties committed counter summaries to it) */
const char* hmme_build_id(void);

#define HMME_NUM_CTU_PARTS 593 /* TLibCommon/TypeDef.h:263 */
#define HMME_CTU_SIZE 64
#define HMME_MAX_SEARCH_RANGE 128 /* any bit depth, frame and per-CTU calls: windows up to 257 x 257 candidates (8-bit windows beyond
                                      129 x 129 run as 2 x 2 tiles) */

enum {
  HMME_OK = 0,
  HMME_ERR_ARG = -1,     /* invalid argument (null pointer, window larger than sr_max, window / predictor beyond int16, ...) */
  HMME_ERR_DEVICE = -2,  /* no usable gfx950 device / HIP runtime error */
  HMME_ERR_RANGE = -3,   /* sample outside the range of the bit depth (bi-prediction origins of hmme_search_ctu excepted) */
  HMME_ERR_NOMEM = -4,
  HMME_ERR_UNSUPPORTED = -5
};

typedef struct hmme_ctx hmme_ctx;
typedef struct hmme_plane hmme_plane;

/* one (CTU, reference picture) search; integer-pel window, quarter-pel predictor */
typedef struct hmme_search_params {
  int lt_x, lt_y;      /* cMvSrchRngLT after xSetSearchRange (TEncSearch.cpp:3814-3830) */
  int rb_x, rb_y;      /* cMvSrchRngRB, inclusive */
  int pred_x, pred_y;  /* m_pcRdCost->setPredictor(*pcMvPred), quarter pels (TEncSearch.cpp:3737) */
  int fen;             /* m_pcEncCfg->getUseFastEnc() (TEncSearch.cpp:3853-3859) */
  int bit_depth;       /* 8 (packed-byte path) or 9..12 (16-bit path): SAD >> (bitDepth-8), TComRdCost.cpp:520-521 */
  int shift_free;      /* 1: no >> (bitDepth-8) on the SAD -- what cl/sad.cl computes for any Pel width;
                          bit_depth then only states the sample range.  A call is refused (HMME_ERR_UNSUPPORTED) when the samples it
                          was handed could produce a 64x64 sum + MV cost >= 8 000 000, i.e. when the largest |cur - ref| its two
                          blocks admit exceeds 1 937: never at <= 10 bit, never at 9 bit with bi-prediction origins */
} hmme_search_params;

/* one whole-picture search: window derived per CTU from the predictor exactly like
 * xSetSearchRange + TComDataCU::clipMv (TComDataCU.cpp:2907-2920) */
typedef struct hmme_frame_params {
  int search_range;  /* SearchRange (cfg/encoder_lowdelay_P_main.cfg:33) */
  int fen;           /* FEN (cfg/encoder_lowdelay_P_main.cfg:34) */
  int bit_depth;
  int ctu_first;     /* first CTU (raster order) and number of CTUs to search; count < 0 = to the end */
  int ctu_count;
} hmme_frame_params;

/* ---- context ------------------------------------------------------------------------- */
int hmme_create(int device, int sr_max, unsigned flags, hmme_ctx** out);
void hmme_destroy(hmme_ctx* ctx);
const char* hmme_last_error(const hmme_ctx* ctx); /* ctx may be NULL: error of the calling thread's last failed hmme_create */
/* A failed call prints its message on stderr (as TEncOpenCL::checkError does, TEncOpenCL.h:93-101) and keeps it for hmme_last_error.
 * on = 0 keeps it only -- for a caller that PROBES with a call it expects to be refused (TEncOpenCL's reference-mode call tries the
 * sample width it has latched and widens it on HMME_ERR_RANGE, instead of scanning every window for its largest sample first).
 * Returns the previous setting (1 / 0; 1 for a NULL context), so that a probe restores what its caller had chosen. */
int hmme_set_error_printing(hmme_ctx* ctx, int on);
const char* hmme_device_info(const hmme_ctx* ctx);
int hmme_device_index(const hmme_ctx* ctx);   /* the HIP device the context lives on (host code that makes its own HIP calls beside the library's) */
/* m_lambda = floor(65536*sqrt(lambda)).  HMME_ERR_ARG, the context's value unchanged, for a lambda that is negative, not a number, or
 * so large that 65536*sqrt(lambda) is not below 2^32 (lambda >= 2^32, infinity included): the conversion to uint32 is undefined there.
 * The largest accepted lambda gives 0xFFFFFFFF; every uint32 can be set through hmme_set_lambda_q16. */
int hmme_set_lambda(hmme_ctx* ctx, double lambda);
int hmme_set_lambda_q16(hmme_ctx* ctx, uint32_t lambda_q16);   /* any value: the MV cost is (lambda_q16 * bits) >> 16 with the product wrapping in 32 bits, as HM's */
uint32_t hmme_get_lambda_q16(const hmme_ctx* ctx);

/* the parameter set that reproduces the reference GPU path's choices */
void hmme_params_ocl_compat(hmme_search_params* p, int lt_x, int lt_y, int search_range);
/* xSetSearchRange + clipMv on the host (exported so callers and tests can derive LT/RB) */
void hmme_set_search_range(int pred_x_q, int pred_y_q, int search_range, int cu_x, int cu_y, int pic_w,
                           int pic_h, int* lt_x, int* lt_y, int* rb_x, int* rb_y);

/* ---- slot layout (TComDataCU::getIndexBlock, TComDataCU.cpp:3379-3391 + case table :4676-6461) ------ */
/* slot 0..592 of a PU: part_size = HM PartSize enum (0 2Nx2N, 1 2NxN, 2 Nx2N, 4 2NxnU, 5 2NxnD, 6 nLx2N, 7 nRx2N),
 * depth 0..3 (CU size 64 >> depth), part_idx 0/1, abs_z_idx = z-order address of the CU in 4x4 units.
 * Returns -1 for combinations the reference does not tabulate (NxN, AMP at 8x8). */
int hmme_slot_index(int part_size, int depth, int part_idx, int abs_z_idx);
/* rectangle of a slot inside the 64x64 CTU; returns 0 or HMME_ERR_ARG */
int hmme_slot_rect(int slot, int* x, int* y, int* w, int* h);
/* the inverse of hmme_slot_index: the key of slot 0..592 (what a reader of hmme_select_pairs_device's out_slot needs); 0 or HMME_ERR_ARG */
int hmme_slot_key(int slot, int* part_size, int* depth, int* part_idx, int* abs_z_idx);
/* The 425-entry table layout of an encoder built with AMP_ENC_SPEEDUP (TypeDef.h:206, :260-261; TComDataCU.cpp:3393-4675; the
 * reference's `calcSAD` kernel, cl/sad.cl:4-138) -- the macro is 0 in the reference tree as shipped, so this is a view for such a
 * build, not a second search: the same rectangles as the 593 layout without the AMP shapes.  hmme_slot_index_amp_off = that build's
 * getIndexBlock (-1 for what it does not tabulate); hmme_amp_off_slot maps an entry of the 425 layout to the slot of the 593
 * layout that holds the same rectangle; hmme_compact_amp_off turns a call's 593 results into the 425 tables. */
int hmme_slot_index_amp_off(int part_size, int depth, int part_idx, int abs_z_idx);
int hmme_amp_off_slot(int index_amp_off);
int hmme_compact_amp_off(const int16_t* mv593, const uint32_t* sad593, int16_t* mv425, uint32_t* sad425);

/* ---- per-CTU drop-in (host buffers, HM `Pel` = int16) --------------------------------- */
/* ctu: 64x64 current block (TEncSearch.cpp:3747); ref_at_ctu_origin: reference plane at the CTU
 * origin inside its padded buffer, as handed to calcMotionVectors.  Synchronous.  Current-block samples may be the
 * bi-prediction origin 2*org - pred (TEncSearch.cpp:3702-3712), i.e. lie in [-maxv, 2*maxv].
 * out_mv: int16[593][2] (hor, ver), out_sad: uint32[593] (pure SAD at the arg-min = ruiCost). */
int hmme_search_ctu(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref_at_ctu_origin,
                    int ref_stride, const hmme_search_params* p, int16_t* out_mv, uint32_t* out_sad);

/* The same search in a slice with explicit weighted prediction (TEncSearch::setWpScalingDistParam, TEncSearch.cpp:3740, :5594-5635:
 * m_cDistParam.bApplyWeight + wpCur): every candidate is priced by TComRdCostWeightPrediction::xGetSADw
 * (TComRdCostWeightPrediction.cpp:55-90), |org - (((w0 * ref + round) >> shift) + offset)| summed over EVERY row (p->fen is not
 * consulted: each xGetSAD* hands over to xGetSADw before it looks at iSubShift, TComRdCost.cpp:467-469), the prediction unclipped,
 * the whole-block sum >> (bitDepth-8).  `wp` = the luma WPScalingParam of the reference picture (w, offset, shift, round; TComSlice.h:1178-
 * 1190).  HMME_ERR_UNSUPPORTED when a weighted sample of the window would leave int16 (HM keeps it in a Pel and wraps; not
 * reproduced) or the sums could exceed the engine's cost field: the caller then searches on the CPU.  Integer search only. */
typedef struct hmme_weight { int w0, offset, shift, round; } hmme_weight;
int hmme_search_ctu_w(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref_at_ctu_origin, int ref_stride,
                      const hmme_search_params* p, const hmme_weight* wp, int16_t* out_mv, uint32_t* out_sad);
/* ... and with xPatternSearchFracDIF of the 593 winners in the same call, as hmme_search_refine_ctu: in such a slice the refinement's
 * distortion is xGetHADsw / xGetSADw (TComRdCostWeightPrediction.cpp:407-470) -- the interpolated, clipped prediction weighted sample by
 * sample before the difference is taken.  Additionally refused (HMME_ERR_UNSUPPORTED; hmme_search_ctu_w still serves the call) when
 * the weighted sample differences of the block could exceed 4095 (the Hadamard sums are kept exactly). */
int hmme_search_refine_ctu_w(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref_at_ctu_origin, int ref_stride,
                             const hmme_search_params* p, const hmme_weight* wp, int use_hadamard, int16_t* out_mv, uint32_t* out_sad,
                             int16_t* out_qmv, uint32_t* out_cost);
int hmme_refine_ctu_w(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref_at_ctu_origin, int ref_stride,
                      const hmme_search_params* p, const hmme_weight* wp, const int16_t* int_mv, int use_hadamard, int16_t* out_qmv,
                      uint32_t* out_cost);   /* the weighted refinement alone, at the caller's integer MVs (as hmme_refine_ctu) */

/* The step after the search, for the same CTU: TEncSearch::xPatternSearchFracDIF (TEncSearch.cpp:4294-4331, called per PU at :3798)
 * for all 593 slots -- half- then quarter-pel refinement around each slot's integer MV, HM's 8-tap interpolation, Hadamard
 * (use_hadamard, HadamardME) or SAD distortion, MV cost against p->pred.  out_qmv: int16[593][2] quarter-pel MVs
 * (int << 2) + (half << 1) + quarter; out_cost: uint32[593], the ruiCost xPatternSearchFracDIF returns (distortion + MV cost).
 * hmme_search_refine_ctu = hmme_search_ctu + the refinement of its winners in ONE call (block and window are staged once);
 * hmme_refine_ctu refines the caller's integer MVs int_mv[593][2] (entries outside the window LT..RB are clamped to it).
 * Unlike hmme_search_ctu these read the reference 4 samples (+ up to 3 for alignment) beyond the window (64 + 2*SR)^2 on every
 * side -- the interpolation filter's support, which xPatternSearchFracDIF reads as well (HM planes carry an 80-sample margin).
 * Bi-prediction origins (current-block samples in [-maxv, 2*maxv]: the bBi pass, TEncSearch.cpp:3702-3712, :3798) are refined
 * like any other block: the interpolated reference is clipped to the sample range, the origin is not.
 * shift_free: hmme_search_refine_ctu's integer leg honours it (out_sad unshifted); the refinement never does -- out_cost is always
 * HM's ((distortion >> (bitDepth-8)) + MV cost), so with shift_free = 1 at more than 8 bits the two outputs are on different
 * scales.  HM-arithmetic callers leave it 0. */
int hmme_search_refine_ctu(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref_at_ctu_origin, int ref_stride,
                           const hmme_search_params* p, int use_hadamard, int16_t* out_mv, uint32_t* out_sad, int16_t* out_qmv,
                           uint32_t* out_cost);
int hmme_refine_ctu(hmme_ctx* ctx, const int16_t* ctu, int ctu_stride, const int16_t* ref_at_ctu_origin, int ref_stride,
                    const hmme_search_params* p, const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost);

/* ---- frame path ------------------------------------------------------------------------ */
/* device-resident luma plane with edge-replicated margins; 8-bit planes store bytes, 9..12-bit planes u16.  Every plane also holds its picture
 * area once more CTU by CTU (64 x 64 blocks, contiguous: what a search reads the CURRENT picture from), so a plane costs about
 * (W + 256) x (H + 160) + W x H samples of device memory -- 17.9 MB for an 8-bit 2160p picture.
 * Any width and any height from 8 to 16384 is served by every call (odd ones too: no size has to be a multiple of anything; only the 4:2:0
 * chroma calls ask for an even luma size); outside that range hmme_plane_create* returns HMME_ERR_ARG.
 * A plane belongs to the context that created it: every frame call refuses planes of another context (HMME_ERR_ARG), and a
 * context's planes are destroyed BEFORE the context (hmme_plane_destroy reads its context). */
int hmme_plane_create(hmme_ctx* ctx, int width, int height, hmme_plane** out);   /* 8-bit */
int hmme_plane_create_ex(hmme_ctx* ctx, int width, int height, int bit_depth, hmme_plane** out);
void hmme_plane_destroy(hmme_plane* plane);
/* upload the width x height picture area of an HM plane (origin = sample (0,0)); borders are
 * re-extended on the device like TComPicYuv::extendPicBorder.  Samples outside [0, 2^bitDepth) are
 * rejected with HMME_ERR_RANGE */
int hmme_plane_upload_pel(hmme_plane* plane, const int16_t* origin, int stride);
int hmme_plane_upload_u8(hmme_plane* plane, const uint8_t* origin, int stride);
/* The same upload, asynchronous on `stream` (hipStream_t): returns once the copy and the border extension are enqueued.  origin:
 * samples of sample_bytes 1 (u8) or 2 (HM's Pel / the little-endian words of a 16-bit YUV file, TVideoIOYuv.cpp:247); any plane
 * bit depth.  The host buffer must stay untouched until the copy has run (the caller's event on `stream`) and should be page-locked
 * (hmme_host_register), otherwise the runtime stages it and the call blocks.  Ordering against searches that still read the
 * plane's previous contents on another stream is the library's (see "Streams").  A sample outside the plane's range cannot be
 * reported by this call: it is latched and returned -- once -- by the next hmme_upload_status (a latch of its own: synchronous
 * uploads of other planes neither see nor clear it). */
int hmme_plane_upload_async(hmme_plane* plane, const void* origin, int stride, int sample_bytes, void* stream);
/* waits for `stream`; HMME_ERR_RANGE if an upload since the last check carried an out-of-range sample */
int hmme_upload_status(hmme_ctx* ctx, void* stream);
/* Optional: page-lock a long-lived host buffer (e.g. the TComPicYuv planes of the decoded picture buffer,
 * TComPicYuv.cpp:80-133) so that uploads from it run at PCIe rate instead of through the runtime's pageable staging.
 * The buffer must stay allocated until hmme_host_unregister; uploads work with or without registration. */
int hmme_host_register(hmme_ctx* ctx, void* buffer, size_t bytes);
int hmme_host_unregister(hmme_ctx* ctx, void* buffer);
/* device-side producers (e.g. a torch tensor): copy a width x height u8 image that already
 * lives in device memory, then extend borders; asynchronous on `stream` (hipStream_t) */
int hmme_plane_set_device_u8(hmme_plane* plane, const void* d_src, int src_pitch, void* stream);
int hmme_plane_width(const hmme_plane* plane);
int hmme_plane_height(const hmme_plane* plane);
int hmme_plane_bit_depth(const hmme_plane* plane);

/* number of CTUs (partial edge CTUs included) of a width x height picture */
int hmme_num_ctus(int width, int height);

/* synchronous, host results.  pred_q: int16[n_ctu][2] quarter-pel predictors indexed by CTU
 * raster address, or NULL for (0,0).  out_mv: int16[count][593][2], out_sad: uint32[count][593] */
int hmme_search_frame(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp,
                      const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad);
/* asynchronous on `stream`, everything device-resident (d_pred_q may be NULL) */
int hmme_search_frame_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref,
                             const hmme_frame_params* fp, const void* d_pred_q, void* d_out_mv, void* d_out_sad,
                             void* stream);

/* several reference pictures of one current picture in ONE launch (HM's low-delay P configuration searches 4 per
 * picture, cfg/encoder_lowdelay_P_main.cfg:24-27).  refs: n_refs (<= 16) planes of the picture size.
 * pred_q: int16[n_refs][n_ctu][2] or NULL; out_mv: int16[n_refs][count][593][2]; out_sad: uint32[n_refs][count][593] */
int hmme_search_frame_multi(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs,
                            const hmme_frame_params* fp, const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad);
int hmme_search_frame_multi_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs,
                                   const hmme_frame_params* fp, const void* d_pred_q, void* d_out_mv, void* d_out_sad,
                                   void* stream);

/* Several (current, reference) picture PAIRS of one size in one launch (<= 16): an open-loop pass over a sequence (BASELINE config 4:
 * the pairs of cfg/encoder_randomaccess_main.cfg:28-31) searches small pictures several pairs at a time -- a single 1080p pair is
 * 510 workgroups, less than one round of the chip's 512 slots.  hmme_search_frame_multi_device is the case curs[i] == cur.
 * pred_q: int16[n_pairs][n_ctu][2] or NULL; out_mv: int16[n_pairs][count][593][2]; out_sad: uint32[n_pairs][count][593] */
int hmme_search_pairs_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, int n_pairs,
                             const hmme_frame_params* fp, const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream);

/* ---- fractional-pel refinement: the step after the integer search ------------------------------------------
 * TEncSearch::xPatternSearchFracDIF (TEncSearch.cpp:4294-4331) for every slot of every CTU: half- then quarter-pel
 * refinement around the slot's integer MV with HM's 8-tap interpolation, Hadamard (HadamardME = 1, xGetHADs) or SAD
 * distortion plus the MV cost.  int_mv: int16[n_refs][count][593][2] as produced by hmme_search_frame*.
 * out_qmv: quarter-pel MV (int << 2) + (half << 1) + quarter; out_cost: distortion + MV cost of the winner (the
 * ruiCost xPatternSearchFracDIF returns).  8..12-bit planes, any search range the search accepts.  Integer MVs outside
 * the CTU's search window (never produced by hmme_search_frame*) are clamped to it first. */
int hmme_refine_frame(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp,
                      const int16_t* pred_q, const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost);
int hmme_refine_frame_multi_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs,
                                   const hmme_frame_params* fp, const void* d_pred_q, const void* d_int_mv, int use_hadamard,
                                   void* d_out_qmv, void* d_out_cost, void* stream);

int hmme_refine_pairs_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, int n_pairs,
                             const hmme_frame_params* fp, const void* d_pred_q, const void* d_int_mv, int use_hadamard,
                             void* d_out_qmv, void* d_out_cost, void* stream);

/* ---- explicit weighted prediction on whole pictures and picture pairs ----------------------------------------
 * The picture-level siblings of hmme_search_ctu_w / hmme_refine_ctu_w (new entry points; no struct and no existing entry point
 * changed, so HMME_ABI_VERSION stays 6).  For pair i and CTU c the search returns what hmme_search_ctu_w returns for that CTU's
 * 64x64 block of curs[i] (partial edge CTUs completed by edge replication, as the plane's CTU-blocked copy holds them), the padded
 * refs[i], the window hmme_set_search_range gives for the CTU's predictor and the weight wps[i]: xGetSADw over EVERY row (fp->fen is
 * not consulted), the prediction unclipped, the block sum >> (bitDepth-8).  The refinement returns what hmme_refine_ctu_w returns at
 * the same inputs (xGetHADsw / xGetSADw: the interpolated, clipped prediction weighted sample by sample).  Lambda is the context's.
 * Array shapes, ctu_first / ctu_count, the limit of 16 pairs, plane ownership and stream ordering are those of
 * hmme_search_pairs_device / hmme_refine_pairs_device; wps: n_pairs weights in HOST memory, read before the call returns.
 * The weighted planes live in scratch of the context (one u16 plane per pair, grown on demand: 19 MB per 2160p pair), ordered
 * across streams like its other scratch.
 *
 * Refusal.  A frame call cannot scan its samples on the host the way the per-CTU call does, so hmme_weight_check decides from the
 * NOMINAL range [0, 2^bitDepth - 1] of both pictures -- the bound is therefore stricter than the per-CTU call's on tame content
 * (a weight that hmme_search_ctu_w accepts for a dark block may be refused here).  With span = the largest
 * |block - weighted sample| those ranges admit:
 *   shift outside 0..15 (or wp == NULL)                                          -> HMME_ERR_ARG
 *   a weighted sample beyond int16 (or w0 * sample + round beyond 32 bits), or block and
 *   weighted plane together spanning more than 16 bits                           -> HMME_ERR_UNSUPPORTED
 *   ((4096 * span) >> (bitDepth-8)) + 65535 >= 8 000 000 (the engine's cost field) -> HMME_ERR_UNSUPPORTED
 *   refine != 0: 4096 * span >= 2^24, or -- identity weights excepted -- |w0 * sample + round|
 *   >= 2^24 (the refinement's sums and its weighting are exact in fp32 below that)  -> HMME_ERR_UNSUPPORTED
 * hmme_weight_check is a pure host function: no context, no GPU.  Every frame call below first runs it for every pair
 * (refine = 1 in the refinement calls) and launches NOTHING if one pair fails: it returns that code, hmme_last_error names the pair;
 * no fallback, no partial work.  Identity weights (w0 == 1 << shift, offset 0, round == (shift ? 1 << (shift-1) : 0)) are served
 * by the unweighted kernels with FEN off. */
int hmme_weight_check(int bit_depth, const hmme_weight* wp, int refine);
int hmme_search_pairs_w_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, int n_pairs,
                               const hmme_frame_params* fp, const hmme_weight* wps, const void* d_pred_q, void* d_out_mv, void* d_out_sad,
                               void* stream);
int hmme_refine_pairs_w_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, int n_pairs,
                               const hmme_frame_params* fp, const hmme_weight* wps, const void* d_pred_q, const void* d_int_mv, int use_hadamard,
                               void* d_out_qmv, void* d_out_cost, void* stream);
/* synchronous, host results, one pair: the weighted siblings of hmme_search_frame / hmme_refine_frame */
int hmme_search_frame_w(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp, const hmme_weight* wp,
                        const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad);
int hmme_refine_frame_w(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_frame_params* fp, const hmme_weight* wp,
                        const int16_t* pred_q, const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost);

/* ---- bi-prediction on whole pictures and picture pairs --------------------------------------------------------
 * The picture-level siblings of the bBi pass that hmme_search_ctu / hmme_refine_ctu serve one CTU at a time (TEncSearch.cpp:3702-3712,
 * :3726-3737, :3798; new entry points, no struct and no existing entry point changed, so HMME_ABI_VERSION stays 6), and the
 * motion compensation they are built on.
 *
 * Motion field.  d_mv_field / d_other_mv: quarter-pel MVs int16[n_pairs][n_ctu][mv_per_ctu][2] (hor, ver), n_ctu = ALL CTUs of the
 * picture in raster order whatever ctu_first / ctu_count select.  mv_per_ctu = 1: one MV per CTU (HM's 64x64 2Nx2N); 64: one per 8x8 block,
 * raster order inside the CTU (hmme_select_pairs_device writes it from the 593-slot tables).  Every MV is first clamped like TComDataCU::clipMv
 * (TComDataCU.cpp:2907-2920) for its CTU's position -- MVs out of the engine's own tables are never changed by that.
 *
 * hmme_predict_pairs_device: for picture i the luma prediction of every 8x8 block from the padded refs[i] at the block's MV: HM's 8-tap
 * DCT-IF, horizontal into the 14-bit intermediate, then vertical, rounded and clipped to the sample range -- the uni-directional
 * prediction TComPrediction::xPredInterBlk writes with bi = false (TComPrediction.cpp:590-594, :669), integer arithmetic, bit-exact at
 * all 16 phases.  d_outs: HOST array of n_pairs device images of out_pitch_bytes per row, samples of the plane's type (u8 for 8-bit
 * planes, u16 otherwise); only samples inside the picture AND inside the CTUs [ctu_first, ctu_first + ctu_count) are written.
 * fp->search_range and fp->fen are not consulted.  hmme_predict_frame: synchronous, one picture, host field and host image (out_stride in
 * samples; samples outside the CTU range keep their values).
 *
 * hmme_search_pairs_bi_device: for pair i and CTU c what hmme_search_ctu returns for
 *   - the 64x64 block O = 2 * B - P (unclipped: DISABLING_CLIP_FOR_BIPREDME), B = the CTU's block of curs[i] (partial edge CTUs completed
 *     by edge replication, as the plane's CTU-blocked copy holds them), P = the prediction above from others[i] with pair i's field;
 *   - refs[i] at the CTU origin; the window hmme_set_search_range(centre, fp->search_range, ...) with centre = d_center_q[i][c]
 *     (int16[n_pairs][n_ctu][2], quarter pels: the list's current MV) or, d_center_q == NULL, the predictor;
 *   - the predictor d_pred_q[i][c] (NULL: (0,0)) for the MV cost, fp->fen (honoured: the bi pass does not set bApplyWeight) and
 *     fp->bit_depth.  fp->search_range is the bi-prediction range (HM's BipredSearchRange, default 4); any range the 16-bit path accepts.
 * hmme_refine_pairs_bi_device: what hmme_refine_ctu returns at the same inputs for the integer MVs d_int_mv; it rebuilds the origin
 * itself.  As in the per-CTU call and the reference ALL 593 slots are searched against the one origin of their CTU; with
 * mv_per_ctu = 64 that origin is built block by block from the caller's field -- which slots that makes meaningful (those whose
 * rectangle the field's MVs describe) is the caller's business.  Lambda is the context's.  Array shapes, ctu_first / ctu_count, the limit
 * of 16 pairs, plane ownership and stream ordering are those of hmme_search_pairs_device / hmme_refine_pairs_device; others[i] must have
 * the size and bit depth of its pair and is ordered like a reference.  Origins and u16 copies live in the scratch of the weighted calls.
 * In a slice with explicit weighted prediction the *_bi_w_* calls further down take their place.
 *
 * Refusal.  hmme_bipred_check decides from the NOMINAL sample range: with maxv = 2^bitDepth - 1 the origin lies in [-maxv, 2 * maxv] and is
 * staged with the bias maxv, so block and reference copy span [0, 3 * maxv]; span = 2 * maxv is the largest |origin - reference sample|:
 *   bit depth outside 8..12                                                           -> HMME_ERR_ARG
 *   3 * maxv > 65535 (the 16-bit search's sample span)                                -> HMME_ERR_UNSUPPORTED
 *   ((4096 * span) >> (bitDepth-8)) + 65535 >= 8 000 000 (the engine's cost field)     -> HMME_ERR_UNSUPPORTED
 *   refine != 0: 4096 * span >= 2^24 (the refinement's sums are exact in fp32 below)   -> HMME_ERR_UNSUPPORTED
 * which gives       bit depth      8    9    10   11   12
 *                   refine = 0     ok   ok   ok   ok   ok
 *                   refine = 1     ok   ok   ok   ok   HMME_ERR_UNSUPPORTED
 * (the per-CTU calls scan their samples instead and refuse none of these).  A pure host function: no context, no GPU.  Every call below
 * runs it first (refine = 1 in the refinement calls, 0 elsewhere) and launches NOTHING when it fails: it returns that code,
 * hmme_last_error says why; no fallback, no partial work. */
int hmme_bipred_check(int bit_depth, int refine);
int hmme_predict_pairs_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_pairs, const hmme_frame_params* fp, const void* d_mv_field,
                              int mv_per_ctu, void* const* d_outs, int out_pitch_bytes, void* stream);
int hmme_predict_frame(hmme_ctx* ctx, const hmme_plane* ref, const hmme_frame_params* fp, const int16_t* mv_field, int mv_per_ctu, void* out,
                       int out_stride);
int hmme_search_pairs_bi_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others,
                                int n_pairs, const hmme_frame_params* fp, const void* d_other_mv, int mv_per_ctu, const void* d_center_q,
                                const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream);
int hmme_refine_pairs_bi_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others,
                                int n_pairs, const hmme_frame_params* fp, const void* d_other_mv, int mv_per_ctu, const void* d_center_q,
                                const void* d_pred_q, const void* d_int_mv, int use_hadamard, void* d_out_qmv, void* d_out_cost, void* stream);
/* synchronous, host arrays, one pair: other_mv int16[n_ctu][mv_per_ctu][2]; center_q / pred_q int16[n_ctu][2] or NULL */
int hmme_search_frame_bi(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_plane* other, const hmme_frame_params* fp,
                         const int16_t* other_mv, int mv_per_ctu, const int16_t* center_q, const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad);
int hmme_refine_frame_bi(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_plane* other, const hmme_frame_params* fp,
                         const int16_t* other_mv, int mv_per_ctu, const int16_t* center_q, const int16_t* pred_q, const int16_t* int_mv,
                         int use_hadamard, int16_t* out_qmv, uint32_t* out_cost);

/* ---- bi-prediction with explicit weighted prediction on whole pictures and picture pairs ------------------------
 * The calls above in a slice with explicit weighted prediction (HM: WeightedPredB), where the *_w and the _bi_ calls meet.  New entry points,
 * no struct and no existing entry point changed, so HMME_ABI_VERSION stays 6.  Every pair carries TWO weights, both arrays of n_pairs in HOST
 * memory, read before the call returns: wps[i] for refs[i] (the searched list) and other_wps[i] for others[i].  THIS TEXT PLUS THE CITATIONS IS
 * THE RULE (paths below source/Lib of the reference).
 *
 * 1. The other list's prediction is what TComPrediction::motionCompensation writes in a slice whose PPS has getUseWP()
 *    (TLibCommon/TComPrediction.cpp:527-541): xPredInterUni with bi = true leaves the 14-bit intermediate P -- no rounding, no clip, the
 *    vertical stage with shift 6 and offset 0, the copy case (src << (14 - bd)) - 8192 --, then xWeightedPredictionUni -> addWeightUni
 *    (TLibCommon/TComWeightPrediction.cpp:52-55, :133-180) with w0, offset, shift of getWpScaling (:250-262), the fields of hmme_weight:
 *        shift' = wp.shift + max(2, 14 - bd)
 *        round' = 1 << (shift' - 1)              (recomputed there: wp.round is NOT used)
 *        pred   = ClipBD(((w0 * (P + 8192) + round') >> shift') + offset)
 *    With w0 == 1 << shift and offset == 0 (whatever wp.round holds) this equals the bi = false prediction of hmme_predict_pairs_device at
 *    every phase and bit depth -- nested floors: ((P + 8192 + 2^(head-1)) >> head) is the rounding of its vertical pass -- and the engine
 *    relies on that: such a weight runs the unweighted prediction.
 *    Quirk of the reference, kept: TComPrediction.cpp:529 tests the P-slice flag getUseWP(), not getWPBiPred().  In a B slice with
 *    WeightedPredB = 1 and WeightedPredP = 0 the other list's prediction is therefore unweighted while the distortion is weighted; the two
 *    weights are independent arguments here, and such a caller passes the identity for the other list.
 * 2. The origin is 2 * org - pred, unclipped (TEncSearch.cpp:3702-3712, TComYuv::removeHighFreq); pred is clipped, so the origin lies in
 *    [-maxv, 2 * maxv] as without weights.
 * 3. The search runs with bApplyWeight and the SEARCHED list's weight (setWpScalingDistParam, TEncSearch.cpp:3740, :5594-5635): the integer
 *    search prices xGetSADw -- every row, fp->fen not consulted, the prediction unclipped, the block sum >> (bd - 8) --, the refinement
 *    xGetHADsw / xGetSADw; the window is centred on the list's own MV, MV bits are priced against the predictor (:3726-3737).
 *
 * hmme_predict_pairs_w_device / hmme_predict_frame_w: hmme_predict_pairs_device / hmme_predict_frame with one weight per picture; they write
 * step 1's pred.
 * hmme_search_pairs_bi_w_device: for pair i and CTU c what hmme_search_ctu_w returns for the block 2 * B - pred(others[i], field, other_wps[i]),
 * refs[i] at the CTU origin, the window around d_center_q (NULL: the predictor) and the weight wps[i].  hmme_refine_pairs_bi_w_device: what
 * hmme_refine_ctu_w returns at the same inputs.  Shapes, the limit of 16 pairs, mv_per_ctu 1 | 64, CTU sub-ranges, plane ownership and stream
 * ordering are those of hmme_search_pairs_bi_device.  A pair whose other weight is the identity uses the unweighted prediction; a launch in
 * which every weight of both lists is the identity IS hmme_search_pairs_bi_device / hmme_refine_pairs_bi_device with fen = 0.
 *
 * Refusal.  hmme_bipred_weight_check decides from the NOMINAL ranges: the origin in [-maxv, 2 * maxv], the reference in [0, maxv].  With
 * wlo / whi the extremes of the searched list's weighted sample ((w0 * v + round) >> shift) + offset over that range,
 * bias = max(maxv, -wlo) (what keeps origin and weighted plane unsigned) and span = max(2 * maxv - wlo, whi + maxv):
 *   bit depth outside 8..12, a NULL weight, a shift outside 0..15 (either weight)          -> HMME_ERR_ARG
 *   searched weight: a weighted sample beyond int16, or w0 * sample + round beyond 32 bits  -> HMME_ERR_UNSUPPORTED
 *   searched weight: max(whi, 2 * maxv) + bias > 65535                                      -> HMME_ERR_UNSUPPORTED
 *   searched weight: ((4096 * span) >> (bitDepth-8)) + 65535 >= 8 000 000                    -> HMME_ERR_UNSUPPORTED
 *   searched weight, refine != 0: 4096 * span >= 2^24, or -- identity weights excepted --
 *   |w0 * sample + round| >= 2^24                                                           -> HMME_ERR_UNSUPPORTED
 *   other weight: |w0| * 40 960 + round' beyond int32 (P is a Pel, so P + 8192 lies within
 *   [-24 576, 40 959]); nothing else, because the result is clipped                         -> HMME_ERR_UNSUPPORTED
 * With the identity for both lists this is hmme_bipred_check: the 12-bit refinement stays refused for every weight.  A pure host function:
 * no context, no GPU.  Every call below runs it for every pair first (refine = 1 in the refinement calls; the prediction calls apply the
 * other weight's lines to their one weight) and launches NOTHING if one pair fails: it returns that code, hmme_last_error names the pair. */
int hmme_bipred_weight_check(int bit_depth, const hmme_weight* wp, const hmme_weight* other_wp, int refine);
int hmme_predict_pairs_w_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_pairs, const hmme_frame_params* fp, const hmme_weight* wps,
                                const void* d_mv_field, int mv_per_ctu, void* const* d_outs, int out_pitch_bytes, void* stream);
int hmme_predict_frame_w(hmme_ctx* ctx, const hmme_plane* ref, const hmme_frame_params* fp, const hmme_weight* wp, const int16_t* mv_field,
                         int mv_per_ctu, void* out, int out_stride);
int hmme_search_pairs_bi_w_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others,
                                  int n_pairs, const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, const void* d_other_mv,
                                  int mv_per_ctu, const void* d_center_q, const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream);
int hmme_refine_pairs_bi_w_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others,
                                  int n_pairs, const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, const void* d_other_mv,
                                  int mv_per_ctu, const void* d_center_q, const void* d_pred_q, const void* d_int_mv, int use_hadamard, void* d_out_qmv,
                                  void* d_out_cost, void* stream);
/* synchronous, host arrays, one pair: the weighted siblings of hmme_search_frame_bi / hmme_refine_frame_bi */
int hmme_search_frame_bi_w(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_plane* other, const hmme_frame_params* fp,
                           const hmme_weight* wp, const hmme_weight* other_wp, const int16_t* other_mv, int mv_per_ctu, const int16_t* center_q,
                           const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad);
int hmme_refine_frame_bi_w(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_plane* other, const hmme_frame_params* fp,
                           const hmme_weight* wp, const hmme_weight* other_wp, const int16_t* other_mv, int mv_per_ctu, const int16_t* center_q,
                           const int16_t* pred_q, const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost);

/* ---- partition decision and motion field from the 593-slot tables ---------------------------------------------
 * The step between the uni-directional searches and the calls that take a motion field (hmme_predict_pairs_device, hmme_search_pairs_bi_device,
 * hmme_refine_pairs_bi_device), on the device: per CTU a bottom-up decision over the 593 costs which of the overlapping PU shapes to use -- a CU
 * quadtree with one PartSize per CU -- written as one MV per block, the slot that covers every block, and the CTU's cost.  The reference has no
 * counterpart (there the choice is HM's serial RD loop reading the tables one PU at a time), so THIS TEXT IS THE RULE.  New entry points and one
 * new struct; nothing existing changed, so HMME_ABI_VERSION stays 6.
 *
 * Inputs, per pair and per searched CTU: mv[593][2] and cost[593] exactly as a search or refinement call wrote them for the same ctu_first /
 * ctu_count (d_mv: int16[n_pairs][count][593][2], d_cost: uint32[n_pairs][count][593]), and optionally the CTU's predictor
 * d_pred_q[i][c] (int16[n_pairs][n_ctu][2], quarter pels, indexed by CTU raster address; NULL: (0,0)).
 *
 * Parameters (hmme_select_params; hmme_select_check returns HMME_ERR_ARG for anything outside these ranges):
 *   mv_per_ctu  64: one MV per 8x8 block, raster order inside the CTU -- the layout of hmme_predict_pairs_device and the _bi_ calls.  A PartSize
 *               of a CU is then a candidate only if all its PU rectangles are 8-aligned in position and size: 2Nx2N only at 8x8, no AMP at
 *               16x16, every shape at 32x32 and 64x64.
 *               256: one MV per 4x4 block, raster order (HM's own motion storage granularity); all 593 slots take part.
 *   mv_unit     0: the MVs are quarter-pel (out_qmv of a refinement) and are copied; 1: integer-pel (out_mv of a search), written << 2.
 *   price_mv    1 adds HM's MV cost to every slot's cost before anything is compared, priced against the CTU's predictor with the context's
 *               lambda: for integer MVs (mv_unit 1) the search's own (lambda_q16 * (bits((x << 2) - px) + bits((y << 2) - py))) >> 16, for
 *               quarter-pel MVs (lambda_q16 * (bits(qx - px) + bits(qy - py))) >> 16 -- TComRdCost::getCost with cost scale 2 / 0, the product
 *               wrapping in 32 bits as there.  For the pure-SAD tables of the integer search, which otherwise always split to the bottom;
 *               refinement costs already contain the MV cost, so callers pass 0 with them.
 *   part_mask   bit p set: PartSize p (0, 1, 2, 4, 5, 6, 7) is allowed.  Bit 0 must be set; bit 3 and bits above 7 must be clear.
 *   min_depth <= max_depth, both in 0..3 (CU size 64 >> depth).
 *   cu_cost, pu_cost   each <= 2^20, added once per coded CU and once per PU: the caller's model of mode bits.
 *
 * Decision.
 *   1. The cost of (CU, PartSize) is cu_cost plus the sum over its PUs of (slot cost + pu_cost).
 *   2. A CU's own best is the smallest cost over the allowed PartSizes; comparison is strict '<' in the order 0, 1, 2, 4, 5, 6, 7, so the lower
 *      enum wins ties.
 *   3. Presence at picture edges.  A CU at depth < max_depth may be a leaf only if depth >= min_depth and it lies wholly inside the picture;
 *      otherwise it must split.  A CU at max_depth exists if and only if its origin is inside the picture; its cost is over the whole
 *      rectangle, as the tables have it (edge replication).  A CU that does not exist costs 0 and codes nothing.
 *   4. Bottom-up: a CU that may be a leaf stays one unless the sum of its four children is strictly smaller -- the parent wins ties.
 *   5. Sums are carried in 64 bits; out_cost saturates at UINT32_MAX; nothing else is clamped (an integer MV << 2 keeps its low 16 bits).
 *
 * Outputs.  d_out_field: int16[n_pairs][n_ctu][mv_per_ctu][2], n_ctu = ALL CTUs of the picture, as the _bi_ calls index their fields; only the
 * entries of the CTUs in [ctu_first, ctu_first + ctu_count) are written.  d_out_slot (may be NULL): uint16[n_pairs][n_ctu][mv_per_ctu], the slot
 * whose PU covers the block -- 0xFFFF, with MV (0,0), for blocks of CUs that do not exist.  d_out_cost (may be NULL): uint32[n_pairs][n_ctu].
 *
 * hmme_select_pairs_device: asynchronous on `stream`, up to 16 pairs.  It takes no planes -- the picture size comes as two ints -- and of fp only
 * ctu_first / ctu_count are consulted.  It uses no scratch of the context, so it is ordered like any kernel of the caller on `stream` and
 * against nothing else.  Buffers: tables, costs and slots 4-byte aligned, the field 8-byte aligned.  It runs hmme_select_check first and
 * launches nothing when that fails.  hmme_select_frame: synchronous, host arrays of the same shapes with n_pairs = 1, on the context's private
 * stream; entries outside the CTU range keep their values. */
typedef struct hmme_select_params {
  int mv_per_ctu;
  int mv_unit;
  int price_mv;
  unsigned part_mask;
  int min_depth, max_depth;
  uint32_t cu_cost, pu_cost;
} hmme_select_params;
int hmme_select_check(const hmme_select_params* sel);
int hmme_select_pairs_device(hmme_ctx* ctx, int width, int height, int n_pairs, const hmme_frame_params* fp, const hmme_select_params* sel,
                             const void* d_mv, const void* d_cost, const void* d_pred_q, void* d_out_field, void* d_out_slot, void* d_out_cost,
                             void* stream);
int hmme_select_frame(hmme_ctx* ctx, int width, int height, const hmme_frame_params* fp, const hmme_select_params* sel, const int16_t* mv,
                      const uint32_t* cost, const int16_t* pred_q, int16_t* out_field, uint16_t* out_slot, uint32_t* out_cost);

/* ---- the reference picture per PU, and the prediction from it ----------------------------------------------------
 * hmme_search_frame_multi_device / hmme_refine_frame_multi_device (and hmme_search_pairs_device in general) leave one 593-slot table per
 * reference picture and CTU; an encoder needs, per PU, the best (refIdx, MV) of the list -- the loop over iRefIdxTemp in
 * TEncSearch::predInterSearch (source/Lib/TLibEncoder/TEncSearch.cpp:3027-3094) -- and the partition decided on those winners.  The calls
 * below do both on the device and predict from the result.  New entry points only; no struct and no existing entry point changed, so
 * HMME_ABI_VERSION stays 6.  THIS TEXT PLUS THE CITATIONS IS THE RULE.
 *
 * Inputs of the decision.  d_mv: int16[n_pics][n_refs][count][593][2], d_cost: uint32[n_pics][n_refs][count][593] -- exactly what
 * hmme_search_frame_multi_device / hmme_refine_frame_multi_device write for one picture (n_pics = 1), and what hmme_search_pairs_device /
 * hmme_refine_pairs_device write when their pairs are ordered picture-major (pair = picture * n_refs + reference).  d_pred_q:
 * int16[n_pics][n_refs][n_ctu][2], quarter pels, one predictor per reference and CTU as the multi-reference search takes them; NULL: (0,0).
 * ref_cost: HOST array of n_refs prices, one per reference index, read before the call returns; NULL: all zero.
 * Limits: n_refs in 1..16, n_pics >= 1, n_pics * n_refs <= 16, every ref_cost[r] <= 2^20; sel as hmme_select_check has it, unchanged.
 * hmme_select_refs_check (a pure host function: no context, no GPU) returns HMME_ERR_ARG for anything outside these limits; the calls run
 * it first and launch NOTHING when it fails.
 *
 * Rule.
 *   1. The priced cost of slot s in reference r is cost[r][s], plus -- if sel->price_mv -- HM's MV cost of mv[r][s] against reference r's
 *      OWN predictor (the two formulas of price_mv above, for mv_unit 1 / 0, the product wrapping in 32 bits), plus ref_cost[r]; the sum
 *      is carried in 64 bits.
 *   2. Slot s takes the reference with the smallest priced cost; comparison is strict '<' in the order r = 0, 1, ..., so the lowest index
 *      wins ties, as a later reference wins in HM only on uiCostTemp < uiCost[iRefList] (:3086).  Every slot of a CTU chooses on its own:
 *      the two PUs of one CU may use different references, as in HM.
 *   3. The decision of hmme_select_pairs_device, its steps 1-5 word for word, runs on the merged slots with the merged priced cost (64
 *      bits, not saturated) standing for "slot cost"; the MV cost is not applied a second time.
 *   4. Outputs -- only the entries of the CTUs in [ctu_first, ctu_first + ctu_count) are written, as in the select call:
 *        d_out_field  int16[n_pics][n_ctu][mv_per_ctu][2]   the winner's MV (<< 2 if mv_unit), (0,0) for blocks of CUs that do not exist
 *        d_out_ref    uint8[n_pics][n_ctu][mv_per_ctu]      the winner's reference index, 0xFF for blocks of CUs that do not exist; not NULL
 *        d_out_slot   uint16[n_pics][n_ctu][mv_per_ctu]     the covering slot, 0xFFFF likewise; may be NULL
 *        d_out_cost   uint32[n_pics][n_ctu]                 the CTU's cost, saturated at UINT32_MAX; may be NULL
 * With n_refs = 1 and ref_cost = {0} field, slots and costs are bit for bit those of hmme_select_pairs_device and every existing block has
 * reference 0.
 *
 * Reference-index bits.  hmme_ref_idx_bits(n_refs, r) is HM's count (:3030-3037): 0 when n_refs == 1, otherwise r + 1, minus 1 when
 * r == n_refs - 1 (the last index needs no terminating bin); -1 for arguments outside 0 <= r < n_refs <= 16.  A caller who wants HM's price
 * passes ref_cost[r] = (lambda_q16 * bits) >> 16.  HM floors getCost ONCE over the summed bits -- MV bits and reference-index bits together
 * (the closing lines of TEncSearch::xMotionEstimation) -- so an additive ref_cost can differ from HM's total by at most 1.  ref_cost is the
 * caller's model, like cu_cost / pu_cost.
 *
 * hmme_select_refs_device: asynchronous on `stream`; like hmme_select_pairs_device it takes no planes, consults of fp only ctu_first /
 * ctu_count, uses no scratch of the context and is ordered like any kernel of the caller on `stream`.  Buffers: tables, costs and slots
 * 4-byte aligned, the field 8-byte, the reference indices 2-byte.  hmme_select_refs_frame: synchronous, host arrays of the same shapes with
 * n_pics = 1, on the context's private stream; entries outside the CTU range keep their values.
 *
 * Prediction.  hmme_predict_refs_device is hmme_predict_pairs_device for ONE picture, except that the block of every MV reads the plane
 * refs[d_ref_field[ctu][block]]: d_mv_field int16[n_ctu][mv_per_ctu][2], d_ref_field uint8[n_ctu][mv_per_ctu], mv_per_ctu 1 | 64 (what the
 * decision writes with mv_per_ctu = 64), d_out one device image of out_pitch_bytes per row.  A block whose index is >= n_refs -- 0xFF
 * included -- is not written and reads nothing.  All refs (1..16) must have one size and fp's bit depth and belong to the context; each is
 * ordered across streams like any reference.  With one explicit weight per reference: hmme_predict_refs_w_device, further down.
 * hmme_predict_refs_frame: synchronous, host motion field, reference field and image (out_stride in samples; samples outside the CTU
 * range and of blocks without a reference keep their values). */
int hmme_ref_idx_bits(int n_refs, int ref_idx);
int hmme_select_refs_check(const hmme_select_params* sel, int n_pics, int n_refs, const uint32_t* ref_cost);
int hmme_select_refs_device(hmme_ctx* ctx, int width, int height, int n_pics, int n_refs, const hmme_frame_params* fp, const hmme_select_params* sel,
                            const uint32_t* ref_cost, const void* d_mv, const void* d_cost, const void* d_pred_q, void* d_out_field, void* d_out_ref,
                            void* d_out_slot, void* d_out_cost, void* stream);
int hmme_select_refs_frame(hmme_ctx* ctx, int width, int height, int n_refs, const hmme_frame_params* fp, const hmme_select_params* sel,
                           const uint32_t* ref_cost, const int16_t* mv, const uint32_t* cost, const int16_t* pred_q, int16_t* out_field, uint8_t* out_ref,
                           uint16_t* out_slot, uint32_t* out_cost);
int hmme_predict_refs_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, const hmme_frame_params* fp, const void* d_mv_field,
                             const void* d_ref_field, int mv_per_ctu, void* d_out, int out_pitch_bytes, void* stream);
int hmme_predict_refs_frame(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, const hmme_frame_params* fp, const int16_t* mv_field,
                            const uint8_t* ref_field, int mv_per_ctu, void* out, int out_stride);

/* ---- L0, L1 or bi per PU, and the prediction of a picture whose blocks are L0, L1 or bi -------------------------------------
 * What TEncSearch::predInterSearch ends in for a B picture (paths below source/Lib/TLibEncoder of the reference): every PU takes the
 * cheapest of list 0, list 1 and bi (TEncSearch.cpp:3291, :3314), the costs being those of xMotionEstimation's closing line (:3808),
 * floor(fWeight * (cost - mvcost)) + getCost(bits) with fWeight 0.5 in the bi pass; and the prediction of a bi PU, TComYuv::addAvg
 * (TLibCommon/TComYuv.cpp:352-390) over the two 14-bit intermediates.  New entry points and one new struct; no struct and no existing entry
 * point changed, so HMME_ABI_VERSION stays 6.  THIS TEXT PLUS THE CITATIONS IS THE RULE.
 *
 * Inputs of the decision, for n_pics B pictures (1..4), four table sets each, all quarter-pel refinement tables written for the same
 * ctu_first / ctu_count:
 *   d_mv_uni  int16[n_pics][2][count][593][2], d_cost_uni uint32[n_pics][2][count][593]: the uni-directional refinement of list 0 and list 1
 *             -- what hmme_refine_pairs_device writes with its pairs ordered (picture, list).
 *   d_mv_bi, d_cost_bi: the same shapes; set [p][l] is what hmme_refine_pairs_bi_device wrote when list l was searched against the origin
 *             built from list 1-l's field.
 *   d_uni_field  int16[n_pics][2][n_ctu][64][2]: list l's uni-directional field, indexed by list and NOT swapped -- the field the bi pass of
 *             list 1-l consumed as d_other_mv.
 *   d_pred_q  int16[n_pics][2][n_ctu][2], quarter pels, or NULL for (0,0): the predictors the searches took.
 *   dirs      HOST array of n_pics hmme_dir_params, read before the call returns: the caller's model of uiMbBits[3] (:2969, :3534-3557;
 *             dir_bits[0], [1], [2] for list 0, list 1 and bi) and of each list's reference-index plus MVP-index bits (list_bits).  Every
 *             value <= 4096.
 *   sel       an hmme_select_params with mv_per_ctu == 64, mv_unit == 0 and price_mv == 0 (the tables are refinement tables, whose costs
 *             contain the MV cost).  8x4 and 4x8 PUs never take part at this granularity, so HM's isBipredRestriction does not arise.
 * hmme_select_dirs_check (a pure host function: no context, no GPU) returns HMME_ERR_ARG for a sel hmme_select_check refuses or with
 * another mv_per_ctu / mv_unit / price_mv, n_pics outside 1..4, a NULL dirs, or a bit count above 4096; the calls run it first and launch
 * NOTHING when it fails.
 *
 * Definitions.  mvb(v, p) = bits(vx - px) + bits(vy - py): HM's getBits at cost scale 0, the count behind price_mv's quarter-pel formula.
 * gc(n) = (lambda_q16 * n) >> 16 with the context's lambda, the product wrapping in 32 bits as in TComRdCost::getCost.  Everything else is
 * carried in 64 bits.
 *
 * Rule, per slot s (pred[l] = list l's predictor of the CTU):
 *   1. D_U[l] = max(0, cost_uni[l][s] - gc(mvb(mv_uni[l][s], pred[l])))
 *      C[l]   = D_U[l] + gc(dir_bits[l] + list_bits[l] + mvb(mv_uni[l][s], pred[l]))
 *      On tables of the engine cost >= gc(mvb) always holds (the cost contains that term): the clamp is a formality.
 *   2. D_B[l] = max(0, cost_bi[l][s] - gc(mvb(mv_bi[l][s], pred[l]))) >> 1
 *      C_B[l] = D_B[l] + gc(dir_bits[2] + list_bits[0] + list_bits[1] + mvb(mv_bi[l][s], pred[l]) + mvb(mv_uni[1-l][s], pred[1-l]))
 *      The other list's motion bits are those of its uni slot s.  That is exact for the slot whose rectangle the consumed field describes
 *      (slot 592 with one MV per CTU); for every other slot it is the caller's model, like dir_bits and list_bits.
 *   3. The bi candidate is C_B[0] unless C_B[1] < C_B[0]: strict, list 0 is tried first (:3183-3186, :3226).
 *   4. C_bi <= C[0] && C_bi <= C[1]: direction 3; otherwise C[0] <= C[1]: direction 1; otherwise direction 2 -- HM's interDir values and HM's
 *      comparisons (:3291, :3314).
 *   5. The decision of hmme_select_pairs_device, its steps 1-5 word for word, runs on the merged slots with the winner's cost (64 bits, not
 *      saturated) standing for "slot cost"; no MV cost is applied again.
 * Outputs -- only the entries of the CTUs in [ctu_first, ctu_first + ctu_count) are written:
 *   d_out_field  int16[n_pics][2][n_ctu][64][2], list-major, so that each half feeds the predict and _bi_ calls.  A block under a
 *                direction-1 or -2 slot holds the winner's MV in its list and (0,0) in the other.  Under a direction-3 slot whose bi
 *                candidate searched list l it holds mv_bi[l][s] in list l and, in list 1-l, THE BLOCK'S OWN ENTRY OF d_uni_field[1-l]:
 *                the motion the bi cost was measured with.  (0,0) in both lists for blocks of CUs that do not exist.
 *   d_out_dir    uint8[n_pics][n_ctu][64]: 1, 2 or 3; 0xFF for blocks of CUs that do not exist; not NULL
 *   d_out_slot   uint16[n_pics][n_ctu][64], the covering slot, 0xFFFF likewise; may be NULL
 *   d_out_cost   uint32[n_pics][n_ctu], the CTU's cost, saturated at UINT32_MAX; may be NULL
 * hmme_select_dirs_device: asynchronous on `stream`; like its siblings it takes no planes, consults of fp only ctu_first / ctu_count, uses
 * no scratch of the context and is ordered like any kernel of the caller on `stream`.  Buffers: tables, costs, the input field and slots
 * 4-byte aligned, the output field 8-byte, the directions 2-byte.  hmme_select_dirs_frame: synchronous, host arrays of the same shapes with
 * n_pics = 1 (dir: the one hmme_dir_params), on the context's private stream; entries outside the CTU range keep their values.
 *
 * Prediction.  hmme_predict_bi_device: for picture i (n_pics >= 1, 2 * n_pics <= 16 planes) the luma prediction from refs0[i] (list 0) and
 * refs1[i] (list 1) with d_mv_field int16[n_pics][2][n_ctu][mv_per_ctu][2] and d_dir_field uint8[n_pics][n_ctu][mv_per_ctu], mv_per_ctu 1 |
 * 64 -- with 64 what the decision above writes.  Every MV is clamped like TComDataCU::clipMv, as in hmme_predict_pairs_device.
 *   direction 1 / 2   bit for bit what hmme_predict_pairs_device writes from that list's plane and MV
 *   direction 3       TComPrediction::motionCompensation without WP (TLibCommon/TComPrediction.cpp:527-541): xPredInterUni with bi = true on
 *                     both lists -- the 14-bit intermediates P0, P1: vertical stage with shift 6 and offset 0, the copy case
 *                     (src << (14 - bd)) - 8192 --, then addAvg: ClipBD((P0 + P1 + offset) >> shift) with shift = max(2, 14 - bd) + 1 and
 *                     offset = (1 << (shift - 1)) + 2 * 8192
 *   anything else     (0xFF included) the block is not written and reads no plane
 * d_outs: HOST array of n_pics device images of out_pitch_bytes per row; the writes are those of hmme_predict_pairs_device: inside the
 * picture and inside the CTU range only.  All planes must have one size and fp's bit depth and belong to the context; each is ordered
 * across streams like any reference.  A bit depth outside 8..12 is HMME_ERR_ARG; every depth in 8..12 is served (the sum stays in int32).
 * In a slice with explicit weighted prediction (addWeightBi): hmme_predict_bi_w_device, further down.  hmme_predict_bi_frame: synchronous, one picture, host motion field
 * int16[2][n_ctu][mv_per_ctu][2], direction field and image (out_stride in samples; samples outside the CTU range and of blocks without a
 * direction keep their values). */
typedef struct hmme_dir_params {
  uint32_t dir_bits[3];    /* uiMbBits: list 0, list 1, bi */
  uint32_t list_bits[2];   /* reference-index + MVP-index bits of list 0, list 1 */
} hmme_dir_params;
int hmme_select_dirs_check(const hmme_select_params* sel, int n_pics, const hmme_dir_params* dirs);
int hmme_select_dirs_device(hmme_ctx* ctx, int width, int height, int n_pics, const hmme_frame_params* fp, const hmme_select_params* sel,
                            const hmme_dir_params* dirs, const void* d_mv_uni, const void* d_cost_uni, const void* d_mv_bi, const void* d_cost_bi,
                            const void* d_uni_field, const void* d_pred_q, void* d_out_field, void* d_out_dir, void* d_out_slot, void* d_out_cost,
                            void* stream);
int hmme_select_dirs_frame(hmme_ctx* ctx, int width, int height, const hmme_frame_params* fp, const hmme_select_params* sel,
                           const hmme_dir_params* dir, const int16_t* mv_uni, const uint32_t* cost_uni, const int16_t* mv_bi, const uint32_t* cost_bi,
                           const int16_t* uni_field, const int16_t* pred_q, int16_t* out_field, uint8_t* out_dir, uint16_t* out_slot,
                           uint32_t* out_cost);
int hmme_predict_bi_device(hmme_ctx* ctx, const hmme_plane* const* refs0, const hmme_plane* const* refs1, int n_pics, const hmme_frame_params* fp,
                           const void* d_mv_field, const void* d_dir_field, int mv_per_ctu, void* const* d_outs, int out_pitch_bytes, void* stream);
int hmme_predict_bi_frame(hmme_ctx* ctx, const hmme_plane* ref0, const hmme_plane* ref1, const hmme_frame_params* fp, const int16_t* mv_field,
                          const uint8_t* dir_field, int mv_per_ctu, void* out, int out_stride);

/* ---- B pictures with several references per list ---------------------------------------------------------------------------------
 * The two sections above joined: a B picture with n0 / n1 references in list 0 / list 1, as HM's loop walks iRefIdxTemp in the uni pass
 * (TEncSearch.cpp:3027-3094) and again inside the bi pass (:3208-3247), against the other list's best (MV, refIdx).  The pipeline:
 *   1. hmme_search_frame_multi_device / hmme_refine_frame_multi_device, once per list;
 *   2. hmme_select_refs_device with the two lists as its two "pictures": uni_field[2] and uni_ref[2];
 *   3. hmme_search_frame_bi_refs_device / hmme_refine_frame_bi_refs_device, once per list: the bi pass of list l over all its references
 *      against ONE origin, built from list 1-l's field and per-block reference indices;
 *   4. hmme_select_dirs_refs_device: L0 / L1 / bi and the reference index per list, per PU, then the partition decision;
 *   5. hmme_predict_bi_refs_device: the prediction from the two-list field, the direction field and the two reference-index fields;
 *   6. hmme_residual_pairs_device.
 * New entry points and one new struct; no struct and no existing entry point changed, so HMME_ABI_VERSION stays 6.
 * THIS TEXT PLUS THE CITATIONS IS THE RULE.  The _w (explicit weighted prediction) forms of the bi pass and of the prediction, and the chroma
 * form of the prediction: "multi-reference B pictures: explicit weights and 4:2:0 chroma" below.  Out of scope:
 * GPB_SIMPLE_UNI's copy of list-0 results into list 1; MvdL1ZeroFlag; HM's further bi iterations (hmme_select_dirs_device, too, takes each
 * list's first iteration only).
 *
 * The bi pass.  hmme_search_frame_bi_refs_device is the bi-pass sibling of hmme_search_frame_multi_device: one current plane, refs[n_refs]
 * the searched list (1..16 planes), others[n_others] the other list (1..16 planes), d_other_mv int16[n_ctu][mv_per_ctu][2] and d_other_ref
 * uint8[n_ctu][mv_per_ctu] the other list's field and reference index per block (mv_per_ctu 1 | 64), d_center_q / d_pred_q
 * int16[n_refs][n_ctu][2] or NULL as in hmme_search_pairs_bi_device, tables [n_refs][count][593].  For every reference r the result is what
 * hmme_search_pairs_bi_device / hmme_refine_pairs_bi_device define for pair r = (cur, refs[r]) with ONE difference: the 8x8 block of the
 * other list's prediction P is read from others[d_other_ref[block]] -- hmme_predict_refs_device's prediction; an index >= n_others is read
 * as reference 0.  That covers the 0xFF hmme_select_refs_device writes for CUs that do not exist, whose blocks lie outside the picture and
 * carry MV (0,0): with n_others == 1 the call equals the existing one on every field the select calls write.  The origin is built once
 * per call and serves all n_refs references.  hmme_bipred_check runs first (refine = 1 in the refinement); every plane of refs and others
 * must have cur's size and fp's bit depth and belong to the context, and is ordered like a reference; a NULL d_other_ref is HMME_ERR_ARG.
 * NOTHING is launched or written on refusal.  hmme_search_frame_bi_refs / hmme_refine_frame_bi_refs: synchronous, host arrays of the same
 * shapes.
 *
 * The decision.  Inputs for n_pics B pictures (1..4), R = n_refs_max in 1..8, all quarter-pel refinement tables of one ctu_first / ctu_count:
 *   d_mv_uni, d_mv_bi    int16[n_pics][2][R][count][593][2]; d_cost_uni, d_cost_bi uint32[n_pics][2][R][count][593].  List l uses its first
 *                        n_refs[l] sets; set [p][l][r] of the bi tables is what the bi pass above wrote for list l's reference r.
 *   d_uni_field  int16[n_pics][2][n_ctu][64][2], d_uni_ref uint8[n_pics][2][n_ctu][64]: what hmme_select_refs_device wrote for the two lists
 *                and what the bi pass of the opposite list consumed.
 *   d_pred_q     int16[n_pics][2][R][n_ctu][2], or NULL for (0,0)
 *   dirs         HOST array of n_pics hmme_dir_refs_params: dir_bits as in hmme_dir_params; n_refs[l] in 1..R; ref_bits[l][r] the caller's
 *                model of the reference-index plus MVP-index bits of list l's reference r (hmme_ref_idx_bits gives HM's index part);
 *                l1_valid_mask: bit r set = list 1's reference r may win direction 2 -- HM sets this where getList1IdxToList0Idx(r) < 0
 *                (:3096-3104, :3282-3285).
 *   sel          as hmme_select_dirs_check requires it: mv_per_ctu 64, mv_unit 0, price_mv 0.
 * hmme_select_dirs_refs_check (a pure host function, run first; on failure the call launches NOTHING) returns HMME_ERR_ARG for anything
 * hmme_select_dirs_check refuses, R outside 1..8, n_refs[l] outside 1..R, any bit count above 4096, or l1_valid_mask bits at or above
 * n_refs[1].
 * Rule, per slot s; mvb, gc, the clamp at 0 and the 64-bit sums as in the hmme_select_dirs_device text; pred[l][r] = the predictor of list
 * l's reference r for the CTU:
 *   1. For r < n_refs[l]:  bu[l][r] = mvb(mv_uni[l][r][s], pred[l][r])
 *                          C[l][r]  = max(0, cost_uni[l][r][s] - gc(bu[l][r])) + gc(dir_bits[l] + ref_bits[l][r] + bu[l][r])
 *      ru[l] = the first r with the smallest C[l][r]: strict < in the order 0, 1, ... (:3086).  C[l] = C[l][ru[l]].
 *      mot[l] = ref_bits[l][ru[l]] + bu[l][ru[l]] (:3154-3155).
 *   2. List 1's direction-2 candidate C_V is the same minimum taken only over the r of l1_valid_mask (rv its index).  With an empty mask
 *      the candidate does not exist and direction 2 cannot win (HM's costValidList1 stays MAX_UINT).  mot[1] and the bi pass still use the
 *      unrestricted ru[1], as HM's cMv[1] / iRefIdx[1] do until :3282.
 *   3. For r < n_refs[l]:  bb[l][r]  = mvb(mv_bi[l][r][s], pred[l][r])
 *                          C_B[l][r] = (max(0, cost_bi[l][r][s] - gc(bb[l][r])) >> 1) + gc(dir_bits[2] + ref_bits[l][r] + bb[l][r] + mot[1-l])
 *      (:3210-3219, :3808).  rb[l] = the first strict minimum (:3226).  The bi candidate is list 0's unless list 1's is strictly cheaper.
 *      As in hmme_select_dirs_device's rule 2 the other list's motion bits are those of its uni slot s.
 *   4. C_bi <= C[0] and (C_V absent or C_bi <= C_V): direction 3; otherwise C_V absent or C[0] <= C_V: direction 1; otherwise direction 2
 *      (:3291, :3314).  Then the decision of hmme_select_pairs_device, steps 1-5, runs on the winners with the MV cost switched off.
 * Outputs -- only the entries of the CTUs in [ctu_first, ctu_first + ctu_count) are written:
 *   d_out_field  int16[n_pics][2][n_ctu][64][2] and d_out_ref uint8[n_pics][2][n_ctu][64] (not NULL).  Under direction 1 or 2 the winner's
 *                MV and reference (ru[0]; rv) in its list, (0,0) and 0xFF in the other.  Under direction 3 with the bi candidate having
 *                searched list l: list l holds mv_bi[l][rb[l]][s] and rb[l], list 1-l THE BLOCK'S OWN ENTRIES of d_uni_field[1-l] and
 *                d_uni_ref[1-l]: the motion the bi cost was measured with.  Blocks of CUs that do not exist: (0,0), 0xFF and 0xFF.
 *   d_out_dir    uint8[n_pics][n_ctu][64]: 1, 2 or 3; 0xFF for blocks of CUs that do not exist; not NULL
 *   d_out_slot   uint16[n_pics][n_ctu][64], may be NULL;  d_out_cost uint32[n_pics][n_ctu], saturated, may be NULL
 * Buffers: tables, costs, the input field and slots 4-byte aligned, the output field 8-byte.  hmme_select_dirs_refs_frame: synchronous,
 * host arrays of the same shapes with n_pics = 1; entries outside the CTU range keep their values.
 *
 * The prediction.  hmme_predict_bi_refs_device: ONE picture, like hmme_predict_refs_device: refs0[n0], refs1[n1] (each 1..16 planes),
 * d_mv_field int16[2][n_ctu][mv_per_ctu][2], d_dir_field uint8[n_ctu][mv_per_ctu], d_ref_field uint8[2][n_ctu][mv_per_ctu], mv_per_ctu 1 | 64,
 * one device image.  A block of direction 1 / 2 / 3 reads refs0[ref0] and / or refs1[ref1]; the result is what hmme_predict_bi_device
 * defines for those planes: the uni tail, or addAvg.  A block whose direction is anything else, or which uses a list whose index is >= that
 * list's count, is not written and reads no plane.  Plane checks and stream ordering are those of hmme_predict_refs_device, for both lists.
 * hmme_predict_bi_refs_frame: synchronous, host fields and image (out_stride in samples). */
typedef struct hmme_dir_refs_params {
  uint32_t dir_bits[3];      /* uiMbBits: list 0, list 1, bi */
  int n_refs[2];             /* references of list 0, list 1 */
  uint32_t ref_bits[2][8];   /* reference-index + MVP-index bits of list l's reference r */
  uint32_t l1_valid_mask;    /* bit r: list 1's reference r may win direction 2 */
} hmme_dir_refs_params;
int hmme_search_frame_bi_refs_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others,
                                     int n_others, const hmme_frame_params* fp, const void* d_other_mv, const void* d_other_ref, int mv_per_ctu,
                                     const void* d_center_q, const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream);
int hmme_refine_frame_bi_refs_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others,
                                     int n_others, const hmme_frame_params* fp, const void* d_other_mv, const void* d_other_ref, int mv_per_ctu,
                                     const void* d_center_q, const void* d_pred_q, const void* d_int_mv, int use_hadamard, void* d_out_qmv, void* d_out_cost,
                                     void* stream);
int hmme_search_frame_bi_refs(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                              const hmme_frame_params* fp, const int16_t* other_mv, const uint8_t* other_ref, int mv_per_ctu, const int16_t* center_q,
                              const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad);
int hmme_refine_frame_bi_refs(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                              const hmme_frame_params* fp, const int16_t* other_mv, const uint8_t* other_ref, int mv_per_ctu, const int16_t* center_q,
                              const int16_t* pred_q, const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost);
int hmme_select_dirs_refs_check(const hmme_select_params* sel, int n_pics, int n_refs_max, const hmme_dir_refs_params* dirs);
int hmme_select_dirs_refs_device(hmme_ctx* ctx, int width, int height, int n_pics, int n_refs_max, const hmme_frame_params* fp, const hmme_select_params* sel,
                                 const hmme_dir_refs_params* dirs, const void* d_mv_uni, const void* d_cost_uni, const void* d_mv_bi, const void* d_cost_bi,
                                 const void* d_uni_field, const void* d_uni_ref, const void* d_pred_q, void* d_out_field, void* d_out_ref, void* d_out_dir,
                                 void* d_out_slot, void* d_out_cost, void* stream);
int hmme_select_dirs_refs_frame(hmme_ctx* ctx, int width, int height, int n_refs_max, const hmme_frame_params* fp, const hmme_select_params* sel,
                                const hmme_dir_refs_params* dir, const int16_t* mv_uni, const uint32_t* cost_uni, const int16_t* mv_bi, const uint32_t* cost_bi,
                                const int16_t* uni_field, const uint8_t* uni_ref, const int16_t* pred_q, int16_t* out_field, uint8_t* out_ref, uint8_t* out_dir,
                                uint16_t* out_slot, uint32_t* out_cost);
int hmme_predict_bi_refs_device(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, const hmme_frame_params* fp,
                                const void* d_mv_field, const void* d_dir_field, const void* d_ref_field, int mv_per_ctu, void* d_out, int out_pitch_bytes,
                                void* stream);
int hmme_predict_bi_refs_frame(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, const hmme_frame_params* fp,
                               const int16_t* mv_field, const uint8_t* dir_field, const uint8_t* ref_field, int mv_per_ctu, void* out, int out_stride);

/* ---- the final prediction in a slice with explicit weighted prediction ---------------------------------------------------------
 * hmme_predict_bi_device and hmme_predict_refs_device with explicit weights: the prediction that belongs to the decisions of
 * hmme_select_dirs_device / hmme_select_refs_device when the searches before them were the *_w and *_bi_w_* calls.  New entry points only; no
 * struct and no existing entry point changed, so HMME_ABI_VERSION stays 6.  THIS TEXT PLUS THE CITATIONS IS THE RULE (paths below source/Lib
 * of the reference).
 *
 * hmme_predict_bi_w_device / hmme_predict_bi_w_frame: hmme_predict_bi_device / hmme_predict_bi_frame with two weights per picture, wps0[i]
 * for refs0[i] and wps1[i] for refs1[i], both HOST arrays of n_pics hmme_weight, read before the call returns.  Fields, directions, mv_per_ctu
 * 1 | 64, the clamp of every MV, CTU sub-ranges, the limit 2 * n_pics <= 16, plane ownership and stream ordering are unchanged.  The rule is
 * TComPrediction::xPredInterBi in a B slice with getWPBiPred() (TLibCommon/TComPrediction.cpp:603-651) -> xWeightedPredictionBi
 * (TLibCommon/TComWeightPrediction.cpp:268-301) with getWpScaling (:189-264):
 *   direction 1 / 2   bit for bit what hmme_predict_pairs_w_device writes from that list's plane, MV and weight: xPredInterUni with bi = true,
 *                     then addWeightUni (:133-180) with the uni-directional getWpScaling (:250-262) -- rule 1 of the section "bi-prediction with
 *                     explicit weighted prediction" above; wp.round is not used
 *   direction 3       addWeightBi (:46-49, :67-129) with the bi-directional getWpScaling (:230-247).  With head = max(2, 14 - bd) and P0, P1 the
 *                     Pel-truncated 14-bit intermediates of hmme_predict_bi_device:
 *                         shift' = wp0.shift + 1 + head
 *                         round' = 1 << (shift' - 1)
 *                         off    = wp0.offset + wp1.offset
 *                         pred   = ClipBD((w0 * (P0 + 8192) + w1 * (P1 + 8192) + round' + off * 2^(shift' - 1)) >> shift')
 *                     The shift is arithmetic.  HM writes offset << (shift - 1); it is the product here, so that a negative offset is defined.
 *   anything else     (0xFF included) the block is not written and reads no plane
 * Luma has ONE log2WeightDenom per slice and getWpScaling uses list 0's shift for both lists (:242-245), so wps0[i].shift != wps1[i].shift is
 * HMME_ERR_ARG.  hmme_wp_estimate called ONCE with the references of both lists shares the denominator among all of them (its step 2) and so
 * delivers weights this call accepts; two calls, one per list, may not.  TComPrediction::xCheckIdenticalMotion does not apply: it is off
 * under getWPBiPred() (TLibCommon/TComPrediction.cpp:501-503).
 * A picture whose two weights are both the identity (w0 == 1 << shift, offset 0, whatever round holds) runs hmme_predict_bi_device's kernel.
 * That is exact: uni blocks by the nested floors of rule 1 above, bi blocks because with d = shift
 *     (2^d * (P0 + P1 + 16384) + 2^(d + head)) >> (d + 1 + head)  =  (P0 + P1 + 16384 + 2^head) >> (head + 1)  =  addAvg
 * (the numerator is a multiple of 2^d).  One identity beside another weight is served by the weighted kernel.
 *
 * hmme_predict_refs_w_device / hmme_predict_refs_w_frame: hmme_predict_refs_device / hmme_predict_refs_frame with one weight per reference
 * (wps: n_refs HOST weights, read before the call returns): every block gets the addWeightUni result (direction 1 / 2 above) of the plane
 * its index names with that plane's weight; a block whose index is >= n_refs is untouched.  If every weight is the identity the unweighted
 * kernel runs; otherwise every block goes through the weighted formula, which for an identity weight equals the unweighted sample (nested
 * floors again).
 *
 * Refusal.  hmme_predict_bi_weight_check(bit_depth, wp0, wp1), a pure host function (no context, no GPU):
 *   bit depth outside 8..12, a NULL weight, a shift outside 0..15, unequal shifts                    -> HMME_ERR_ARG
 *   either weight alone: |w0| * 40 960 + round'_uni beyond int32 (the "other weight" line of
 *   hmme_bipred_weight_check, round'_uni = 1 << (shift + head - 1): uni blocks use it)                -> HMME_ERR_UNSUPPORTED
 *   the pair: (|w0| + |w1|) * 40 960 + round' + |off| * 2^(shift' - 1) beyond int32, evaluated in 64 bits  -> HMME_ERR_UNSUPPORTED
 * The pair's bound is derived, not measured: P is a Pel, so P + 8192 lies within [-24 576, 40 959] for each list whatever the planes hold,
 * and below the bound the int32 numerator cannot wrap.  HM wraps there; the engine refuses.  HM's own range -- |w| <= 255, shift <= 7,
 * |offset| <= 128 << (bd - 8) per list -- is served entirely at every depth 8..12: its largest numerator is 510 * 40 960 + 2^9 + 4096 * 2^9
 * < 2^25 at 12 bits and 510 * 40 960 + 2^13 + 256 * 2^13 < 2^25 at 8.  The bi_w calls run the check for every picture first, the refs_w calls
 * its single-weight line for every reference, and launch NOTHING if one fails: they return that code, hmme_last_error names the picture /
 * the reference. */
int hmme_predict_bi_weight_check(int bit_depth, const hmme_weight* wp0, const hmme_weight* wp1);
int hmme_predict_bi_w_device(hmme_ctx* ctx, const hmme_plane* const* refs0, const hmme_plane* const* refs1, int n_pics, const hmme_frame_params* fp,
                             const hmme_weight* wps0, const hmme_weight* wps1, const void* d_mv_field, const void* d_dir_field, int mv_per_ctu,
                             void* const* d_outs, int out_pitch_bytes, void* stream);
int hmme_predict_bi_w_frame(hmme_ctx* ctx, const hmme_plane* ref0, const hmme_plane* ref1, const hmme_frame_params* fp, const hmme_weight* wp0,
                            const hmme_weight* wp1, const int16_t* mv_field, const uint8_t* dir_field, int mv_per_ctu, void* out, int out_stride);
int hmme_predict_refs_w_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, const hmme_frame_params* fp, const hmme_weight* wps,
                               const void* d_mv_field, const void* d_ref_field, int mv_per_ctu, void* d_out, int out_pitch_bytes, void* stream);
int hmme_predict_refs_w_frame(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, const hmme_frame_params* fp, const hmme_weight* wps,
                              const int16_t* mv_field, const uint8_t* ref_field, int mv_per_ctu, void* out, int out_stride);

/* ---- 4:2:0 chroma motion compensation from the luma motion fields ------------------------------------------------
 * What TComPrediction::motionCompensation (TComPrediction.cpp:527-541) does for Cb and Cr right after the luma block, with the SAME motion
 * field, reference field and direction field the luma call of the same form takes: the caller of a 4:2:0 picture downloads nothing.  New
 * entry points only; no struct and no existing entry point changed, so HMME_ABI_VERSION stays 6.  THIS TEXT PLUS THE CITATIONS IS THE RULE
 * (paths below source/Lib/TLibCommon/).
 *
 * Planes.  A chroma component is an ordinary hmme_plane of (width / 2) x (height / 2) samples, width x height being the LUMA size, which
 * the calls take explicitly (even, at least 16 x 16).  The planes' 128 / 80-sample margins hold every displacement: a clamped MV moves a
 * chroma block at most 36 samples beyond the picture, the filter adds 2.  Planes, images and weights come in COMPONENT PAIRS: entry 2 i
 * is Cb of picture / reference i, entry 2 i + 1 is Cr.  Both components are written by one launch.  All planes of a call share one bit
 * depth (fp->bit_depth) and one context; a launch takes at most 16 planes: 8 pictures (pairs), 8 references (refs), 4 pictures (bi).
 *
 * Block rule (TComPrediction.cpp:669-707 xPredInterBlk for a chroma component, ChromaFormat 4:2:0).  One 8x8 luma block is one 4x4 block
 * per component at half the luma position.  Its quarter-pel luma MV is first clamped like TComDataCU::clipMv with the LUMA picture size and
 * the CTU's LUMA position -- exactly the clamp of hmme_predict_pairs_device.  The clamped MV, read in eighth chroma pels, gives the integer
 * offset mv >> 3 (arithmetic: negative MVs floor) and the phases mv & 7.  Taps: m_chromaFilter (TComInterpolationFilter.cpp:65-75), four per
 * phase.  HM's three branches -- horizontal only when yFrac == 0, vertical only when xFrac == 0, else horizontal over rows -1 .. h + 1 into
 * the 14-bit intermediate and then vertical -- are ONE two-stage formula with phase 0 as the filter {0, 64, 0, 0}, head = max(2, 14 -
 * bitDepth):
 *   first stage           (sum - (8192 << sh1)) >> sh1, sh1 = 6 - head, kept in an int16
 *   second stage, uni     ClipBD((sum + (1 << (sh2 - 1)) + (8192 << 6)) >> sh2), sh2 = 6 + head
 *   second stage, bi / WP P = sum >> 6 in an int16
 * The tails are the luma tails per sample, with the COMPONENT'S OWN {w0, offset, shift}: TComYuv::addAvg for direction 3, addWeightUni in a
 * slice with weights (hmme_predict_pairs_w_device), addWeightBi for direction 3 with weights (hmme_predict_bi_w_device).
 *
 * Fields.  d_mv_field, d_ref_field, d_dir_field, mv_per_ctu (1 | 64) and fp->ctu_first / ctu_count are what the luma call of the same
 * form takes, indexed by LUMA CTUs: a CTU is a 32 x 32 area of each component.  A block is live if its luma block starts inside the luma
 * picture and -- refs -- its index is < n_refs, -- bi -- its direction is 1, 2 or 3.  A block that is not live reads no plane and writes
 * nothing (0xFF and every other sentinel keep the image's samples).  Stores are samples of the planes' type (u8 at 8 bits, else u16), only
 * inside the chroma picture and inside the CTU range.  d_outs: HOST array of device images, one per plane pair entry, out_pitch_bytes per
 * row (>= a chroma row).
 *
 * Weights are optional: NULL runs the unweighted kernel, and so do identity weights (w0 == 1 << shift, offset 0, whatever round holds).
 *   pairs   wps: 2 * n_pairs HOST weights (Cb, Cr per picture); each passes the "other weight" line of hmme_bipred_weight_check
 *   refs    wps: 2 * n_refs HOST weights (Cb, Cr per reference); the same check
 *   bi      wps0 / wps1: 2 * n_pics HOST weights each (list 0 / list 1; both or neither); each component's pair passes
 *           hmme_predict_bi_weight_check, so the two lists' shifts are equal WITHIN a component; Cb and Cr may differ from each other
 *
 * Refusal.  Nothing is launched and hmme_last_error names the entry:
 *   an odd luma width or height, or one below 16; a plane whose size is not (width / 2, height / 2)  -> HMME_ERR_ARG
 *   planes whose bit depth is not fp->bit_depth (so: Cb / Cr or lists of different depth)            -> HMME_ERR_ARG
 *   planes of another context; more planes than a launch takes; a null argument; mv_per_ctu          -> HMME_ERR_ARG
 *   a CTU range outside the LUMA picture's CTUs                                                      -> HMME_ERR_ARG
 *   weights: the codes of hmme_bipred_weight_check / hmme_predict_bi_weight_check, per component
 *
 * The _frame forms are synchronous, one picture: host fields, `ref` / `ref0` / `ref1` / `outs` arrays of two entries (Cb, Cr), host images
 * of the chroma size with out_stride in samples; samples that are not written come back as they were. */
int hmme_predict_chroma_pairs_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_pairs, int width, int height, const hmme_frame_params* fp,
                                     const hmme_weight* wps, const void* d_mv_field, int mv_per_ctu, void* const* d_outs, int out_pitch_bytes, void* stream);
int hmme_predict_chroma_frame(hmme_ctx* ctx, const hmme_plane* const* ref, int width, int height, const hmme_frame_params* fp, const hmme_weight* wp,
                              const int16_t* mv_field, int mv_per_ctu, void* const* outs, int out_stride);
int hmme_predict_chroma_refs_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, int width, int height, const hmme_frame_params* fp,
                                    const hmme_weight* wps, const void* d_mv_field, const void* d_ref_field, int mv_per_ctu, void* d_out_cb, void* d_out_cr,
                                    int out_pitch_bytes, void* stream);
int hmme_predict_chroma_refs_frame(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, int width, int height, const hmme_frame_params* fp,
                                   const hmme_weight* wps, const int16_t* mv_field, const uint8_t* ref_field, int mv_per_ctu, void* const* outs, int out_stride);
int hmme_predict_chroma_bi_device(hmme_ctx* ctx, const hmme_plane* const* refs0, const hmme_plane* const* refs1, int n_pics, int width, int height,
                                  const hmme_frame_params* fp, const hmme_weight* wps0, const hmme_weight* wps1, const void* d_mv_field, const void* d_dir_field,
                                  int mv_per_ctu, void* const* d_outs, int out_pitch_bytes, void* stream);
int hmme_predict_chroma_bi_frame(hmme_ctx* ctx, const hmme_plane* const* ref0, const hmme_plane* const* ref1, int width, int height, const hmme_frame_params* fp,
                                 const hmme_weight* wp0, const hmme_weight* wp1, const int16_t* mv_field, const uint8_t* dir_field, int mv_per_ctu, void* const* outs,
                                 int out_stride);

/* ---- multi-reference B pictures: explicit weights and 4:2:0 chroma -------------------------------------------------------
 * Steps 3 and 5 of the pipeline of "B pictures with several references per list" for a slice with explicit weighted prediction, and step 5
 * for the Cb / Cr of a 4:2:0 picture: the bi pass with a weight per reference of both lists, hmme_predict_bi_refs_device with a weight per
 * reference of each list, and its chroma form with optional weights.  The weights are what hmme_wp_estimate / hmme_wp_estimate_420 deliver
 * for the references of both lists in ONE call.  New entry points only; no struct and no existing entry point changed, so HMME_ABI_VERSION
 * stays 6.  THIS TEXT PLUS THE CITATIONS IS THE RULE (paths below source/Lib/TLibCommon/ unless they name another directory).  Every weight
 * array is HOST memory, read before the call returns.  "Identity" means w0 == 1 << shift and offset == 0, whatever round holds -- the
 * prediction family's meaning; the SEARCHED list of the bi pass is the exception: there the *_w family's meaning applies, which also asks
 * for round == (shift ? 1 << (shift - 1) : 0).
 * The decision between the two (hmme_select_dirs_refs_device) needs no weighted form: it reads cost tables only, as hmme_select_dirs_device
 * does in the single-reference WP pipeline.
 *
 * Luma.  hmme_predict_bi_refs_w_device / _frame: hmme_predict_bi_refs_device / _frame with wps0[n0] and wps1[n1].  Fields, liveness, the
 * clamp of every MV, CTU sub-ranges, the limit of 16 planes per list, plane checks and stream ordering are unchanged.  A live block of
 * direction d with indices (r0, r1) is bit for bit what hmme_predict_bi_w_frame(refs0[r0], refs1[r1], wps0[r0], wps1[r1], ...) writes for that
 * block -- TComWeightPrediction::getWpScaling(pcCU, iRefIdx0, iRefIdx1, ...) (TComWeightPrediction.cpp:189-264), called with the PU's own
 * indices (:268-301 xWeightedPredictionBi, :312-329 xWeightedPredictionUni):
 *   direction 1 / 2   addWeightUni with that reference's weight (the index of the list the direction does not name is not looked at)
 *   direction 3       addWeightBi with w0 = wps0[r0].w0, w1 = wps1[r1].w0, off = wps0[r0].offset + wps1[r1].offset,
 *                     shift' = shift + 1 + head, round' = 1 << (shift' - 1)   -- the formula of hmme_predict_bi_w_device
 * If every weight of both lists is the identity the kernel of hmme_predict_bi_refs_device runs.  Otherwise every block goes through the
 * weighted tails, which for identity weights equal the unweighted sample: the nested floors (uni) and the addAvg identity (bi) proved in
 * "the final prediction in a slice with explicit weighted prediction".
 *
 * hmme_predict_bi_refs_weight_check(bit_depth, wps0, n0, wps1, n1), a pure host function (no context, no GPU).  The _w calls run it first
 * and launch and write NOTHING if it fails; they return its code, hmme_last_error names the list and the reference(s).  In this order, the
 * first failure deciding:
 *   1. argument errors of list 0, then of list 1: bit depth outside 8..12, a NULL array, n outside 1..16,
 *      a shift outside 0..15 (in the order of the references)                                            -> HMME_ERR_ARG
 *   2. two unequal shifts anywhere among the n0 + n1 weights (luma has ONE log2WeightDenom per slice)     -> HMME_ERR_ARG
 *   3. each weight alone, list 0 in order, then list 1: the single-weight line of
 *      hmme_predict_bi_weight_check (|w0| * 40 960 + round'_uni beyond int32)                             -> HMME_ERR_UNSUPPORTED
 *   4. every pair (r0, r1), r0-major: the pair line of hmme_predict_bi_weight_check                       -> HMME_ERR_UNSUPPORTED
 * So an argument error of list 1 is reported before a range of list 0, and n0 = n1 = 1 is hmme_predict_bi_weight_check.  Every pair is
 * checked, whether or not a block names it: the launch is safe for any field.
 *
 * 4:2:0.  hmme_predict_chroma_bi_refs_device / _frame: the Cb and Cr of the same picture from the luma call's three fields, in the
 * conventions of "4:2:0 chroma motion compensation": refs0 holds 2 * n0 planes, (Cb, Cr) per reference, refs1 2 * n1; width x height is the
 * LUMA size; wps0 / wps1 hold 2 * n0 / 2 * n1 weights in the planes' order, or both are NULL (one NULL beside an array: HMME_ERR_ARG).  A
 * launch takes at most 16 planes, so n0 + n1 <= 8 -- 4 + 4 is HM's low-delay B exactly; more is HMME_ERR_ARG.  A block is live if its luma
 * block starts inside the luma picture, its direction is 1..3 and every list the direction names has an index < that list's count; a block
 * that is not live reads nothing and writes nothing.  The two 4x4 blocks of a live luma block are what hmme_predict_chroma_bi_frame writes with
 * the planes -- and the component's weights -- the indices name.  Each component's weights go through the four steps above on their own:
 * shifts are equal WITHIN a component over all references of both lists, Cb and Cr may differ from each other; Cb answers before Cr.  NULL
 * weights, or identities throughout, run the unweighted form.  Every other refusal is that of hmme_predict_chroma_bi_device.  The _frame form
 * is synchronous: host fields, outs = (Cb, Cr) host images of the chroma size, out_stride in samples.
 *
 * The bi pass.  hmme_search_frame_bi_refs_w_device / hmme_refine_frame_bi_refs_w_device: hmme_search_frame_bi_refs_device /
 * hmme_refine_frame_bi_refs_device with wps[n_refs] for the searched list and other_wps[n_others] for the other list.  For reference r and
 * CTU c the result is what hmme_search_ctu_w / hmme_refine_ctu_w return with the weight wps[r] on the origin 2 * B - P, each 8x8 block of P
 * being the addWeightUni prediction -- rule 1 of "bi-prediction with explicit weighted prediction", with its getUseWP() quirk -- from
 * others[o] with other_wps[o], o = d_other_ref[block].  An index >= n_others reads reference 0 AND reference 0's weight.  fp->fen is not
 * consulted (xGetSADw reads every row).  A launch in which every weight of both lists is the identity IS the unweighted call with fen = 0;
 * if only the other weights are all identities the origin is the unweighted one; otherwise every block of P goes through addWeightUni
 * (nested floors: an identity weight gives the unweighted sample).  Shapes, limits, plane checks and stream ordering are those of the
 * unweighted calls.  hmme_search_frame_bi_refs_w / hmme_refine_frame_bi_refs_w: synchronous, host arrays of the same shapes.
 * One origin, one bias.  The origin is built once per call and serves all n_refs references, so it carries ONE bias B for all of them:
 * B = max(maxv, max_r(-wlo_r)), wlo_r the smallest weighted sample of wps[r] over [0, maxv] (hmme_bipred_weight_check's wlo).  Reference r's
 * weighted u16 copy carries offset_r + B, the refinement takes B + offset_r off again; the results do not depend on B.  The 16-bit span
 * line of hmme_bipred_weight_check, max(whi, 2 * maxv) + bias <= 65 535, cannot fail for the common bias once every weight passes its
 * own lines: each weighted sample fits a Pel, so whi_r <= 32 767 and -wlo_r <= 32 768 for every r, hence B <= 32 768 (maxv <= 4095) and
 * whi_r + B <= 65 535, while 2 * maxv + B <= 8 190 + 32 768.  That is derived, not measured.  So a set of weights is served exactly when
 * every weight passes its lines of hmme_bipred_weight_check:
 * hmme_bipred_refs_weight_check(bit_depth, wps, n_refs, other_wps, n_others, refine), a pure host function, run first by the four calls
 * (refine = 1 in the refinement), which launch and write NOTHING if it fails.  In this order, the first failure deciding:
 *   1. argument errors of the searched weights, then of the other weights: bit depth outside 8..12, a NULL array, a count outside
 *      1..16, a shift outside 0..15 (in the order of the references)                                       -> HMME_ERR_ARG
 *   2. the searched-weight lines of hmme_bipred_weight_check per reference, in order, with `refine`         -> HMME_ERR_UNSUPPORTED
 *   3. the "other weight" line of hmme_bipred_weight_check per other reference, in order                     -> HMME_ERR_UNSUPPORTED
 * The 12-bit refinement stays refused for every weight.  With one reference per list this is hmme_bipred_weight_check.
 *
 * The pipeline of a 4:2:0 B picture of a WP slice with n0 / n1 references, all on the device: hmme_wp_estimate_420 once for both lists;
 *   1. hmme_search_pairs_w_device / hmme_refine_pairs_w_device per list (its references as pairs with the one current picture);
 *   2. hmme_select_refs_device;
 *   3. hmme_search_frame_bi_refs_w_device / hmme_refine_frame_bi_refs_w_device, once per list;
 *   4. hmme_select_dirs_refs_device, unchanged (cost tables only);
 *   5. hmme_predict_bi_refs_w_device and hmme_predict_chroma_bi_refs_device with the component weights;
 *   6. hmme_residual_pairs_device per component.
 * Without WP: steps 1-6 as they were, plus hmme_predict_chroma_bi_refs_device with NULL weights in step 5.
 * Out of scope: GPB_SIMPLE_UNI; MvdL1ZeroFlag; HM's further bi iterations; the sequence layer (sequence.run_rank, tools/me_sequence.py). */
int hmme_bipred_refs_weight_check(int bit_depth, const hmme_weight* wps, int n_refs, const hmme_weight* other_wps, int n_others, int refine);
int hmme_search_frame_bi_refs_w_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others,
                                       int n_others, const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, const void* d_other_mv,
                                       const void* d_other_ref, int mv_per_ctu, const void* d_center_q, const void* d_pred_q, void* d_out_mv, void* d_out_sad,
                                       void* stream);
int hmme_refine_frame_bi_refs_w_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others,
                                       int n_others, const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, const void* d_other_mv,
                                       const void* d_other_ref, int mv_per_ctu, const void* d_center_q, const void* d_pred_q, const void* d_int_mv, int use_hadamard,
                                       void* d_out_qmv, void* d_out_cost, void* stream);
int hmme_search_frame_bi_refs_w(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                                const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, const int16_t* other_mv, const uint8_t* other_ref,
                                int mv_per_ctu, const int16_t* center_q, const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad);
int hmme_refine_frame_bi_refs_w(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                                const hmme_frame_params* fp, const hmme_weight* wps, const hmme_weight* other_wps, const int16_t* other_mv, const uint8_t* other_ref,
                                int mv_per_ctu, const int16_t* center_q, const int16_t* pred_q, const int16_t* int_mv, int use_hadamard, int16_t* out_qmv,
                                uint32_t* out_cost);
int hmme_predict_bi_refs_weight_check(int bit_depth, const hmme_weight* wps0, int n0, const hmme_weight* wps1, int n1);
int hmme_predict_bi_refs_w_device(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, const hmme_frame_params* fp,
                                  const hmme_weight* wps0, const hmme_weight* wps1, const void* d_mv_field, const void* d_dir_field, const void* d_ref_field,
                                  int mv_per_ctu, void* d_out, int out_pitch_bytes, void* stream);
int hmme_predict_bi_refs_w_frame(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, const hmme_frame_params* fp,
                                 const hmme_weight* wps0, const hmme_weight* wps1, const int16_t* mv_field, const uint8_t* dir_field, const uint8_t* ref_field,
                                 int mv_per_ctu, void* out, int out_stride);
int hmme_predict_chroma_bi_refs_device(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, int width, int height,
                                       const hmme_frame_params* fp, const hmme_weight* wps0, const hmme_weight* wps1, const void* d_mv_field, const void* d_dir_field,
                                       const void* d_ref_field, int mv_per_ctu, void* d_out_cb, void* d_out_cr, int out_pitch_bytes, void* stream);
int hmme_predict_chroma_bi_refs_frame(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, int width, int height,
                                      const hmme_frame_params* fp, const hmme_weight* wps0, const hmme_weight* wps1, const int16_t* mv_field, const uint8_t* dir_field,
                                      const uint8_t* ref_field, int mv_per_ctu, void* const* outs, int out_stride);

/* ---- prediction from one MV per 4x4 block: all 593 PU shapes of a P picture ------------------------------------------------
 * hmme_select_pairs_device and hmme_select_refs_device with mv_per_ctu = 256 write HM's own motion storage -- one (MV, reference index)
 * per 4x4 block -- and only there all 593 slots take part (8x4 / 4x8 PUs of an 8x8 CU, AMP at 16x16).  The calls below compensate such a
 * decision on the device, for Y and for the Cb / Cr of a 4:2:0 picture, uni-directionally with a reference per block and optional
 * weights: what a P picture needs between the decision and hmme_residual_pairs_device's 256 form.  New entry points only; no struct and no
 * existing entry point changed (every existing hmme_predict_* call still refuses 256 MVs per CTU), so HMME_ABI_VERSION stays 6.  THIS
 * TEXT PLUS THE CITATIONS IS THE RULE (paths below source/Lib/TLibCommon/ of the reference).
 *
 * Fields.  There is no mv_per_ctu argument: the family IS the 256 layout.  d_mv_field int16[n_ctu][256][2], quarter-pel luma MVs;
 * d_ref_field uint8[n_ctu][256], or NULL: every block has index 0.  Entry b of a CTU is the 4x4 luma block at ((b & 15) * 4, (b >> 4) * 4),
 * as the select calls write it; n_ctu counts all CTUs of the picture.  n_refs is 1..16 for luma and 1..8 for chroma (16 planes per launch,
 * as in the existing chroma calls).  With n_refs = 1 and a NULL reference field the luma call is the hmme_predict_pairs_device /
 * hmme_predict_pairs_w_device form for one picture: what hmme_select_pairs_device at 256 feeds.
 *
 * Liveness.  A 4x4 block is live if it starts inside the luma picture and its index is < n_refs; 0xFF and every index >= n_refs is not
 * live.  A block that is not live reads no plane and writes nothing.
 *
 * Samples of a live block.  Its MV is clamped exactly as in hmme_predict_refs_device: TComDataCU::clipMv with the CTU's position.  Every
 * sample of the block is what hmme_predict_refs_device writes for that sample when the 8x8 block that holds it carries this 4x4 block's
 * (MV, index); with weights it is hmme_predict_refs_w_device's sample.  Identity weights (w0 == 1 << shift, offset 0) run the unweighted
 * tail.  HM's interpolation is separable and per sample -- TComPrediction::xPredInterBlk (TComPrediction.cpp:669-707) filters a width x
 * height block with TComInterpolationFilter::filterHor / filterVer (TComInterpolationFilter.cpp:341-404, the loop over width and height:
 * :172-257), whose every output depends only on the MV and on its own 8 x 8 neighbourhood of the reference -- so this is also what xPredInterBlk writes for an 8x4, 4x8, 16x4 or 4x16 PU
 * (and for any larger PU whose 4x4 blocks all carry its entry), followed by addWeightUni (TComWeightPrediction.cpp:133-180) in a slice with
 * weights.
 *
 * Chroma (4:2:0, TComPrediction.cpp:669-707 for a chroma component).  A 4x4 luma block is a 2x2 block per component at half its position,
 * taking the MV, the index and the COMPONENT'S OWN weight of its luma block; planes and weights come in component pairs (entry 2 i: Cb,
 * 2 i + 1: Cr of reference i), width x height is the LUMA size, as in hmme_predict_chroma_refs_device.  Sample for sample it is what
 * hmme_predict_chroma_refs_device writes when the 8x8 luma block carries that entry.
 *
 * Margins.  The patch a 4x4 block reads (11 x 11 luma, 5 x 5 chroma samples) is a subset of the 15 x 15 / 7 x 7 patch the 64 form reads at
 * the same MV for the 8x8 block around it, so the planes' 128 / 80-sample margins hold by the argument given for those calls.
 *
 * Stores go only inside the picture and inside the CTU range [fp->ctu_first, + ctu_count); samples are of the planes' type.  Weights:
 * wps NULL for none, else n_refs (chroma: 2 * n_refs) HOST weights, each under the "other weight" line of hmme_bipred_weight_check.
 * Refusals -- codes and order -- are those of hmme_predict_refs_device / _w_device and hmme_predict_chroma_refs_device (and of their
 * _frame forms), except that a NULL reference field is an argument, not an error; hmme_last_error names the entry that was called.
 * Stream ordering, plane ownership and CTU sub-ranges are those of hmme_predict_refs_device.  The _frame forms are synchronous: host
 * field, host reference field or NULL, host image(s) with out_stride in samples (chroma: outs = {Cb, Cr} of the chroma size); every sample
 * that is not written comes back as it was.
 *
 * Not in this family: 4:2:2 / 4:4:4 chroma.  The bi / direction forms at 4x4 and the bi-pass origin from a 4x4 field: "B pictures from one
 * MV per 4x4 block" below. */
int hmme_predict_refs4_device(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, const hmme_frame_params* fp,
                              const hmme_weight* wps /* n_refs HOST weights, or NULL */, const void* d_mv_field /* int16[n_ctu][256][2] */,
                              const void* d_ref_field /* uint8[n_ctu][256], or NULL: every block index 0 */, void* d_out, int out_pitch_bytes, void* stream);
int hmme_predict_refs4_frame(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, const hmme_frame_params* fp, const hmme_weight* wps,
                             const int16_t* mv_field, const uint8_t* ref_field, void* out, int out_stride);
int hmme_predict_chroma_refs4_device(hmme_ctx* ctx, const hmme_plane* const* refs /* 2 * n_refs: Cb, Cr per reference */, int n_refs, int width,
                                     int height /* LUMA */, const hmme_frame_params* fp, const hmme_weight* wps /* 2 * n_refs or NULL */,
                                     const void* d_mv_field, const void* d_ref_field, void* d_out_cb, void* d_out_cr, int out_pitch_bytes, void* stream);
int hmme_predict_chroma_refs4_frame(hmme_ctx* ctx, const hmme_plane* const* refs, int n_refs, int width, int height, const hmme_frame_params* fp,
                                    const hmme_weight* wps, const int16_t* mv_field, const uint8_t* ref_field, void* const* outs, int out_stride);

/* ---- B pictures from one MV per 4x4 block: bi pass, decision, prediction ("bi4") ----------------------------------------------
 * What the refs4 family above is for a P picture, for a B picture with ONE reference per list, unweighted, Y plus the Cb / Cr of 4:2:0: the
 * bi pass against an origin built from a 4x4 field, the L0 / L1 / bi decision over all 593 slots, and the prediction from its output.  The
 * chain: hmme_refine_pairs_device (both lists) -> hmme_select_pairs_device at mv_per_ctu = 256 per list -> hmme_refine_pairs_bi4_device per
 * list -> hmme_select_dirs4_device -> hmme_predict_bi4_device + hmme_predict_chroma_bi4_device -> hmme_residual_pairs_device at 256.  New
 * entry points only; no struct and no existing entry point changed (hmme_select_dirs_*, the *_bi_* calls and hmme_predict_*bi_* still refuse
 * 256 MVs per CTU), so HMME_ABI_VERSION stays 6.  THIS TEXT PLUS THE CITATIONS IS THE RULE (paths below source/Lib of the reference).
 *
 * Fields.  As in the refs4 family there is no mv_per_ctu argument: the family IS the 256 layout.  Entry b of a CTU is the 4x4 luma block at
 * ((b & 15) * 4, (b >> 4) * 4); n_ctu counts all CTUs of the picture.
 *
 * 1. The bi pass.  hmme_search_pairs_bi4_device, hmme_refine_pairs_bi4_device, hmme_search_frame_bi4, hmme_refine_frame_bi4 are
 * hmme_search_pairs_bi_device, hmme_refine_pairs_bi_device, hmme_search_frame_bi, hmme_refine_frame_bi with d_other_mv
 * int16[n_pairs][n_ctu][256][2].  Everything is as in those calls except how the other list's prediction P inside the origin O = 2 B - P is
 * formed: every 4x4 block of the CTU's 64x64 block -- those beyond the picture edge included, as the 64 form does with its 8x8 blocks -- is
 * compensated from others[i] at its own entry, clamped with the CTU's clipMv; sample for sample what the 64 form puts there when the
 * surrounding 8x8 block carries that entry.  The results are, per CTU, what hmme_search_ctu / hmme_refine_ctu return on that origin; with a
 * field whose four entries per 8x8 block agree the tables are bit for bit those of the 64 form.  Refusals: hmme_bipred_check's and those of
 * the 64 form, in their order; hmme_last_error names the entry called.
 *
 * 2. The decision.  hmme_select_dirs4_check / _device / _frame have the signatures of hmme_select_dirs_*, and the rule of
 * hmme_select_dirs_device (its inputs, definitions, steps 1-5 and outputs above) holds word for word with three differences:
 *   a. Layouts.  sel->mv_per_ctu == 256 (mv_unit == 0 and price_mv == 0 as before).  d_uni_field and d_out_field are
 *      int16[n_pics][2][n_ctu][256][2], d_out_dir uint8[n_pics][n_ctu][256], d_out_slot uint16[n_pics][n_ctu][256].  All 593 slots take part,
 *      as in hmme_select_pairs_device at 256.
 *   b. Bi restriction: TComDataCU::isBipredRestriction (TLibCommon/TComDataCU.cpp:2892-2904), tested at TLibEncoder/TEncSearch.cpp:3109.  A
 *      slot whose hmme_slot_key has depth 3 and part_size 1 or 2 -- an 8x4 or 4x8 PU -- forms no bi candidate: steps 2 and 3 are not
 *      carried out for it, what mv_bi / cost_bi hold at that slot influences no output, and step 4 reduces to C[0] <= C[1]: direction 1,
 *      otherwise direction 2.  Every other slot, the AMP slots of a 16x16 CU included, decides as before.
 *   c. Other-list entry.  Under a direction-3 slot the other list's entry of a block is that 4x4 BLOCK'S OWN ENTRY of d_uni_field[1-l].
 * Buffers: tables, costs, the input field and slots 4-byte aligned, the output field 8-byte, the directions 2-byte (a lane stores pairs, as
 * out.ref at 256).  hmme_select_dirs4_check is hmme_select_dirs_check with 256 in place of 64.
 *
 * 3. The prediction.  hmme_predict_bi4_device / _frame are hmme_predict_bi_device / _frame without mv_per_ctu: d_mv_field
 * int16[n_pics][2][n_ctu][256][2], d_dir_field uint8[n_pics][n_ctu][256].  A 4x4 block is live if it starts inside the picture and its
 * direction is 1, 2 or 3; a block that is not live reads no plane and writes nothing.  Every sample of a live block is what
 * hmme_predict_bi_device writes for it when the 8x8 block around it carries this block's (direction, MV0, MV1) -- which, by the
 * separability argument of the refs4 family, is xPredInterBlk + TComYuv::addAvg for a 16x4 / 4x16 / 12x16 / 16x12 PU.  The margins hold:
 * the 11 x 11 patch is a subset of the 15 x 15 one.
 * hmme_predict_chroma_bi4_device / _frame are hmme_predict_chroma_bi_device / _frame without mv_per_ctu AND WITHOUT WEIGHTS.  A 4x4 luma
 * block is a 2x2 block per component; sample for sample the output is what hmme_predict_chroma_bi_device (NULL weights) writes when the 8x8
 * luma block carries the entry.  Sizes as in the existing chroma calls: an even luma size of at least 16 x 16.
 * Refusals -- codes and order -- are those of the 64 forms; hmme_last_error names the entry called.
 *
 * Every refusal of the entries of this family names the entry in hmme_last_error -- also those of the checks all families share (the CTU
 * range, a plane of another context, a NULL table), whose messages the 64 forms give bare.
 *
 * Not part of this family: explicit weights (_bi4_w), 4:2:2 / 4:4:4, and the plumbing into the sequence driver (hmme/sequence.py, run_rank).
 * Several references per list at 4x4: "B pictures with several references per list from one MV per 4x4 block" below. */
int hmme_search_pairs_bi4_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others,
                                 int n_pairs, const hmme_frame_params* fp, const void* d_other_mv /* int16[n_pairs][n_ctu][256][2] */, const void* d_center_q,
                                 const void* d_pred_q, void* d_out_mv, void* d_out_sad, void* stream);
int hmme_refine_pairs_bi4_device(hmme_ctx* ctx, const hmme_plane* const* curs, const hmme_plane* const* refs, const hmme_plane* const* others,
                                 int n_pairs, const hmme_frame_params* fp, const void* d_other_mv, const void* d_center_q, const void* d_pred_q,
                                 const void* d_int_mv, int use_hadamard, void* d_out_qmv, void* d_out_cost, void* stream);
int hmme_search_frame_bi4(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_plane* other, const hmme_frame_params* fp,
                          const int16_t* other_mv, const int16_t* center_q, const int16_t* pred_q, int16_t* out_mv, uint32_t* out_sad);
int hmme_refine_frame_bi4(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* ref, const hmme_plane* other, const hmme_frame_params* fp,
                          const int16_t* other_mv, const int16_t* center_q, const int16_t* pred_q, const int16_t* int_mv, int use_hadamard,
                          int16_t* out_qmv, uint32_t* out_cost);
int hmme_select_dirs4_check(const hmme_select_params* sel, int n_pics, const hmme_dir_params* dirs);
int hmme_select_dirs4_device(hmme_ctx* ctx, int width, int height, int n_pics, const hmme_frame_params* fp, const hmme_select_params* sel,
                             const hmme_dir_params* dirs, const void* d_mv_uni, const void* d_cost_uni, const void* d_mv_bi, const void* d_cost_bi,
                             const void* d_uni_field, const void* d_pred_q, void* d_out_field, void* d_out_dir, void* d_out_slot, void* d_out_cost,
                             void* stream);
int hmme_select_dirs4_frame(hmme_ctx* ctx, int width, int height, const hmme_frame_params* fp, const hmme_select_params* sel,
                            const hmme_dir_params* dir, const int16_t* mv_uni, const uint32_t* cost_uni, const int16_t* mv_bi, const uint32_t* cost_bi,
                            const int16_t* uni_field, const int16_t* pred_q, int16_t* out_field, uint8_t* out_dir, uint16_t* out_slot,
                            uint32_t* out_cost);
int hmme_predict_bi4_device(hmme_ctx* ctx, const hmme_plane* const* refs0, const hmme_plane* const* refs1, int n_pics, const hmme_frame_params* fp,
                            const void* d_mv_field, const void* d_dir_field, void* const* d_outs, int out_pitch_bytes, void* stream);
int hmme_predict_bi4_frame(hmme_ctx* ctx, const hmme_plane* ref0, const hmme_plane* ref1, const hmme_frame_params* fp, const int16_t* mv_field,
                           const uint8_t* dir_field, void* out, int out_stride);
int hmme_predict_chroma_bi4_device(hmme_ctx* ctx, const hmme_plane* const* refs0, const hmme_plane* const* refs1, int n_pics, int width, int height,
                                   const hmme_frame_params* fp, const void* d_mv_field, const void* d_dir_field, void* const* d_outs, int out_pitch_bytes,
                                   void* stream);
int hmme_predict_chroma_bi4_frame(hmme_ctx* ctx, const hmme_plane* const* ref0, const hmme_plane* const* ref1, int width, int height,
                                  const hmme_frame_params* fp, const int16_t* mv_field, const uint8_t* dir_field, void* const* outs, int out_stride);

/* ---- B pictures with several references per list from one MV per 4x4 block ("bi_refs4") -----------------------------------------
 * The two B-picture families joined: what "B pictures with several references per list" (the 64 form above) is at one MV per 8x8 block, at
 * full partition depth -- the bi pass against an origin built from a 4x4 field with a reference index per block, the L0 / L1 / bi decision
 * with the reference index per list over all 593 slots, and the prediction from its output; unweighted, Y plus the Cb / Cr of 4:2:0.  HM's B
 * configurations have two references per list (random access) or four (low-delay B).  The chain:
 *   1. hmme_refine_frame_multi_device, once per list;
 *   2. hmme_select_refs_device at mv_per_ctu = 256 with the two lists as its two pictures: uni_field[2] and uni_ref[2], 256 entries per CTU;
 *   3. hmme_refine_frame_bi_refs4_device, once per list;
 *   4. hmme_select_dirs_refs4_device;
 *   5. hmme_predict_bi_refs4_device + hmme_predict_chroma_bi_refs4_device;
 *   6. hmme_residual_pairs_device at 256.
 * New entry points only; no struct (hmme_dir_refs_params is reused as it is) and no existing entry point changed -- hmme_select_dirs_refs_*,
 * the *_bi_refs* calls and hmme_predict_*bi_refs_* still refuse 256 MVs per CTU --, so HMME_ABI_VERSION stays 6.  THIS TEXT PLUS THE CITATIONS
 * IS THE RULE (paths below source/Lib of the reference).
 *
 * Fields.  As in the refs4 and bi4 families there is no mv_per_ctu argument: the family IS the 256 layout.  Entry b of a CTU is the 4x4 luma
 * block at ((b & 15) * 4, (b >> 4) * 4); n_ctu counts all CTUs of the picture.
 *
 * 1. The bi pass.  hmme_search_frame_bi_refs4_device, hmme_refine_frame_bi_refs4_device, hmme_search_frame_bi_refs4 and
 * hmme_refine_frame_bi_refs4 are hmme_search_frame_bi_refs_device, hmme_refine_frame_bi_refs_device, hmme_search_frame_bi_refs and
 * hmme_refine_frame_bi_refs without mv_per_ctu: d_other_mv int16[n_ctu][256][2], d_other_ref uint8[n_ctu][256].  The 64 form's text holds
 * word for word with one difference -- how the other list's prediction P inside the origin O = 2 B - P (TLibEncoder/TEncSearch.cpp:3702-3712)
 * is formed: every 4x4 block of the CTU's 64x64 block, those beyond the picture edge included, is compensated from
 * others[d_other_ref[block]] at its own MV, clamped with the CTU's clipMv; an index >= n_others (the 0xFF of CUs that do not exist
 * included) reads reference 0.  Sample for sample it is what the 64 form puts there when the surrounding 8x8 block carries that (MV, index).
 * The origin is built once per call and serves all n_refs searched references.  The results are, per CTU and reference, what hmme_search_ctu
 * / hmme_refine_ctu return on that origin; with a field and reference field whose four entries per 8x8 block agree the tables are bit for
 * bit the 64 form's, and with n_others == 1 they are those of hmme_search_frame_bi4 / hmme_refine_frame_bi4.  Refusals: hmme_bipred_check's
 * and those of the 64 form, in their order; a NULL d_other_ref is HMME_ERR_ARG.
 *
 * 2. The decision.  hmme_select_dirs_refs4_check / _device / _frame have the signatures of hmme_select_dirs_refs_*, and the rule of
 * hmme_select_dirs_refs_device (its inputs, steps 1-4, l1_valid_mask, ref_bits, the 64-bit sums, its outputs) holds word for word with
 * these differences, which are those of hmme_select_dirs4_device:
 *   a. Layouts.  sel->mv_per_ctu == 256 (mv_unit == 0 and price_mv == 0 as before).  d_uni_field and d_out_field are
 *      int16[n_pics][2][n_ctu][256][2], d_uni_ref and d_out_ref uint8[n_pics][2][n_ctu][256], d_out_dir uint8[n_pics][n_ctu][256], d_out_slot
 *      uint16[n_pics][n_ctu][256].  All 593 slots take part, as in hmme_select_refs_device at 256.
 *   b. Bi restriction: TComDataCU::isBipredRestriction (TLibCommon/TComDataCU.cpp:2892-2904), tested at TLibEncoder/TEncSearch.cpp:3109.  A
 *      slot whose hmme_slot_key has depth 3 and part_size 1 or 2 -- an 8x4 or 4x8 PU: slots 0..255 -- forms no bi candidate for any
 *      reference: step 3 is not carried out for it, its bi tables are not loaded, and what mv_bi / cost_bi hold at that slot reaches no
 *      output.  Step 4 for it: C_V absent or C[0] <= C_V: direction 1; otherwise direction 2.  Every other slot, the AMP slots of a 16x16 CU
 *      included, decides as before.
 *   c. Other-list entry.  Under a direction-3 block, list 1-l's MV and reference index are that 4x4 BLOCK'S OWN ENTRIES of d_uni_field[1-l]
 *      and d_uni_ref[1-l].
 * Buffers: tables, costs, the input field and slots 4-byte aligned, the output field 8-byte; d_out_ref and d_out_dir 2-byte (a lane stores
 * pairs).  hmme_select_dirs_refs4_check is hmme_select_dirs_refs_check with 256 in place of 64.
 *
 * 3. The prediction.  hmme_predict_bi_refs4_device / _frame are hmme_predict_bi_refs_device / _frame without mv_per_ctu: ONE picture,
 * refs0[n0], refs1[n1] (each 1..16 planes), d_mv_field int16[2][n_ctu][256][2], d_dir_field uint8[n_ctu][256], d_ref_field
 * uint8[2][n_ctu][256].  A 4x4 block is live if it starts inside the picture, its direction is 1, 2 or 3, and every list it uses has an
 * index below that list's count (the index of a list it does not use is not looked at); a block that is not live reads no plane and writes
 * nothing.  Every sample of a live block is what hmme_predict_bi_refs_device writes for it when the 8x8 block around it carries this block's
 * (direction, MV0, MV1, ref0, ref1) -- xPredInterBlk (TLibCommon/TComPrediction.cpp:669-707) + TComYuv::addAvg, by the separability argument
 * of the refs4 family.  The margins hold: the 11 x 11 patch is a subset of the 15 x 15 one.
 * hmme_predict_chroma_bi_refs4_device / _frame are hmme_predict_chroma_bi_refs_device / _frame without mv_per_ctu AND WITHOUT WEIGHTS: up to
 * 4 + 4 references (2 * (n0 + n1) <= 16 planes, refs_l = (Cb, Cr) per reference), an even luma size of at least 16 x 16.  A 4x4 luma block is
 * a 2x2 block per component; sample for sample the output is what hmme_predict_chroma_bi_refs_device (NULL weights) writes when the 8x8 luma
 * block carries the entry.
 * Refusals -- codes and order -- are those of the 64 forms.
 *
 * Every refusal of the entries of this family names the entry called in hmme_last_error -- also those of the checks all families share.
 *
 * Out of scope: explicit weights (_bi_refs4_w), 4:2:2 / 4:4:4, GPB_SIMPLE_UNI's copy of list-0 results into list 1, MvdL1ZeroFlag, HM's
 * further bi iterations, and the plumbing into the sequence driver (hmme/sequence.py, run_rank). */
int hmme_search_frame_bi_refs4_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others,
                                      int n_others, const hmme_frame_params* fp, const void* d_other_mv /* int16[n_ctu][256][2] */,
                                      const void* d_other_ref /* uint8[n_ctu][256] */, const void* d_center_q, const void* d_pred_q, void* d_out_mv,
                                      void* d_out_sad, void* stream);
int hmme_refine_frame_bi_refs4_device(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others,
                                      int n_others, const hmme_frame_params* fp, const void* d_other_mv, const void* d_other_ref, const void* d_center_q,
                                      const void* d_pred_q, const void* d_int_mv, int use_hadamard, void* d_out_qmv, void* d_out_cost, void* stream);
int hmme_search_frame_bi_refs4(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                               const hmme_frame_params* fp, const int16_t* other_mv, const uint8_t* other_ref, const int16_t* center_q, const int16_t* pred_q,
                               int16_t* out_mv, uint32_t* out_sad);
int hmme_refine_frame_bi_refs4(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, const hmme_plane* const* others, int n_others,
                               const hmme_frame_params* fp, const int16_t* other_mv, const uint8_t* other_ref, const int16_t* center_q, const int16_t* pred_q,
                               const int16_t* int_mv, int use_hadamard, int16_t* out_qmv, uint32_t* out_cost);
int hmme_select_dirs_refs4_check(const hmme_select_params* sel, int n_pics, int n_refs_max, const hmme_dir_refs_params* dirs);
int hmme_select_dirs_refs4_device(hmme_ctx* ctx, int width, int height, int n_pics, int n_refs_max, const hmme_frame_params* fp, const hmme_select_params* sel,
                                  const hmme_dir_refs_params* dirs, const void* d_mv_uni, const void* d_cost_uni, const void* d_mv_bi, const void* d_cost_bi,
                                  const void* d_uni_field, const void* d_uni_ref, const void* d_pred_q, void* d_out_field, void* d_out_ref, void* d_out_dir,
                                  void* d_out_slot, void* d_out_cost, void* stream);
int hmme_select_dirs_refs4_frame(hmme_ctx* ctx, int width, int height, int n_refs_max, const hmme_frame_params* fp, const hmme_select_params* sel,
                                 const hmme_dir_refs_params* dir, const int16_t* mv_uni, const uint32_t* cost_uni, const int16_t* mv_bi, const uint32_t* cost_bi,
                                 const int16_t* uni_field, const uint8_t* uni_ref, const int16_t* pred_q, int16_t* out_field, uint8_t* out_ref, uint8_t* out_dir,
                                 uint16_t* out_slot, uint32_t* out_cost);
int hmme_predict_bi_refs4_device(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, const hmme_frame_params* fp,
                                 const void* d_mv_field, const void* d_dir_field, const void* d_ref_field, void* d_out, int out_pitch_bytes, void* stream);
int hmme_predict_bi_refs4_frame(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, const hmme_frame_params* fp,
                                const int16_t* mv_field, const uint8_t* dir_field, const uint8_t* ref_field, void* out, int out_stride);
int hmme_predict_chroma_bi_refs4_device(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, int width, int height,
                                        const hmme_frame_params* fp, const void* d_mv_field, const void* d_dir_field, const void* d_ref_field, void* d_out_cb,
                                        void* d_out_cr, int out_pitch_bytes, void* stream);
int hmme_predict_chroma_bi_refs4_frame(hmme_ctx* ctx, const hmme_plane* const* refs0, int n0, const hmme_plane* const* refs1, int n1, int width, int height,
                                       const hmme_frame_params* fp, const int16_t* mv_field, const uint8_t* dir_field, const uint8_t* ref_field,
                                       void* const* outs, int out_stride);

/* ---- residual and distortion of a prediction ------------------------------------------------------------------------
 * The first things HM does with a prediction, on the device: the residual, what the prediction costs per PU, and what coding no residual
 * would cost per CU -- one pass over the current picture, the predicted image as any hmme_predict_*_device call wrote it, and the covering-slot
 * map (d_out_slot) of the hmme_select_*_device calls.  New entry points only; nothing existing changed, so HMME_ABI_VERSION stays 6.
 *
 * Inputs.  curs[i]: planes of this context, of one size, bit depth 8..12; fp->bit_depth must be theirs, and of fp only ctu_first, ctu_count and
 * bit_depth are consulted.  d_preds: a HOST array of n_pairs device images, samples of the planes' type (u8 for 8-bit planes, u16 otherwise),
 * pred_pitch_bytes per row.  mv_per_ctu: 64 (blocks of 8x8) or 256 (blocks of 4x4), raster order inside the CTU.  d_slot:
 * uint16[n_pairs][n_ctu][mv_per_ctu] as a select call wrote it -- n_ctu = ALL CTUs of the picture -- or NULL: every block is then its own PU and
 * its own CU, which gives a per-block cost map.  The NULL form is also how a chroma plane is served; a chroma form driven by the luma slot map is
 * out of scope.  A block whose entry is 0xFFFF (no CU covers it; any value above 592 is read that way) carries 0 in both outputs and
 * contributes nothing.  The blocks that carry a slot are taken to be the slot's rectangle (hmme_slot_rect), as the select calls write them.
 *
 * Difference.  D = cur - pred at samples inside the picture, D = 0 at samples outside it.  HM never evaluates outside a picture, so this
 * sentence is the rule for partial edge CTUs, and for CUs that straddle the edge when max_depth < 3.
 *
 * d_out_resid (may be NULL, as may any entry of it): a HOST array of n_pairs device images of int16, resid_pitch_bytes per row, holding D --
 * TComYuv::subtract (TComYuv.cpp:320).  Written only inside the picture and inside the CTUs [ctu_first, ctu_first + ctu_count).
 *
 * d_out_pu (may be NULL): uint32[n_pairs][n_ctu][mv_per_ctu].  Every block carries the prediction error of the PU whose slot covers it:
 * TEncSearch::xGetInterPredictionError (TEncSearch.cpp:2816-2836), what xMergeEstimation (:2876) and the AMP merge check (:3368, :3374)
 * compare -- the distortion of original against prediction over the PU's rectangle with bApplyWeight = false:
 *   use_hadamard 1: xGetHADs (TComRdCost.cpp:1537-1604).  A PU whose width and height are both multiples of 8 is the sum of xCalcHADs8x8 over
 *                   its 8x8 blocks, each (sum |coefficient| + 2) >> 2; any other PU the sum of xCalcHADs4x4 over its 4x4 blocks, each
 *                   (sum |coefficient| + 1) >> 1.  The PU's total is then >> (bitDepth - 8).
 *   use_hadamard 0: xGetSAD over all rows; the PU's total >> (bitDepth - 8).
 *
 * d_out_cu (may be NULL): the same shape.  Every block carries the SSE of the CU that holds it -- the CU named by the depth and abs_z_idx of
 * the slot's key (hmme_slot_key): TComRdCost::getDistPart with DF_SSE (TComRdCost.cpp:433), the zero-residual distortion of the skip check of
 * encodeResAndCalcRdInterCU.  As xGetSSE (TComRdCost.cpp:970-1000) computes it: the sum of (D * D) >> ((bitDepth - 8) << 1), every sample
 * shifted before it is added (FULL_NBIT is 0, TypeDef.h:276, so DISTORTION_PRECISION_ADJUSTMENT is its argument, :280-284).
 *
 * d_out_ctu (may be NULL): uint32[n_pairs][n_ctu][2].  Entry 0: the sum of the PU errors over the distinct PUs of the CTU; entry 1: the sum of
 * the CU SSEs over its distinct CUs.  At least one of the four outputs must be given.
 *
 * Overflow.  Nothing saturates and nothing can wrap: at 12 bits the Hadamard total of a 64x64 PU stays below 2^32 before the shift
 * (<= 64 * ((64 * 64 * 4095 + 2) >> 2) = 268 369 920), a SAD is at most 4096 * 4095, a CU's or a CTU's SSE at most
 * 4096 * ((4095 * 4095) >> 8) = 268 304 384 (8 bits: 4096 * 255 * 255), and a CTU's PU errors sum to no more than the 64x64 bound.
 *
 * hmme_residual_pairs_device: asynchronous on `stream`, up to 16 pairs.  Limits, plane ownership and stream ordering are those of
 * hmme_predict_pairs_device; the call uses no scratch of the context.  HMME_ERR_ARG, with nothing launched, for: a null context, plane list,
 * plane, image list, image or fp; no output at all; n_pairs outside 1..16; mv_per_ctu other than 64 or 256; use_hadamard other than 0 or 1;
 * planes whose bit depth is not fp->bit_depth; a plane of another context; planes of different sizes; a CTU range outside the picture;
 * pred_pitch_bytes below a picture row, resid_pitch_bytes below 2 bytes per sample of one; a misaligned buffer -- predicted images and d_slot
 * 4 bytes, residual images AND their pitch 8 bytes, the uint32 outputs 4 bytes.  A predicted image whose pitch is not a multiple of 4 is
 * served, sample by sample.
 * hmme_residual_frame: synchronous, one picture, host arrays of the same shapes with n_pairs = 1 (pred_stride and resid_stride in samples, at
 * least the picture width), on the context's private stream; entries and samples outside the CTU range keep their values. */
int hmme_residual_pairs_device(hmme_ctx* ctx, const hmme_plane* const* curs, const void* const* d_preds, int pred_pitch_bytes, int n_pairs,
                               const hmme_frame_params* fp, const void* d_slot, int mv_per_ctu, int use_hadamard, void* const* d_out_resid,
                               int resid_pitch_bytes, void* d_out_pu, void* d_out_cu, void* d_out_ctu, void* stream);
int hmme_residual_frame(hmme_ctx* ctx, const hmme_plane* cur, const hmme_frame_params* fp, const void* pred, int pred_stride, const uint16_t* slot,
                        int mv_per_ctu, int use_hadamard, int16_t* out_resid, int resid_stride, uint32_t* out_pu, uint32_t* out_cu, uint32_t* out_ctu);

/* ---- estimating explicit weighted-prediction parameters --------------------------------------------------------
 * Where the weights of the *_w calls come from when the caller has none: the luma part of HM's estimator, WeightPredAnalysis::
 * xCalcACDCParamSlice, xEstimateWPParamSlice, xUpdatingWPParameters, xSelectWP and xCalcSADvalueWP (source/Lib/TLibEncoder/
 * WeightPredAnalysis.cpp:67-120, :172-351), bit-identical to what HM computes for a 4:0:0 slice without high-precision weighting (for a
 * 4:2:0 slice, where HM decides jointly over Y, Cb and Cr and the luma weights differ too: hmme_wp_estimate_420 below).  The
 * whole-picture sums run on the device over the picture area of the planes (margins are never counted); the scalar steps run on the host in
 * HM's own double / Int64 arithmetic.  New entry points and one new struct; nothing existing changed, so HMME_ABI_VERSION stays 6.
 *
 * hmme_plane_stats: xCalcACDCParamSlice (:67-120) for one picture, N = width * height:
 *   dc_sum = sum of the samples (:86-97);  ac = sum of |sample - normDC| with normDC = (dc_sum + (N >> 1)) / N (:99-112).
 * Synchronous.  The two sums are kept in the plane and returned without device work until the next upload / hmme_plane_set_device_u8 into
 * it, which drops them.
 *
 * hmme_wp_estimate: xEstimateWPParamSlice for one current picture and the n_refs (1..16) references of its slice.  With bd = the bit depth
 * and DC of a picture = (dc_sum + (N >> 1)) / N (:115):
 *   1. d = log2_denom_start (3..7; HM starts at 6, at 7 with more than three references in list 0, :174-180).
 *   2. For every reference (:227-258):
 *        dWeight = refAC == 0 ? 1.0 : Clip3(-16.0, 15.0, (double)curAC / (double)refAC)
 *        weight  = (int)(0.5 + dWeight * (double)(1 << d))
 *        offset  = (int)(((curDC << d) - (int64)weight * refDC + (1 << (d + bd - 8 - 1))) >> (d + bd - 8)), then clipped to [-128, 127]
 *      If (1 << d) - weight lies outside [-128, 128) for ANY reference, d is decremented and step 2 starts again (:182-189): all
 *      references of a call share the denominator.  It ends at d = 3 at the latest: the clip to 15 keeps weight within [0, 120] there.
 *   3. For every reference (xSelectWP, :285-316; xCalcSADvalueWP, :336-350), sums over the picture area:
 *        sad_wp   = (sum of |(org << d) - (ref * weight + (offset << (d + bd - 8)))|) / N
 *        sad_nowp = (sum of |(org << d) - (ref << d)|) / N
 *        ratio    = (double)sad_wp / (double)sad_nowp;  ratio >= 0.99 (DTHRESH, :46): not present -- weight = 1 << d, offset = 0.
 *      HM's corner cases are kept: identical pictures give 0 / 0 = NaN, NaN >= 0.99 is false, the (identity) weight stays PRESENT;
 *      a positive sad_wp over sad_nowp == 0 is +inf and disables the weight.
 *   4. out_wp[r] is the reference's luma WPScalingParam after TComSlice::initWpScaling (TComSlice.cpp:1487-1512): w0 = weight,
 *      offset = offset << (bd - 8), shift = d, round = d ? 1 << (d - 1) : 0 -- what hmme_search_pairs_w_device and its siblings take.
 * out_info (may be NULL) tells how each came about.  A weight that hmme_weight_check would refuse is still returned, with served_* = 0: the
 * estimator describes HM's choice, the search calls keep their own refusal.  The same plane given twice gives equal entries.
 * HMME_ERR_ARG (nothing launched, nothing written to the outputs): a null argument, planes of another context, a reference whose size or bit
 * depth differs from the current picture's, n_refs outside 1..16, log2_denom_start outside 3..7.
 * Ordering: the planes are read like any frame call reads them -- after their last fill, and recorded so that a refill on another stream
 * waits; the work runs on the context's private stream (as hmme_select_frame) and the call returns when the results are there. */
int hmme_plane_stats(const hmme_plane* plane, int64_t* dc_sum, int64_t* ac);
typedef struct hmme_wp_info {
  int64_t cur_dc_sum, cur_ac, ref_dc_sum, ref_ac;   /* xCalcACDCParamSlice */
  int64_t sad_wp, sad_nowp;                         /* xCalcSADvalueWP: each already divided by W*H */
  int log2_denom, weight, offset;                   /* iWeight, clipped iOffset (8-bit units), after xSelectWP */
  int present;                                      /* bPresentFlag after xSelectWP */
  int served_search, served_refine;                 /* hmme_weight_check(bit_depth, &wp, 0 / 1) == HMME_OK */
} hmme_wp_info;
int hmme_wp_estimate(hmme_ctx* ctx, const hmme_plane* cur, const hmme_plane* const* refs, int n_refs, int log2_denom_start, hmme_weight* out_wp,
                     hmme_wp_info* out_info);

/* hmme_wp_estimate_420: xEstimateWPParamSlice for a 4:2:0 slice, bit-identical to HM without high-precision weighting and with one bit depth
 * bd for all planes.  HM's estimator is joint over the three components, so neither the chroma NOR THE LUMA weights of a 4:2:0 slice are
 * what hmme_wp_estimate gives for the luma planes alone: one chroma weight out of range lowers the denominator luma uses, and the
 * present / not present decision is taken on the three components' SADs together.  cur = Y, Cb, Cr of the current picture; refs = Y, Cb, Cr
 * of reference r at 3 r .. 3 r + 2; Cb and Cr are (W / 2) x (H / 2) for a W x H luma.  One new entry point, no new or changed struct:
 * HMME_ABI_VERSION stays 6.
 *   Statistics per component: those of hmme_plane_stats (:67-120) with N_c the component's own sample count; DC = (dc_sum + (N_c >> 1)) / N_c.
 *   1. d = log2_denom_start (3..7), as above.
 *   2. (:218-264) For every reference and, inside, every component (HM's order): dWeight, weight and the raw offset as in step 2 of
 *      hmme_wp_estimate from that component's AC / DC.  Luma: offset clipped to [-128, 127] (:248).  Chroma (:241-244):
 *        pred    = 128 - ((128 * weight) >> d)
 *        delta   = Clip3(-512, 511, offset - pred)
 *        clipped = Clip3(-128, 127, delta + pred)
 *      If (1 << d) - weight lies outside [-128, 128) for ANY component of ANY reference (:255), d is decremented and step 2 starts again:
 *      all 3 * n_refs entries share d.
 *   3. (xSelectWP, :287-315) Per reference, with N_c and (weight_c, offset_c) the component's:
 *        sad_wp   = sum over c of ((sum of |(org << d) - (ref * weight_c + (offset_c << (d + bd - 8)))|) / N_c)
 *        sad_nowp = sum over c of ((sum of |(org << d) - (ref << d)|) / N_c)
 *      -- every component is divided by its own N_c before the three are added, as xCalcSADvalueWP returns them (:350, :301-302).
 *      ratio = (double)sad_wp / (double)sad_nowp >= 0.99: ALL THREE components of the reference get weight 1 << d, offset 0, not present
 *      (:306-314); otherwise all three stay.  NaN (0 / 0) keeps them present and +inf disables them, as above, now on the summed values.
 *   4. Every component goes through TComSlice::initWpScaling (TComSlice.cpp:1487-1512): w0 = weight, offset << (bd - 8), shift = d,
 *      round = d ? 1 << (d - 1) : 0.  out_wp_luma[r] is what the *_w search / refinement / prediction calls take; out_wp_chroma[2 r],
 *      [2 r + 1] = Cb, Cr of reference r, the layout hmme_predict_chroma_pairs_device, _refs_device and _bi_device take.
 * out_info (may be NULL; 3 * n_refs entries): entry 3 r + c carries component c's own sums and parameters: sad_wp / sad_nowp are that
 * component's quotient (the ratio is formed on their sums over c), present is the joint decision.  served_search / served_refine of a luma
 * entry are those of hmme_wp_estimate; of a chroma entry both are 1 exactly when the hmme_predict_chroma_* calls accept that weight for a
 * component.
 * HMME_ERR_ARG (nothing launched, nothing written to the outputs): a null argument other than out_info, n_refs outside 1..16,
 * log2_denom_start outside 3..7, a plane of another context, a luma size that is odd or below 16 x 16, a chroma plane that is not
 * (W / 2) x (H / 2), any plane whose bit depth differs from cur[0]'s, a reference luma plane of another size.
 * Ordering and caching as hmme_wp_estimate: the context's private stream, planes read after their fills and recorded for refills; the
 * per-plane sums are the ones hmme_plane_stats keeps in the planes (every fill drops them), so a picture that was a reference of the previous
 * call costs nothing the second time.  On the device, in this call and in hmme_wp_estimate alike, the planes without cached sums go through
 * two launches together and all (reference, component) pairs through one (me_kernels.hpp, me_plane_set_stats_kernel / me_wp_sad_set_kernel). */
int hmme_wp_estimate_420(hmme_ctx* ctx, const hmme_plane* const* cur, const hmme_plane* const* refs, int n_refs, int log2_denom_start,
                         hmme_weight* out_wp_luma, hmme_weight* out_wp_chroma, hmme_wp_info* out_info);

/* ---- environment (diagnostics and A/B measurements; none of these changes a result) ---------
 *   HMME_TRACE=1          one stderr line per context about launch geometry the library derives at run time (with HMME_FRAC_GRID=-1:
 *                         workgroups of the refinement kernel per CU); the TEncOpenCL host module prints its call summary in its destructor
 *   HMME_FRAC_GRID=<n>    workgroups of a refinement launch: default (0) = one per job; n > 0 = exactly n, each taking job after
 *                         job from a counter; -1 = as many of those as the chip holds at a time
 *   HMME_FRAC_JOB_TABLE=1 whole-picture refinement launches: job table written by a kernel in front of the launch (as before round 4's
 *                         end) instead of every workgroup deriving its job itself
 *   HMME_TAIL_PARTS=<n>   the jobs beyond a launch's last full round of workgroups ("tail"): 1 = no tail plan (they run whole, like the others);
 *                         n > 1 = n workgroups per tail job (8-bit: equal segments of the tail's task list; 16-bit: n strips per tail job);
 *                         default = the planner's choice (DESIGN.md 4.1 "tails")
 *   HMME_TAIL_LAUNCHES=<1|2> 8-bit launches with a tail: head and tail in one segment launch / the head's whole jobs, then the tail's segments
 *                         (default: one launch where the tail is at least a third of the head)
 * Measurement and test entry points live in include/hmme_test.h, not here. */

#ifdef __cplusplus
}
#endif
#endif
