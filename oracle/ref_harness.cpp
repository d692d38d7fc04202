// ref_harness.cpp -- thin C entry points onto the REFERENCE's own code, compiled from the
// sources where they lie under /root/reference (see oracle/Makefile).  TEST INFRASTRUCTURE:
// it validates oracle/hm_oracle.c and generates tests/golden/*.  Nothing under
// hm-opencl_amd/ links it.  Output goes to oracle/_ref/ only (git-ignored, travels with gpurun).
//
// The reference keeps the functions we need protected/private; the harness opens them with
// the usual test-only macro trick (the reference sources themselves are untouched).
#define protected public
#define private public
#include "TLibCommon/TComRom.h"
#include "TLibCommon/TComRdCost.h"
#include "TLibCommon/TComPattern.h"
#include "TLibCommon/TComDataCU.h"
#include "TLibCommon/TComSlice.h"
#include "TLibEncoder/TEncCfg.h"
#include "TLibCommon/TComPic.h"
#include "TLibCommon/TComYuv.h"
#include "TLibEncoder/TEncSearch.h"
#include "TLibEncoder/WeightPredAnalysis.h"
#undef protected
#undef private

#include <stdint.h>
#include <string.h>
#include <new>
#include <vector>

namespace {

struct Rig {
  TEncSearch* search;
  TEncCfg* cfg;
  TComRdCost* rd;
  TComDataCU* cu;
  TComSlice* slice;
  TComSPS* sps;
  Rig() {
    initROM();
    // heap objects, never destroyed: ~TEncSearch dereferences members init() would have set
    search = new TEncSearch;
    cfg = new TEncCfg;
    rd = new TComRdCost;
    cu = new TComDataCU;
    slice = new TComSlice;
    sps = new TComSPS;
    rd->init();
    search->m_pcEncCfg = cfg;
    search->m_pcRdCost = rd;
    slice->setSPS(sps);
    cu->m_pcSlice = slice;
    cu->m_pePartSize = new Char[4]();
    cu->m_puhDepth = new UChar[4]();
    cu->m_puhWidth = new UChar[4]();
    cu->m_puhHeight = new UChar[4]();
  }
};

Rig& rig() {
  static Rig* r = new Rig;
  return *r;
}

void setup_cost(double lambda, int pred_x, int pred_y, int bit_depth) {
  Rig& r = rig();
  BitDepths bd;
  for (int i = 0; i < MAX_NUM_CHANNEL_TYPE; ++i) bd.recon[i] = bit_depth;
  r.rd->setLambda(lambda, bd);
  r.rd->getMotionCost(true, 0, false);  // TEncSearch.cpp:3735
  TComMv pred((Short)pred_x, (Short)pred_y);
  r.rd->setPredictor(pred);             // :3737
  r.rd->setCostScale(2);                // :3738
}

void setup_cu(int cu_x, int cu_y, int pic_w, int pic_h, int max_cu) {
  Rig& r = rig();
  r.sps->setPicWidthInLumaSamples(pic_w);
  r.sps->setPicHeightInLumaSamples(pic_h);
  r.sps->setMaxCUWidth(max_cu);
  r.sps->setMaxCUHeight(max_cu);
  r.cu->m_uiCUPelX = cu_x;
  r.cu->m_uiCUPelY = cu_y;
}

}  // namespace

extern "C" {

// TComRdCost::xGetComponentBits
uint32_t ref_component_bits(int v) { return rig().rd->xGetComponentBits(v); }

// m_uiLambdaMotionSAD[0] after TComRdCost::setLambda
uint32_t ref_lambda_q16(double lambda) {
  setup_cost(lambda, 0, 0, 8);
  return rig().rd->m_uiCost;
}

// TComRdCost::getCost(x, y) with cost scale 2
uint32_t ref_mv_cost(double lambda, int x, int y, int pred_x, int pred_y) {
  setup_cost(lambda, pred_x, pred_y, 8);
  return rig().rd->getCost(x, y);
}

// the SAD function TComRdCost::setDistParam(pattern, ...) selects for this width
uint32_t ref_sad(int16_t* org, int org_stride, int16_t* cur, int cur_stride, int w, int h, int sub_shift,
                 int bit_depth) {
  Rig& r = rig();
  TComPattern pat;
  pat.initPattern(org, w, h, org_stride, bit_depth);
  DistParam dp;
  dp.bApplyWeight = false;
  r.rd->setDistParam(&pat, cur, cur_stride, dp);
  dp.iSubShift = sub_shift;
  dp.bitDepth = bit_depth;
  return dp.DistFunc(&dp);
}

// TComDataCU::getIndexBlock
int ref_index_block(int part_size, int depth, int part_idx, int abs_z_idx, int cu_h, int cu_w) {
  Rig& r = rig();
  r.cu->m_pePartSize[0] = (Char)part_size;
  r.cu->m_puhDepth[0] = (UChar)depth;
  r.cu->m_absZIdxInCtu = abs_z_idx;
  r.cu->m_puhHeight[0] = (UChar)cu_h;
  r.cu->m_puhWidth[0] = (UChar)cu_w;
  return r.cu->getIndexBlock(part_idx);
}

// TEncSearch::xSetSearchRange (+ TComDataCU::clipMv)
void ref_set_search_range(int pred_x_q, int pred_y_q, int sr, int cu_x, int cu_y, int pic_w, int pic_h,
                          int max_cu, int* lt_x, int* lt_y, int* rb_x, int* rb_y) {
  Rig& r = rig();
  setup_cu(cu_x, cu_y, pic_w, pic_h, max_cu);
  TComMv pred((Short)pred_x_q, (Short)pred_y_q), lt, rb;
  r.search->xSetSearchRange(r.cu, pred, sr, lt, rb);
  *lt_x = lt.getHor(); *lt_y = lt.getVer(); *rb_x = rb.getHor(); *rb_y = rb.getVer();
}

// TEncSearch::xPatternSearch for one PU.  `ref_at_pu` = reference plane at the PU origin.
void ref_pattern_search(int16_t* org, int org_stride, int w, int h, int16_t* ref_at_pu, int ref_stride, int lt_x,
                        int lt_y, int rb_x, int rb_y, int pred_x, int pred_y, double lambda, int fen,
                        int bit_depth, int* mvx, int* mvy, uint32_t* sad) {
  Rig& r = rig();
  setup_cost(lambda, pred_x, pred_y, bit_depth);
  r.cfg->setUseFastEnc(fen != 0);
  r.cfg->setFastSearch(0);
  TComPattern pat;
  pat.initPattern(org, w, h, org_stride, bit_depth);
  TComMv lt((Short)lt_x, (Short)lt_y), rb((Short)rb_x, (Short)rb_y), mv;
  Distortion d = 0;
  r.search->xPatternSearch(&pat, ref_at_pu, ref_stride, &lt, &rb, mv, d);
  *mvx = mv.getHor(); *mvy = mv.getVer(); *sad = d;
}

// the same with explicit weighted prediction switched on for the search (what setWpScalingDistParam, TEncSearch.cpp:5594-5635, leaves
// in m_cDistParam for a slice with weighted prediction): bApplyWeight + the luma WPScalingParam of the reference picture.
// Every candidate's DistFunc is then TComRdCostWeightPrediction::xGetSADw.
void ref_pattern_search_w(int16_t* org, int org_stride, int w, int h, int16_t* ref_at_pu, int ref_stride, int lt_x,
                          int lt_y, int rb_x, int rb_y, int pred_x, int pred_y, double lambda, int fen,
                          int bit_depth, int w0, int offset, int shift, int round, int* mvx, int* mvy, uint32_t* sad) {
  Rig& r = rig();
  setup_cost(lambda, pred_x, pred_y, bit_depth);
  r.cfg->setUseFastEnc(fen != 0);
  r.cfg->setFastSearch(0);
  static WPScalingParam wp[MAX_NUM_COMPONENT];
  memset(wp, 0, sizeof wp);
  wp[COMPONENT_Y].w = w0; wp[COMPONENT_Y].offset = offset; wp[COMPONENT_Y].shift = shift; wp[COMPONENT_Y].round = round;
  r.search->m_cDistParam.bApplyWeight = true;
  r.search->m_cDistParam.wpCur = wp;
  TComPattern pat;
  pat.initPattern(org, w, h, org_stride, bit_depth);
  TComMv lt((Short)lt_x, (Short)lt_y), rb((Short)rb_x, (Short)rb_y), mv;
  Distortion d = 0;
  r.search->xPatternSearch(&pat, ref_at_pu, ref_stride, &lt, &rb, mv, d);
  r.search->m_cDistParam.bApplyWeight = false;
  r.search->m_cDistParam.wpCur = NULL;
  *mvx = mv.getHor(); *mvy = mv.getVer(); *sad = d;
}

// TComRdCostWeightPrediction::xGetSADw through the DistFunc TComRdCost::setDistParam selects (which hands over to it)
uint32_t ref_sad_w(int16_t* org, int org_stride, int16_t* cur, int cur_stride, int w, int h, int sub_shift, int bit_depth, int w0, int offset,
                   int shift, int round) {
  Rig& r = rig();
  TComPattern pat;
  pat.initPattern(org, w, h, org_stride, bit_depth);
  WPScalingParam wp[MAX_NUM_COMPONENT];
  memset(wp, 0, sizeof wp);
  wp[COMPONENT_Y].w = w0; wp[COMPONENT_Y].offset = offset; wp[COMPONENT_Y].shift = shift; wp[COMPONENT_Y].round = round;
  DistParam dp;
  r.rd->setDistParam(&pat, cur, cur_stride, dp);
  dp.bApplyWeight = true;
  dp.wpCur = wp;
  dp.compIdx = COMPONENT_Y;
  dp.iSubShift = sub_shift;     // set as the FEN path sets it: xGetSADw never looks at it
  dp.bitDepth = bit_depth;
  return dp.DistFunc(&dp);
}

// TEncSearch::xTZSearch for one PU (FastSearch=1).  start_q = *pcMvPred (TEncSearch.cpp:3778).
// has_int_mv: pass pIntegerMv2Nx2NPred.  Window LT/RB as computed by the caller.
void ref_tz_search(int16_t* org, int org_stride, int w, int h, int16_t* ref_at_pu, int ref_stride, int lt_x,
                   int lt_y, int rb_x, int rb_y, int pred_x, int pred_y, double lambda, int fen, int bit_depth,
                   int sr, int cu_x, int cu_y, int pic_w, int pic_h, int max_cu, int has_int_mv, int int_mv_x,
                   int int_mv_y, int* mvx, int* mvy, uint32_t* sad) {
  Rig& r = rig();
  setup_cost(lambda, pred_x, pred_y, bit_depth);
  setup_cu(cu_x, cu_y, pic_w, pic_h, max_cu);
  r.cfg->setUseFastEnc(fen != 0);
  r.cfg->setFastSearch(1);
  r.search->m_iSearchRange = sr;
  r.search->m_iFastSearch = 1;
  TComPattern pat;
  pat.initPattern(org, w, h, org_stride, bit_depth);
  TComMv lt((Short)lt_x, (Short)lt_y), rb((Short)rb_x, (Short)rb_y);
  TComMv mv((Short)pred_x, (Short)pred_y);
  TComMv imv((Short)int_mv_x, (Short)int_mv_y);
  Distortion d = 0;
  r.search->xTZSearch(r.cu, &pat, ref_at_pu, ref_stride, &lt, &rb, mv, d, has_int_mv ? &imv : 0);
  *mvx = mv.getHor(); *mvy = mv.getVer(); *sad = d;
}

// The reference's fast search over every PU shape of CTUs [ctu_first, ctu_first + ctu_count) of a picture pair: xTZSearch (what HM runs
// with FastSearch=1, its default) for the 64x64 2Nx2N PU first, then the other 592 shapes seeded with its result like
// m_integerMv2Nx2N (TEncSearch.cpp:3780-3789); predictor (0,0), window from xSetSearchRange.  rects: int32[593][4] (x, y, w, h) in slot
// order.  The CPU baseline bench.py times on the GPU node's host (kind "reference", one core: HM is single-threaded); the same loop
// as oracle/hm_oracle.c tz_worker, whose results must be identical.  Returns the number of PU searches.
long ref_tz_frame(int16_t* cur, int cur_stride, int16_t* ref, int ref_stride, int pic_w, int pic_h, int sr, double lambda, int fen,
                  int bit_depth, int ctu_first, int ctu_count, const int32_t* rects, int32_t* out_x, int32_t* out_y, uint32_t* out_sad) {
  const int ctus_x = (pic_w + 63) / 64;
  long n_searches = 0;
  for (int i = 0; i < ctu_count; ++i) {
    const int ctu = ctu_first + i, cu_x = (ctu % ctus_x) * 64, cu_y = (ctu / ctus_x) * 64;
    int ltx, lty, rbx, rby;
    ref_set_search_range(0, 0, sr, cu_x, cu_y, pic_w, pic_h, 64, &ltx, &lty, &rbx, &rby);
    int imv_x = 0, imv_y = 0;
    for (int n = 0; n < 593; ++n) {
      const int s = n == 0 ? 592 : n - 1;
      const int32_t* r = rects + 4 * s;
      int mx, my;
      uint32_t sad;
      ref_tz_search(cur + (long)(cu_y + r[1]) * cur_stride + cu_x + r[0], cur_stride, r[2], r[3],
                    ref + (long)(cu_y + r[1]) * ref_stride + cu_x + r[0], ref_stride, ltx, lty, rbx, rby, 0, 0, lambda, fen, bit_depth, sr,
                    cu_x, cu_y, pic_w, pic_h, 64, n == 0 ? 0 : 1, imv_x, imv_y, &mx, &my, &sad);
      if (n == 0) { imv_x = mx; imv_y = my; }
      if (out_x) { out_x[(long)i * 593 + s] = mx; out_y[(long)i * 593 + s] = my; out_sad[(long)i * 593 + s] = sad; }
      ++n_searches;
    }
  }
  return n_searches;
}

// TEncSearch::xPatternSearchFracDIF for one PU, set up like xMotionEstimation does (TEncSearch.cpp:3792-3798):
// getMotionCost(true, 0, ...), cost scale 1; the function itself switches to scale 0 for the quarter stage.
static bool g_frac_bipred = false;
void ref_frac_refine(int16_t* org, int org_stride, int w, int h, int16_t* ref_at_pu, int ref_stride, int int_x, int int_y,
                     int pred_x, int pred_y, double lambda, int use_had, int bit_depth, int* half_x, int* half_y,
                     int* qter_x, int* qter_y, uint32_t* cost) {
  Rig& r = rig();
  static bool buffers = false;
  if (!buffers) { r.search->initTempBuff(CHROMA_420); buffers = true; }
  setup_cost(lambda, pred_x, pred_y, bit_depth);
  r.rd->setCostScale(1);
  r.cfg->setUseHADME(use_had != 0);
  TComPattern pat;
  pat.initPattern(org, w, h, org_stride, bit_depth);
  TComMv mv((Short)int_x, (Short)int_y), half, qter;
  Distortion d = 0;
  r.search->xPatternSearchFracDIF(false, &pat, ref_at_pu, ref_stride, &mv, half, qter, d, g_frac_bipred);
  *half_x = half.getHor(); *half_y = half.getVer(); *qter_x = qter.getHor(); *qter_y = qter.getVer(); *cost = d;
}

// xPatternSearchFracDIF in a slice with explicit weighted prediction: m_cDistParam carries bApplyWeight + wpCur from
// setWpScalingDistParam (TEncSearch.cpp:3740) into the refinement (:3798), whose distortion functions are then xGetHADsw / xGetSADw
void ref_frac_refine_w(int16_t* org, int org_stride, int w, int h, int16_t* ref_at_pu, int ref_stride, int int_x, int int_y,
                       int pred_x, int pred_y, double lambda, int use_had, int bit_depth, int w0, int offset, int shift, int round,
                       int* half_x, int* half_y, int* qter_x, int* qter_y, uint32_t* cost) {
  Rig& r = rig();
  static WPScalingParam wp[MAX_NUM_COMPONENT];
  memset(wp, 0, sizeof wp);
  wp[COMPONENT_Y].w = w0; wp[COMPONENT_Y].offset = offset; wp[COMPONENT_Y].shift = shift; wp[COMPONENT_Y].round = round;
  r.search->m_cDistParam.bApplyWeight = true;
  r.search->m_cDistParam.wpCur = wp;
  ref_frac_refine(org, org_stride, w, h, ref_at_pu, ref_stride, int_x, int_y, pred_x, pred_y, lambda, use_had, bit_depth, half_x, half_y,
                  qter_x, qter_y, cost);
  r.search->m_cDistParam.bApplyWeight = false;
  r.search->m_cDistParam.wpCur = NULL;
}

// the bBi call of TEncSearch::xMotionEstimation (TEncSearch.cpp:3798 with bBi = true): `org` is the bi-prediction origin
// 2*org - pred_other (TEncSearch.cpp:3702-3712, TComYuv::removeHighFreq: unclipped, so samples lie in [-maxv, 2*maxv])
void ref_frac_refine_bi(int16_t* org, int org_stride, int w, int h, int16_t* ref_at_pu, int ref_stride, int int_x, int int_y,
                        int pred_x, int pred_y, double lambda, int use_had, int bit_depth, int* half_x, int* half_y,
                        int* qter_x, int* qter_y, uint32_t* cost) {
  g_frac_bipred = true;
  ref_frac_refine(org, org_stride, w, h, ref_at_pu, ref_stride, int_x, int_y, pred_x, pred_y, lambda, use_had, bit_depth, half_x, half_y,
                  qter_x, qter_y, cost);
  g_frac_bipred = false;
}

// TComPicYuv::create + extendPicBorder (TComPicYuv.cpp:80-133, :214-262): a w x h luma picture goes in, the whole padded buffer
// (margin maxCU + 16 on every side) comes out.  out must hold (*out_stride) * (h + 2 * margin) samples; returns the margin.
int ref_extend_border(const int16_t* img, int img_stride, int w, int h, int max_cu, int16_t* out, int out_capacity, int* out_stride) {
  initROM();
  TComPicYuv pic;
  pic.create(w, h, CHROMA_400, max_cu, max_cu, 4, true);
  const int stride = pic.getStride(COMPONENT_Y), total_h = pic.getTotalHeight(COMPONENT_Y), margin = pic.getMarginX(COMPONENT_Y);
  *out_stride = stride;
  if (stride * total_h > out_capacity) { pic.destroy(); return -1; }
  Pel* org = pic.getAddr(COMPONENT_Y);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) org[y * stride + x] = img[y * img_stride + x];
  pic.extendPicBorder();
  const Pel* buf = pic.getBuf(COMPONENT_Y);
  for (int i = 0; i < stride * total_h; ++i) out[i] = buf[i];
  pic.destroy();
  return margin;
}

}  // extern "C"

// ---- prediction blocks, prediction tails, the weighted-prediction estimator and the block distortions --------------------------------
namespace {

// a second rig beside the search's: a CU inside a 4:2:0 picture whose slice carries a WP table, a 64x64 reference picture with margins, and
// three 64x64 TComYuv.  Heap objects, never destroyed, like Rig's.
struct TailRig {
  TComDataCU* cu;
  TComSlice* slice;
  TComSPS* sps;
  TComPPS* pps;
  TComPic* pic;
  TComPicYuv* ref;
  TComYuv *src0, *src1, *dst;
  TailRig() {
    rig();   // initROM, the TEncSearch whose TComPrediction / TComWeightPrediction parts are used below
    cu = new TComDataCU;
    slice = new TComSlice;
    sps = new TComSPS;
    pps = new TComPPS;
    pic = new TComPic;
    ref = new TComPicYuv;
    ref->create(64, 64, CHROMA_420, 64, 64, 4, true);
    pic->m_apcPicYuv[TComPic::PIC_YUV_ORG] = ref;
    pic->m_apcPicYuv[TComPic::PIC_YUV_REC] = ref;
    pic->m_picSym.m_apSlices.push_back(slice);
    slice->setSPS(sps);
    slice->setPPS(pps);
    slice->setPic(pic);
    pps->setUseWP(true);
    pps->setWPBiPred(true);
    cu->m_pcSlice = slice;
    cu->m_pcPic = pic;
    cu->m_ctuRsAddr = 0;
    cu->m_absZIdxInCtu = 0;
    src0 = new TComYuv; src1 = new TComYuv; dst = new TComYuv;
    src0->create(64, 64, CHROMA_420);
    src1->create(64, 64, CHROMA_420);
    dst->create(64, 64, CHROMA_420);
    rig().search->initTempBuff(CHROMA_420);
  }
  void depth(int bd) {
    for (int i = 0; i < MAX_NUM_CHANNEL_TYPE; ++i) sps->setBitDepth(ChannelType(i), bd);
  }
};

TailRig& tail_rig() {
  static TailRig* r = new TailRig;
  return *r;
}

bool tail_block_ok(int w, int h, int comp) {
  const int lim = comp ? 32 : 64;
  return comp >= 0 && comp < 3 && w >= 2 && h >= 1 && w <= lim && h <= lim;
}

void put_block(TComYuv* yuv, int comp, const int16_t* p, int w, int h) {
  for (int c = 0; c < 3; ++c) {
    const ComponentID id = ComponentID(c);
    memset(yuv->getAddr(id), 0, sizeof(Pel) * yuv->getStride(id) * yuv->getHeight(id));
  }
  const ComponentID id = ComponentID(comp);
  Pel* d = yuv->getAddr(id);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) d[y * yuv->getStride(id) + x] = p[y * w + x];
}

void get_block(TComYuv* yuv, int comp, int16_t* out, int w, int h) {
  const ComponentID id = ComponentID(comp);
  const Pel* s = yuv->getAddr(id);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) out[y * w + x] = s[y * yuv->getStride(id) + x];
}

// the slice's WP table as the slice header carries it: HM's syntax triple per list for `comp`, the identity at the same denominator for the
// other components
void set_wp_table(TComSlice* slice, int comp, int log2_denom, const int* weight, const int* offset) {
  for (int l = 0; l < 2; ++l)
    for (int c = 0; c < 3; ++c) {
      WPScalingParam* p = &slice->m_weightPredTable[l][0][c];
      memset(p, 0, sizeof *p);
      p->bPresentFlag = true;
      p->uiLog2WeightDenom = log2_denom;
      p->iWeight = c == comp ? weight[l] : 1 << log2_denom;
      p->iOffset = c == comp ? offset[l] : 0;
    }
}

}  // namespace

extern "C" {

// TComPrediction::xPredInterBlk for one block of component `comp` (0 luma; 1, 2 chroma of a 4:2:0 picture): w x h samples of that component
// whose top-left sample is `src`, displaced by the fraction (x_frac, y_frac) -- quarter luma pels, eighth chroma pels.  src must have 3 rows /
// columns before and 4 after the block for luma, 1 and 2 for chroma.  bi = 0: the clipped sample; bi = 1: the Pel intermediate.
int ref_pred_block(const int16_t* src, int src_stride, int w, int h, int x_frac, int y_frac, int bd, int bi, int comp, int16_t* out) {
  if (!tail_block_ok(w, h, comp)) return -1;
  TailRig& t = tail_rig();
  t.depth(bd);
  const ComponentID id = ComponentID(comp);
  const int before = comp ? 1 : 3, after = comp ? 2 : 4, stride = t.ref->getStride(id);
  Pel* origin = t.ref->getAddr(id);
  for (int y = -before; y < h + after; ++y)
    for (int x = -before; x < w + after; ++x) origin[y * stride + x] = src[y * src_stride + x];
  TComMv mv((Short)x_frac, (Short)y_frac);
  const int sx = t.ref->getComponentScaleX(id), sy = t.ref->getComponentScaleY(id);
  rig().search->xPredInterBlk(id, t.cu, t.ref, 0, &mv, w << sx, h << sy, t.dst, bi != 0, bd);
  get_block(t.dst, comp, out, w, h);
  return 0;
}

int ref_luma_block(const int16_t* src, int src_stride, int w, int h, int x_frac, int y_frac, int bd, int bi, int16_t* out) {
  return ref_pred_block(src, src_stride, w, h, x_frac, y_frac, bd, bi, 0, out);
}

// TComYuv::addAvg on two TComYuv holding the w x h intermediates p0, p1 (contiguous) in component `comp`
int ref_add_avg(const int16_t* p0, const int16_t* p1, int w, int h, int bd, int comp, int16_t* out) {
  if (!tail_block_ok(w, h, comp) || (w & 1)) return -1;
  TailRig& t = tail_rig();
  t.depth(bd);
  put_block(t.src0, comp, p0, w, h);
  put_block(t.src1, comp, p1, w, h);
  const ComponentID id = ComponentID(comp);
  t.dst->addAvg(t.src0, t.src1, 0, w << t.dst->getComponentScaleX(id), h << t.dst->getComponentScaleY(id), t.sps->getBitDepths());
  get_block(t.dst, comp, out, w, h);
  return 0;
}

// TComWeightPrediction::xWeightedPredictionUni -> getWpScaling -> addWeightUni with the slice's WP table set to HM's syntax triple
int ref_add_weight_uni(const int16_t* p, int w, int h, int bd, int comp, int weight, int offset, int log2_denom, int16_t* out) {
  if (!tail_block_ok(w, h, comp)) return -1;
  TailRig& t = tail_rig();
  t.depth(bd);
  const int ws[2] = {weight, 1 << log2_denom}, os[2] = {offset, 0};
  set_wp_table(t.slice, comp, log2_denom, ws, os);
  put_block(t.src0, comp, p, w, h);
  const ComponentID id = ComponentID(comp);
  rig().search->xWeightedPredictionUni(t.cu, t.src0, 0, w << t.dst->getComponentScaleX(id), h << t.dst->getComponentScaleY(id), REF_PIC_LIST_0, t.dst, 0);
  get_block(t.dst, comp, out, w, h);
  return 0;
}

// TComWeightPrediction::xWeightedPredictionBi -> getWpScaling -> addWeightBi, both lists used
int ref_add_weight_bi(const int16_t* p0, const int16_t* p1, int w, int h, int bd, int comp, int weight0, int offset0, int weight1, int offset1,
                      int log2_denom, int16_t* out) {
  if (!tail_block_ok(w, h, comp)) return -1;
  TailRig& t = tail_rig();
  t.depth(bd);
  const int ws[2] = {weight0, weight1}, os[2] = {offset0, offset1};
  set_wp_table(t.slice, comp, log2_denom, ws, os);
  put_block(t.src0, comp, p0, w, h);
  put_block(t.src1, comp, p1, w, h);
  const ComponentID id = ComponentID(comp);
  rig().search->xWeightedPredictionBi(t.cu, t.src0, t.src1, 0, 0, 0, w << t.dst->getComponentScaleX(id), h << t.dst->getComponentScaleY(id), t.dst);
  get_block(t.dst, comp, out, w, h);
  return 0;
}

// TComRdCost::getDistPart: kind 0 DF_SSE, 1 DF_HADS, 2 DF_SAD; the reference's own dispatch over its size variants runs
uint32_t ref_dist(int16_t* org, int org_stride, int16_t* pred, int pred_stride, int w, int h, int bd, int kind) {
  const DFunc f = kind == 0 ? DF_SSE : kind == 1 ? DF_HADS : DF_SAD;
  return rig().rd->getDistPart(bd, pred, pred_stride, org, org_stride, w, h, COMPONENT_Y, f);
}

// the weighted-prediction estimation of TEncSlice::precompressSlice (TEncSlice.cpp:675-694) for one picture and its n_l0 + n_l1 references:
// xCalcACDCParamSlice on every picture, xEstimateWPParamSlice, initWpScaling, xCheckWPEnable.  planes: the current picture's component
// planes, then each reference's (list 0 first), every plane contiguous; 1 plane per picture for chroma_format 400, 3 (Y, Cb, Cr; chroma
// (w / 2) x (h / 2)) for 420.  A reference's org and rec are the same plane.  n_l1 = 0: a P slice, else a B slice.
// out[(r * 3 + c) * 4 + ...] = bPresentFlag, iWeight, iOffset, uiLog2WeightDenom of reference r (list 0 first), component c, as
// initWpScaling leaves them; out_final the same after xCheckWPEnable; flags = the slice's m_bTestWeightPred, m_bTestWeightBiPred.
// log2_denom_start is HM's own choice (6, or 7 with more than three references in list 0): another value is refused (-2).
int ref_wp_estimate(const int16_t* const* planes, int n_l0, int n_l1, int w, int h, int chroma_format, int bd, int log2_denom_start, int32_t* out,
                    int32_t* out_final, int32_t* flags) {
  const int n_refs = n_l0 + n_l1, n_comp = chroma_format == 400 ? 1 : 3;
  if ((chroma_format != 400 && chroma_format != 420) || n_l0 < 1 || n_l1 < 0 || n_l0 > MAX_NUM_REF || n_l1 > MAX_NUM_REF) return -1;
  if (log2_denom_start != (n_l0 > 3 ? 7 : 6)) return -2;
  rig();
  const ChromaFormat fmt = chroma_format == 400 ? CHROMA_400 : CHROMA_420;
  TComSPS sps;
  TComPPS pps;
  for (int i = 0; i < MAX_NUM_CHANNEL_TYPE; ++i) sps.setBitDepth(ChannelType(i), bd);
  sps.setChromaFormatIdc(fmt);
  pps.setUseWP(true);
  pps.setWPBiPred(true);
  std::vector<TComPic*> pics;
  std::vector<TComPicYuv*> yuvs;
  std::vector<TComSlice*> slices;
  WeightPredAnalysis wpa;
  for (int p = 0; p <= n_refs; ++p) {
    TComPicYuv* yuv = new TComPicYuv;
    yuv->create(w, h, fmt, 64, 64, 4, true);
    for (int c = 0; c < n_comp; ++c) {
      const ComponentID id = ComponentID(c);
      const int16_t* s = planes[p * n_comp + c];
      const int cw = yuv->getWidth(id), ch = yuv->getHeight(id);
      for (int y = 0; y < ch; ++y)
        for (int x = 0; x < cw; ++x) yuv->getAddr(id)[y * yuv->getStride(id) + x] = s[y * cw + x];
    }
    TComPic* pic = new TComPic;
    TComSlice* slice = new TComSlice;
    pic->m_apcPicYuv[TComPic::PIC_YUV_ORG] = yuv;
    pic->m_apcPicYuv[TComPic::PIC_YUV_REC] = yuv;
    pic->m_picSym.m_apSlices.push_back(slice);
    slice->setSPS(&sps);
    slice->setPPS(&pps);
    slice->setPic(pic);
    slice->initWpAcDcParam();
    wpa.xCalcACDCParamSlice(slice);
    pics.push_back(pic); yuvs.push_back(yuv); slices.push_back(slice);
  }
  TComSlice* cur = slices[0];
  cur->setSliceType(n_l1 ? B_SLICE : P_SLICE);
  cur->setNumRefIdx(REF_PIC_LIST_0, n_l0);
  cur->setNumRefIdx(REF_PIC_LIST_1, n_l1);
  for (int r = 0; r < n_l0; ++r) cur->setRefPic(pics[1 + r], REF_PIC_LIST_0, r);
  for (int r = 0; r < n_l1; ++r) cur->setRefPic(pics[1 + n_l0 + r], REF_PIC_LIST_1, r);
  cur->resetWpScaling();
  wpa.xEstimateWPParamSlice(cur);
  cur->initWpScaling(&sps);
  for (int pass = 0; pass < 2; ++pass) {
    int32_t* o = pass ? out_final : out;
    for (int r = 0; r < n_refs; ++r)
      for (int c = 0; c < 3; ++c) {
        const WPScalingParam* p = &cur->m_weightPredTable[r < n_l0 ? 0 : 1][r < n_l0 ? r : r - n_l0][c];
        int32_t* e = o + (r * 3 + c) * 4;
        e[0] = c < n_comp ? p->bPresentFlag : 0; e[1] = c < n_comp ? p->iWeight : 0; e[2] = c < n_comp ? p->iOffset : 0;
        e[3] = c < n_comp ? (int)p->uiLog2WeightDenom : 0;
      }
    if (!pass) wpa.xCheckWPEnable(cur);
  }
  flags[0] = cur->m_bTestWeightPred;
  flags[1] = cur->m_bTestWeightBiPred;
  for (size_t i = 0; i < pics.size(); ++i) {
    pics[i]->m_picSym.m_apSlices.clear();
    delete slices[i];
    yuvs[i]->destroy();
    delete yuvs[i];
    delete pics[i];
  }
  return 0;
}

}  // extern "C"
