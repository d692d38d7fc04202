"""The final prediction of a slice with explicit weighted prediction (hmme_predict_bi_w_device, hmme_predict_refs_w_device) restated in numpy
int64 from the rule in include/hmme.h, and the rule of hmme_predict_bi_weight_check restated.  Plain numpy, no GPU: the reference of
tests/test_predict_bi_w_cpu.py, tests/test_gpu_predict_bi_w.py and tests/test_gpu_predict_refs_w.py.  Citations: source/Lib of the
reference encoder.

The intermediates are bipred_wp_model.inter_qpel (xPredInterUni with bi = true), blocks of one list bipred_wp_model.add_weight_uni -- both
pinned elsewhere (tests/test_bipred_wp_cpu.py)."""
import numpy as np

import bipred_wp_model as bwm
from frame_helpers import clip_mv, dims

INT32_MAX = (1 << 31) - 1
PEL_REACH = 40960          # |P + 8192| <= 40 959 for a Pel P


def add_weight_bi(p0, p1, bd, wp0, wp1, clip=True):
    """TComWeightPrediction::addWeightBi (TLibCommon/TComWeightPrediction.cpp:67-129) with weightBidir (:46-49) on the intermediates P0, P1;
    wp = (w0, offset, shift, round) per list, turned into the bi-directional parameters as getWpScaling does (:230-247): both lists use list
    0's log2WeightDenom, offset = o0 + o1, shift = log2WeightDenom + 1"""
    w0, o0, d, _ = (int(v) for v in wp0)
    w1, o1, d1, _ = (int(v) for v in wp1)
    assert d == d1                                               # luma has one log2WeightDenom per slice
    offset = o0 + o1                                             # :241
    shift = d + 1 + max(2, 14 - bd)                              # :242 wp0.shift = log2WeightDenom + 1; :95-96 shift = wp0.shift + shiftNum
    rnd = 1 << (shift - 1)                                       # :97 bRoundLuma is true for xWeightedPredictionBi (the default)
    a = np.asarray(p0).astype(np.int64) + 8192                   # :48 + IF_INTERNAL_OFFS
    b = np.asarray(p1).astype(np.int64) + 8192
    v = (w0 * a + w1 * b + rnd + offset * (1 << (shift - 1))) >> shift   # :48 offset << (shift - 1), written as the product
    return np.clip(v, 0, (1 << bd) - 1) if clip else v           # ClipBD


def pred_bi_w(plane0, plane1, x, y, w, h, mv0, mv1, bd, wp0, wp1, clip=True):
    """xPredInterBi in a B slice with getWPBiPred(), both lists used (TLibCommon/TComPrediction.cpp:603-651): xPredInterUni(bi = true) twice,
    xWeightedPredictionBi -> addWeightBi"""
    return add_weight_bi(bwm.inter_qpel(plane0, x, y, w, h, int(mv0[0]), int(mv0[1]), bd), bwm.inter_qpel(plane1, x, y, w, h, int(mv1[0]), int(mv1[1]), bd),
                         bd, wp0, wp1, clip)


def pred_block(planes, x, y, n, mvs, direction, bd, wps):
    """an n x n block of direction 1, 2 or 3 at (x, y) of the padded planes, mvs = the (clamped) MV of each list, wps = the weight of each"""
    if direction == 3:
        return pred_bi_w(planes[0], planes[1], x, y, n, n, mvs[0], mvs[1], bd, wps[0], wps[1])
    l = direction - 1
    return bwm.pred_w(planes[l], x, y, n, n, int(mvs[l][0]), int(mvs[l][1]), bd, wps[l])


def pred_picture(hmo, planes, w, h, bd, field, dirs, wps, out, ctus=None):
    """what hmme_predict_bi_w_frame writes into `out` ([h, w], changed in place and returned): field int16[2, n_ctu, 1 | 64, 2], dirs
    uint8[n_ctu, 1 | 64], wps = (wp0, wp1); every MV clamped by hmo_clip_mv for its CTU; blocks of another direction than 1, 2, 3 and samples
    beyond the picture or outside the CTUs `ctus` (None: all) keep their values"""
    from hmme import synth
    m = synth.MARGIN
    cx_n, cy_n = dims(w, h)
    per = field.shape[2]
    g = 64 if per == 1 else 8
    for ctu in (range(cx_n * cy_n) if ctus is None else ctus):
        cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        for b in range(per):
            bx, by = (b % 8) * g, (b // 8) * g
            d = int(dirs[ctu, b])
            if d not in (1, 2, 3) or cu_x + bx >= w or cu_y + by >= h:
                continue
            mvs = [clip_mv(hmo, field[l, ctu, b, 0], field[l, ctu, b, 1], cu_x, cu_y, w, h) for l in range(2)]
            p = pred_block(planes, m + cu_x + bx, m + cu_y + by, g, mvs, d, bd, wps)
            x1, y1 = min(cu_x + bx + g, w), min(cu_y + by + g, h)
            out[cu_y + by:y1, cu_x + bx:x1] = p[:y1 - cu_y - by, :x1 - cu_x - bx]
    return out


def refs_picture(hmo, planes, w, h, bd, field, ref_field, wps, out, ctus=None):
    """what hmme_predict_refs_w_frame writes into `out`: field int16[n_ctu, 1 | 64, 2], ref_field uint8[n_ctu, 1 | 64], wps one weight per
    plane; every block bipred_wp_model.pred_w of the plane its index names with that plane's weight; blocks whose index is >= len(planes)
    keep their values"""
    from hmme import synth
    m = synth.MARGIN
    cx_n, cy_n = dims(w, h)
    per = field.shape[1]
    g = 64 if per == 1 else 8
    for ctu in (range(cx_n * cy_n) if ctus is None else ctus):
        cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        for b in range(per):
            bx, by = (b % 8) * g, (b // 8) * g
            r = int(ref_field[ctu, b])
            if r >= len(planes) or cu_x + bx >= w or cu_y + by >= h:
                continue
            qx, qy = clip_mv(hmo, field[ctu, b, 0], field[ctu, b, 1], cu_x, cu_y, w, h)
            p = bwm.pred_w(planes[r], m + cu_x + bx, m + cu_y + by, g, g, qx, qy, bd, wps[r])
            x1, y1 = min(cu_x + bx + g, w), min(cu_y + by + g, h)
            out[cu_y + by:y1, cu_x + bx:x1] = p[:y1 - cu_y - by, :x1 - cu_x - bx]
    return out


# ---- the rule of hmme_predict_bi_weight_check as include/hmme.h states it ----------------------------------------------------------------
ERR_ARG, ERR_UNSUPPORTED = -1, -5            # HMME_ERR_ARG, HMME_ERR_UNSUPPORTED


def single_reach(bd, wp):
    """|w0| * 40 960 + round'_uni: the "other weight" line, which a block of one list goes through"""
    return abs(int(wp[0])) * PEL_REACH + (1 << (int(wp[2]) + max(2, 14 - bd) - 1))


def pair_reach(bd, wp0, wp1):
    """(|w0| + |w1|) * 40 960 + round' + |off| * 2^(shift' - 1)"""
    shift = int(wp0[2]) + 1 + max(2, 14 - bd)
    return (abs(int(wp0[0])) + abs(int(wp1[0]))) * PEL_REACH + (1 << (shift - 1)) + abs(int(wp0[1]) + int(wp1[1])) * (1 << (shift - 1))


def check(bd, wp0, wp1):
    """-> 0, ERR_ARG or ERR_UNSUPPORTED, as the header orders them: arguments first, each weight alone, then the pair"""
    if bd < 8 or bd > 12 or wp0 is None or wp1 is None:
        return ERR_ARG
    if not (0 <= int(wp0[2]) <= 15 and 0 <= int(wp1[2]) <= 15) or int(wp0[2]) != int(wp1[2]):
        return ERR_ARG
    if single_reach(bd, wp0) > INT32_MAX or single_reach(bd, wp1) > INT32_MAX:
        return ERR_UNSUPPORTED
    return ERR_UNSUPPORTED if pair_reach(bd, wp0, wp1) > INT32_MAX else 0


def ident(shift):
    return (1 << shift, 0, shift, (1 << (shift - 1)) if shift else 0)


# ---- content: the fade of a three-band picture -------------------------------------------------------------------------------------------------
FADE_MV = ((3, -2), (-2, 1))                     # full-pel displacement of list 0 and list 1
FADE_GAIN, FADE_DENOM, FADE_OFFSET = 45, 6, 12   # cur = ((45 * x + 32) >> 6) + (12 << (bd - 8)): a fade to 70 % with a lift
FADE_BANDS = (48, 96)                            # columns below 48: list 0's picture; from 96: list 1's; between: the rounded average of both


def fade_pictures(w, h, bd, seed):
    """-> (cur_img [h, w] int64, refs: two padded int16 planes).  Before the fade the left band is list 0's picture moved by FADE_MV[0], the
    right band list 1's moved by FADE_MV[1], the middle band the rounded average of both; the fade is applied to all of it and clipped"""
    from hmme import synth
    m = synth.MARGIN
    refs = [synth.make_pair(w, h, seed=seed + 7 * k, bit_depth=bd, max_mv=2)[1] for k in range(2)]
    moved = [r[m + dy:m + dy + h, m + dx:m + dx + w].astype(np.int64) for r, (dx, dy) in zip(refs, FADE_MV)]
    a, b = FADE_BANDS
    x = moved[0].copy()
    x[:, a:b] = (moved[0][:, a:b] + moved[1][:, a:b] + 1) >> 1
    x[:, b:] = moved[1][:, b:]
    cur = ((FADE_GAIN * x + (1 << (FADE_DENOM - 1))) >> FADE_DENOM) + (FADE_OFFSET << (bd - 8))
    return np.clip(cur, 0, (1 << bd) - 1), refs


def fade_wps(bd):
    """the weights that undo the fade: the same for both lists, so a bi block gets gain * average + offset"""
    return ((FADE_GAIN, FADE_OFFSET << (bd - 8), FADE_DENOM, 1 << (FADE_DENOM - 1)),) * 2


def fade_truth(w, h):
    """-> (field int16[2, n_ctu, 64, 2], dirs uint8[n_ctu, 64]): the true motion and direction of every 8x8 block of the fade"""
    cx_n, cy_n = dims(w, h)
    n = cx_n * cy_n
    field = np.zeros((2, n, 64, 2), np.int16)
    dirs = np.zeros((n, 64), np.uint8)
    for l in range(2):
        field[l, :, :] = (4 * FADE_MV[l][0], 4 * FADE_MV[l][1])
    for c in range(n):
        for b in range(64):
            x0 = (c % cx_n) * 64 + (b % 8) * 8
            dirs[c, b] = 1 if x0 < FADE_BANDS[0] else 3 if x0 < FADE_BANDS[1] else 2
    return field, dirs
