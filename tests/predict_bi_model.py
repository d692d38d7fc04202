"""The prediction of a picture whose blocks are L0, L1 or bi (hmme_predict_bi_device) restated in numpy int64 from the rule in
include/hmme.h: TComYuv::addAvg (TLibCommon/TComYuv.cpp:352-390) over the two 14-bit intermediates of bipred_wp_model.inter_qpel
(xPredInterUni with bi = true), and range_content.pred_qpel -- pinned to the oracle by tests/test_range_edges_cpu.py -- for a block of one
list.  Plain numpy, no GPU: the reference of tests/test_predict_bi_cpu.py and tests/test_gpu_predict_bi.py."""
import numpy as np

import bipred_wp_model as bwm
import range_content as rc
from frame_helpers import clip_mv, dims


def add_avg(p0, p1, bd):
    """TComYuv::addAvg: ClipBD((P0 + P1 + offset) >> shift), shift = max(2, 14 - bd) + 1, offset = (1 << (shift - 1)) + 2 * IF_INTERNAL_OFFS"""
    shift = max(2, 14 - bd) + 1
    offset = (1 << (shift - 1)) + 2 * 8192
    v = (np.asarray(p0).astype(np.int64) + np.asarray(p1).astype(np.int64) + offset) >> shift
    return np.clip(v, 0, (1 << bd) - 1)


def pred_bi(plane0, plane1, x, y, w, h, mv0, mv1, bd):
    """the bi-directional prediction of the w x h block at (x, y) of the padded planes (TLibCommon/TComPrediction.cpp:527-541 without WP)"""
    return add_avg(bwm.inter_qpel(plane0, x, y, w, h, int(mv0[0]), int(mv0[1]), bd), bwm.inter_qpel(plane1, x, y, w, h, int(mv1[0]), int(mv1[1]), bd), bd)


def pred_block(planes, x, y, n, mvs, direction, bd):
    """an n x n block of direction 1, 2 or 3 at (x, y) of the padded planes, mvs = the (clamped) MV of each list"""
    if direction == 3:
        return pred_bi(planes[0], planes[1], x, y, n, n, mvs[0], mvs[1], bd)
    l = direction - 1
    return rc.pred_qpel(planes[l], x, y, n, n, int(mvs[l][0]), int(mvs[l][1]), bd)


def pred_picture(hmo, planes, w, h, bd, field, dirs, out, ctus=None):
    """what hmme_predict_bi_frame writes into `out` ([h, w], changed in place and returned): field int16[2, n_ctu, 1 | 64, 2], dirs
    uint8[n_ctu, 1 | 64]; every MV clamped by hmo_clip_mv for its CTU; blocks of another direction than 1, 2, 3 and samples beyond the
    picture or outside the CTUs `ctus` (None: all) keep their values"""
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
            p = pred_block(planes, m + cu_x + bx, m + cu_y + by, g, mvs, d, bd)
            x1, y1 = min(cu_x + bx + g, w), min(cu_y + by + g, h)
            out[cu_y + by:y1, cu_x + bx:x1] = p[:y1 - cu_y - by, :x1 - cu_x - bx]
    return out
