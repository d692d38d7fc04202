"""4:2:0 chroma motion compensation (hmme_predict_chroma_*_device) restated in numpy int64 from the rule in include/hmme.h:
TComPrediction::xPredInterBlk for a chroma component (TLibCommon/TComPrediction.cpp:669-707) with m_chromaFilter
(TComInterpolationFilter.cpp:65-75), and the picture models of the three forms on frame_helpers.clip_mv and the luma tails -- TComYuv::addAvg
(predict_bi_model.add_avg), addWeightUni (bipred_wp_model.add_weight_uni) and addWeightBi (predict_bi_w_model.add_weight_bi), which HM runs
per component with the component's own weight.  Plain numpy, no GPU: the reference of tests/test_predict_chroma_cpu.py and
tests/test_gpu_predict_chroma.py."""
import numpy as np

import bipred_wp_model as bwm
import predict_bi_w_model as pbw
from frame_helpers import clip_mv, dims
from predict_bi_model import add_avg

# m_chromaFilter[8][4]: the four-tap DCT-IF at eighth-pel phases; phase 0 is the copy written as a filter
CHROMA_TAPS = np.array([[0, 64, 0, 0], [-2, 58, 10, -2], [-4, 54, 16, -2], [-6, 46, 28, -4], [-4, 36, 36, -4], [-4, 28, 46, -6], [-2, 16, 54, -4],
                        [-2, 10, 58, -2]], np.int64)


def _two_stage(plane, x, y, w, h, ex, ey, bd):
    """both stages' sums: the w x h block at (x, y) of `plane` displaced by (ex, ey) EIGHTH chroma pels (= the quarter-pel luma MV): integer
    offset e >> 3 (arithmetic), phase e & 7; the first stage (sum - (8192 << sh1)) >> sh1 is kept in an int16"""
    ix, fx, iy, fy = ex >> 3, ex & 7, ey >> 3, ey & 7
    head = max(14 - bd, 2)
    sh1 = 6 - head
    src = np.asarray(plane)[y + iy - 1:y + iy + h + 2, x + ix - 1:x + ix + w + 2].astype(np.int64)
    mid = sum(CHROMA_TAPS[fx, k] * src[:, k:k + w] for k in range(4))
    mid = ((mid - (8192 << sh1)) >> sh1).astype(np.int16).astype(np.int64)
    return sum(CHROMA_TAPS[fy, k] * mid[k:k + h] for k in range(4)), head


def inter_epel(plane, x, y, w, h, ex, ey, bd):
    """xPredInterBlk with bi = true: the 14-bit intermediate P = sum >> 6, a Pel"""
    v, _ = _two_stage(plane, x, y, w, h, ex, ey, bd)
    return (v >> 6).astype(np.int16).astype(np.int64)


def pred_epel(plane, x, y, w, h, ex, ey, bd, clip=True):
    """xPredInterBlk with bi = false: (sum + offset) >> shift, shift = 6 + head, offset = (1 << (shift - 1)) + (8192 << 6), clipped"""
    v, head = _two_stage(plane, x, y, w, h, ex, ey, bd)
    sh2 = 6 + head
    v = (v + (1 << (sh2 - 1)) + (8192 << 6)) >> sh2
    return np.clip(v, 0, (1 << bd) - 1) if clip else v


def pred_block(planes, x, y, n, mvs, direction, bd, wps=None):
    """an n x n chroma block of direction 1, 2 or 3 at (x, y) of one component's padded planes (list 0, list 1); mvs = the clamped luma MV of
    each list; wps = the component's weight of each list, or None"""
    if direction == 3:
        p0, p1 = (inter_epel(planes[l], x, y, n, n, int(mvs[l][0]), int(mvs[l][1]), bd) for l in range(2))
        return add_avg(p0, p1, bd) if wps is None else pbw.add_weight_bi(p0, p1, bd, wps[0], wps[1])
    l = direction - 1
    if wps is None:
        return pred_epel(planes[l], x, y, n, n, int(mvs[l][0]), int(mvs[l][1]), bd)
    return bwm.add_weight_uni(inter_epel(planes[l], x, y, n, n, int(mvs[l][0]), int(mvs[l][1]), bd), bd, wps[l])


def _blocks(w, h, per, ctus):
    """(ctu, b, luma CTU origin, luma block origin inside the CTU, luma block size) of every block that starts inside the w x h LUMA picture"""
    cx_n, cy_n = dims(w, h)
    g = 64 if per == 1 else 8
    for ctu in (range(cx_n * cy_n) if ctus is None else ctus):
        cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        for b in range(per):
            bx, by = (b % 8) * g, (b // 8) * g
            if cu_x + bx < w and cu_y + by < h:
                yield ctu, b, cu_x, cu_y, bx, by, g


def _store(out, p, w, h, cu_x, cu_y, bx, by, g):
    x0, y0 = (cu_x + bx) // 2, (cu_y + by) // 2
    x1, y1 = min(x0 + g // 2, w // 2), min(y0 + g // 2, h // 2)
    out[y0:y1, x0:x1] = p[:y1 - y0, :x1 - x0]


def bi_picture(hmo, comps, w, h, bd, field, dirs, outs, wps=None, ctus=None):
    """what hmme_predict_chroma_bi_frame writes into outs = (cb, cr) ([h / 2, w / 2] each, changed in place and returned).  w, h: the LUMA size;
    comps[c] = (list 0, list 1) padded planes of component c; field int16[2, n_ctu, 1 | 64, 2], dirs uint8[n_ctu, 1 | 64] of the luma CTUs;
    wps[c] = (wp0, wp1) of component c or None.  Every MV clamped by hmo_clip_mv with the luma size for its luma CTU; blocks of another
    direction than 1, 2, 3 and samples outside the CTUs `ctus` (None: all) keep their values"""
    from hmme import synth
    m = synth.MARGIN
    for ctu, b, cu_x, cu_y, bx, by, g in _blocks(w, h, field.shape[2], ctus):
        d = int(dirs[ctu, b])
        if d not in (1, 2, 3):
            continue
        mvs = [clip_mv(hmo, field[l, ctu, b, 0], field[l, ctu, b, 1], cu_x, cu_y, w, h) for l in range(2)]
        for c in range(2):
            p = pred_block(comps[c], m + (cu_x + bx) // 2, m + (cu_y + by) // 2, g // 2, mvs, d, bd, None if wps is None else wps[c])
            _store(outs[c], p, w, h, cu_x, cu_y, bx, by, g)
    return outs


def refs_picture(hmo, comps, w, h, bd, field, ref_field, outs, wps=None, ctus=None):
    """what hmme_predict_chroma_refs_frame writes: comps[c][r] = the padded plane of component c of reference r; field int16[n_ctu, 1 | 64, 2],
    ref_field uint8[n_ctu, 1 | 64]; wps[c][r] or None; blocks whose index is >= the number of references keep their values"""
    from hmme import synth
    m = synth.MARGIN
    for ctu, b, cu_x, cu_y, bx, by, g in _blocks(w, h, field.shape[1], ctus):
        r = int(ref_field[ctu, b])
        if r >= len(comps[0]):
            continue
        mv = clip_mv(hmo, field[ctu, b, 0], field[ctu, b, 1], cu_x, cu_y, w, h)
        for c in range(2):
            p = pred_block((comps[c][r], None), m + (cu_x + bx) // 2, m + (cu_y + by) // 2, g // 2, (mv, None), 1, bd,
                           None if wps is None else (wps[c][r], None))
            _store(outs[c], p, w, h, cu_x, cu_y, bx, by, g)
    return outs


def pairs_picture(hmo, comps, w, h, bd, field, outs, wps=None, ctus=None):
    """what hmme_predict_chroma_frame writes: comps = (cb, cr) padded planes, field int16[n_ctu, 1 | 64, 2], wps = (wp_cb, wp_cr) or None"""
    ref_field = np.zeros(field.shape[:2], np.uint8)
    return refs_picture(hmo, [[comps[0]], [comps[1]]], w, h, bd, field, ref_field, outs, None if wps is None else [[wps[0]], [wps[1]]], ctus)
