"""The prediction of a B picture with several references per list in a slice with explicit weighted prediction
(hmme_predict_bi_refs_w_device) restated from the rule in include/hmme.h ("multi-reference B pictures: explicit weights and 4:2:0
chroma"): predict_bi_refs_model's walk over the blocks with predict_bi_w_model.pred_block -- addWeightUni / addWeightBi -- on the two planes
AND the two weights the block's reference indices name.  And the rule of hmme_predict_bi_refs_weight_check restated.  Plain numpy, no
GPU: the reference of tests/test_bi_refs_w_cpu.py and tests/test_gpu_predict_bi_refs_w.py."""
import predict_bi_w_model as pbw
from frame_helpers import clip_mv, dims

ERR_ARG, ERR_UNSUPPORTED, INT32_MAX = pbw.ERR_ARG, pbw.ERR_UNSUPPORTED, pbw.INT32_MAX


def live_blocks(w, h, per, dirs, refs, n0, n1, ctus=None):
    """(ctu, b, cu_x, cu_y, bx, by, g, direction, (r0, r1)) of every block that is written: it starts inside the picture, its direction is
    1, 2 or 3 and every list the direction names has an index below that list's count"""
    cx_n, cy_n = dims(w, h)
    g = 64 if per == 1 else 8
    for ctu in (range(cx_n * cy_n) if ctus is None else ctus):
        cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        for b in range(per):
            bx, by = (b % 8) * g, (b // 8) * g
            d = int(dirs[ctu, b])
            if d not in (1, 2, 3) or cu_x + bx >= w or cu_y + by >= h:
                continue
            idx = (int(refs[0, ctu, b]), int(refs[1, ctu, b]))
            if any((d >> l) & 1 and idx[l] >= (n0, n1)[l] for l in range(2)):
                continue
            yield ctu, b, cu_x, cu_y, bx, by, g, d, idx


def pred_picture(hmo, planes0, planes1, wps0, wps1, w, h, bd, field, dirs, refs, out, ctus=None):
    """what hmme_predict_bi_refs_w_frame writes into `out` ([h, w], changed in place and returned): planes0 / planes1 the padded pictures of
    list 0 / list 1, wps0 / wps1 one (w0, offset, shift, round) per plane, field int16[2, n_ctu, 1 | 64, 2], dirs uint8[n_ctu, 1 | 64], refs
    uint8[2, n_ctu, 1 | 64]; every MV clamped by hmo_clip_mv for its CTU.  Blocks that are not live keep their values"""
    from hmme import synth
    m = synth.MARGIN
    lists, wps = (planes0, planes1), (wps0, wps1)
    for ctu, b, cu_x, cu_y, bx, by, g, d, idx in live_blocks(w, h, field.shape[2], dirs, refs, len(planes0), len(planes1), ctus):
        two = [lists[l][idx[l]] if (d >> l) & 1 else None for l in range(2)]   # a list the direction does not name is not looked at
        wt = [wps[l][idx[l]] if (d >> l) & 1 else None for l in range(2)]
        mvs = [clip_mv(hmo, field[l, ctu, b, 0], field[l, ctu, b, 1], cu_x, cu_y, w, h) for l in range(2)]
        p = pbw.pred_block(two, m + cu_x + bx, m + cu_y + by, g, mvs, d, bd, wt)
        x1, y1 = min(cu_x + bx + g, w), min(cu_y + by + g, h)
        out[cu_y + by:y1, cu_x + bx:x1] = p[:y1 - cu_y - by, :x1 - cu_x - bx]
    return out


# ---- the rule of hmme_predict_bi_refs_weight_check as include/hmme.h states it -------------------------------------------------------------
def check(bd, wps0, wps1, n0=None, n1=None):
    """-> 0, ERR_ARG or ERR_UNSUPPORTED in the header's order: 1. the argument errors of every weight of list 0, then of list 1; 2. unequal
    shifts anywhere among the n0 + n1 weights; 3. each weight alone, list 0 then list 1; 4. every pair (r0, r1), r0-major"""
    n0 = (0 if wps0 is None else len(wps0)) if n0 is None else n0
    n1 = (0 if wps1 is None else len(wps1)) if n1 is None else n1
    for wps, n in ((wps0, n0), (wps1, n1)):
        if bd < 8 or bd > 12 or wps is None or n < 1 or n > 16:
            return ERR_ARG
        if any(not 0 <= int(wp[2]) <= 15 for wp in wps[:n]):
            return ERR_ARG
    both = list(wps0[:n0]) + list(wps1[:n1])
    if any(int(wp[2]) != int(both[0][2]) for wp in both):
        return ERR_ARG
    if any(pbw.single_reach(bd, wp) > INT32_MAX for wp in both):
        return ERR_UNSUPPORTED
    if any(pbw.pair_reach(bd, a, b) > INT32_MAX for a in wps0[:n0] for b in wps1[:n1]):
        return ERR_UNSUPPORTED
    return 0
