"""The prediction of a B picture with several references per list (hmme_predict_bi_refs_device) restated from the rule in include/hmme.h
("B pictures with several references per list", the prediction): per block predict_bi_model.pred_block on the two planes the block's
reference indices name.  Plain numpy, no GPU: the reference of tests/test_gpu_predict_bi_refs.py."""
import predict_bi_model as pbm
from frame_helpers import clip_mv, dims


def pred_picture(hmo, planes0, planes1, w, h, bd, field, dirs, refs, out, ctus=None):
    """what hmme_predict_bi_refs_frame writes into `out` ([h, w], changed in place and returned): planes0 / planes1 the padded pictures of
    list 0 / list 1, field int16[2, n_ctu, 1 | 64, 2], dirs uint8[n_ctu, 1 | 64], refs uint8[2, n_ctu, 1 | 64]; every MV clamped by
    hmo_clip_mv for its CTU.  Blocks of another direction than 1, 2, 3, blocks that use a list whose index is >= that list's count and
    samples beyond the picture or outside the CTUs `ctus` (None: all) keep their values"""
    from hmme import synth
    m = synth.MARGIN
    lists = (planes0, planes1)
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
            idx = [int(refs[l, ctu, b]) for l in range(2)]
            if any((d >> l) & 1 and idx[l] >= len(lists[l]) for l in range(2)):
                continue
            two = [lists[l][idx[l]] if (d >> l) & 1 else None for l in range(2)]   # a list the direction does not name is not looked at
            mvs = [clip_mv(hmo, field[l, ctu, b, 0], field[l, ctu, b, 1], cu_x, cu_y, w, h) for l in range(2)]
            p = pbm.pred_block(two, m + cu_x + bx, m + cu_y + by, g, mvs, d, bd)
            x1, y1 = min(cu_x + bx + g, w), min(cu_y + by + g, h)
            out[cu_y + by:y1, cu_x + bx:x1] = p[:y1 - cu_y - by, :x1 - cu_x - bx]
    return out
