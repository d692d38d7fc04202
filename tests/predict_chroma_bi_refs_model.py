"""The 4:2:0 chroma prediction of a B picture with several references per list (hmme_predict_chroma_bi_refs_device) restated from the rule
in include/hmme.h ("multi-reference B pictures: explicit weights and 4:2:0 chroma"): per live luma block predict_chroma_model.pred_block for
Cb and Cr on the planes -- and with the component's weights -- the block's two reference indices name.  Plain numpy, no GPU: the reference
of tests/test_bi_refs_w_cpu.py and tests/test_gpu_predict_bi_refs_w.py."""
import predict_chroma_model as pcm
from frame_helpers import clip_mv
from predict_bi_refs_w_model import live_blocks


def bi_refs_picture(hmo, comps, w, h, bd, field, dirs, refs, outs, wps=None, ctus=None):
    """what hmme_predict_chroma_bi_refs_frame writes into outs = (cb, cr) ([h / 2, w / 2] each, changed in place and returned).  w, h: the
    LUMA size; comps[c][l][r] = the padded plane of component c of list l's reference r; field int16[2, n_ctu, 1 | 64, 2], dirs uint8[n_ctu,
    1 | 64], refs uint8[2, n_ctu, 1 | 64] of the luma CTUs; wps[c][l][r] = that plane's weight, or wps None.  Every MV clamped by hmo_clip_mv
    with the luma size for its luma CTU; blocks that are not live keep their values"""
    from hmme import synth
    m = synth.MARGIN
    n0, n1 = len(comps[0][0]), len(comps[0][1])
    for ctu, b, cu_x, cu_y, bx, by, g, d, idx in live_blocks(w, h, field.shape[2], dirs, refs, n0, n1, ctus):
        mvs = [clip_mv(hmo, field[l, ctu, b, 0], field[l, ctu, b, 1], cu_x, cu_y, w, h) for l in range(2)]
        for c in range(2):
            two = [comps[c][l][idx[l]] if (d >> l) & 1 else None for l in range(2)]
            wt = None if wps is None else [wps[c][l][idx[l]] if (d >> l) & 1 else None for l in range(2)]
            p = pcm.pred_block(two, m + (cu_x + bx) // 2, m + (cu_y + by) // 2, g // 2, mvs, d, bd, wt)
            pcm._store(outs[c], p, w, h, cu_x, cu_y, bx, by, g)
    return outs
