"""Prediction from one MV per 4x4 block (hmme_predict_refs4_* / hmme_predict_chroma_refs4_*) restated in numpy from the rule in
include/hmme.h ("prediction from one MV per 4x4 block"): every live 4x4 luma block through bipred_wp_model.pred_w at the MV
frame_helpers.clip_mv gives for its CTU, every 2x2 chroma block through predict_chroma_model.pred_block -- the models the 64 forms are tested
against, called with smaller blocks.  Plain numpy, no GPU: the reference of tests/test_predict4_cpu.py and tests/test_gpu_predict4.py, with
the fields those tests feed."""
import numpy as np

import bipred_wp_model as bwm
import predict_chroma_model as cm
from frame_helpers import clip_mv, dims

PER = 256
NO_REF = 0xFF


def block_xy(b):
    """entry b of a CTU: the 4x4 luma block at this position inside it"""
    return (b & 15) * 4, (b >> 4) * 4


def live_blocks(w, h, ref_field, n_refs, ctus=None):
    """(ctu, b, luma CTU origin, block origin inside the CTU, index) of every live block: it starts inside the w x h luma picture and its index
    (0 where ref_field is None) is < n_refs"""
    cx_n, cy_n = dims(w, h)
    for ctu in (range(cx_n * cy_n) if ctus is None else ctus):
        cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        for b in range(PER):
            bx, by = block_xy(b)
            r = 0 if ref_field is None else int(ref_field[ctu, b])
            if cu_x + bx < w and cu_y + by < h and r < n_refs:
                yield ctu, b, cu_x, cu_y, bx, by, r


def luma_picture(hmo, refs, w, h, bd, field, ref_field, out, wps=None, ctus=None):
    """what hmme_predict_refs4_frame writes into out ([h, w], changed in place and returned): refs[r] = the padded plane of reference r, field
    int16[n_ctu, 256, 2], ref_field uint8[n_ctu, 256] or None, wps[r] or None (the identity: addWeightUni then IS the rounded sample)"""
    from hmme import synth
    m = synth.MARGIN
    for ctu, b, cu_x, cu_y, bx, by, r in live_blocks(w, h, ref_field, len(refs), ctus):
        qx, qy = clip_mv(hmo, field[ctu, b, 0], field[ctu, b, 1], cu_x, cu_y, w, h)
        x, y = cu_x + bx, cu_y + by
        p = bwm.pred_w(refs[r], m + x, m + y, 4, 4, qx, qy, bd, bwm.IDENT if wps is None else wps[r])
        x1, y1 = min(x + 4, w), min(y + 4, h)
        out[y:y1, x:x1] = p[:y1 - y, :x1 - x]
    return out


def chroma_picture(hmo, comps, w, h, bd, field, ref_field, outs, wps=None, ctus=None):
    """what hmme_predict_chroma_refs4_frame writes into outs = (cb, cr) ([h / 2, w / 2] each): comps[c][r] = the padded plane of component c of
    reference r, w x h the LUMA size, wps[c][r] or None"""
    from hmme import synth
    m = synth.MARGIN
    for ctu, b, cu_x, cu_y, bx, by, r in live_blocks(w, h, ref_field, len(comps[0]), ctus):
        mv = clip_mv(hmo, field[ctu, b, 0], field[ctu, b, 1], cu_x, cu_y, w, h)
        x, y = (cu_x + bx) // 2, (cu_y + by) // 2
        x1, y1 = min(x + 2, w // 2), min(y + 2, h // 2)
        for c in range(2):
            p = cm.pred_block((comps[c][r], None), m + x, m + y, 2, (mv, None), 1, bd, None if wps is None else (wps[c][r], None))
            outs[c][y:y1, x:x1] = p[:y1 - y, :x1 - x]
    return outs


# ---- between the two layouts -----------------------------------------------------------------------------------------------------------
def replicate(field64):
    """a 64-entry field ([n, 64, ...]: one entry per 8x8 block) in the 256 layout: every 4x4 block carries its 8x8 block's entry"""
    f = np.asarray(field64)
    n = f.shape[0]
    g = f.reshape((n, 8, 8) + f.shape[2:])
    return np.ascontiguousarray(np.repeat(np.repeat(g, 2, axis=1), 2, axis=2).reshape((n, PER) + f.shape[2:]))


def quadrant_fields(field, ref_field):
    """the four 64-entry fields F_q, q = 2 * (lower half) + (right half): every 8x8 block carries the entry of its quadrant q ->
    [(field int16[n, 64, 2], ref uint8[n, 64])]"""
    n = field.shape[0]
    f = np.asarray(field).reshape(n, 16, 16, 2)
    r = np.asarray(ref_field).reshape(n, 16, 16)
    return [(np.ascontiguousarray(f[:, q >> 1::2, q & 1::2].reshape(n, 64, 2)), np.ascontiguousarray(r[:, q >> 1::2, q & 1::2].reshape(n, 64))) for q in range(4)]


def quadrant_mask(w, h, q, sub=1):
    """boolean [h / sub, w / sub]: the samples of quadrant q of every 8x8 luma block (sub = 2: of every 4x4 chroma block)"""
    g = 4 // sub
    ys, xs = np.arange(h // sub), np.arange(w // sub)
    return ((ys // g) % 2 == q >> 1)[:, None] & ((xs // g) % 2 == (q & 1))[None, :]


def compose(images, w, h, sub=1):
    """quadrant q of every block taken from images[q]"""
    out = images[0].copy()
    for q in range(1, 4):
        m = quadrant_mask(w, h, q, sub)
        out[m] = images[q][m]
    return out


def mixed_blocks(field, ref_field):
    """how many 8x8 blocks hold 4x4 entries that differ"""
    n = field.shape[0]
    key = np.concatenate([np.asarray(field).reshape(n, 16, 16, 2).astype(np.int32), np.asarray(ref_field).reshape(n, 16, 16, 1).astype(np.int32)], axis=3)
    quads = key.reshape(n, 8, 2, 8, 2, 3)
    return int((quads != quads[:, :, :1, :, :1]).any(axis=(2, 4, 5)).sum())


# ---- fields -----------------------------------------------------------------------------------------------------------------------------
def random_field4(w, h, n_refs, seed):
    """random entries per 4x4 block: MVs of up to 40 luma pels with every quarter-pel phase, indices from 0 .. n_refs - 1 plus 0xFF plus n_refs
    itself; four blocks inside the picture, nearest its corners, carry MVs at +-32767 and just beyond the picture, so that the clamp acts on
    every side -> (field int16[n, 256, 2], ref uint8[n, 256])"""
    cx_n, cy_n = dims(w, h)
    n = cx_n * cy_n
    rng = np.random.default_rng(seed)
    field = rng.integers(-160, 161, size=(n, PER, 2)).astype(np.int16)
    ref = rng.choice(np.array(list(range(n_refs)) * 3 + [NO_REF, n_refs], np.uint8), size=(n, PER))
    inside = [(c, b) for c in range(n) for b in range(PER) if (c % cx_n) * 64 + block_xy(b)[0] < w and (c // cx_n) * 64 + block_xy(b)[1] < h]
    pos = {cb: ((cb[0] % cx_n) * 64 + block_xy(cb[1])[0], (cb[0] // cx_n) * 64 + block_xy(cb[1])[1]) for cb in inside}
    far = ((-32767, -32767), (32767, -32768), (-4 * (w + 70) - 1, 32767), (4 * (w + 70) + 3, 4 * (h + 70) + 2))
    for (sx, sy), mv in zip(((0, 0), (1, 0), (0, 1), (1, 1)), far):
        c, b = max(inside, key=lambda cb: (pos[cb][0] if sx else -pos[cb][0]) + (pos[cb][1] if sy else -pos[cb][1]))
        field[c, b] = mv
        ref[c, b] = 0
    return field, ref


def phases_seen(w, h, field, ref_field, n_refs):
    """({horizontal phases}, {vertical phases}, {(px, py)}) of the live blocks"""
    live = [(int(field[c, b, 0]) & 3, int(field[c, b, 1]) & 3) for c, b, *_ in live_blocks(w, h, ref_field, n_refs)]
    return {p[0] for p in live}, {p[1] for p in live}, set(live)


PATTERNS = ("uniform", "top_bottom", "left_right", "four_mvs", "four_refs", "dead_quadrant", "dead")


def pattern_ctu(n_refs, seed):
    """one CTU whose 8x8 blocks cycle through PATTERNS with a step of one per block and a shift of three per block row: the four waves of an
    iteration (four blocks side by side) see four different patterns, and every dead block has live neighbours -> (field int16[1, 256, 2],
    ref uint8[1, 256], pattern name per 8x8 block [8][8])"""
    assert n_refs >= 4
    rng = np.random.default_rng(seed)
    field = np.zeros((16, 16, 2), np.int16)
    ref = np.zeros((16, 16), np.uint8)
    names = [[PATTERNS[(bx + 3 * by) % len(PATTERNS)] for bx in range(8)] for by in range(8)]
    for by in range(8):
        for bx in range(8):
            mvs = rng.integers(-90, 91, size=(4, 2)).astype(np.int16)
            while len({tuple(v) for v in mvs.tolist()}) < 4:                              # four distinct MVs
                mvs = rng.integers(-90, 91, size=(4, 2)).astype(np.int16)
            r0 = int(rng.integers(0, n_refs))
            name = names[by][bx]
            quad_mv = {"uniform": [0, 0, 0, 0], "top_bottom": [0, 0, 1, 1], "left_right": [0, 1, 0, 1], "four_mvs": [0, 1, 2, 3], "four_refs": [0, 0, 0, 0],
                       "dead_quadrant": [0, 1, 2, 3], "dead": [0, 1, 2, 3]}[name]
            quad_ref = [r0] * 4
            if name == "four_refs":
                quad_ref = [(r0 + q) % 4 for q in range(4)]
            elif name == "dead_quadrant":
                quad_ref[int(rng.integers(0, 4))] = NO_REF
            elif name == "dead":
                quad_ref = [NO_REF, n_refs, NO_REF, n_refs]
            for q in range(4):
                field[2 * by + (q >> 1), 2 * bx + (q & 1)] = mvs[quad_mv[q]]
                ref[2 * by + (q >> 1), 2 * bx + (q & 1)] = quad_ref[q]
    return field.reshape(1, PER, 2), ref.reshape(1, PER), names
