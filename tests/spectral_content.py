"""Pictures whose Hadamard sums sit AT the bound the packed refinement sums are sized for (me_kernels.hpp, frac_pack3), for
tests/test_spectral_cpu.py and tests/test_gpu_refine_spectral.py.  Plain numpy, no GPU.

The Sylvester matrix H8[y][x] = (-1)^popcount(x & y) is a bent sign pattern: every one of the 64 coefficients of its 8x8 Walsh-Hadamard
transform has magnitude 8 (H8 H8 H8^T = 8 H8), so a difference of +-span in that pattern gives an 8x8 block sum of (512 * span + 2) >> 2 =
128 * span -- Parseval's bound with equality -- and, each 4x4 quadrant being +-H4, four 4x4 block sums of (64 * span + 1) >> 1 = 32 * span at
the same time.  Every one of the 593 slots then holds w * h * 2 * span before the shift by bitDepth - 8.

  bent_sign / bent_plane / complement     the pattern tiled over a picture, as signs and as samples in {0, maxv}
  bent_pair(kind, w, h, bd)               (cur, ref): ref the complement of cur (difference +-maxv), or flat 0 / flat maxv
  bi_triple(w, h, bd)                     (cur, ref, other): origin 2 * cur - other in {2 * maxv, -maxv}, difference against ref +-2 * maxv
  weighted_pair(w, h, bd, wp)             (cur, ref): difference against the weighted ref maxv - wlo / -whi in the pattern
  slot_rects / slot_bound                 the 593 rectangles (api.slot_rect) and w * h * 2 * span >> (bd - 8)
  block_maps / slot_sums                  the Hadamard (residual_model.had_rule) and SAD sums of every slot of a 64x64 difference, int64
  position_sums / refine_model            the 49 quarter-pel positions around an integer MV of one CTU (range_content.pred_qpel) and HM's
                                          two-stage refinement over them, every slot: the restatement the oracle is held to
"""
import functools

import numpy as np

import range_content as rc
import residual_model as rm
from tie_content import REFINE_H, REFINE_Q

KINDS = ("complement", "flat0", "flatmax")
NUM_PARTS = 593


def bent_sign(w, h, x0=0, y0=0):
    """+1 / -1 [h, w]: H8 tiled, sample (0, 0) of the tiling at (x0, y0)"""
    ys, xs = np.mgrid[0:h, 0:w]
    v = ((xs - x0) & 7) & ((ys - y0) & 7)
    par = (v ^ (v >> 1) ^ (v >> 2)) & 1
    return 1 - 2 * par.astype(np.int64)


def bent_plane(w, h, bd):
    return np.where(bent_sign(w, h) > 0, (1 << bd) - 1, 0).astype(np.int64)


def complement(p, bd):
    return ((1 << bd) - 1) - np.asarray(p).astype(np.int64)


def pad(p):
    from hmme import synth
    return synth.pad_plane(p)


def bent_pair(kind, w, h, bd):
    """-> (cur, ref) padded int16 planes (the engine's margin, edge-replicated)"""
    cur = bent_plane(w, h, bd)
    ref = {"complement": complement(cur, bd), "flat0": np.zeros_like(cur), "flatmax": np.full_like(cur, (1 << bd) - 1)}[kind]
    return pad(cur), pad(ref)


def bi_triple(w, h, bd):
    """-> (cur, ref, other) padded: other = the complement of cur (read at MV 0), ref the same picture"""
    cur = bent_plane(w, h, bd)
    other = complement(cur, bd)
    return pad(cur), pad(other), pad(other)


def weighted_pair(w, h, bd, wp):
    """-> (cur, ref) padded: where the pattern is positive cur = maxv over the reference sample whose weighted value is the lower one (wlo),
    elsewhere cur = 0 over the one weighted to whi"""
    maxv = (1 << bd) - 1
    at0, atmax = int(rc.weigh(0, wp)), int(rc.weigh(maxv, wp))
    v_lo, v_hi = (0, maxv) if at0 <= atmax else (maxv, 0)
    pos = bent_sign(w, h) > 0
    return pad(np.where(pos, maxv, 0)), pad(np.where(pos, v_lo, v_hi))


def weighted_differences(bd, wp):
    """(maxv - wlo, -whi): the two values the difference of weighted_pair takes at the integer position"""
    maxv = (1 << bd) - 1
    a, b = int(rc.weigh(0, wp)), int(rc.weigh(maxv, wp))
    return maxv - min(a, b), -max(a, b)


@functools.lru_cache(maxsize=None)
def slot_rects():
    from hmme import api
    return tuple(tuple(int(v) for v in api.slot_rect(s)) for s in range(NUM_PARTS))


def slot_bound(slot, bd, span):
    _, _, w, h = slot_rects()[slot]
    return (w * h * 2 * span) >> (bd - 8)


def small_slots():
    """the slots of at most 64 samples: the 320 of the 8x8 CUs (8x8, 8x4, 4x8) and the 64 AMP slivers of the 16x16 CUs (16x4, 4x16)"""
    return [s for s, (_, _, w, h) in enumerate(slot_rects()) if w * h <= 64]


# ---- the Hadamard and SAD rules on a 64x64 difference -------------------------------------------------------------------------------
def block_maps(d):
    """d: int64 [64, 64] -> (b8 [8, 8], b4 [16, 16], sad4 [16, 16]): every 8x8 block's (sum + 2) >> 2, every 4x4 block's (sum + 1) >> 1
    (residual_model.had_rule on the block, bit depth 8: no shift) and every 4x4 block's sum of absolute differences"""
    d = np.asarray(d).astype(np.int64)
    assert d.shape == (64, 64)
    b8 = np.array([[rm.had_rule(d[8 * j:8 * j + 8, 8 * i:8 * i + 8], 8) for i in range(8)] for j in range(8)], np.int64)
    b4 = np.array([[rm.had_rule(d[4 * j:4 * j + 4, 4 * i:4 * i + 4], 8) for i in range(16)] for j in range(16)], np.int64)
    sad4 = np.abs(d).reshape(16, 4, 16, 4).sum(axis=(1, 3))
    return b8, b4, sad4


def slot_sums(d):
    """int64 [2, 593]: the SAD ([0]) and xGetHADs ([1]: 8x8 blocks where both sides are multiples of 8, else 4x4 blocks) of every slot's
    rectangle of the CTU's difference d, BEFORE the shift by bitDepth - 8"""
    b8, b4, sad4 = block_maps(d)
    out = np.zeros((2, NUM_PARTS), np.int64)
    for s, (x, y, w, h) in enumerate(slot_rects()):
        out[0, s] = sad4[y >> 2:(y + h) >> 2, x >> 2:(x + w) >> 2].sum()
        if w % 8 == 0 and h % 8 == 0:
            out[1, s] = b8[y >> 3:(y + h) >> 3, x >> 3:(x + w) >> 3].sum()
        else:
            out[1, s] = b4[y >> 2:(y + h) >> 2, x >> 2:(x + w) >> 2].sum()
    return out


def ctu_difference(org, ref, bd, qx, qy, origin=None, org_origin=None, wp=None):
    """the 64x64 difference of CTU 0 at the quarter-pel displacement (qx, qy): org - clip(interpolation of ref) (weighted by wp after the
    clip, as xGetHADsw / xGetSADw do).  origin / org_origin: sample (0, 0) inside ref / org (default: the engine's margin)"""
    from hmme import synth
    ox, oy = origin if origin is not None else (synth.MARGIN, synth.MARGIN)
    cx, cy = org_origin if org_origin is not None else (synth.MARGIN, synth.MARGIN)
    p = rc.pred_qpel(ref, ox, oy, 64, 64, qx, qy, bd)
    if wp is not None:
        p = rc.weigh(p, wp)
    return np.asarray(org)[cy:cy + 64, cx:cx + 64].astype(np.int64) - p


def position_sums(org, ref, bd, imv=(0, 0), **kw):
    """{(qx, qy) relative to 4 * imv, each in -3..3: slot_sums} for the 49 positions the refinement can visit"""
    return {(qx, qy): slot_sums(ctu_difference(org, ref, bd, 4 * imv[0] + qx, 4 * imv[1] + qy, **kw)) for qy in range(-3, 4) for qx in range(-3, 4)}


def component_bits(v):
    """xGetComponentBits"""
    t = (-v << 1) + 1 if v <= 0 else v << 1
    n = 1
    while t != 1:
        t >>= 1
        n += 2
    return n


def mv_cost(lq, qx, qy, pred):
    """getCost of a quarter-pel MV: the 32-bit product of lambda_q16 and the bits, >> 16"""
    return ((lq * (component_bits(qx - pred[0]) + component_bits(qy - pred[1]))) & 0xffffffff) >> 16


def refine_model(sums, had, bd, lq, pred, imv=(0, 0)):
    """xPatternSearchFracDIF of every slot over position_sums (had: 1 Hadamard, 0 SAD): the half-pel stage in the order of s_acMvRefineH,
    the quarter-pel stage around its winner in the order of s_acMvRefineQ, strict '<' -> (qmv int64 [593, 2], cost int64 [593])"""
    qmv = np.zeros((NUM_PARTS, 2), np.int64)
    cost = np.zeros(NUM_PARTS, np.int64)
    bx, by = 4 * imv[0], 4 * imv[1]
    for s in range(NUM_PARTS):
        centre = (0, 0)
        for step, order in ((2, REFINE_H), (1, REFINE_Q)):
            best, at = None, None
            for dx, dy in order:
                p = (centre[0] + step * dx, centre[1] + step * dy)
                c = (int(sums[p][had][s]) >> (bd - 8)) + mv_cost(lq, bx + p[0], by + p[1], pred)
                if best is None or c < best:
                    best, at = c, p
            centre = at
        qmv[s], cost[s] = (bx + centre[0], by + centre[1]), best
    return qmv, cost
