"""The other list's prediction of a slice with explicit weighted prediction, and the bi-prediction origin built from it, restated in numpy
int64 for tests/test_bipred_wp_cpu.py and tests/test_gpu_bipred_wp.py; and the rule of hmme_bipred_weight_check restated from
include/hmme.h.  Plain numpy, no GPU.  Citations: source/Lib of the reference encoder.

The interpolation is the one tests/test_range_edges_cpu.py pins to the oracle (range_content.pred_qpel and its taps): the same two passes,
stopped before the rounding."""
import numpy as np

import range_content as rc
from frame_helpers import as_field, clip_mv, dims, origin_picture

IDENT = (64, 0, 6, 32)
INT32_MAX = (1 << 31) - 1


def inter_qpel(plane, x, y, w, h, qx, qy, bd):
    """xPredInterUni(..., bi = true) -> xPredInterBlk (TLibCommon/TComPrediction.cpp:590-594, :669): the 14-bit intermediate P of the w x h block
    at (x, y) of `plane` displaced by (qx, qy) quarter pels.  No rounding, no clip: the vertical stage has shift 6 and offset 0
    (TComInterpolationFilter.cpp:170-212, isLast = false); the copy case comes out as (src << (14 - bd)) - 8192 (filterCopy, :75-118)"""
    ix, fx, iy, fy = qx >> 2, qx & 3, qy >> 2, qy & 3
    head = max(14 - bd, 2)                                       # headRoom = IF_INTERNAL_PREC - bitDepth, at least 2
    sh1 = 6 - head
    src = np.asarray(plane)[y + iy - 3:y + iy + h + 4, x + ix - 3:x + ix + w + 4].astype(np.int64)
    mid = sum(rc.LUMA_TAPS[fx, k] * src[:, k:k + w] for k in range(8))
    mid = (mid - (8192 << sh1)) >> sh1                           # first stage: offset -IF_INTERNAL_OFFS << shift
    v = sum(rc.LUMA_TAPS[fy, k] * mid[k:k + h] for k in range(8))
    return v >> 6                                                # second stage, not last: shift 6, offset 0


def add_weight_uni(p, bd, wp, clip=True):
    """TComWeightPrediction::addWeightUni (TLibCommon/TComWeightPrediction.cpp:133-180) on the intermediate P; wp = (w0, offset, shift, round)
    as getWpScaling delivers it (:250-262)"""
    w0, offset, shift, _unused_round = (int(v) for v in wp)
    shift2 = shift + max(2, 14 - bd)                             # :146 shiftNum = IF_INTERNAL_PREC - bitDepth; :147 shift = wp.shift + shiftNum
    round2 = 1 << (shift2 - 1)                                   # :148 recomputed: wp.round is NOT used
    v = ((w0 * (np.asarray(p).astype(np.int64) + 8192) + round2) >> shift2) + offset   # :52-55 weightUnidir: + IF_INTERNAL_OFFS
    return np.clip(v, 0, (1 << bd) - 1) if clip else v           # ClipBD


def pred_w(plane, x, y, w, h, qx, qy, bd, wp, clip=True):
    """TComPrediction::motionCompensation in a slice with getUseWP() (TLibCommon/TComPrediction.cpp:527-541): xPredInterUni(bi = true), then
    xWeightedPredictionUni -> addWeightUni"""
    return add_weight_uni(inter_qpel(plane, x, y, w, h, qx, qy, bd), bd, wp, clip)


def pred_picture(hmo, ref, w, h, bd, field, wp, clip=True):
    """pred_w for every CTU of the picture, whole 64x64 blocks (partial edge CTUs too: the padded plane serves them), every MV clamped by
    hmo_clip_mv for its CTU.  field: [n_ctu, 1 | 64, 2].  -> int64 [ctus_y * 64, ctus_x * 64]"""
    from hmme import synth
    m = synth.MARGIN
    cx_n, cy_n = dims(w, h)
    field = as_field(field, cx_n * cy_n)
    out = np.zeros((cy_n * 64, cx_n * 64), np.int64)
    for ctu in range(cx_n * cy_n):
        cu_x, cu_y = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        if field.shape[1] == 1:
            blocks = [(0, 0, 64, field[ctu, 0])]
        else:
            blocks = [((b & 7) * 8, (b >> 3) * 8, 8, field[ctu, b]) for b in range(64)]
        for bx, by, n, mv in blocks:
            qx, qy = clip_mv(hmo, mv[0], mv[1], cu_x, cu_y, w, h)
            out[cu_y + by:cu_y + by + n, cu_x + bx:cu_x + bx + n] = pred_w(ref, m + cu_x + bx, m + cu_y + by, n, n, qx, qy, bd, wp, clip)
    return out


def origin(cur, pred_full, w, h):
    """2 * org - pred, unclipped (TLibEncoder/TEncSearch.cpp:3702-3712, TComYuv::removeHighFreq) -> int16 [ctus_y * 64, ctus_x * 64]"""
    return origin_picture(cur, pred_full, w, h)


# ---- the rule of hmme_bipred_weight_check as include/hmme.h states it ------------------------------------------------------------------
SEARCHED_CONDITIONS = ("pel", "span16", "cost", "hadamard", "fp32")


def searched_terms(bd, wp):
    """-> (wlo, whi, bias, span, p0, p1) of the searched list's weight against a bi-prediction origin in [-maxv, 2 * maxv]"""
    w0, offset, shift, rnd = (int(v) for v in wp)
    maxv = (1 << bd) - 1
    p0, p1 = rnd, w0 * maxv + rnd
    a, b = (p0 >> shift) + offset, (p1 >> shift) + offset
    wlo, whi = min(a, b), max(a, b)
    return wlo, whi, max(maxv, -wlo), max(2 * maxv - wlo, whi + maxv), p0, p1


def failing(bd, wp, other_wp, refine):
    """every UNSUPPORTED line of the rule the pair fails -> tuple of names ("other" = the other list's one line)"""
    w0, offset, shift, rnd = (int(v) for v in wp)
    assert 0 <= shift <= 15 and 0 <= int(other_wp[2]) <= 15
    maxv = (1 << bd) - 1
    wlo, whi, bias, span, p0, p1 = searched_terms(bd, wp)
    identity = w0 == 1 << shift and offset == 0 and rnd == ((1 << (shift - 1)) if shift else 0)
    out = []
    if wlo < -32768 or whi > 32767 or min(p0, p1) < -(1 << 31) or max(p0, p1) > INT32_MAX:
        out.append("pel")
    if max(whi, 2 * maxv) + bias > 65535:
        out.append("span16")
    if ((4096 * span) >> (bd - 8)) + 65535 >= rc.INV_COST16:
        out.append("cost")
    if refine and 4096 * span >= 1 << 24:
        out.append("hadamard")
    if refine and not identity and max(abs(p0), abs(p1)) >= 1 << 24:
        out.append("fp32")
    shift2 = int(other_wp[2]) + max(2, 14 - bd)
    if abs(int(other_wp[0])) * 40960 + (1 << (shift2 - 1)) > INT32_MAX:
        out.append("other")
    return tuple(out)


def last_accepted(member, check):
    """member(k): a family of arguments whose acceptance falls monotonically with k, member(0) accepted -> (k, member(k)) of the last one
    check() accepts (0); gallop upward, then bisect"""
    assert check(member(0)) == 0, member(0)
    hi = 1
    while check(member(hi)) == 0:
        hi *= 2
        assert hi < 1 << 26, member(hi)
    lo = hi // 2 if hi > 1 else 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if check(member(mid)) == 0:
            lo = mid
        else:
            hi = mid
    return lo, member(lo)


def boundary_weights(bd, refine):
    """the searched-list weight of each family of range_content.families nearest to a refusal of hmme_bipred_weight_check (the other list at
    the identity) -> list of dicts(family, wp, next, condition); a family whose first member is already refused (the refinement at 12 bits
    refuses every weight) is left out"""
    from hmme import api
    out = []
    for name, member in rc.families(bd).items():
        check = lambda wp: api.bipred_weight_check(bd, wp, IDENT, refine)
        if check(member(0)) != 0:
            continue
        k, wp = last_accepted(member, check)
        nxt = member(k + 1)
        why = failing(bd, nxt, IDENT, refine)
        assert why and failing(bd, wp, IDENT, refine) == (), (bd, name, wp, nxt)
        out.append(dict(family=name, wp=wp, next=nxt, condition=why[0]))
    return out
