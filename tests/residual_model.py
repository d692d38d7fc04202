"""The residual and the per-PU / per-CU distortion of hmme_residual_pairs_device restated from the rule in include/hmme.h ("residual and
distortion of a prediction"): the difference with pred := cur outside the picture, the PU error through the oracle's hmo_had / hmo_sad on the
rectangle hmme_slot_rect names (both pinned to the reference by the goldens), the CU's SSE restated from xGetSSE (TComRdCost.cpp:970-1000) with
its per-sample shift, the CU from hmme_slot_key.  This is the reference of tests/test_residual_cpu.py and tests/test_gpu_residual.py -- written
from the rule, not from the kernel.  Plain numpy and Python integers; no GPU."""
import ctypes as C
import functools

import numpy as np

NO_SLOT = 0xFFFF


def n_ctus(w, h):
    return ((w + 63) // 64) * ((h + 63) // 64)


def extended(cur, pred, w, h):
    """cur, pred: the picture areas [h, w] -> int16 [ctus_y * 64, ctus_x * 64]: cur completed by edge replication (what the plane's CTU blocks
    hold; any completion would do), pred := cur outside the picture, so that the difference is 0 there"""
    H, W = (h + 63) // 64 * 64, (w + 63) // 64 * 64
    c = np.pad(np.asarray(cur)[:h, :w].astype(np.int16), ((0, H - h), (0, W - w)), mode="edge")
    p = c.copy()
    p[:h, :w] = np.asarray(pred)[:h, :w].astype(np.int16)
    return np.ascontiguousarray(c), np.ascontiguousarray(p)


def difference(cur, pred, w, h):
    """TComYuv::subtract inside the picture, 0 outside: int16 over the CTU-completed area"""
    c, p = extended(cur, pred, w, h)
    return (c.astype(np.int32) - p.astype(np.int32)).astype(np.int16)


def sse(d, bd):
    """xGetSSE: every squared difference is shifted by (bitDepth - 8) << 1 BEFORE it is added"""
    sq = np.asarray(d).astype(np.int64) ** 2
    return int((sq >> ((bd - 8) << 1)).sum())


def sse_shifted_total(d, bd):
    """what xGetSSE does NOT compute: the shift applied to the total"""
    return int((np.asarray(d).astype(np.int64) ** 2).sum()) >> ((bd - 8) << 1)


def _hadamard(n):
    h = np.array([[1]], np.int64)
    while h.shape[0] < n:
        h = np.kron(np.array([[1, 1], [1, -1]], np.int64), h)
    return h


def had_abs_sum(d):
    """sum of |coefficients| of the unnormalised square Walsh-Hadamard transform of the block d (any ordering of the rows gives the same sum)"""
    hm = _hadamard(d.shape[0])
    return int(np.abs(hm @ np.asarray(d).astype(np.int64) @ hm.T).sum())


def had_rule(d, bd, wide=False):
    """xGetHADs as include/hmme.h states it, in int64: 8x8 blocks of (sum + 2) >> 2 when both sides are multiples of 8, else 4x4 blocks of
    (sum + 1) >> 1; the PU's total >> (bitDepth - 8).  wide: -> (total before the shift, result)"""
    h, w = d.shape
    n, add, sh = (8, 2, 2) if (w % 8 == 0 and h % 8 == 0) else (4, 1, 1)
    total = sum((had_abs_sum(d[y:y + n, x:x + n]) + add) >> sh for y in range(0, h, n) for x in range(0, w, n))
    return (total, total >> (bd - 8)) if wide else total >> (bd - 8)


def had8_from_quadrants(d):
    """the 8x8 sum as the kernel assembles it: the 2x2 butterfly over the 4x4 transforms of the four quadrants (H8 = H2 (x) H4)"""
    h4 = _hadamard(4)
    t = [[h4 @ np.asarray(d[4 * j:4 * j + 4, 4 * i:4 * i + 4]).astype(np.int64) @ h4.T for i in range(2)] for j in range(2)]
    a, b, c, e = t[0][0], t[0][1], t[1][0], t[1][1]
    return int(sum(np.abs(v).sum() for v in (a + b + c + e, a - b + c - e, a + b - c - e, a - b - c + e)))


def _p16(a, y, x):
    return C.cast(a.ctypes.data + 2 * (y * a.shape[1] + x), C.POINTER(C.c_int16))


def pu_error(hmo, c_ext, p_ext, x, y, w, h, bd, use_had):
    """xGetInterPredictionError's distortion over the rectangle (x, y, w, h) of the extended pictures: xGetHADs or xGetSAD, bApplyWeight false"""
    o, p = _p16(c_ext, y, x), _p16(p_ext, y, x)
    if use_had:
        return int(hmo.hmo_had(o, c_ext.shape[1], p, p_ext.shape[1], w, h, bd))
    return int(hmo.hmo_sad(o, c_ext.shape[1], p, p_ext.shape[1], w, h, 0, bd))


@functools.lru_cache(maxsize=None)
def slot_geometry(slot):
    """-> (PU rectangle (x, y, w, h), CU (x, y, size)) inside the CTU, from hmme_slot_rect and the depth / abs_z_idx of hmme_slot_key"""
    from hmme import api
    _, depth, _, z = api.slot_key(slot)
    x = y = 0
    for b in range(4):
        x |= ((z >> (2 * b)) & 1) << b
        y |= ((z >> (2 * b + 1)) & 1) << b
    return api.slot_rect(slot), (4 * x, 4 * y, 64 >> depth)


def residual_picture(hmo, cur, pred, w, h, bd, slot, per, use_had, first=0, count=-1):
    """cur, pred: [h, w]; slot: uint16 [n_ctu, per] over ALL CTUs, or None (every block its own PU and CU)
    -> (difference int16 [h, w], pu uint32 [count, per], cu uint32 [count, per], ctu uint32 [count, 2]) for the CTUs [first, first + count)"""
    n, ctus_x = n_ctus(w, h), (w + 63) // 64
    count = n - first if count < 0 else count
    c_ext, p_ext = extended(cur, pred, w, h)
    d_ext = c_ext.astype(np.int32) - p_ext.astype(np.int32)
    g, nb = (8, 8) if per == 64 else (4, 16)
    pu = np.zeros((count, per), np.uint32)
    cu = np.zeros((count, per), np.uint32)
    ctu = np.zeros((count, 2), np.uint32)
    for k in range(count):
        x0, y0 = ((first + k) % ctus_x) * 64, ((first + k) // ctus_x) * 64
        if slot is None:
            for b in range(per):
                bx, by = x0 + (b % nb) * g, y0 + (b // nb) * g
                pu[k, b] = pu_error(hmo, c_ext, p_ext, bx, by, g, g, bd, use_had)
                cu[k, b] = sse(d_ext[by:by + g, bx:bx + g], bd)
            tot = (int(pu[k].astype(np.int64).sum()), int(cu[k].astype(np.int64).sum()))
        else:
            pus, cus = {}, {}
            for b in range(per):
                s = int(slot[first + k, b])
                if s == NO_SLOT:
                    continue
                (rx, ry, rw, rh), (qx, qy, qs) = slot_geometry(s)
                if s not in pus:
                    pus[s] = pu_error(hmo, c_ext, p_ext, x0 + rx, y0 + ry, rw, rh, bd, use_had)
                if (qx, qy, qs) not in cus:
                    cus[(qx, qy, qs)] = sse(d_ext[y0 + qy:y0 + qy + qs, x0 + qx:x0 + qx + qs], bd)
                pu[k, b] = pus[s]
                cu[k, b] = cus[(qx, qy, qs)]
            tot = (sum(pus.values()), sum(cus.values()))
        assert max(tot) < 1 << 32
        ctu[k] = tot
    return d_ext[:h, :w].astype(np.int16), pu, cu, ctu


def range_mask(w, h, first, count):
    """bool [h, w]: the samples of the CTUs [first, first + count)"""
    n, ctus_x = n_ctus(w, h), (w + 63) // 64
    count = n - first if count < 0 else count
    m = np.zeros((h, w), bool)
    for c in range(first, first + count):
        x0, y0 = (c % ctus_x) * 64, (c // ctus_x) * 64
        m[y0:y0 + 64, x0:x0 + 64] = True
    return m

