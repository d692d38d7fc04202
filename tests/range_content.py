"""Inputs at the edge of what hmme_weight_check / hmme_bipred_check accept, for tests/test_range_edges_cpu.py and
tests/test_gpu_range_edges.py.  Plain numpy, no GPU.

  boundary_weights(bd, refine)   the accepted weight nearest to each refusal, found by walking one parameter of a weight family until
                                 api.weight_check flips (a pure host function of libhmme.so); nothing here is a hard-coded bound
  extreme_pair / extreme_triple  pictures of samples in {0, maxv} that make a block reach the sample differences the rule admits
  extreme_lists                  the same for the bi pass over several references: every plane of the other list flat where the origin peaks
  ramp_pair                      a reference that holds every sample value
  sad_w, pred_qpel               int64 restatements of the weighted SAD and of the two-stage luma interpolation
"""
import numpy as np

SEARCH_CONDITIONS = ("pel", "span16", "cost")     # the refusals of weight_eval (hm-opencl_amd/csrc/hmme.hip) that apply to search and refinement,
REFINE_CONDITIONS = ("hadamard", "fp32")          # and the two that apply to the refinement only; in the order weight_eval tests them
INV_COST16 = 8000000                              # me_kernels.hpp kInvCost16

# (bit depth, condition) pairs that no weight can sit next to, with the reason.  With span = max(maxv - wlo, whi) the cost field,
# ((4096 * span) >> (bd - 8)) + 65535 < 8 000 000, admits span <= 1937, 3874, 7748, 15 497, 30 994 at 8..12 bit (COST_SPAN, asserted in
# tests/test_range_edges_cpu.py):
#   "pel" needs whi > 32 767 or wlo < -32 768, either of which makes span > 32 767 > 30 994;
#   "span16" needs max(whi, maxv) - min(wlo, 0) > 65 535, but both terms are bounded by span: the sum stays at or below 2 * 30 994.
# So whatever these two refuse the cost field refuses as well, and a walk in steps of one sample meets the cost field first.
# "hadamard" (4096 * span < 2^24: span <= 4095) lies above the cost field's span at 8 and 9 bit (1937, 3874).
# "fp32" (|w0 * sample + round| < 2^24) binds at every depth: a weight of shift 15 and gain 2 has span 2 * maxv.
COST_SPAN = {8: 1937, 9: 3874, 10: 7748, 11: 15497, 12: 30994}
CANNOT_BIND = {(bd, c): "the cost field refuses first: it admits no span above 30 994" for bd in range(8, 13) for c in ("pel", "span16")}
CANNOT_BIND.update({(bd, "hadamard"): "the cost field admits a smaller span (1937 / 3874) than 4096 * span < 2^24 does (4095)" for bd in (8, 9)})


def failing(bd, wp, refine):
    """every condition of weight_eval the weight fails, from the nominal range [0, 2^bd - 1] of both pictures -> tuple of names, in its order"""
    w0, offset, shift, rnd = (int(v) for v in wp)
    assert 0 <= shift <= 15
    maxv = (1 << bd) - 1
    p0, p1 = rnd, w0 * maxv + rnd
    a, b = (p0 >> shift) + offset, (p1 >> shift) + offset
    wlo, whi = min(a, b), max(a, b)
    bias = -wlo if wlo < 0 else 0
    span = max(maxv - wlo, whi)
    identity = w0 == 1 << shift and offset == 0 and rnd == ((1 << (shift - 1)) if shift else 0)
    out = []
    if wlo < -32768 or whi > 32767:
        out.append("pel")
    if max(whi, maxv) + bias > 65535:
        out.append("span16")
    if ((4096 * span) >> (bd - 8)) + 65535 >= INV_COST16:
        out.append("cost")
    if refine and 4096 * span >= 1 << 24:
        out.append("hadamard")
    if refine and not identity and max(abs(p0), abs(p1)) >= 1 << 24:
        out.append("fp32")
    return tuple(out)


def span_of(bd, wp):
    """largest |block sample - weighted reference sample| the nominal ranges admit, as weight_eval computes it"""
    w0, offset, shift, rnd = (int(v) for v in wp)
    maxv = (1 << bd) - 1
    a, b = (rnd >> shift) + offset, ((w0 * maxv + rnd) >> shift) + offset
    return max(maxv - min(a, b), max(a, b))


def families(bd):
    """name -> (k -> weight): k = 0 is accepted at every bit depth for search and refinement, acceptance falls monotonically with k"""
    maxv = (1 << bd) - 1
    return {
        "positive_offset": lambda k: (64, k, 6, 32),                       # identity scale, the weighted samples move up
        "negative_offset": lambda k: (64, -k, 6, 32),                      # ... and down: bias > 0
        "inverting": lambda k: (-64, maxv + k, 6, 32),                     # maxv - v at k = 0
        "large_gain": lambda k: (1 + k, 0, 15, 1 << 14),                   # the largest shift, w0 up from 1
        "large_negative_gain": lambda k: (-(1 + k), maxv, 15, 1 << 14),
        "no_shift": lambda k: (1 + k, 0, 0, 0),                            # shift = 0, round = 0
    }


FAMILIES = tuple(families(8))


def boundary_weights(bd, refine, check=None):
    """-> list of dicts(family, wp, next, condition): wp the last member of the family that check(bd, wp, refine) accepts (0), next the
    first it refuses, condition the first test of weight_eval that next fails.  check: api.weight_check unless given"""
    if check is None:
        from hmme import api
        check = api.weight_check
    out = []
    for name, member in families(bd).items():
        assert check(bd, member(0), refine) == 0, (bd, name, member(0))
        hi = 1
        while check(bd, member(hi), refine) == 0:   # gallop upward, then bisect: the walk in steps of one without its million calls
            hi *= 2
            assert hi < 1 << 24, (bd, name)
        lo = hi // 2 if hi > 1 else 0
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if check(bd, member(mid), refine) == 0:
                lo = mid
            else:
                hi = mid
        wp, nxt = member(lo), member(lo + 1)
        why = failing(bd, nxt, refine)
        assert why, (bd, name, nxt)
        out.append(dict(family=name, wp=wp, next=nxt, condition=why[0]))
    return out


def boundary_weight(bd, refine, family):
    return next(b["wp"] for b in boundary_weights(bd, refine) if b["family"] == family)


# ---- restatements ------------------------------------------------------------------------------------------------------------------
def weigh(a, wp):
    return ((int(wp[0]) * np.asarray(a).astype(np.int64) + int(wp[3])) >> int(wp[2])) + int(wp[1])


def sad_w(org, ref, bd, wp):
    """sum over every row of |org - (((w0 * ref + round) >> shift) + offset)|, then >> (bd - 8); int64 throughout"""
    return int(np.abs(np.asarray(org).astype(np.int64) - weigh(ref, wp)).sum()) >> (bd - 8)


LUMA_TAPS = np.array([[0, 0, 0, 64, 0, 0, 0, 0], [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 40, 40, -11, 4, -1], [0, 1, -5, 17, 58, -10, 4, -1]], np.int64)


def pred_qpel(plane, x, y, w, h, qx, qy, bd, clip=True):
    """the w x h luma prediction of the block at (x, y) of `plane` displaced by (qx, qy) quarter pels: horizontal 8-tap pass into the 14-bit
    intermediate, vertical pass, rounding and (unless clip is False) the clip to [0, maxv]; int64"""
    ix, fx, iy, fy = qx >> 2, qx & 3, qy >> 2, qy & 3
    head = max(14 - bd, 2)
    sh1, sh2 = 6 - head, 6 + head
    off1, off2 = -(8192 << sh1), (1 << (sh2 - 1)) + (8192 << 6)
    src = np.asarray(plane)[y + iy - 3:y + iy + h + 4, x + ix - 3:x + ix + w + 4].astype(np.int64)
    mid = sum(LUMA_TAPS[fx, k] * src[:, k:k + w] for k in range(8))
    mid = (mid + off1) >> sh1
    v = sum(LUMA_TAPS[fy, k] * mid[k:k + h] for k in range(8))
    v = (v + off2) >> sh2
    return np.clip(v, 0, (1 << bd) - 1) if clip else v


# ---- content -----------------------------------------------------------------------------------------------------------------------
# The saturated CTUs lie in the bottom CTU row, the binary pattern fills the rest.  FLAT_REACH: samples around a saturated CTU that are flat too
# (a search range of 8; or an MV of 6 pels and the filter's 4 taps)
FLAT_REACH = 12


def _layout(w, h):
    """the two saturated CTUs: the first and the last of the bottom CTU row (partial CTUs where the picture ends inside them: their 64x64
    blocks are whole through the edge replication, which the engine has to reproduce).  -> ctu numbers, column ranges, first flat row"""
    cx_n, cy_n = (w + 63) // 64, (h + 63) // 64
    assert cx_n >= 3 and h - (cy_n - 1) * 64 + FLAT_REACH <= 64
    y0 = (cy_n - 1) * 64
    lo_ctu, hi_ctu = (cy_n - 1) * cx_n, cy_n * cx_n - 1
    return lo_ctu, hi_ctu, (0, 64 + FLAT_REACH), ((cx_n - 1) * 64 - FLAT_REACH, w), y0 - FLAT_REACH


def _binary(rng, h, w, maxv):
    return np.where(rng.integers(0, 2, size=(h, w)) == 1, maxv, 0).astype(np.int64)


def _reference(rng, w, h, maxv):
    _, _, (a0, a1), (b0, b1), fy = _layout(w, h)
    ref = _binary(rng, h, w, maxv)
    ref[fy:, a0:a1] = 0
    ref[fy:, b0:b1] = maxv
    return ref


def saturated_ctus(w, h):
    """(the CTU whose reference block and window are flat 0, the one where they are flat maxv)"""
    return _layout(w, h)[:2]


def extreme_pair(w, h, bd, wp, seed):
    """-> (cur, ref, true_mv): padded int16 planes (synth.pad_plane) and the displacement int[n_ctu, 2] built into each CTU.
    ref: samples in {0, maxv} only -- a seeded per-sample binary pattern, flat 0 over one CTU of the bottom row and its window, flat maxv
    over another.  cur, per CTU: in the two saturated CTUs the value of {0, maxv} farthest from the weighted reference (flat against flat:
    every candidate ties, the MV cost and then the scan order decide); elsewhere the weighted reference displaced by true_mv and clipped,
    with one sample in 16 replaced by binary noise"""
    from hmme import synth
    maxv = (1 << bd) - 1
    rng = np.random.default_rng(seed)
    ref = _reference(rng, w, h, maxv)
    pref = np.pad(ref, synth.MARGIN, mode="edge")
    m = synth.MARGIN
    cx_n, cy_n = (w + 63) // 64, (h + 63) // 64
    lo_ctu, hi_ctu = saturated_ctus(w, h)
    cur = np.zeros((h, w), np.int64)
    true_mv = np.zeros((cx_n * cy_n, 2), np.int64)
    for ctu in range(cx_n * cy_n):
        x0, y0 = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        x1, y1 = min(x0 + 64, w), min(y0 + 64, h)
        if ctu in (lo_ctu, hi_ctu):
            wv = int(weigh(0 if ctu == lo_ctu else maxv, wp))
            cur[y0:y1, x0:x1] = 0 if abs(wv) >= abs(maxv - wv) else maxv
            continue
        dx, dy = (int(v) for v in rng.integers(-3, 4, size=2))
        true_mv[ctu] = (dx, dy)
        moved = np.clip(weigh(pref[m + y0 + dy:m + y1 + dy, m + x0 + dx:m + x1 + dx], wp), 0, maxv)
        noise = _binary(rng, y1 - y0, x1 - x0, maxv)
        cur[y0:y1, x0:x1] = np.where(rng.integers(0, 16, size=moved.shape) == 0, noise, moved)
    return synth.pad_plane(cur), synth.pad_plane(ref), true_mv


def extreme_triple(w, h, bd, seed):
    """-> (cur, ref, other) padded int16 planes for the bi-prediction pass.  ref: the binary pattern.  other: an independent binary pattern, flat
    maxv around the first saturated CTU and flat 0 around the second, FLAT_REACH samples wide: the prediction of those CTUs is flat for every
    MV of up to 6 pels.  cur: 0 in the first and maxv in the second (origins -maxv and 2 * maxv over the whole CTU), elsewhere ref displaced
    per CTU with one sample in 16 replaced by binary noise"""
    from hmme import synth
    maxv = (1 << bd) - 1
    rng = np.random.default_rng(seed)
    lo_ctu, hi_ctu, (a0, a1), (b0, b1), fy = _layout(w, h)
    ref = _binary(rng, h, w, maxv)
    other = _binary(rng, h, w, maxv)
    other[fy:, a0:a1] = maxv
    other[fy:, b0:b1] = 0
    pref = np.pad(ref, synth.MARGIN, mode="edge")
    m = synth.MARGIN
    cx_n, cy_n = (w + 63) // 64, (h + 63) // 64
    cur = np.zeros((h, w), np.int64)
    for ctu in range(cx_n * cy_n):
        x0, y0 = (ctu % cx_n) * 64, (ctu // cx_n) * 64
        x1, y1 = min(x0 + 64, w), min(y0 + 64, h)
        if ctu in (lo_ctu, hi_ctu):
            cur[y0:y1, x0:x1] = 0 if ctu == lo_ctu else maxv
            continue
        dx, dy = (int(v) for v in rng.integers(-2, 3, size=2))
        moved = pref[m + y0 + dy:m + y1 + dy, m + x0 + dx:m + x1 + dx]
        noise = _binary(rng, y1 - y0, x1 - x0, maxv)
        cur[y0:y1, x0:x1] = np.where(rng.integers(0, 16, size=moved.shape) == 0, noise, moved)
    return synth.pad_plane(cur), synth.pad_plane(ref), synth.pad_plane(other)


def extreme_lists(w, h, bd, seed, n_refs=2, n_others=2, band=32):
    """-> (cur, [refs], [others]) padded int16 planes for the bi pass over several references.  refs: binary patterns of the same scene, each
    displaced as a whole.  others: independent binary patterns, ALL flat maxv over the first `band` columns and FLAT_REACH beyond, all flat 0
    over the last `band` columns and FLAT_REACH before them, over the whole height: whichever plane a block's index names and whatever its
    MV of up to 6 pels, the prediction there is flat.  cur: 0 over the first band and maxv over the last -- origins of -maxv and 2 * maxv --,
    elsewhere refs[0]'s scene with one sample in 16 replaced by binary noise"""
    from hmme import synth
    maxv = (1 << bd) - 1
    assert w >= 2 * (band + FLAT_REACH) + 16
    rng = np.random.default_rng(seed)
    scene = np.pad(_binary(rng, h, w, maxv), 8, mode="edge")
    refs = [scene[8 + dy:8 + dy + h, 8 + dx:8 + dx + w] for dx, dy in [(0, 0), (2, -1), (-1, 2), (-2, -2)][:n_refs]]
    others = []
    for _ in range(n_others):
        o = _binary(rng, h, w, maxv)
        o[:, :band + FLAT_REACH] = maxv
        o[:, w - band - FLAT_REACH:] = 0
        others.append(o)
    cur = np.where(rng.integers(0, 16, size=(h, w)) == 0, _binary(rng, h, w, maxv), refs[0])
    cur[:, :band] = 0
    cur[:, w - band:] = maxv
    return synth.pad_plane(cur), [synth.pad_plane(r) for r in refs], [synth.pad_plane(o) for o in others]


def ramp_pair(w, h, bd, seed):
    """-> (cur, ref) padded int16 planes: ref counts through every value 0..maxv in raster order (several times over where the picture has
    more samples than values), cur is the binary pattern"""
    from hmme import synth
    maxv = (1 << bd) - 1
    assert w * h > maxv
    ref = (np.arange(w * h, dtype=np.int64) * 7 % (maxv + 1)).reshape(h, w)   # 7 is coprime to 2^bd: every value, neighbours 7 apart
    cur = _binary(np.random.default_rng(seed), h, w, maxv)
    return synth.pad_plane(cur), synth.pad_plane(ref)
