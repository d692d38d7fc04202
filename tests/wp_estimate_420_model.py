"""numpy restatement of HM's weighted-prediction estimator for a 4:2:0 slice -- the yardstick of tests/test_wp_estimate_420_cpu.py and
tests/test_gpu_wp_estimate_420.py.  source/Lib/TLibEncoder/WeightPredAnalysis.cpp of the reference without high-precision weighting, one
bit depth for all components.  The per-plane pieces are those of tests/wp_estimate_model.py; what is added here is what HM does across
the components:

    xUpdatingWPParameters  :208-266    update_parameters: reference outer, component inner (:212, :218), the chroma offset rule (:239-245),
                                       the first weight out of range of ANY component ends the pass (:255-258)
    xSelectWP              :285-316    estimate: the three components' SADs, each already divided by its own size (:350), are added (:301-302)
                                       before the ratio (:305); all three components are switched off together (:308-314)

A picture is a triple (y, cb, cr) of 2-D integer arrays holding the picture area only, cb and cr half of y each way."""
from wp_estimate_model import norm_dc, plane_stats, ratio_disables, sad_value

import numpy as np

RANGE = 128   # :222 without high-precision weighting


def clip3(lo, hi, v):
    return min(max(lo, v), hi)


def chroma_offset(offset, weight, log2_denom):
    """:241-244 -> (pred, clippedOffset)"""
    pred = RANGE - ((RANGE * weight) >> log2_denom)                          # :241
    delta = clip3(-4 * RANGE, 4 * RANGE - 1, offset - pred)                  # :242 "signed 10bit"
    return pred, clip3(-RANGE, RANGE - 1, delta + pred)                      # :244 "signed 8bit"


def raw_parameters(cur_stat, ref_stat, n, bit_depth, log2_denom):
    """:223-236 for one component of one reference -> (weight, offset before any clip)"""
    real_log2_denom = log2_denom + (bit_depth - 8)                           # :223
    real_offset = 1 << (real_log2_denom - 1)                                 # :224
    cur_dc, cur_ac = norm_dc(cur_stat[0], n), cur_stat[1]                    # :227-228
    ref_dc, ref_ac = norm_dc(ref_stat[0], n), ref_stat[1]                    # :230-231
    d_weight = 1.0 if ref_ac == 0 else min(max(-16.0, float(cur_ac) / float(ref_ac)), 15.0)      # :234
    weight = int(0.5 + d_weight * float(1 << log2_denom))                                        # :235
    offset = ((cur_dc << log2_denom) - weight * ref_dc + real_offset) >> real_log2_denom         # :236
    return weight, offset


def update_parameters(cur_stats, ref_stats, sizes, bit_depth, log2_denom):
    """xUpdatingWPParameters -> (in_range, [[(weight, clipped offset) per component] per reference]); cur_stats = the three components'
    (dc_sum, ac), ref_stats = one such triple per reference, sizes = the three sample counts.  As in HM the first entry out of range ends the
    pass (:255-258); what it has filled in by then is returned for inspection"""
    out = []
    for ref in ref_stats:                                                     # :212
        out.append([])
        for c in range(3):                                                    # :218
            weight, offset = raw_parameters(cur_stats[c], ref[c], sizes[c], bit_depth, log2_denom)
            clipped = chroma_offset(offset, weight, log2_denom)[1] if c else clip3(-RANGE, RANGE - 1, offset)   # :239-249
            delta = (1 << log2_denom) - weight                                # :252-253
            if delta >= RANGE or delta < -RANGE:                              # :255
                return False, out
            out[-1].append((weight, clipped))                                 # :260-263
    return True, out


def estimate(cur3, refs3, bit_depth, log2_denom_start=6, stats=None):
    """xEstimateWPParamSlice -> one list per reference of three dicts (Y, Cb, Cr) with the fields of hmme_wp_info (sad_wp / sad_nowp: the
    component's own quotient) plus "ratio" (of the reference: the same in its three entries) and "wp" = (w0, offset, shift, round) after
    TComSlice::initWpScaling.  stats: optional {id(plane): (dc_sum, ac)} shared between calls"""
    stats = {} if stats is None else stats

    def st(p):
        if id(p) not in stats:
            stats[id(p)] = plane_stats(p)
        return stats[id(p)]
    sizes = [int(np.asarray(p).size) for p in cur3]
    cur_st, ref_st = [st(p) for p in cur3], [[st(p) for p in ref] for ref in refs3]
    d = log2_denom_start                                                      # :174-180: the caller's choice
    while True:                                                               # :182-189
        ok, params = update_parameters(cur_st, ref_st, sizes, bit_depth, d)
        if ok:
            break
        d -= 1
        assert d >= 0
    out = []
    for ref, rst, par in zip(refs3, ref_st, params):                          # :285
        sad_wp = [sad_value(cur3[c], ref[c], bit_depth, d, par[c][0], par[c][1]) for c in range(3)]   # :301
        sad_nowp = [sad_value(cur3[c], ref[c], bit_depth, d, 1 << d, 0) for c in range(3)]            # :302
        ratio, disabled = ratio_disables(sum(sad_wp), sum(sad_nowp))          # :305-306
        entries = []
        for c in range(3):                                                    # :308-314
            weight, offset = (1 << d, 0) if disabled else par[c]
            wp = (weight, offset * (1 << (bit_depth - 8)), d, (1 << (d - 1)) if d >= 1 else 0)        # TComSlice.cpp:1505-1508
            entries.append({"cur_dc_sum": cur_st[c][0], "cur_ac": cur_st[c][1], "ref_dc_sum": rst[c][0], "ref_ac": rst[c][1],
                            "sad_wp": sad_wp[c], "sad_nowp": sad_nowp[c], "log2_denom": d, "weight": weight, "offset": offset,
                            "present": 0 if disabled else 1, "ratio": ratio, "wp": wp})
        out.append(entries)
    return out


# ---- pictures whose numbers can be checked by hand (luma 32 x 16, chroma 16 x 8, 8 bit) ----------------------------------------------------------
def checkerboard(w, h, a, b):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((xx + yy) & 1, b, a).astype(np.int64)


def flat(w, h, v):
    return np.full((h, w), v, np.int64)


def pictures(case, w=32, h=16):
    """(cur3, ref3) of the three cases of the table in DESIGN.md 7 (item "the estimator for 4:2:0")"""
    rng = np.random.default_rng(420)
    cw, ch = w // 2, h // 2
    if case == 1:      # luma identical; Cb's AC ratio 5 forces d = 5 and its offset goes through the chroma rule; Cr flat on both sides
        y = rng.integers(0, 256, (h, w)).astype(np.int64)
        return (y, checkerboard(cw, ch, 190, 210), flat(cw, ch, 128)), (y.copy(), checkerboard(cw, ch, 18, 22), flat(cw, ch, 128))
    if case == 2:      # unrelated luma; the chroma fades (ref + 60) are predicted exactly and carry the ratio
        rng = np.random.default_rng(79)   # a noise pair whose luma estimate alone is weight 66 with ratio 1.014: disabled on its own
        y, ry = (rng.integers(0, 256, (h, w)).astype(np.int64) for _ in range(2))
        rcb, rcr = (rng.integers(30, 190, (ch, cw)).astype(np.int64) for _ in range(2))
        return (y, rcb + 60, rcr + 60), (ry, rcb, rcr)
    if case == 3:      # luma a pure offset of 2; both chroma planes the checkerboard whose clipped offset makes the weighted SAD 15 times worse
        ry = rng.integers(30, 200, (h, w)).astype(np.int64)
        return (ry + 2, checkerboard(cw, ch, 100, 135), checkerboard(cw, ch, 100, 135)), (ry, checkerboard(cw, ch, 120, 130), checkerboard(cw, ch, 120, 130))
    raise KeyError(case)
