"""numpy restatement of the luma part of HM's weighted-prediction estimator -- the yardstick of tests/test_wp_estimate_cpu.py and
tests/test_gpu_wp_estimate.py.  Five functions of source/Lib/TLibEncoder/WeightPredAnalysis.cpp of the reference, for a 4:0:0 slice without
high-precision weighting:

    xCalcACDCParamSlice    :67-120     plane_stats
    xEstimateWPParamSlice  :172-196    estimate (the loop over the denominator)
    xUpdatingWPParameters  :200-268    update_parameters
    xSelectWP              :272-320    estimate (the ratio test)
    xCalcSADvalueWP        :324-351    sad_value

and TComSlice::initWpScaling (TLibCommon/TComSlice.cpp:1487-1512) for the weight that is handed out.  Sums are int64 (HM: Int64), the two
`Double` expressions are Python floats (IEEE doubles, as HM's), and the two divisions HM leaves to IEEE (0 / 0, x / 0) are written out.
Pictures are 2-D integer arrays holding the picture area only."""
import math

import numpy as np

DTHRESH = 0.99   # WeightPredAnalysis.cpp:45


def _c_div(a, b):
    """C's integer division (truncation towards zero); every dividend here is >= 0, where it is floor division"""
    assert a >= 0 and b > 0
    return a // b


def plane_stats(pic):
    """:84-112 -> (iOrgDC, iOrgAC) = (sum of the samples, sum of |sample - iOrgNormDC|)"""
    p = np.asarray(pic).astype(np.int64)
    n = p.size                                            # :84 iSample
    dc_sum = int(p.sum())                                 # :86-97
    norm_dc = _c_div(dc_sum + (n >> 1), n)                # :99
    ac = int(np.abs(p - norm_dc).sum())                   # :101-112
    return dc_sum, ac


def norm_dc(dc_sum, n):
    """:115 with fixedBitShift = 0: weightACDCParam.iDC"""
    return _c_div(dc_sum + (n >> 1), n)


def update_parameters(cur_stats, ref_stats, n, bit_depth, log2_denom):
    """xUpdatingWPParameters for luma -> (in_range, [(weight, clipped offset)] per reference).  As in HM, the first reference out of range
    ends the pass (:255-258)"""
    real_log2_denom = log2_denom + (bit_depth - 8)        # :223
    real_offset = 1 << (real_log2_denom - 1)              # :224
    cur_dc, cur_ac = norm_dc(cur_stats[0], n), cur_stats[1]
    out = []
    for ref_sum, ref_ac in ref_stats:
        ref_dc = norm_dc(ref_sum, n)
        d_weight = 1.0 if ref_ac == 0 else min(max(-16.0, float(cur_ac) / float(ref_ac)), 15.0)         # :234 (Clip3 = min(max(lo, x), hi))
        weight = int(0.5 + d_weight * float(1 << log2_denom))                                           # :235 ((Int) truncates, as int())
        offset = ((cur_dc << log2_denom) - weight * ref_dc + real_offset) >> real_log2_denom            # :236 (>> of an Int64: arithmetic)
        clipped = min(max(-128, offset), 127)                                                           # :222, :248 (range = 128)
        delta = (1 << log2_denom) - weight                                                              # :252-253
        if delta >= 128 or delta < -128:                                                                # :255
            return False, out
        out.append((weight, clipped))
    return True, out


def sad_value(org, ref, bit_depth, log2_denom, weight, offset):
    """xCalcSADvalueWP (:336-350)"""
    o, r = np.asarray(org).astype(np.int64), np.asarray(ref).astype(np.int64)
    real_log2_denom = log2_denom + (bit_depth - 8)                                                       # :337
    sad = int(np.abs((o << log2_denom) - (r * weight + offset * (1 << real_log2_denom))).sum())          # :344 (offset << n as a product: offset < 0)
    return _c_div(sad, o.size)                                                                           # :350


def ratio_disables(sad_wp, sad_nowp):
    """:305-306 `(Double)iSADWP / (Double)iSADnoWP >= DTHRESH` with IEEE's divisions by zero spelled out -> (ratio, disabled)"""
    if sad_nowp == 0:
        ratio = math.nan if sad_wp == 0 else math.inf     # 0 / 0 = NaN: no comparison with NaN is true; x / 0 = +inf for x > 0
    else:
        ratio = float(sad_wp) / float(sad_nowp)
    return ratio, (not math.isnan(ratio)) and ratio >= DTHRESH


def estimate(cur, refs, bit_depth, log2_denom_start=6, stats=None):
    """xEstimateWPParamSlice for one current picture and its references -> list of dicts, one per reference, with the fields of hmme_wp_info
    plus "ratio" and "wp" = (w0, offset, shift, round) after TComSlice::initWpScaling.
    stats: optional {id(picture): (dc_sum, ac)} cache shared between calls"""
    stats = {} if stats is None else stats

    def st(p):
        if id(p) not in stats:
            stats[id(p)] = plane_stats(p)
        return stats[id(p)]
    n = int(np.asarray(cur).size)
    cur_st, ref_st = st(cur), [st(r) for r in refs]
    d = log2_denom_start                                   # :174-180 (6, or 7 with more than three references: the caller's choice)
    while True:                                            # :182-189
        ok, params = update_parameters(cur_st, ref_st, n, bit_depth, d)
        if ok:
            break
        d -= 1
        assert d >= 0
    out = []
    for ref, (ref_sum, ref_ac), (weight, offset) in zip(refs, ref_st, params):
        sad_wp = sad_value(cur, ref, bit_depth, d, weight, offset)       # :301
        sad_nowp = sad_value(cur, ref, bit_depth, d, 1 << d, 0)          # :302
        ratio, disabled = ratio_disables(sad_wp, sad_nowp)
        present = 1
        if disabled:                                                      # :308-314
            present, weight, offset = 0, 1 << d, 0
        wp = (weight, offset * (1 << (bit_depth - 8)), d, (1 << (d - 1)) if d >= 1 else 0)   # TComSlice.cpp:1505-1508
        out.append({"cur_dc_sum": cur_st[0], "cur_ac": cur_st[1], "ref_dc_sum": ref_sum, "ref_ac": ref_ac, "sad_wp": sad_wp, "sad_nowp": sad_nowp,
                    "log2_denom": d, "weight": weight, "offset": offset, "present": present, "ratio": ratio, "wp": wp})
    return out


INFO_FIELDS = ("cur_dc_sum", "cur_ac", "ref_dc_sum", "ref_ac", "sad_wp", "sad_nowp", "log2_denom", "weight", "offset", "present")


# ---- pictures whose numbers can be checked by hand ---------------------------------------------------------------------------------------------
def checkerboard(w, h, a, b):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((xx + yy) & 1, b, a).astype(np.int64)


def pictures(case, w=64, h=48, bd=8):
    """(cur, ref) of the five hand-checkable cases of tests/test_wp_estimate_cpu.py; tests/test_gpu_wp_estimate.py runs the same on the device"""
    maxv = (1 << bd) - 1
    rng = np.random.default_rng(4242)
    if case == "checkerboard":      # AC ratio 3.5
        return checkerboard(w, h, 100, 135), checkerboard(w, h, 120, 130)
    if case == "identical":
        p = rng.integers(0, maxv + 1, (h, w))
        return p, p.copy()
    if case == "flat_reference":    # refAC == 0
        return rng.integers(0, maxv + 1, (h, w)), np.full((h, w), 77, np.int64)
    if case == "offset_fade":       # cur = ref + 20, nothing clipped
        ref = rng.integers(30, 200, (h, w))
        return ref + 20, ref
    if case == "noise":             # unrelated pictures
        return rng.integers(0, maxv + 1, (h, w)), rng.integers(0, maxv + 1, (h, w))
    raise KeyError(case)


CASES = ("checkerboard", "identical", "flat_reference", "offset_fade", "noise")
