"""The numpy models and the oracle against the reference's own compiled code for everything behind the interpolation: the luma and chroma
blocks of TComPrediction::xPredInterBlk, TComYuv::addAvg, xWeightedPredictionUni / Bi with getWpScaling, the slice-level weighted-prediction
estimator, and TComRdCost::getDistPart for SSE, Hadamard and SAD.  The questions and the reference's recorded answers are
tests/golden/ref_*.npz (tests/golden/gen_ref_tails_golden.py); where oracle/_ref/libhmref.so is built the reference is also asked live and
must give the recorded answer, so the check runs on every machine and the recording cannot go stale.  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import bipred_wp_model as bwm
import oracle_py
import predict_bi_model as pbm
import predict_bi_w_model as pbw
import predict_chroma_model as pcm
import range_content as rc
import ref_tails as rt
import residual_model as rm
import wp_estimate_420_model as wm420
import wp_estimate_model as wm
from frame_helpers import bind_hmo

BDS = (8, 9, 10, 11, 12)


class Reference:
    """answer(recorded, question): the recorded answer, after the live library -- where it is built with these entry points -- gave the same"""

    def __init__(self):
        self.live = oracle_py.ref_available() and hasattr(oracle_py.ref(), "ref_pred_block")

    def answer(self, recorded, question):
        if self.live:
            got = np.asarray(question()).astype(np.int64)
            assert np.array_equal(got, np.asarray(recorded).astype(np.int64)), "the live reference differs from its recorded answer"
        return np.asarray(recorded).astype(np.int64)


@pytest.fixture(scope="module")
def reference(oracle_lib):      # after the session's build of the checker libraries
    return Reference()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


def same(a, b):
    return np.array_equal(np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64))


def test_files_are_the_documented_ones():
    B, T = rt.load("ref_blocks"), rt.load("ref_tails")
    assert tuple(B["bds"]) == BDS and tuple(T["bds"]) == BDS
    assert B["luma_src"].shape == (5, 35, 15, 15) and B["chroma_src"].shape == (5, 131, 7, 7)
    assert T["triples"].shape == (60, 3) and T["bi_weights"].shape == (60, 5)
    # HM's whole syntax range is there: both ends of the denominator, of the weight and of the offset
    for d in (0, 7):
        for w in (-128, -1, 0, 1, 127, 1 << d):
            for o in (-128, 127):
                assert ((T["triples"] == (w, o, d)).all(axis=1)).any(), (w, o, d)


@pytest.mark.parametrize("kind", ["luma", "chroma"])
def test_interpolated_blocks_match_reference(kind, reference, hmo):
    """bipred_wp_model.inter_qpel / predict_chroma_model.inter_epel (bi = true, the Pel intermediate) and range_content.pred_qpel /
    predict_chroma_model.pred_epel and the oracle's hmo_pred_block_qpel (bi = false) on random, binary, all-maximum and tap-sign content, every
    bit depth 8..12, every phase"""
    size, before, nfrac = rt.geometry(kind)
    comp = 0 if kind == "luma" else 1
    p16 = C.POINTER(C.c_int16)
    for i, bd in enumerate(BDS):
        for content, ph in rt.all_block_cases(kind):
            src = rt.source(kind, i, content)
            fx, fy = ph % nfrac, ph // nfrac
            for bi in (0, 1):
                want = reference.answer(rt.block(kind, i, content, ph, bi), lambda: oracle_py.ref_pred_block(src, size, size, fx, fy, bd, bi, comp))
                if kind == "luma":
                    got = bwm.inter_qpel(src, 3, 3, 8, 8, fx, fy, bd) if bi else rc.pred_qpel(src, 3, 3, 8, 8, fx, fy, bd)
                else:
                    got = pcm.inter_epel(src, 1, 1, 4, 4, fx, fy, bd) if bi else pcm.pred_epel(src, 1, 1, 4, 4, fx, fy, bd)
                assert same(got, want), (kind, bd, content, ph, bi)
            if kind == "luma":
                s = np.ascontiguousarray(src)
                out = np.zeros((8, 8), np.int16)
                hmo.hmo_pred_block_qpel(C.cast(s.ctypes.data + 2 * (3 * 15 + 3), p16), 15, 8, 8, fx, fy, bd, out.ctypes.data_as(p16), 8)
                assert same(out, rt.block(kind, i, content, ph, 0)), ("oracle", bd, content, ph)


@pytest.mark.parametrize("kind", ["luma", "chroma"])
def test_tap_sign_content_reaches_the_recorded_extremes(kind):
    """the recorded smallest and largest intermediate per bit depth are those of the tap-sign blocks, beyond every other content's, and lie
    inside int16 with room to spare: the (int16_t) casts of the kernels' intermediates never wrap"""
    B = rt.load("ref_blocks")
    for i, bd in enumerate(BDS):
        lo, hi = (int(v) for v in B[kind + "_extremes"][i])
        sign, other = B[kind + "_sign_out"][i, :, :, 1], B[kind + "_out"][i, :, :, 1]
        assert (int(sign.min()), int(sign.max())) == (lo, hi)
        assert lo < int(other.min()) and hi > int(other.max())
        assert -(1 << 15) + 4096 < lo and hi < (1 << 15) - 4096
        for e, (ph, k) in enumerate(B[kind + "_extreme_at"][i]):
            assert int(sign[int(ph), int(k), 0, 0]) == (lo, hi)[e]
    if kind == "luma":
        assert int(B["luma_extremes"].min()) == -25085 and int(B["luma_extremes"].max()) == 25079
    else:
        assert int(B["chroma_extremes"].min()) == -14112 and int(B["chroma_extremes"].max()) == 14106


def _components(kind):
    return ((0, 0),) if kind == "luma" else ((0, 1), (1, 2))


def _recorded(T, name, kind, i, ci):
    a = T[name + "_" + kind][i]
    return a if kind == "luma" else a[ci]


@pytest.mark.parametrize("kind", ["luma", "chroma"])
def test_add_avg_matches_reference(kind, reference):
    """predict_bi_model.add_avg on max + max, min + min, max + min and random operands"""
    T = rt.load("ref_tails")
    for i, bd in enumerate(BDS):
        P = [rt.operand(kind, i, o)[2] for o in range(4)]
        for ci, comp in _components(kind):
            for j, (a, b) in enumerate(T["pairs"]):
                want = reference.answer(_recorded(T, "avg", kind, i, ci)[j], lambda: oracle_py.ref_add_avg(P[a], P[b], bd, comp))
                assert same(pbm.add_avg(P[a], P[b], bd), want), (kind, bd, comp, j)


@pytest.mark.parametrize("kind", ["luma", "chroma"])
def test_add_weight_uni_matches_reference(kind, reference):
    """bipred_wp_model.add_weight_uni with the hmme_weight the header's mapping gives for HM's syntax triple: log2WeightDenom 0 and 7, weights
    -128 .. 127 and the identity, offsets -128 and 127, and random triples"""
    T = rt.load("ref_tails")
    for i, bd in enumerate(BDS):
        P = [rt.operand(kind, i, o)[2] for o in range(4)]
        for ci, comp in _components(kind):
            for k in range(rt.N_WEIGHTS):
                w, o, d = (int(v) for v in T["triples"][rt.cr_index(k) if comp == 2 else k])
                for op in range(4):
                    want = reference.answer(_recorded(T, "uni", kind, i, ci)[op, k], lambda: oracle_py.ref_add_weight_uni(P[op], bd, comp, w, o, d))
                    assert same(bwm.add_weight_uni(P[op], bd, rt.hmme_weight((w, o, d), bd)), want), (kind, bd, comp, (w, o, d), op)


@pytest.mark.parametrize("kind", ["luma", "chroma"])
def test_add_weight_bi_matches_reference(kind, reference):
    """predict_bi_w_model.add_weight_bi with the two lists' hmme_weight"""
    T = rt.load("ref_tails")
    for i, bd in enumerate(BDS):
        P = [rt.operand(kind, i, o)[2] for o in range(4)]
        for ci, comp in _components(kind):
            for k in range(rt.N_WEIGHTS):
                e = T["bi_weights"][rt.cr_index(k) if comp == 2 else k]
                wp0, wp1 = rt.bi_weights(e, bd)
                for j, (a, b) in enumerate(T["pairs"]):
                    want = reference.answer(_recorded(T, "bi", kind, i, ci)[j, k], lambda: oracle_py.ref_add_weight_bi(P[a], P[b], bd, comp, *[int(v) for v in e]))
                    assert same(pbw.add_weight_bi(P[a], P[b], bd, wp0, wp1), want), (kind, bd, comp, tuple(e), j)


def check_estimate(case, entries_of):
    """entries_of(r, c) -> the model's dict for reference r, component c; against the reference's table after initWpScaling and its flags"""
    ncomp = 3 if case["fmt"] == 420 else 1
    table, final, flags = case["table"], case["final"], case["flags"]
    for r in range(case["n_l0"] + case["n_l1"]):
        for c in range(ncomp):
            e = entries_of(r, c)
            present, weight, offset, denom = (int(v) for v in table[r, c])
            assert (e["present"], e["weight"], e["offset"], e["log2_denom"]) == (present, weight, offset, denom), (case["name"], r, c, e, table[r, c])
            assert tuple(e["wp"]) == rt.hmme_weight((weight, offset, denom), case["bd"]), (case["name"], r, c)
    # the two flags xCheckWPEnable leaves in the slice: on exactly when some entry is present; off resets the table to weight 1, denominator 0
    on = bool(table[:, :ncomp, 0].any())
    assert tuple(flags) == (int(on), int(on)), case["name"]
    if on:
        assert np.array_equal(final, table)
    else:
        assert (final[:, :ncomp] == (0, 1, 0, 0)).all()


def _model_parameters(stats, sizes, comps, bd, start):
    """the loop over the denominator (:182-189) around the models' update_parameters -> (d, [(weight, clipped offset)] per entry comps r + c)"""
    cur, refs = stats[:comps], [stats[i:i + comps] for i in range(comps, len(stats), comps)]
    d = start
    while True:
        if comps == 1:
            ok, params = wm.update_parameters(cur[0], [r[0] for r in refs], sizes[0], bd, d)
        else:
            ok, params = wm420.update_parameters(cur, refs, sizes, bd, d)
            params = [e for ref in params for e in ref]
        if ok:
            return d, params
        d -= 1


def _library_estimate(L, pics, comps, bd, start):
    """hmme_test_wp_parameters and hmme_test_wp_select of libhmme.so -- the arithmetic of hmme_wp_estimate (comps = 1) and hmme_wp_estimate_420
    (comps = 3) without its kernels -- on the statistics of wp_estimate_model.plane_stats and on the two raw sums per entry, formed here as the
    comment at me_wp_sad_set_kernel defines them; what the parameter function gives is compared with the models' update_parameters on the way.
    -> one dict per entry comps r + c: the fields of hmme_wp_info and "wp", the hmme_weight"""
    from hmme import api
    planes = [np.asarray(p).astype(np.int64) for pic in pics for p in (pic if comps == 3 else (pic,))]
    n_refs, n = len(pics) - 1, comps * (len(pics) - 1)
    model_stats = [wm.plane_stats(p) for p in planes]
    sizes = [int(p.size) for p in planes[:comps]]
    stats, c_sizes = (C.c_int64 * (2 * len(planes)))(*[v for st in model_stats for v in st]), (C.c_int64 * 3)(*sizes)
    c_d, weight, offset = C.c_int(-1), (C.c_int * n)(), (C.c_int * n)()
    assert L.hmme_test_wp_parameters(stats, c_sizes, comps, n_refs, bd, start, C.byref(c_d), weight, offset) == 0
    d = c_d.value
    assert (d, list(zip(weight, offset))) == _model_parameters(model_stats, sizes, comps, bd, start)
    sums = (C.c_uint64 * (2 * n))()
    for i in range(n):
        org, ref = planes[i % comps], planes[comps + i]
        sums[2 * i] = int(np.abs((org << d) - (ref * weight[i] + offset[i] * (1 << (d + bd - 8)))).sum())
        sums[2 * i + 1] = int(np.abs(org - ref).sum())
    wps, infos = (api.Weight * n)(), (api.WpInfo * n)()
    assert L.hmme_test_wp_select(stats, c_sizes, comps, n_refs, bd, d, weight, offset, sums, wps, infos) == 0
    return [dict(infos[i].as_dict(), wp=(wps[i].w0, wps[i].offset, wps[i].shift, wps[i].round)) for i in range(n)]


def test_wp_estimate_models_match_reference(reference):
    """wp_estimate_model.estimate (4:0:0), wp_estimate_420_model.estimate and the library's own arithmetic (_library_estimate) on fades,
    identical, unrelated and constant pictures, 12-bit extremes, 1, 2 and 4 references and the 2 + 2 split of a B slice; each event the cases
    were built for occurs in the reference's own answer"""
    from hmme import api
    api.build()
    L = api.load()
    cases = rt.wp_cases()
    names = {c["name"] for c in cases}
    g = rt.load("ref_wp_estimate")
    for event in ("weight_lowers_denominator", "chroma_lowers_luma_denominator", "ratio_switches_off", "chroma_offset_clamps", "all_off_resets_table",
                  "nan_ratio_stays_present", "ratio_exactly_threshold"):
        assert len(g["event_" + event]) and set(str(n) for n in g["event_" + event]) <= names, event
    assert {(c["fmt"], c["n_l0"], c["n_l1"]) for c in cases} >= {(f, a, b) for f in (400, 420) for a, b in ((1, 0), (2, 0), (4, 0), (2, 2))}
    for case in cases:
        cur, refs = case["pics"][0], case["pics"][1:]
        want = reference.answer(np.concatenate([case["table"].ravel(), case["final"].ravel(), case["flags"].ravel()]),
                                lambda: np.concatenate([np.ravel(a) for a in oracle_py.ref_wp_estimate(cur, refs, case["n_l0"], case["n_l1"], case["bd"], case["start"])]))
        assert want.size == 2 * case["table"].size + 2
        assert case["start"] == (7 if case["n_l0"] > 3 else 6)      # HM's own choice (WeightPredAnalysis.cpp:174-180)
        comps = 3 if case["fmt"] == 420 else 1
        if comps == 1:
            est = wm.estimate(cur, refs, case["bd"], case["start"])
            model = lambda r, c: est[r]
        else:
            est = wm420.estimate(cur, refs, case["bd"], case["start"])
            model = lambda r, c: est[r][c]
        check_estimate(case, model)
        lib = _library_estimate(L, case["pics"], comps, case["bd"], case["start"])
        check_estimate(case, lambda r, c: lib[comps * r + c])
        for r in range(len(refs)):
            for c in range(comps):
                got, e = lib[comps * r + c], model(r, c)
                assert {k: got[k] for k in wm.INFO_FIELDS} == {k: e[k] for k in wm.INFO_FIELDS}, (case["name"], r, c, got, e)


def test_distortions_match_reference(reference, oracle_lib):
    """residual_model.sse (per-sample shift), residual_model.had_rule (8x8 blocks, 4x4 where a side is no multiple of 8) and the oracle's hmo_had /
    hmo_sad on every distinct PU rectangle of the 593 slots and on 4x4, at 8, 10 and 12 bit"""
    L = oracle_lib.oracle()
    p16 = C.POINTER(C.c_int16)
    sizes, fallback, dropped = set(), 0, 0
    for w, h, bd, content, org, pred, want in rt.dist_cases():
        want = tuple(int(v) for v in reference.answer(want, lambda: [oracle_py.ref_dist(org, pred, bd, k) for k in range(3)]))
        d = org.astype(np.int64) - pred.astype(np.int64)
        where = (w, h, bd, rt.DIST_CONTENTS[content])
        assert rm.sse(d, bd) == want[rt.SSE], where
        assert rm.had_rule(d, bd) == want[rt.HADS], where
        o, p = np.ascontiguousarray(org), np.ascontiguousarray(pred)
        assert int(L.hmo_had(o.ctypes.data_as(p16), w, p.ctypes.data_as(p16), w, w, h, bd)) == want[rt.HADS], where
        assert int(L.hmo_sad(o.ctypes.data_as(p16), w, p.ctypes.data_as(p16), w, w, h, 0, bd)) == want[rt.SAD], where
        sizes.add((w, h))
        fallback += (w % 8 != 0 or h % 8 != 0) and content == 2
        dropped += rm.sse_shifted_total(d, bd) > want[rt.SSE]
    assert sizes == {(int(w), int(h)) for _, _, w, h in oracle_lib.slot_table()} | {(4, 4)}
    assert (12, 16) in sizes and (16, 12) in sizes and fallback == 3 * 7 and dropped >= 25   # seven sizes take the 4x4 transform



def _refine_all_slots(oracle_lib, table, org_p, ref_p, pred, lam_or_q16, had, bd, live, bi):
    from hmme import synth
    m = synth.MARGIN
    out = np.zeros((593, 3), np.int64)
    for s in range(593):
        x, y, w, h = (int(v) for v in table[s])
        hx, hy, qx, qy, cost = oracle_lib.frac_refine(org_p, (m + x, m + y), ref_p, (m + x, m + y), w, h, (0, 0), pred, lam_or_q16, had, bd, use_ref=live, bi=bi)
        out[s] = (2 * hx + qx, 2 * hy + qy, cost)
    return out


def test_refinement_on_tap_sign_content_matches_reference(reference, oracle_lib):
    """the oracle's xPatternSearchFracDIF on references in the taps' sign pattern -- where the half-pel points' intermediates reach their bounds --
    against the complement and a random picture, 8, 10 and 12 bit, SAD and Hadamard, all 593 slots; and on the bi-prediction origin in
    {2 maxv, -maxv}, 8 and 10 bit"""
    from hmme import synth
    g = rt.load("ref_refine")
    table = oracle_lib.slot_table()
    pad = synth.pad_plane
    lam_of = lambda lq: 57.9 if lq else 0.0
    assert int(g["lambda_q16"]) == oracle_lib.oracle().hmo_lambda_q16(57.9)
    for i, bd in enumerate(g["bds"]):
        for r in range(4):
            for c in range(2):
                for had in range(2):
                    lq, px, py = (int(v) for v in g["plain_meta"][i, r, c, had])
                    org_p, ref_p = pad(g["cur"][i, r, c]), pad(g["ref"][i, r])
                    want = reference.answer(g["plain"][i, r, c, had], lambda: _refine_all_slots(oracle_lib, table, org_p, ref_p, (px, py), lam_of(lq), had, int(bd), True, False))
                    got = _refine_all_slots(oracle_lib, table, org_p, ref_p, (px, py), lq, had, int(bd), False, False)
                    assert np.array_equal(got, want), (int(bd), r, c, had, np.argwhere(got != want)[:3].tolist())
    for j, bd in enumerate(g["bi_bds"]):
        org_p = (2 * pad(g["bi_cur"][j]).astype(np.int32) - pad(g["bi_other"][j])).astype(np.int16)
        for r in range(4):
            for had in range(2):
                lq, px, py = (int(v) for v in g["bi_meta"][j, r, had])
                ref_p = pad(g["ref"][list(g["bds"]).index(bd), r])
                want = reference.answer(g["bi"][j, r, had], lambda: _refine_all_slots(oracle_lib, table, org_p, ref_p, (px, py), lam_of(lq), had, int(bd), True, True))
                got = _refine_all_slots(oracle_lib, table, org_p, ref_p, (px, py), lq, had, int(bd), False, True)
                assert np.array_equal(got, want), ("bi", int(bd), r, had, np.argwhere(got != want)[:3].tolist())
    # the cases are not degenerate: most slots leave the integer point, and both lambdas and both predictors occur
    assert (g["plain"][..., :2] != 0).any(axis=-1).mean() > 0.8
    assert {tuple(v) for v in g["plain_meta"].reshape(-1, 3)} == {(lq, 0, py) for lq in (0, int(g["lambda_q16"])) for py in (0, -2)}


def test_luma_tails_on_tap_sign_content_of_every_phase_match_reference(reference):
    """add_avg, add_weight_uni and add_weight_bi on the tap-sign intermediate of each of the 16 phases and its complement, four weights"""
    T, B = rt.load("ref_tails"), rt.load("ref_blocks")
    for i, bd in enumerate(BDS):
        for n in range(32):
            a, b = B["luma_sign_out"][i, n >> 1, n & 1, 1], B["luma_sign_out"][i, n >> 1, (n & 1) ^ 1, 1]
            want = reference.answer(T["sign_avg_luma"][i, n], lambda: oracle_py.ref_add_avg(a, b, bd, 0))
            assert same(pbm.add_avg(a, b, bd), want), (bd, n)
            for j, k in enumerate(T["sign_weights"]):
                w, o, d = (int(v) for v in T["triples"][k])
                want = reference.answer(T["sign_uni_luma"][i, n, j], lambda: oracle_py.ref_add_weight_uni(a, bd, 0, w, o, d))
                assert same(bwm.add_weight_uni(a, bd, rt.hmme_weight((w, o, d), bd)), want), (bd, n, (w, o, d))
                e = T["bi_weights"][k]
                want = reference.answer(T["sign_bi_luma"][i, n, j], lambda: oracle_py.ref_add_weight_bi(a, b, bd, 0, *[int(v) for v in e]))
                assert same(pbw.add_weight_bi(a, b, bd, *rt.bi_weights(e, bd)), want), (bd, n, tuple(e))
