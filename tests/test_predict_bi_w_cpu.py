"""The final prediction of a WP slice without a GPU: the exported names, hmme_predict_bi_weight_check against the rule restated in
tests/predict_bi_w_model.py, the model of TComWeightPrediction::addWeightBi against what the oracle already pins (addAvg, the bi = false
rounding), and what the feature is for: a faded picture is predicted better with its weights than without."""
import ctypes as C

import numpy as np
import pytest

import bipred_wp_model as bwm
import predict_bi_model as pbm
import predict_bi_w_model as pm
import range_content as rc
from frame_helpers import bind_hmo

NEW = ("hmme_predict_bi_weight_check", "hmme_predict_bi_w_device", "hmme_predict_bi_w_frame", "hmme_predict_refs_w_device", "hmme_predict_refs_w_frame")
DEPTHS = (8, 9, 10, 11, 12)


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


def test_exported_names_and_null_contexts():
    from hmme import api
    L = api.load()
    for name in NEW:
        assert name in api.SYMBOLS and hasattr(L, name), name
    assert L.hmme_abi_version() == 6
    fp = api.FrameParams(1, 0, 8, 0, -1)
    w = api.Weight(64, 0, 6, 32)
    a = C.c_void_p(256)   # never dereferenced
    pa = (C.c_void_p * 1)(256)
    assert L.hmme_predict_bi_w_device(None, pa, pa, 1, C.byref(fp), C.byref(w), C.byref(w), a, a, 64, pa, 64, None) == pm.ERR_ARG
    assert L.hmme_predict_bi_w_frame(None, a, a, C.byref(fp), C.byref(w), C.byref(w), a, a, 64, a, 64) == pm.ERR_ARG
    assert L.hmme_predict_refs_w_device(None, pa, 1, C.byref(fp), C.byref(w), a, a, 64, a, 64, None) == pm.ERR_ARG
    assert L.hmme_predict_refs_w_frame(None, pa, 1, C.byref(fp), C.byref(w), a, a, 64, a, 64) == pm.ERR_ARG


# ---- hmme_predict_bi_weight_check -----------------------------------------------------------------------------------------------------------
def test_argument_limits_and_their_accepted_neighbours():
    from hmme import api
    chk = api.predict_bi_weight_check
    idw = pm.ident(6)
    for bd, want in ((7, pm.ERR_ARG), (8, 0), (12, 0), (13, pm.ERR_ARG)):
        assert chk(bd, idw, idw) == want == pm.check(bd, idw, idw)
    assert chk(8, None, idw) == chk(8, idw, None) == chk(8, None, None) == pm.ERR_ARG == pm.check(8, None, idw)
    for shift, want in ((-1, pm.ERR_ARG), (0, 0), (15, 0), (16, pm.ERR_ARG)):
        w = (1, 0, shift, 0)
        assert chk(8, w, w) == want, shift
        if want == 0:
            assert pm.check(8, w, w) == 0
    # one slice, one luma denominator: every unequal pair, whichever list holds the larger
    for a in range(16):
        for b in range(16):
            got = chk(10, (3, 0, a, 0), (-2, 5, b, 0))
            assert got == (0 if a == b else pm.ERR_ARG) == pm.check(10, (3, 0, a, 0), (-2, 5, b, 0)), (a, b)
    # an argument error wins over an unsupported weight
    assert chk(8, (1 << 30, 0, 5, 0), (1, 0, 6, 0)) == pm.ERR_ARG


@pytest.mark.parametrize("bd", DEPTHS)
def test_last_accepted_member_of_every_family_in_either_list(bd):
    from hmme import api
    for name, member in rc.families(bd).items():
        other = pm.ident(member(0)[2])
        for order in (lambda w: (w, other), lambda w: (other, w)):
            check = lambda w: api.predict_bi_weight_check(bd, *order(w))
            k, wp = bwm.last_accepted(member, check)
            nxt = member(k + 1)
            assert check(wp) == 0 == pm.check(bd, *order(wp)), (name, wp)
            assert check(nxt) == pm.ERR_UNSUPPORTED == pm.check(bd, *order(nxt)), (name, nxt)
            # the walk ends at the int32 line: one of the two reaches crosses it between the two members
            reach = lambda w: max(pm.single_reach(bd, w), pm.pair_reach(bd, *order(w)))
            assert reach(wp) <= pm.INT32_MAX < reach(nxt), (name, wp, nxt)


@pytest.mark.parametrize("bd", DEPTHS)
def test_the_pair_line_binds_where_each_weight_alone_passes(bd):
    from hmme import api
    # two equal gains: each alone reaches half of what the pair does
    member = lambda k: (1 + k, 0, 0, 0)
    k, wp = bwm.last_accepted(member, lambda w: api.predict_bi_weight_check(bd, w, w))
    nxt = member(k + 1)
    assert pm.single_reach(bd, nxt) <= pm.INT32_MAX < pm.pair_reach(bd, nxt, nxt) and pm.pair_reach(bd, wp, wp) <= pm.INT32_MAX
    assert api.predict_bi_weight_check(bd, nxt, nxt) == pm.ERR_UNSUPPORTED and api.bipred_weight_check(bd, pm.ident(0), nxt) == 0
    # offsets of opposite sign cancel: the sum is what counts
    big = 1 << 24
    assert api.predict_bi_weight_check(bd, (64, big, 6, 32), (64, -big, 6, 32)) == 0 == pm.check(bd, (64, big, 6, 32), (64, -big, 6, 32))
    assert api.predict_bi_weight_check(bd, (64, big, 6, 32), (64, big, 6, 32)) == pm.ERR_UNSUPPORTED == pm.check(bd, (64, big, 6, 32), (64, big, 6, 32))


@pytest.mark.parametrize("bd", DEPTHS)
def test_all_of_hms_range_is_served(bd):
    """|w| <= 255, shift <= 7, |offset| <= 128 << (bd - 8) per list: every corner, and the reach of the worst one"""
    from hmme import api
    omax = 128 << (bd - 8)
    worst = 0
    for shift in (0, 7):
        for w0 in (-255, 0, 255):
            for w1 in (-255, 0, 255):
                for o0 in (-omax, 0, omax):
                    for o1 in (-omax, 0, omax):
                        a, b = (w0, o0, shift, 0), (w1, o1, shift, 0)
                        assert api.predict_bi_weight_check(bd, a, b) == 0 == pm.check(bd, a, b), (a, b)
                        worst = max(worst, pm.pair_reach(bd, a, b))
    assert worst < 1 << 25                                                       # what include/hmme.h states


# ---- the model against what is pinned already ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", DEPTHS)
def test_two_identities_are_add_avg(bd):
    rng = np.random.default_rng(60 + bd)
    p0, p1 = (rng.integers(-32768, 32768, size=(64, 64)) for _ in range(2))      # every Pel, not only what a picture can produce
    for d in (0, 1, 6, 7, 15):
        assert np.array_equal(pm.add_weight_bi(p0, p1, bd, pm.ident(d), pm.ident(d)), pbm.add_avg(p0, p1, bd)), d


@pytest.mark.parametrize("bd", DEPTHS)
def test_twice_list_0_and_nothing_of_list_1_is_the_uni_directional_prediction(bd):
    """(2^(d+1) * (P0 + 8192) + 2^(d+head)) >> (d + 1 + head) = (P0 + 8192 + 2^(head-1)) >> head: the rounding of bi = false"""
    from hmme import synth
    m, n = synth.MARGIN, 16
    ref, other = (synth.make_pair(96, 80, seed=70 + bd + 100 * k, bit_depth=bd, max_mv=2)[1] for k in range(2))
    phases = set()
    for qy in range(-5, -1):
        for qx in range(9, 13):
            for d in (0, 6):
                got = pm.pred_bi_w(ref, other, m + 24, m + 16, n, n, (qx, qy), (-qx, qy + 7), bd, (2 << d, 0, d, 0), (0, 0, d, 0))
                assert np.array_equal(got, rc.pred_qpel(ref, m + 24, m + 16, n, n, qx, qy, bd)), (bd, qx, qy, d)
            phases.add((qx & 3, qy & 3))
    assert len(phases) == 16


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_equal_unit_weights_and_an_even_offset_shift_add_avg(bd):
    rng = np.random.default_rng(80 + bd)
    p0, p1 = (rng.integers(-8192, 8192 + (1 << 13), size=(32, 32)) for _ in range(2))
    shift = max(2, 14 - bd) + 1
    raw = (p0 + p1 + (1 << (shift - 1)) + 2 * 8192) >> shift                     # addAvg before its clip
    maxv = (1 << bd) - 1
    for d in (0, 6):
        for k in (-maxv, -7, 1, 40, maxv):
            got = pm.add_weight_bi(p0, p1, bd, (1 << d, 2 * k, d, 0), (1 << d, 0, d, 0))
            assert np.array_equal(got, np.clip(raw + k, 0, maxv)), (d, k)
            assert np.array_equal(got, pm.add_weight_bi(p0, p1, bd, (1 << d, k - 3, d, 0), (1 << d, k + 3, d, 0)))   # only the sum counts


@pytest.mark.parametrize("bd", (8, 10))
def test_both_clip_ends_are_reached_on_binary_pictures(bd):
    from hmme import synth
    w, h, m = 192, 72, synth.MARGIN
    maxv = (1 << bd) - 1
    _, ref0, ref1 = rc.extreme_triple(w, h, bd, seed=90 + bd)
    lo = hi = inside = 0
    for k, (mv0, mv1) in enumerate((((2, 2), (2, 2)), ((1, 3), (3, 1)), ((-6, 5), (6, -5)), ((2, 0), (0, 2)))):
        for wp0, wp1 in (((150, 3, 6, 32), (-40, -2, 6, 32)), ((40, 0, 6, 32), (40, 0, 6, 32))):
            x, y = m + 8 + 16 * k, m + 8
            raw = pm.pred_bi_w(ref0, ref1, x, y, 32, 32, mv0, mv1, bd, wp0, wp1, clip=False)
            got = pm.pred_bi_w(ref0, ref1, x, y, 32, 32, mv0, mv1, bd, wp0, wp1)
            assert np.array_equal(got, np.clip(raw, 0, maxv))
            lo, hi, inside = lo + int((raw < 0).sum()), hi + int((raw > maxv).sum()), inside + int(((raw > 0) & (raw < maxv)).sum())
    assert lo > 0 and hi > 0 and inside > 0


# ---- what it is for ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", (8, 10))
def test_a_fade_is_predicted_better_with_its_weights(hmo, bd):
    w, h = 136, 72
    cur, refs = pm.fade_pictures(w, h, bd, seed=900 + bd)
    field, dirs = pm.fade_truth(w, h)
    assert {1, 2, 3} == set(dirs.reshape(-1).tolist())
    weighted = pm.pred_picture(hmo, refs, w, h, bd, field, dirs, pm.fade_wps(bd), np.zeros((h, w), np.int64))
    plain = pbm.pred_picture(hmo, refs, w, h, bd, field, dirs, np.zeros((h, w), np.int64))
    sad = lambda p, cols=slice(None): int(np.abs(p[:, cols] - cur[:, cols]).sum())
    bi = slice(*pm.FADE_BANDS)
    assert sad(weighted) < sad(plain) and sad(weighted, bi) < sad(plain, bi), (sad(weighted), sad(plain))
    # the weights undo the fade up to its two roundings: at most one level per sample (<< (bd - 8): nothing, the offset is exact)
    assert np.abs(weighted - cur).max() <= 1
