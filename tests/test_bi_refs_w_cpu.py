"""Multi-reference B pictures with explicit weights and 4:2:0 chroma (include/hmme.h, "multi-reference B pictures: explicit weights and
4:2:0 chroma"), the part that needs no GPU: the new names declared, exported and bound; every refusal of hmme_predict_bi_refs_weight_check and
hmme_bipred_refs_weight_check with its accepted neighbour and in the documented order; with one reference per list both are the
single-reference checks; the common-bias derivation by brute force; the two new models against the ones they are composed of; and the
end-to-end content's condition on the models alone."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import b_refs_wp_420_content as content
import bipred_wp_model as bwm
import predict_bi_refs_model as pbrm
import predict_bi_refs_w_model as pbrw
import predict_bi_w_model as pbw
import predict_chroma_bi_refs_model as pcbr
import predict_chroma_model as cm
from conftest import ROOT
from frame_helpers import bind_hmo, dims

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
NAMES = ["hmme_predict_bi_refs_weight_check", "hmme_predict_bi_refs_w_device", "hmme_predict_bi_refs_w_frame", "hmme_predict_chroma_bi_refs_device",
         "hmme_predict_chroma_bi_refs_frame", "hmme_bipred_refs_weight_check", "hmme_search_frame_bi_refs_w_device", "hmme_refine_frame_bi_refs_w_device",
         "hmme_search_frame_bi_refs_w", "hmme_refine_frame_bi_refs_w"]
METHODS = ["predict_bi_refs_w_device", "predict_bi_refs_w_frame", "predict_chroma_bi_refs_device", "predict_chroma_bi_refs_frame", "search_frame_bi_refs_w",
           "search_frame_bi_refs_w_device", "refine_frame_bi_refs_w", "refine_frame_bi_refs_w_device"]
GOOD = (70, -9, 6, 32)
ALONE = (60000, 0, 6, 32)      # |w0| * 40 960 beyond int32: the single-weight line
HALF = (26300, 0, 6, 32)       # passes alone and beside GOOD, not beside another of its size: the pair line


@pytest.fixture(scope="module")
def api():
    from hmme import api
    api.build()
    return api


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


def test_the_new_names_are_declared_exported_and_bound(api):
    L = api.load()
    header = open(os.path.join(ROOT, "include", "hmme.h")).read()
    declared = set(re.findall(r"\b(hmme_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/hmme.h"
        assert hasattr(L, name), f"libhmme.so does not export {name}"
        assert name in api.SYMBOLS
        assert getattr(L, name).argtypes is not None, f"api.py binds no argument types for {name}"
    for method in METHODS:
        assert callable(getattr(api.Engine, method)), method
    assert callable(api.predict_bi_refs_weight_check) and callable(api.bipred_refs_weight_check)
    assert re.search(r"#define HMME_ABI_VERSION 6\b", header) and L.hmme_abi_version() == 6 and api.ABI_VERSION == 6   # new functions only
    section = header.split("multi-reference B pictures: explicit weights and 4:2:0 chroma ---")[1].split("int hmme_bipred_refs_weight_check")[0]
    assert "THIS TEXT PLUS THE CITATIONS IS THE RULE" in section and "Out of scope" in section and "hmme_select_dirs_refs_device) needs no weighted form" in section


def test_a_null_context_is_refused_by_every_new_entry_point(api):
    L = api.load()
    fp, w = api.FrameParams(1, 0, 8, 0, -1), api.Weight(64, 0, 6, 32)
    a, pa = C.c_void_p(256), (C.c_void_p * 2)(256, 256)                          # never dereferenced
    assert L.hmme_predict_bi_refs_w_device(None, pa, 1, pa, 1, C.byref(fp), C.byref(w), C.byref(w), a, a, a, 64, a, 64, None) == ERR_ARG
    assert L.hmme_predict_bi_refs_w_frame(None, pa, 1, pa, 1, C.byref(fp), C.byref(w), C.byref(w), a, a, a, 64, a, 64) == ERR_ARG
    assert L.hmme_predict_chroma_bi_refs_device(None, pa, 1, pa, 1, 64, 64, C.byref(fp), None, None, a, a, a, 64, a, a, 32, None) == ERR_ARG
    assert L.hmme_predict_chroma_bi_refs_frame(None, pa, 1, pa, 1, 64, 64, C.byref(fp), None, None, a, a, a, 64, pa, 32) == ERR_ARG
    assert L.hmme_search_frame_bi_refs_w_device(None, a, pa, 1, pa, 1, C.byref(fp), C.byref(w), C.byref(w), a, a, 64, None, None, a, a, None) == ERR_ARG
    assert L.hmme_refine_frame_bi_refs_w_device(None, a, pa, 1, pa, 1, C.byref(fp), C.byref(w), C.byref(w), a, a, 64, None, None, a, 1, a, a, None) == ERR_ARG
    assert L.hmme_search_frame_bi_refs_w(None, a, pa, 1, pa, 1, C.byref(fp), C.byref(w), C.byref(w), a, a, 64, None, None, a, a) == ERR_ARG
    assert L.hmme_refine_frame_bi_refs_w(None, a, pa, 1, pa, 1, C.byref(fp), C.byref(w), C.byref(w), a, a, 64, None, None, a, 1, a, a) == ERR_ARG


# ---- hmme_predict_bi_refs_weight_check ------------------------------------------------------------------------------------------------------------
def test_prediction_check_every_refusal_its_neighbour_and_the_order(api):
    chk = api.predict_bi_refs_weight_check

    def both(bd, w0, w1, want, **kw):
        assert chk(bd, w0, w1, **kw) == want == pbrw.check(bd, w0, w1, *(kw.get(k) for k in ("n0", "n1"))), (bd, w0, w1, kw)
    # 1. arguments
    for bd, want in ((7, ERR_ARG), (8, OK), (12, OK), (13, ERR_ARG)):
        both(bd, [GOOD, GOOD], [GOOD], want)
    both(8, None, [GOOD], ERR_ARG); both(8, [GOOD], None, ERR_ARG)
    for n, want in ((0, ERR_ARG), (1, OK), (16, OK), (17, ERR_ARG)):
        both(8, [GOOD] * 17, [GOOD], want, n0=n, n1=1)
        both(8, [GOOD], [GOOD] * 17, want, n0=1, n1=n)
    for shift, want in ((-1, ERR_ARG), (0, OK), (15, OK), (16, ERR_ARG)):
        near, w = (1, 0, max(0, min(15, shift)), 0), (1, 0, shift, 0)
        for l0, l1 in (([near, w], [near]), ([near], [w, near]), ([near], [near, w])):   # in list 0's last weight, list 1's first, list 1's last
            both(8, l0, l1, want)
    # 2. unequal shifts: inside list 0, inside list 1, and only between the lists
    both(10, [GOOD, (35, 0, 5, 16)], [GOOD], ERR_ARG)
    both(10, [GOOD], [GOOD, (35, 0, 5, 16)], ERR_ARG)
    both(10, [GOOD, GOOD], [(35, 0, 5, 16), (35, 0, 5, 16)], ERR_ARG)
    both(10, [(35, 0, 5, 16)] * 2, [(35, 0, 5, 16)] * 2, OK)
    # 3. each weight alone, wherever it stands
    for l0, l1 in (([ALONE, GOOD], [GOOD]), ([GOOD, ALONE], [GOOD]), ([GOOD, GOOD], [GOOD, ALONE])):
        both(8, l0, l1, ERR_UNSUPPORTED)
    # 4. a pair that fails where each weight alone passes -- only the pair (1, 1) of 2 x 2
    assert pbw.single_reach(8, HALF) <= pbw.INT32_MAX < pbw.pair_reach(8, HALF, HALF) and pbw.pair_reach(8, HALF, GOOD) <= pbw.INT32_MAX
    both(8, [GOOD, HALF], [GOOD, HALF], ERR_UNSUPPORTED)
    both(8, [GOOD, HALF], [GOOD, GOOD], OK); both(8, [GOOD, GOOD], [GOOD, HALF], OK)
    # the order: an argument error of list 1 beats an UNSUPPORTED of list 0; a shift mismatch beats a range; a single line beats a pair line
    both(8, [ALONE], [(1, 0, 16, 0)], ERR_ARG)
    both(8, [ALONE], [GOOD], ERR_UNSUPPORTED, n0=1, n1=1); both(8, [ALONE], [GOOD], ERR_ARG, n0=1, n1=0)
    both(8, [ALONE, GOOD], [(35, 0, 5, 16)], ERR_ARG)
    both(13, [ALONE], [GOOD], ERR_ARG)


def test_prediction_check_with_one_reference_per_list_is_the_single_reference_check(api):
    grid = [(w0, off, d, 0) for w0 in (-70000, -255, 64, 26300, 60000) for off in (-(1 << 24), 0, 1 << 24) for d in (0, 6, 15, 16)]
    seen = set()
    for bd in (8, 10, 12):
        for a, b in itertools.product(grid, grid):
            want = api.predict_bi_weight_check(bd, a, b)
            assert api.predict_bi_refs_weight_check(bd, [a], [b]) == want == pbrw.check(bd, [a], [b]), (bd, a, b)
            seen.add(want)
    assert seen == {OK, ERR_ARG, ERR_UNSUPPORTED}


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_all_of_hms_range_is_served_whatever_the_indices(api, bd):
    omax = 128 << (bd - 8)
    for shift in (0, 7):
        corners = [(w0, o, shift, 0) for w0 in (-255, 255) for o in (-omax, omax)]
        assert api.predict_bi_refs_weight_check(bd, corners * 4, corners * 4) == OK


# ---- hmme_bipred_refs_weight_check ------------------------------------------------------------------------------------------------------------------
def test_bipred_check_every_refusal_its_neighbour_and_the_order(api):
    chk = api.bipred_refs_weight_check
    far = (32767, 0, 0, 0)                                                       # searched: a weighted sample beyond a Pel
    rough = (70000, 0, 15, 1 << 14)                                              # searched: served by the search, not by the refinement (fp32)
    for refine in (False, True):
        for bd, want in ((7, ERR_ARG), (8, OK), (10, OK), (13, ERR_ARG)):
            assert chk(bd, [GOOD, GOOD], [GOOD], refine) == want
        assert chk(8, None, [GOOD], refine) == chk(8, [GOOD], None, refine) == ERR_ARG
        for n, want in ((0, ERR_ARG), (1, OK), (16, OK), (17, ERR_ARG)):
            assert chk(8, [GOOD] * 17, [GOOD], refine, n_refs=n) == want and chk(8, [GOOD], [GOOD] * 17, refine, n_others=n) == want
        for shift, want in ((-1, ERR_ARG), (0, OK), (15, OK), (16, ERR_ARG)):
            w = (1, 0, shift, (1 << (shift - 1)) if 0 < shift < 16 else 0)
            assert chk(8, [GOOD, w], [GOOD], refine) == want and chk(8, [GOOD], [GOOD, w], refine) == want
        # shifts need not be equal here: every weight is used alone
        assert chk(8, [GOOD, (35, 0, 5, 16)], [(18, 0, 4, 8)], refine) == OK
        # 2. the searched lines per reference, 3. the other line per other reference
        assert chk(8, [GOOD, far], [GOOD], refine) == ERR_UNSUPPORTED and chk(8, [far, GOOD], [GOOD], refine) == ERR_UNSUPPORTED
        assert chk(8, [GOOD], [GOOD, ALONE], refine) == ERR_UNSUPPORTED and chk(8, [GOOD], [GOOD, HALF], refine) == OK
        assert chk(8, [ALONE], [GOOD], refine) == ERR_UNSUPPORTED                # as a searched weight it is beyond a Pel
        # the order: an argument error of the other list beats an UNSUPPORTED of the searched one
        assert chk(8, [far], [(1, 0, 16, 0)], refine) == ERR_ARG and chk(8, [far], [GOOD], refine, n_others=0) == ERR_ARG
        assert chk(12, [GOOD], [GOOD], refine) == (ERR_UNSUPPORTED if refine else OK)   # the 12-bit refinement stays refused
        assert chk(12, [(64, 0, 6, 32)], [(64, 0, 6, 32)], refine) == (ERR_UNSUPPORTED if refine else OK)
    assert chk(8, [GOOD, rough], [GOOD], False) == OK and chk(8, [GOOD, rough], [GOOD], True) == ERR_UNSUPPORTED


def test_bipred_check_with_one_reference_per_list_is_the_single_reference_check(api):
    grid = [(w0, off, d, rnd) for w0 in (-300, -20, 1, 40, 64, 128, 32767, 70000) for off in (-40000, -300, -12, 0, 200, 33000) for d, rnd in ((0, 0), (5, 16), (6, 32), (6, 0), (15, 1 << 14))]
    others = [(64, 0, 6, 32), (-20, 200, 5, 16), (60000, 0, 6, 32), (1, 0, 16, 0)]
    seen = set()
    for bd in (8, 10, 12):
        for refine in (False, True):
            for a, b in itertools.product(grid, others):
                want = api.bipred_weight_check(bd, a, b, refine)
                assert api.bipred_refs_weight_check(bd, [a], [b], refine) == want, (bd, refine, a, b)
                seen.add(want)
    assert seen == {OK, ERR_ARG, ERR_UNSUPPORTED}


@pytest.mark.parametrize("bd", (8, 10, 12))
def test_a_common_bias_never_breaks_the_sixteen_bit_span(api, bd):
    """include/hmme.h derives it: once every weight passes its own lines, max(whi_r, 2 * maxv) + max_q(bias_q) <= 65 535 for every r.  Brute
    force over the extremes of HM's weight range -- weight = (1 << d) + delta, delta in [-128, 127], d in 0..7, |offset| <= 128 << (bd - 8) --
    and over the two ends of a Pel"""
    maxv = (1 << bd) - 1
    omax = 128 << (bd - 8)
    ws = [((1 << d) + delta, o, d, (1 << (d - 1)) if d else 0) for d in (0, 1, 6, 7) for delta in (-128, -1, 0, 127) for o in (-omax, 0, omax - 1)]
    # the derivation itself, at the ends of a Pel: whatever passes the Pel line has whi <= 32 767 and -wlo <= 32 768
    assert max(32767, 2 * maxv) + max(maxv, 32768) <= 65535
    served = [w for w in ws if api.bipred_weight_check(bd, w, (64, 0, 6, 32), False) == OK]
    assert len(served) >= 12 and any(bwm.searched_terms(bd, w)[2] > maxv for w in served) and any(bwm.searched_terms(bd, w)[2] == maxv for w in served)
    terms = {w: bwm.searched_terms(bd, w) for w in served}                       # (wlo, whi, bias, span, p0, p1)
    worst = 0
    for a, b in itertools.product(served, served):
        common = max(terms[a][2], terms[b][2])
        assert common == max(maxv, -terms[a][0], -terms[b][0])
        worst = max(worst, max(terms[a][1], 2 * maxv) + common)
        assert terms[a][0] + common >= 0 and -maxv + common >= 0                 # weighted plane and origin stay unsigned
        assert api.bipred_refs_weight_check(bd, [a, b], [(64, 0, 6, 32)], False) == OK
    assert 2 * maxv + maxv < worst <= 65535


# ---- the models against the ones they are composed of ----------------------------------------------------------------------------------------------------
def fields(w, h, seed, n0, n1):
    rng = np.random.default_rng(seed)
    n = dims(w, h)[0] * dims(w, h)[1]
    field = rng.integers(-40, 41, size=(2, n, 64, 2)).astype(np.int16)
    dirs = rng.choice(np.array([1, 2, 3, 3, 0xFF, 0], np.uint8), size=(n, 64))
    refs = np.stack([rng.integers(0, n0 + 1, size=(n, 64)), rng.integers(0, n1 + 1, size=(n, 64))]).astype(np.uint8)   # n: beyond the list
    return field, dirs, refs


@pytest.mark.parametrize("bd", (8, 10))
def test_the_luma_model_against_its_single_reference_and_unweighted_siblings(hmo, bd):
    from hmme import synth
    w, h = 100, 70
    pics = [synth.make_pair(w, h, seed=500 + bd + 7 * k, bit_depth=bd, max_mv=2)[1] for k in range(4)]
    wps0, wps1 = [(70, -9 << (bd - 8), 6, 32), (55, 14 << (bd - 8), 6, 32)], [(40, -5 << (bd - 8), 6, 32), (90, 11 << (bd - 8), 6, 32)]
    field, dirs, refs = fields(w, h, 510 + bd, 2, 2)
    blank = lambda: np.full((h, w), -1, np.int64)
    # 1 + 1 references: predict_bi_w_model (an index of 1 is beyond the list there: not written)
    one = pbrw.pred_picture(hmo, pics[:1], pics[2:3], wps0[:1], wps1[:1], w, h, bd, field, dirs, np.zeros_like(refs), blank())
    assert np.array_equal(one, pbw.pred_picture(hmo, (pics[0], pics[2]), w, h, bd, field, dirs, (wps0[0], wps1[0]), blank())) and (one >= 0).any()
    # all identities: predict_bi_refs_model
    ids = [(64, 0, 6, 7), (64, 0, 6, 32)]
    same = pbrw.pred_picture(hmo, pics[:2], pics[2:], ids, ids, w, h, bd, field, dirs, refs, blank())
    assert np.array_equal(same, pbrm.pred_picture(hmo, pics[:2], pics[2:], w, h, bd, field, dirs, refs, blank()))
    got = pbrw.pred_picture(hmo, pics[:2], pics[2:], wps0, wps1, w, h, bd, field, dirs, refs, blank())
    assert np.array_equal(got < 0, same < 0) and (got < 0).any() and not np.array_equal(got, same)   # the same blocks are live


@pytest.mark.parametrize("bd", (8, 10))
def test_the_chroma_model_against_its_single_reference_sibling(hmo, bd):
    from hmme import synth
    w, h = 100, 70
    tex = [[synth.make_pair(w // 2, h // 2, seed=600 + bd + 7 * k + 3 * c, bit_depth=bd, max_mv=2)[1] for c in range(2)] for k in range(4)]
    comps = [[[tex[0][c], tex[1][c]], [tex[2][c], tex[3][c]]] for c in range(2)]
    wps = [[[(70, 9, 6, 32), (55, -14, 6, 32)], [(45, -6, 6, 32), (80, 3, 6, 32)]], [[(40, -5, 5, 16), (29, 11, 5, 16)], [(36, 7, 5, 16), (25, -12, 5, 16)]]]
    field, dirs, refs = fields(w, h, 610 + bd, 2, 2)
    blank = lambda: tuple(np.full((h // 2, w // 2), -1, np.int64) for _ in range(2))
    for weighted in (False, True):
        one = pcbr.bi_refs_picture(hmo, [[[comps[c][0][0]], [comps[c][1][0]]] for c in range(2)], w, h, bd, field, dirs, np.zeros_like(refs), blank(),
                                   [[[wps[c][0][0]], [wps[c][1][0]]] for c in range(2)] if weighted else None)
        sib = cm.bi_picture(hmo, [(comps[c][0][0], comps[c][1][0]) for c in range(2)], w, h, bd, field, dirs, blank(),
                            [(wps[c][0][0], wps[c][1][0]) for c in range(2)] if weighted else None)
        assert all(np.array_equal(one[c], sib[c]) and (one[c] >= 0).any() for c in range(2))
    ids = [[[(64, 0, 6, 0)] * 2] * 2, [[(8, 0, 3, 1)] * 2] * 2]
    plain = pcbr.bi_refs_picture(hmo, comps, w, h, bd, field, dirs, refs, blank())
    same = pcbr.bi_refs_picture(hmo, comps, w, h, bd, field, dirs, refs, blank(), ids)
    got = pcbr.bi_refs_picture(hmo, comps, w, h, bd, field, dirs, refs, blank(), wps)
    for c in range(2):
        assert np.array_equal(plain[c], same[c]) and np.array_equal(got[c] < 0, plain[c] < 0) and (got[c] < 0).any() and not np.array_equal(got[c], plain[c])


# ---- what it is for ---------------------------------------------------------------------------------------------------------------------------
def test_the_end_to_end_content_is_predicted_better_with_its_weights(api, hmo):
    """tests/b_refs_wp_420_content.py at its planted motion, on the models alone: the weights are served by both checks, and the weighted luma
    prediction is closer to the current picture (SSE) than the unweighted one on the same fields -- what tests/test_gpu_b_refs_wp_420.py asserts
    again on the device's own fields"""
    W, H = content.W, content.H
    cur, luma, _, _ = content.content()
    assert api.predict_bi_refs_weight_check(8, content.WPS[0], content.WPS[1]) == OK
    for l in range(2):
        assert api.bipred_refs_weight_check(8, content.WPS[l], content.WPS[1 - l], True) == OK
    for c in range(2):
        assert api.predict_bi_refs_weight_check(8, content.CHROMA_WPS[c][0], content.CHROMA_WPS[c][1]) == OK
    field, dirs, refs = content.planted_fields()
    assert {1, 2, 3} <= set(dirs.reshape(-1).tolist()) and {0, 1} <= set(refs[0].reshape(-1).tolist()) and {0, 1} <= set(refs[1].reshape(-1).tolist())
    weighted = pbrw.pred_picture(hmo, luma[0], luma[1], content.WPS[0], content.WPS[1], W, H, 8, field, dirs, refs, np.zeros((H, W), np.int64))
    plain = pbrm.pred_picture(hmo, luma[0], luma[1], W, H, 8, field, dirs, refs, np.zeros((H, W), np.int64))
    assert content.sse(weighted, cur) < content.sse(plain, cur) // 4, (content.sse(weighted, cur), content.sse(plain, cur))
