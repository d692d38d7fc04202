"""Bi-prediction with explicit weighted prediction, the parts that need no GPU: the new names declared, exported and bound; the numpy model
of the other list's prediction (tests/bipred_wp_model.py) against the CPU oracle and against cases worked by hand; and
hmme_bipred_weight_check -- a pure host function -- against the rule of include/hmme.h restated in the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bipred_wp_model as model
import range_content as rc
from frame_helpers import bind_hmo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
IDENT = model.IDENT
NAMES = ("hmme_bipred_weight_check", "hmme_predict_pairs_w_device", "hmme_predict_frame_w", "hmme_search_pairs_bi_w_device",
         "hmme_refine_pairs_bi_w_device", "hmme_search_frame_bi_w", "hmme_refine_frame_bi_w")
BDS = (8, 9, 10, 11, 12)


@pytest.fixture(scope="module")
def api():
    from hmme import api
    api.build()
    return api


def test_the_new_names_are_declared_exported_and_bound(api):
    L = api.load()
    header = open(os.path.join(ROOT, "include", "hmme.h")).read()
    declared = set(re.findall(r"\b(hmme_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/hmme.h"
        assert hasattr(L, name), f"libhmme.so does not export {name}"
        assert name in api.SYMBOLS
        assert getattr(L, name).argtypes is not None, f"api.py binds no argument types for {name}"
    for method in ("predict_pairs_w_device", "predict_frame_w", "search_pairs_bi_w_device", "refine_pairs_bi_w_device", "search_frame_bi_w",
                   "refine_frame_bi_w"):
        assert callable(getattr(api.Engine, method))
    assert callable(api.bipred_weight_check)
    assert re.search(r"#define HMME_ABI_VERSION 6\b", header) and L.hmme_abi_version() == 6   # new functions only: the version stays
    assert "not offered" not in header


def test_a_null_context_is_refused_by_every_new_entry_point(api):
    L = api.load()
    fp = api.FrameParams(4, 1, 8, 0, -1)
    one = (C.c_void_p * 1)(None)
    w = api.Weight(*IDENT)
    assert L.hmme_predict_pairs_w_device(None, one, 1, C.byref(fp), C.byref(w), None, 1, one, 0, None) == ERR_ARG
    assert L.hmme_predict_frame_w(None, None, C.byref(fp), C.byref(w), None, 1, None, 0) == ERR_ARG
    assert L.hmme_search_pairs_bi_w_device(None, one, one, one, 1, C.byref(fp), C.byref(w), C.byref(w), None, 1, None, None, None, None, None) == ERR_ARG
    assert L.hmme_refine_pairs_bi_w_device(None, one, one, one, 1, C.byref(fp), C.byref(w), C.byref(w), None, 1, None, None, None, 1, None, None, None) == ERR_ARG
    assert L.hmme_search_frame_bi_w(None, None, None, None, C.byref(fp), C.byref(w), C.byref(w), None, 1, None, None, None, None) == ERR_ARG
    assert L.hmme_refine_frame_bi_w(None, None, None, None, C.byref(fp), C.byref(w), C.byref(w), None, 1, None, None, None, 1, None, None) == ERR_ARG


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_the_model_at_identity_weights_is_the_oracle_prediction_at_every_phase(oracle_lib, bd):
    """w0 == 1 << shift, offset 0: addWeightUni on the intermediate IS the bi = false prediction (nested floors) -- what lets the engine run
    its unweighted kernel for such a weight.  On the binary pattern: the filter overshoots and the clip runs in both directions"""
    from hmme import synth
    hmo = bind_hmo(oracle_lib)
    m, maxv = synth.MARGIN, (1 << bd) - 1
    _, ref, _ = rc.extreme_pair(136, 72, bd, IDENT, seed=90 + bd)
    p16 = C.POINTER(C.c_int16)
    out = np.zeros((64, 64), np.int16)
    head = max(14 - bd, 2)
    for ph in range(16):
        qx, qy = 4 * (ph - 7) + (ph & 3), 4 * (5 - ph) + (ph >> 2)
        src = C.cast(ref.ctypes.data + 2 * ((m + 3) * ref.shape[1] + m + 5), p16)
        hmo.hmo_pred_block_qpel(src, ref.shape[1], 64, 64, qx, qy, bd, out.ctypes.data_as(p16), 64)
        for ident in (IDENT, (1, 0, 0, 0), (1 << 15, 0, 15, 12345)):   # (the last: wp.round is whatever it is)
            assert np.array_equal(model.pred_w(ref, m + 5, m + 3, 64, 64, qx, qy, bd, ident), out), (bd, ph, ident)
        # the intermediate is the one range_content.pred_qpel rounds: ((P + 8192 + 2^(head-1)) >> head) is its vertical pass
        p = model.inter_qpel(ref, m + 5, m + 3, 64, 64, qx, qy, bd)
        raw = rc.pred_qpel(ref, m + 5, m + 3, 64, 64, qx, qy, bd, clip=False)
        assert np.array_equal((p + 8192 + (1 << (head - 1))) >> head, raw), (bd, ph)
        assert p.min() >= -32768 and p.max() <= 32767 and -24576 <= p.min() + 8192 and p.max() + 8192 <= 40959   # P is a Pel
        if ph:
            assert raw.min() < 0 and raw.max() > maxv, (bd, ph)
        else:
            assert np.array_equal(p, (ref[m + 3 + (qy >> 2):m + 67 + (qy >> 2), m + 5 + (qx >> 2):m + 69 + (qx >> 2)].astype(np.int64) << (14 - bd)) - 8192)


def test_a_flat_picture_by_hand():
    """100 everywhere: P = (100 << 6) - 8192 at every phase (the taps sum to 64); w0 = 48, shift = 5, offset = -10:
    shift' = 5 + 6 = 11, (48 * 6400 + 1024) >> 11 = 150, 150 - 10 = 140.  At 10 bits: 400, offset -40 -> 600 - 40 = 560"""
    for bd, flat, offset, want in ((8, 100, -10, 140), (10, 400, -40, 560)):
        plane = np.full((96, 96), flat, np.int16)
        for ph in range(16):
            got = model.pred_w(plane, 16, 16, 8, 8, 4 * 2 + (ph & 3), -4 + (ph >> 2), bd, (48, offset, 5, 16))
            assert np.all(got == want), (bd, ph, got[0, 0])


def test_the_model_ignores_wp_round():
    rng = np.random.default_rng(3)
    plane = rng.integers(0, 256, size=(96, 96)).astype(np.int16)
    a = model.pred_w(plane, 16, 16, 64, 64, 5, 7, 8, (40, -12, 5, 16))
    for rnd in (0, 1, 31, -7, 1 << 20):
        assert np.array_equal(model.pred_w(plane, 16, 16, 64, 64, 5, 7, 8, (40, -12, 5, rnd)), a)
    # ... while shift and w0 do matter
    assert not np.array_equal(model.pred_w(plane, 16, 16, 64, 64, 5, 7, 8, (40, -12, 6, 16)), a)


# ---- hmme_bipred_weight_check ------------------------------------------------------------------------------------------------------------
def test_the_identity_pair_is_hmme_bipred_check(api):
    for bd in BDS:
        for refine in (0, 1):
            want = api.bipred_check(bd, refine)
            for a in (IDENT, (1, 0, 0, 0)):
                for b in (IDENT, (1, 0, 0, 0), (64, 0, 6, 0)):
                    assert api.bipred_weight_check(bd, a, b, refine) == want, (bd, refine, a, b)
    assert api.bipred_weight_check(12, IDENT, IDENT, 1) == ERR_UNSUPPORTED and api.bipred_weight_check(12, IDENT, IDENT, 0) == OK
    for bd in (7, 13):
        assert api.bipred_weight_check(bd, IDENT, IDENT, 0) == api.bipred_check(bd, 0) == ERR_ARG


def test_null_weights_and_shift_16_are_argument_errors(api):
    for bd in BDS:
        for refine in (0, 1):
            assert api.bipred_weight_check(bd, None, IDENT, refine) == ERR_ARG
            assert api.bipred_weight_check(bd, IDENT, None, refine) == ERR_ARG
            for bad in ((1 << 16, 0, 16, 1 << 15), (1, 0, -1, 0)):
                assert api.bipred_weight_check(bd, bad, IDENT, refine) == ERR_ARG
                assert api.bipred_weight_check(bd, IDENT, bad, refine) == ERR_ARG
            assert api.bipred_weight_check(bd, (1 << 15, 0, 15, 1 << 14), (1 << 15, 0, 15, 0), 0) == OK


def test_the_restated_rule_is_the_rule(api):
    rng = np.random.default_rng(2025)
    seen = set()
    for _ in range(20000):
        bd = int(rng.integers(8, 13))
        shift = int(rng.integers(0, 16))
        gain = float(rng.choice([0.01, 0.5, 1, 2, 8, 40, 300])) * float(rng.uniform(0.5, 1.5)) * (-1 if rng.integers(0, 4) == 0 else 1)
        w0 = int(round(gain * (1 << shift)))
        offset = int(rng.integers(-70000, 70001)) if rng.integers(0, 2) else int(rng.integers(-300, 301)) << (bd - 8)
        wp = (w0, offset, shift, (1 << (shift - 1)) if shift else 0)
        oshift = int(rng.integers(0, 16))
        other = (int(rng.integers(-70000, 70001)), int(rng.integers(-5000, 5001)), oshift, int(rng.integers(0, 100)))
        for refine in (0, 1):
            why = model.failing(bd, wp, other, refine)
            assert (api.bipred_weight_check(bd, wp, other, refine) == OK) == (why == ()), (bd, wp, other, refine, why)
            assert api.bipred_weight_check(bd, wp, other, refine) in (OK, ERR_UNSUPPORTED)
            seen.update(why)
    assert seen == set(model.SEARCHED_CONDITIONS) | {"other"}   # every refusal line was reached


def test_each_refusal_line_and_the_accepted_weight_next_to_it(api):
    """per line of the table in include/hmme.h: a weight that fails this line (and, where the ranges allow one, no other), refused; and the
    member of its family just before it, accepted"""
    for bd in BDS:
        maxv = (1 << bd) - 1
        # the cost field: the identity scale with a growing offset -> span = 2 * maxv + k
        for refine in (0,):
            k, wp = model.last_accepted(lambda k: (64, k, 6, 32), lambda w: api.bipred_weight_check(bd, w, IDENT, refine))
            nxt = (64, k + 1, 6, 32)
            assert model.failing(bd, nxt, IDENT, refine) == ("cost",) and api.bipred_weight_check(bd, nxt, IDENT, refine) == ERR_UNSUPPORTED
            assert model.searched_terms(bd, wp)[3] == rc.COST_SPAN[bd] == 2 * maxv + k
        # a weighted sample beyond a Pel / samples spanning more than 16 bits: the cost field refuses such a weight as well (its span is
        # beyond 30 994 in both cases), so the accepted neighbour of these two lines is the cost field's
        for bad, name in (((64, 32768 - maxv, 6, 32), "pel"), ((64, -32769, 6, 32), "pel"), ((64, -(65536 - 2 * maxv), 6, 32), "span16")):
            why = model.failing(bd, bad, IDENT, 0)
            assert name in why and "cost" in why and api.bipred_weight_check(bd, bad, IDENT, 0) == ERR_UNSUPPORTED, (bd, bad, why)
        # ... and the numerator beyond 32 bits
        big = (1 << 30, 0, 15, 1 << 14)
        assert "pel" in model.failing(bd, big, IDENT, 0) and api.bipred_weight_check(bd, big, IDENT, 0) == ERR_UNSUPPORTED
        # the refinement: 4096 * span < 2^24 (span <= 4095) binds where the cost field admits more (10 and 11 bit) and the identity's own
        # span 2 * maxv lies below it; at 12 bits the identity's span is 8190: every weight is refused
        if bd in (10, 11):
            k, wp = model.last_accepted(lambda k: (64, k, 6, 32), lambda w: api.bipred_weight_check(bd, w, IDENT, 1))
            assert model.searched_terms(bd, wp)[3] == 4095 and model.failing(bd, (64, k + 1, 6, 32), IDENT, 1) == ("hadamard",)
            assert api.bipred_weight_check(bd, (64, k + 1, 6, 32), IDENT, 1) == ERR_UNSUPPORTED and api.bipred_weight_check(bd, (64, k + 1, 6, 32), IDENT, 0) == OK
        if bd == 12:
            for member in rc.families(bd).values():
                assert api.bipred_weight_check(bd, member(0), IDENT, 1) == ERR_UNSUPPORTED and "hadamard" in model.failing(bd, member(0), IDENT, 1)
        else:
            # the refinement's fp32 numerator: shift 15, w0 up from 1 (spans stay at 2 * maxv: nothing else fails)
            k, wp = model.last_accepted(lambda k: (1 + k, 0, 15, 1 << 14), lambda w: api.bipred_weight_check(bd, w, IDENT, 1))
            nxt = (2 + k, 0, 15, 1 << 14)
            assert model.failing(bd, nxt, IDENT, 1) == ("fp32",) and api.bipred_weight_check(bd, nxt, IDENT, 1) == ERR_UNSUPPORTED
            assert api.bipred_weight_check(bd, nxt, IDENT, 0) == OK and wp[0] * maxv + wp[3] < 1 << 24 <= nxt[0] * maxv + nxt[3]
            # the identity is excepted from that line: 32768 * maxv is far beyond 2^24
            assert api.bipred_weight_check(bd, (1 << 15, 0, 15, 1 << 14), IDENT, 1) == OK
        # the other list: |w0| * 40960 + round' within int32, for both signs and at the smallest and the largest shift
        for shift in (0, 15):
            for sign in (1, -1):
                k, ow = model.last_accepted(lambda k: (sign * (1 + k), 7, shift, 0), lambda w: api.bipred_weight_check(bd, IDENT, w, 0))
                rnd = 1 << (shift + max(2, 14 - bd) - 1)
                assert abs(ow[0]) * 40960 + rnd <= model.INT32_MAX < (abs(ow[0]) + 1) * 40960 + rnd
                nxt = (sign * (2 + k), 7, shift, 0)
                assert model.failing(bd, IDENT, nxt, 0) == ("other",) and api.bipred_weight_check(bd, IDENT, nxt, 0) == ERR_UNSUPPORTED
        # nothing else applies to the other list: any offset, any round
        assert api.bipred_weight_check(bd, IDENT, (-50000, -(1 << 30), 3, -99), 0) == OK


def test_the_boundary_weights_of_the_gpu_tests(api):
    """tests/test_gpu_bipred_wp.py takes its range-edge weights from model.boundary_weights: each is the last accepted member of its family,
    at every depth the search boundaries reach the cost field's span, and the 12-bit refinement has none"""
    for bd in BDS:
        bs = model.boundary_weights(bd, 0)
        assert [b["family"] for b in bs] == list(rc.FAMILIES)
        for b in bs:
            assert api.bipred_weight_check(bd, b["wp"], IDENT, 0) == OK and api.bipred_weight_check(bd, b["next"], IDENT, 0) == ERR_UNSUPPORTED
            assert b["condition"] == "cost"
        assert max(model.searched_terms(bd, b["wp"])[3] for b in bs) == rc.COST_SPAN[bd]
        assert any(model.searched_terms(bd, b["wp"])[2] > (1 << bd) - 1 for b in bs)   # one of them carries a bias above maxv
        br = model.boundary_weights(bd, 1)
        assert (br == []) == (bd == 12)
        for b in br:
            assert api.bipred_weight_check(bd, b["wp"], IDENT, 1) == OK and api.bipred_weight_check(bd, b["next"], IDENT, 1) == ERR_UNSUPPORTED
            assert api.bipred_weight_check(bd, b["wp"], IDENT, 0) == OK
        if bd != 12:
            assert {b["condition"] for b in br} == ({"cost", "fp32"} if bd < 10 else {"hadamard", "fp32"})
