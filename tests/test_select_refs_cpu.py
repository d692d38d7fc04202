"""The reference picture per PU (hmme_select_refs_*, hmme_predict_refs_*, hmme_ref_idx_bits), the part that needs no GPU: the new names
declared, exported and bound; hmme_ref_idx_bits against HM's rule; hmme_select_refs_check at every limit include/hmme.h states; the model
tests/select_refs_model.py against the partition model with one reference; and the proof that the table recipes of
tests/test_gpu_select_refs.py exercise the choice of the reference at all (nothing here touches a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lambda_cases as lc
import select_model as sm
import select_refs_model as srm
from conftest import ROOT

OK, ERR_ARG = 0, -1
NAMES = ["hmme_ref_idx_bits", "hmme_select_refs_check", "hmme_select_refs_device", "hmme_select_refs_frame", "hmme_predict_refs_device",
         "hmme_predict_refs_frame"]


@pytest.fixture(scope="module")
def api():
    from hmme import api
    api.build()
    return api


@pytest.fixture(scope="module")
def mv_cost(oracle_lib):
    L = oracle_lib.oracle()
    return lambda lq, x, y, px, py, scale: L.hmo_mv_cost(lq, x, y, px, py, scale)


def test_the_new_names_are_declared_exported_and_bound(api):
    L = api.load()
    header = open(os.path.join(ROOT, "include", "hmme.h")).read()
    declared = set(re.findall(r"\b(hmme_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/hmme.h"
        assert hasattr(L, name), f"libhmme.so does not export {name}"
        assert name in api.SYMBOLS
        assert getattr(L, name).argtypes is not None, f"api.py binds no argument types for {name}"
    for method in ("select_refs_device", "select_refs_frame", "predict_refs_device", "predict_refs_frame"):
        assert callable(getattr(api.Engine, method))
    assert callable(api.ref_idx_bits) and callable(api.select_refs_check)
    assert re.search(r"#define HMME_ABI_VERSION 6\b", header) and L.hmme_abi_version() == 6 and api.ABI_VERSION == 6   # new functions only


def test_a_null_context_is_refused_by_every_new_entry_point(api):
    """HMME_ERR_ARG before anything else is looked at: no device is touched (this test runs where there is none)"""
    L = api.load()
    fp = api.FrameParams(1, 0, 8, 0, -1)
    sel = api.SelectParams(64)
    assert L.hmme_select_refs_device(None, 64, 64, 1, 1, C.byref(fp), C.byref(sel), None, None, None, None, None, None, None, None, None) == ERR_ARG
    assert L.hmme_select_refs_frame(None, 64, 64, 1, C.byref(fp), C.byref(sel), None, None, None, None, None, None, None, None) == ERR_ARG
    assert L.hmme_predict_refs_device(None, None, 1, C.byref(fp), None, None, 64, None, 64, None) == ERR_ARG
    assert L.hmme_predict_refs_frame(None, None, 1, C.byref(fp), None, None, 64, None, 64) == ERR_ARG


def test_ref_idx_bits_is_hms_count(api):
    for n_refs in range(1, 17):
        for r in range(n_refs):
            # TEncSearch.cpp:3030-3037, literally
            bits = r + 1
            if r == n_refs - 1:
                bits -= 1
            if n_refs == 1:
                bits = 0
            assert api.ref_idx_bits(n_refs, r) == bits == srm.hm_ref_idx_bits(n_refs, r), (n_refs, r)
    assert [api.ref_idx_bits(4, r) for r in range(4)] == [1, 2, 3, 3] and api.ref_idx_bits(2, 1) == 1 and api.ref_idx_bits(1, 0) == 0
    for n_refs, r in ((0, 0), (17, 0), (17, 16), (4, 4), (4, -1), (1, 1), (-1, 0), (16, 16)):
        assert api.ref_idx_bits(n_refs, r) == -1, (n_refs, r)


def test_select_refs_check_at_every_limit(api):
    sel = api.SelectParams(64)
    check = api.select_refs_check
    assert api.load().hmme_select_refs_check(None, 1, 1, None) == ERR_ARG
    for n_refs, want in ((0, ERR_ARG), (1, OK), (16, OK), (17, ERR_ARG), (-1, ERR_ARG)):
        assert check(sel, 1, n_refs) == want, n_refs
    for n_pics, n_refs, want in ((16, 1, OK), (17, 1, ERR_ARG), (8, 2, OK), (4, 4, OK), (5, 3, OK), (6, 3, ERR_ARG), (2, 8, OK), (2, 9, ERR_ARG),
                                 (0, 1, ERR_ARG), (-1, 1, ERR_ARG), (1 << 30, 16, ERR_ARG)):
        assert check(sel, n_pics, n_refs) == want, (n_pics, n_refs)
    for v, want in ((0, OK), (1 << 20, OK), ((1 << 20) + 1, ERR_ARG), (0xFFFFFFFF, ERR_ARG)):
        for at in range(4):
            rc = [0] * 4
            rc[at] = v
            assert check(sel, 1, 4, rc) == want, (v, at)
    assert check(sel, 1, 2, [0, 0, (1 << 20) + 1]) == OK      # only n_refs entries are read
    assert check(sel, 4, 4, None) == OK                       # NULL: zeros
    # sel is checked by hmme_select_check, unchanged
    for bad in (api.SelectParams(128), api.SelectParams(64, part_mask=0x06), api.SelectParams(64, min_depth=2, max_depth=1),
                api.SelectParams(64, cu_cost=(1 << 20) + 1), api.SelectParams(64, mv_unit=2)):
        assert api.select_check(bad) == ERR_ARG and check(bad, 1, 1) == ERR_ARG
    for good in (api.SelectParams(256, mv_unit=1, price_mv=1, cu_cost=1 << 20, pu_cost=1 << 20), api.SelectParams(64, part_mask=0x01, min_depth=3, max_depth=3)):
        assert api.select_check(good) == OK and check(good, 4, 4, [1 << 20] * 4) == OK


@pytest.mark.parametrize("per,unit,price", [(64, 0, 0), (256, 1, 1), (64, 1, 1), (256, 0, 0)])
def test_the_model_with_one_reference_is_the_partition_model(api, mv_cost, per, unit, price):
    mv, cost = sm.random_tables(6, seed=1, noise=64 if price else 2)
    pred = srm.ref_predictors(1, 6, seed=5)
    sel = api.SelectParams(per, mv_unit=unit, price_mv=price, cu_cost=40, pu_cost=12)
    for w, h in ((136, 72), (192, 128)):
        want = sm.select_picture(mv, cost, sel, w, h, 0, pred[0], srm.LAMBDA_Q16, mv_cost)
        got = srm.select_refs_picture(mv[None], cost[None], sel, w, h, [0], 0, pred, srm.LAMBDA_Q16, mv_cost)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[1]) and np.array_equal(got[3], want[2]) and got[4] == want[3]
        assert ((got[1] == 0) == (want[1] != sm.NO_SLOT)).all() and ((got[1] == srm.NO_REF) == (want[1] == sm.NO_SLOT)).all()
        assert (got[1] == srm.NO_REF).any() == (w == 136)


@pytest.mark.parametrize("price", [0, 1])
@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("per", [64, 256])
@pytest.mark.parametrize("n_refs", [2, 4, 16])
def test_the_recipes_of_the_gpu_cases_exercise_the_choice(api, mv_cost, n_refs, per, unit, price):
    """a test in which one reference always wins checks nothing: on the very tables the GPU cases feed, the model alone has every reference
    index winning at least one written block, and at least two different references inside one CTU"""
    w, h, mv, cost, pred, ref_cost, min_depth = srm.case(n_refs, price)
    sel = api.SelectParams(per, mv_unit=unit, price_mv=price, min_depth=min_depth)
    _, ref, slot, _, _ = srm.select_refs_picture(mv, cost, sel, w, h, ref_cost, 0, pred, srm.LAMBDA_Q16, mv_cost)
    written = ref[slot != sm.NO_SLOT]
    assert set(written.tolist()) == set(range(n_refs))
    assert max(len(set(ref[c][slot[c] != sm.NO_SLOT].tolist())) for c in range(ref.shape[0])) >= 2
    assert (ref[slot == sm.NO_SLOT] == srm.NO_REF).all() and (slot == sm.NO_SLOT).any()      # partial CTUs: blocks no CU covers
    assert any((pred[a] != pred[b]).any() for a in range(n_refs) for b in range(a))           # distinct predictors
    assert len(set(ref_cost)) > 1 or n_refs == 2                                               # HM's prices differ by index


# ---- the MV cost where its product wraps (tests/lambda_cases.py) -----------------------------------------------------------------------
def _wide(lq, x, y, px, py, scale):
    return lc.get_cost_64(lq, lc.mv_bits(x << scale, y << scale, px, py))


def _wrapped(lq, x, y, px, py, scale):
    return lc.get_cost(lq, lc.mv_bits(x << scale, y << scale, px, py))


@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("lq", lc.LAMBDA_Q16)
def test_the_model_prices_mvs_with_the_wrapping_product(api, mv_cost, lq, unit):
    """three references, each with its own far predictor: the oracle's hmo_mv_cost == the Python restatement, at every lambda of the set"""
    mv, cost = srm.random_ref_tables(3, 2, seed=92, noise=64)
    pred = np.array([[[-1900, 1733], [37, -1012]], [[1999, -8], [-640, 1500]], [[12, 1024], [-2000, -2000]]], np.int16)
    sel = api.SelectParams(64, mv_unit=unit, price_mv=1, cu_cost=40, pu_cost=12)
    a = srm.select_refs_picture(mv, cost, sel, 128, 64, srm.hm_ref_cost(3), 0, pred, lq, mv_cost)
    b = srm.select_refs_picture(mv, cost, sel, 128, 64, srm.hm_ref_cost(3), 0, pred, lq, _wrapped)
    assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
    if lq in lc.WRAPPING:
        assert not np.array_equal(srm.select_refs_picture(mv, cost, sel, 128, 64, srm.hm_ref_cost(3), 0, pred, lq, _wide)[3], a[3])


def test_the_wrap_changes_the_reference_by_hand(api):
    """one 64x64 2Nx2N CU, two references at lambda_q16 = 178956971: reference 0 costs 1000 at an MV of 24 bits (wrapped price 0, 64-bit
    price 65536), reference 1 costs 900 at an MV of 2 bits (price 5461: 6361).  HM's wrapping product takes reference 0, a 64-bit one reference 1"""
    whole = api.slot_index(0, 0, 0, 0)
    mv, cost = np.zeros((2, 1, 593, 2), np.int16), np.full((2, 1, 593), 1 << 20, np.uint32)
    mv[0, 0, whole], cost[0, 0, whole], cost[1, 0, whole] = (1024, 0), 1000, 900
    sel = api.SelectParams(64, price_mv=1, part_mask=0x01, max_depth=0)
    _, ref, _, total, _ = srm.select_refs_picture(mv, cost, sel, 64, 64, None, 0, None, lc.WRAP24, _wrapped)
    assert set(ref.reshape(-1).tolist()) == {0} and total.tolist() == [1000]
    _, ref, _, total, _ = srm.select_refs_picture(mv, cost, sel, 64, 64, None, 0, None, lc.WRAP24, _wide)
    assert set(ref.reshape(-1).tolist()) == {1} and total.tolist() == [6361]
