"""L0, L1 or bi per PU (hmme_select_dirs_*, hmme_predict_bi_*), the part that needs no GPU: the new names declared, exported and bound;
hmme_select_dirs_check at every limit include/hmme.h states and at its accepted neighbour; the model tests/select_dirs_model.py against
tests/select_refs_model.py in the degenerate case; the clamp of rule 1 on real refinement tables; and the proof that the recipes of
tests/test_gpu_select_dirs.py exercise every direction and every tie (nothing here touches a device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lambda_cases as lc
import select_dirs_model as sdm
import select_model as sm
import select_refs_model as srm
from conftest import ROOT

OK, ERR_ARG = 0, -1
NAMES = ["hmme_select_dirs_check", "hmme_select_dirs_device", "hmme_select_dirs_frame", "hmme_predict_bi_device", "hmme_predict_bi_frame"]


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
    for method in ("select_dirs_device", "select_dirs_frame", "predict_bi_device", "predict_bi_frame"):
        assert callable(getattr(api.Engine, method))
    assert callable(api.select_dirs_check) and C.sizeof(api.DirParams) == 20
    assert re.search(r"#define HMME_ABI_VERSION 6\b", header) and L.hmme_abi_version() == 6 and api.ABI_VERSION == 6   # new functions only
    assert "THIS TEXT PLUS THE CITATIONS IS THE RULE" in header.split("L0, L1 or bi per PU")[1].split("typedef struct hmme_dir_params")[0]


def test_a_null_context_is_refused_by_every_new_entry_point(api):
    """HMME_ERR_ARG before anything else is looked at: no device is touched (this test runs where there is none)"""
    L = api.load()
    fp, sel, dp = api.FrameParams(1, 0, 8, 0, -1), api.SelectParams(64), api.DirParams()
    assert L.hmme_select_dirs_device(None, 64, 64, 1, C.byref(fp), C.byref(sel), C.byref(dp), *([None] * 11)) == ERR_ARG
    assert L.hmme_select_dirs_frame(None, 64, 64, C.byref(fp), C.byref(sel), C.byref(dp), *([None] * 10)) == ERR_ARG
    assert L.hmme_predict_bi_device(None, None, None, 1, C.byref(fp), None, None, 64, None, 64, None) == ERR_ARG
    assert L.hmme_predict_bi_frame(None, None, None, C.byref(fp), None, None, 64, None, 64) == ERR_ARG


def test_select_dirs_check_at_every_limit(api):
    sel, check, D = api.SelectParams(64), api.select_dirs_check, api.DirParams
    assert api.load().hmme_select_dirs_check(None, 1, C.byref(D())) == ERR_ARG
    assert check(sel, 1, None) == ERR_ARG                                     # the bit counts are not optional
    for n_pics, want in ((0, ERR_ARG), (1, OK), (4, OK), (5, ERR_ARG), (-1, ERR_ARG), (1 << 30, ERR_ARG)):
        assert check(sel, n_pics, [D()] * 4) == want, n_pics
    for v, want in ((0, OK), (4096, OK), (4097, ERR_ARG), (0xFFFFFFFF, ERR_ARG)):
        for at in range(5):
            b = [0] * 5
            b[at] = v
            for pic in range(4):                                              # in every picture of the launch
                dirs = [D()] * 4
                dirs[pic] = D(b[:3], b[3:])
                assert check(sel, 4, dirs) == want, (v, at, pic)
    assert check(sel, 2, [D(), D(), D((4097, 0, 0))]) == OK                   # only n_pics entries are read
    # mv_per_ctu 64, mv_unit 0, price_mv 0 and nothing else; the rest of sel as hmme_select_check has it
    for bad in (api.SelectParams(256), api.SelectParams(64, mv_unit=1), api.SelectParams(64, price_mv=1), api.SelectParams(128),
                api.SelectParams(64, part_mask=0x06), api.SelectParams(64, min_depth=2, max_depth=1), api.SelectParams(64, cu_cost=(1 << 20) + 1)):
        assert check(bad, 1, [D()]) == ERR_ARG
    assert api.select_check(api.SelectParams(256, mv_unit=1, price_mv=1)) == OK   # fine for the siblings
    for good in (api.SelectParams(64, cu_cost=1 << 20, pu_cost=1 << 20), api.SelectParams(64, part_mask=0x01, min_depth=3, max_depth=3)):
        assert check(good, 4, [D((4096, 4096, 4096), (4096, 4096))] * 4) == OK


def test_the_models_bit_count_is_the_oracles(oracle_lib):
    L = oracle_lib.oracle()
    for v in list(range(-70, 71)) + [-32768 - 300, 32767 + 300, 1 << 14, -(1 << 14)]:
        assert sdm.component_bits(v) == L.hmo_component_bits(v), v
    for x, y, px, py in ((5, -3, 0, 0), (-200, 117, 40, -7), (300, -300, -40, 40)):
        assert sdm.gc(1 << 16, sdm.mvb((x, y), (px, py))) == L.hmo_mv_cost(1 << 16, x, y, px, py, 0)
        assert sdm.gc(sdm.LAMBDA_Q16, sdm.mvb((x, y), (px, py))) == L.hmo_mv_cost(sdm.LAMBDA_Q16, x, y, px, py, 0)
    assert sdm.gc(0xFFFFFFFF, 4096 * 3 + 100) == ((0xFFFFFFFF * (4096 * 3 + 100)) % (1 << 32)) >> 16   # wraps like getCost


@pytest.mark.parametrize("w,h", sdm.SIZES)
def test_without_bits_and_without_bi_the_model_is_the_reference_choice(api, w, h):
    """all bits 0 and bi costs of UINT32_MAX: list l is reference l at price 0, direction = reference + 1"""
    n = sdm.n_ctus(w, h)
    pred = sdm.predictors(n, seed=11)
    mv_uni, cost_uni, mv_bi, cost_bi, uni_field = sdm.random_dir_tables(n, n, seed=12, pred=pred)
    cost_bi = np.full_like(cost_bi, 0xFFFFFFFF)
    sel = api.SelectParams(64, cu_cost=40, pu_cost=12, min_depth=2)             # CUs of 16x16 at most: enough of them for both lists to win some
    zero = ((0, 0, 0), (0, 0))
    for k in range(n):                                                         # at zero bits C[l] is cost_uni[l] exactly
        for s in range(0, 593, 7):
            c, c_b = sdm.slot_candidates(mv_uni[:, k, s], cost_uni[:, k, s], mv_bi[:, k, s], cost_bi[:, k, s], pred[:, k], zero, sdm.LAMBDA_Q16)
            assert c == [int(cost_uni[0, k, s]), int(cost_uni[1, k, s])] and min(c_b) > max(c)
    field, dirs, slot, cost = sdm.select_dirs_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, sel, w, h, zero, 0, pred)
    rf, rr, rs, rc_, _ = srm.select_refs_picture(mv_uni, cost_uni, sel, w, h, [0, 0], 0, pred, sdm.LAMBDA_Q16, None)
    assert np.array_equal(slot, rs) and np.array_equal(cost, rc_)
    assert np.array_equal(dirs, np.where(rr == srm.NO_REF, sdm.NO_DIR, rr + 1).astype(np.uint8))
    for l in range(2):
        assert np.array_equal(field[l], np.where((rr == l)[..., None], rf, 0))
    assert {1, 2} <= set(dirs.reshape(-1).tolist()) and 3 not in dirs and ((dirs == sdm.NO_DIR).any() == (w != 64))


def test_cost_covers_the_mv_cost_in_every_slot_of_real_tables(oracle_lib):
    """what makes the clamp of rule 1 a formality: a refinement's cost contains gc(mvb) of its own MV"""
    from hmme import synth
    w, h, sr, m = 136, 72, 8, synth.MARGIN
    lq = sdm.LAMBDA_Q16
    cur, ref, _ = synth.make_pair(w, h, seed=5, max_mv=5, region=32)
    pred = synth.random_predictors(sdm.n_ctus(w, h), seed=6, max_pel=4)
    ox, oy, _ = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pred, lq, 1, 8, n_threads=4)
    imv = np.stack([ox, oy], axis=-1).astype(np.int16)
    first, count = 1, 2
    qmv, cost = oracle_lib.refine_frame(cur, ref, (m, m), w, h, imv[first:first + count], pred, lq, 1, 8, first, count, n_threads=4)
    price = sdm.mv_cost_table(qmv, pred, range(first, first + count), lq)
    assert (cost.astype(np.int64) >= price).all() and (price > 0).all()
    assert ((qmv & 3) != 0).any()                                              # quarter-pel MVs, not the integer ones handed in


@pytest.mark.parametrize("bits", [sdm.HM_BITS, ((0, 0, 0), (0, 0))])
def test_the_recipes_of_the_gpu_cases_exercise_every_direction_and_every_tie(api, bits):
    w, h = 136, 72
    n = sdm.n_ctus(w, h)
    sel = api.SelectParams(64)
    pred = sdm.predictors(n, seed=21)
    tabs = sdm.random_dir_tables(n, n, seed=22, pred=pred)
    _, dirs, slot, _ = sdm.select_dirs_picture(*tabs, sel, w, h, bits, 0, pred)
    assert set(dirs.reshape(-1).tolist()) == {1, 2, 3, sdm.NO_DIR} and ((dirs == sdm.NO_DIR) == (slot == sm.NO_SLOT)).all()
    assert (pred[0] != pred[1]).any()
    ties, pat = sdm.tie_tables(n, 23, bits, pred)
    assert set(pat.reshape(-1).tolist()) == set(range(27))
    _, dirs, _, _ = sdm.select_dirs_picture(*ties, sdm.tie_sel(api), w, h, bits, 0, pred, 1 << 16)
    assert {1, 2, 3} <= set(dirs.reshape(-1).tolist())
    # the rule at the ties themselves
    assert sdm.decide([10, 10], [10, 10]) == (3, 0, 10) and sdm.decide([10, 10], [11, 11]) == (1, 0, 10) and sdm.decide([10, 9], [10, 10]) == (2, 0, 9)
    assert sdm.decide([10, 10], [10, 9]) == (3, 1, 9) and sdm.decide([9, 10], [10, 9]) == (3, 1, 9) and sdm.decide([9, 10], [10, 10]) == (1, 0, 9)


# ---- getCost where its product wraps (tests/lambda_cases.py) -----------------------------------------------------------------------------
@pytest.mark.parametrize("lq", lc.LAMBDA_Q16)
def test_the_models_get_cost_is_the_wrapping_product(oracle_lib, lq):
    L = oracle_lib.oracle()
    for n in list(range(0, 80)) + [4096, 3 * 4096 + 77, 20000]:
        assert sdm.gc(lq, n) == lc.get_cost(lq, n) == ((lq * n) % (1 << 32)) >> 16
    for x, y, px, py in ((5, -3, 0, 0), (-200, 117, 1900, -7), (300, -300, -2000, 2000), (1024, 0, 0, 0)):
        assert sdm.gc(lq, sdm.mvb((x, y), (px, py))) == L.hmo_mv_cost(lq, x, y, px, py, 0)
    assert all(sdm.mvb((x, y), (px, py)) % 2 == 0 for x in range(-9, 10) for y in (-300, 0, 7) for px in (-2000, 3) for py in (0, 11))   # two odd lengths


@pytest.mark.parametrize("lq", lc.WRAPPING)
def test_the_direction_model_at_the_wrapping_lambdas_differs_from_a_64_bit_product(api, monkeypatch, lq):
    """both uses of gc wrap, and the floor of rule 1 is hit: distortion-only tables (written at lambda_q16 = 1) priced at lq"""
    w, h = 136, 72
    n = sdm.n_ctus(w, h)
    rng = np.random.default_rng(93)
    pred = rng.integers(-2000, 2001, size=(2, n, 2)).astype(np.int16)
    tabs = sdm.random_dir_tables(n, n, seed=94, pred=pred, lambda_q16=lc.TINY)
    floor = sum(int(tabs[1][l, k, s]) < sdm.gc(lq, sdm.mvb(tabs[0][l, k, s], pred[l][k])) for l in range(2) for k in range(n) for s in range(0, 593, 5))
    assert floor > 0 or lq == lc.HALF      # an MV's bit count is even: at 0x80000000 gc(mv bits) is 0, only the bits put back cost
    sel = api.SelectParams(64, cu_cost=40, pu_cost=12)
    bits = ((3, 3, 5), (2, 1))
    want = sdm.select_dirs_picture(*tabs, sel, w, h, bits, 0, pred, lq)
    monkeypatch.setattr(sdm, "gc", lc.get_cost_64)
    wide = sdm.select_dirs_picture(*tabs, sel, w, h, bits, 0, pred, lq)
    assert not np.array_equal(want[3], wide[3])


def test_the_wrap_changes_the_direction_by_hand(monkeypatch):
    """one slot at lambda_q16 = 178956971, no direction or list bits, no bi candidate (cost 2^32 - 1).  List 0: cost 1000 at an MV of 24 bits --
    gc(24) = 0 wrapped: C[0] = 1000 - 0 + 0 = 1000; with a 64-bit product gc(24) = 65536: max(0, 1000 - 65536) + 65536 = 65536.  List 1: cost 7000
    at an MV of 2 bits, gc(2) = 5461: C[1] = 1539 + 5461 = 7000 either way.  HM's wrapping product codes L0, a 64-bit one L1.  And the floor:
    a cost of 3000 under gc(2) = 5461 leaves a distortion of 0"""
    zero = ((0, 0, 0), (0, 0))
    mu, cu = np.array([[1024, 0], [0, 0]], np.int16), [1000, 7000]
    mb, cb = np.zeros((2, 2), np.int16), [0xFFFFFFFF, 0xFFFFFFFF]
    pred = [(0, 0), (0, 0)]
    c, c_b = sdm.slot_candidates(mu, cu, mb, cb, pred, zero, lc.WRAP24)
    assert c == [1000, 7000] and sdm.decide(c, c_b)[0] == 1
    assert sdm.slot_candidates(mu, [1000, 3000], mb, cb, pred, zero, lc.WRAP24)[0] == [1000, 0 + 5461]
    monkeypatch.setattr(sdm, "gc", lc.get_cost_64)
    c, c_b = sdm.slot_candidates(mu, cu, mb, cb, pred, zero, lc.WRAP24)
    assert c == [65536, 7000] and sdm.decide(c, c_b)[0] == 2
