"""B pictures from one MV per 4x4 block (the "bi4" family of include/hmme.h), the part that needs no GPU: the eleven names declared, exported
and bound; a NULL context; hmme_select_dirs4_check against a table of cases taken from the rule; the model tests/bi4_model.py against the
models of the 64 forms -- the decision on replicated input, the bi restriction of 8x4 / 4x8 PUs, the prediction on replicated fields and
quadrant by quadrant; and the proof that the recipes of the end-to-end test in tests/test_gpu_bi4.py choose the shapes and directions only
this family can hold."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bi4_model as b4
import predict4_model as p4
import predict_bi_model as pbm
import predict_chroma_model as cm
import select_dirs_model as sdm
import select_model as sm
from conftest import ROOT
from frame_helpers import bind_hmo, dims, random_field

ERR_ARG = -1
NAMES = ["hmme_search_pairs_bi4_device", "hmme_refine_pairs_bi4_device", "hmme_search_frame_bi4", "hmme_refine_frame_bi4", "hmme_select_dirs4_check",
         "hmme_select_dirs4_device", "hmme_select_dirs4_frame", "hmme_predict_bi4_device", "hmme_predict_bi4_frame", "hmme_predict_chroma_bi4_device",
         "hmme_predict_chroma_bi4_frame"]
METHODS = ["search_frame_bi4", "refine_frame_bi4", "search_pairs_bi4_device", "refine_pairs_bi4_device", "select_dirs4_device", "select_dirs4_frame",
           "predict_bi4_device", "predict_bi4_frame", "predict_chroma_bi4_device", "predict_chroma_bi4_frame"]


@pytest.fixture(scope="module")
def api():
    from hmme import api
    api.build()
    return api


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


def planes(w, h, bd, seed, n):
    from hmme import synth
    return [synth.make_pair(w, h, seed=seed + 11 * k, bit_depth=bd, max_mv=3)[1] for k in range(n)]


# ---- names -----------------------------------------------------------------------------------------------------------------------------
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
        assert callable(getattr(api.Engine, method))
    assert callable(api.select_dirs4_check)
    assert re.search(r"#define HMME_ABI_VERSION 6\b", header) and L.hmme_abi_version() == 6 and api.ABI_VERSION == 6   # new functions only
    assert "at 4x4 it would first need" not in header                                      # the sentence this family makes untrue


def test_a_null_context_is_refused_by_every_new_entry_point(api):
    """HMME_ERR_ARG before anything else is looked at: no device is touched (this test runs where there is none)"""
    L = api.load()
    fp, sel, dp = api.FrameParams(1, 0, 8, 0, -1), api.SelectParams(256), api.DirParams()
    f, s, d = C.byref(fp), C.byref(sel), C.byref(dp)
    assert L.hmme_search_pairs_bi4_device(None, None, None, None, 1, f, None, None, None, None, None, None) == ERR_ARG
    assert L.hmme_refine_pairs_bi4_device(None, None, None, None, 1, f, None, None, None, None, 1, None, None, None) == ERR_ARG
    assert L.hmme_search_frame_bi4(None, None, None, None, f, None, None, None, None, None) == ERR_ARG
    assert L.hmme_refine_frame_bi4(None, None, None, None, f, None, None, None, None, 1, None, None) == ERR_ARG
    assert L.hmme_select_dirs4_device(None, 64, 64, 1, f, s, d, *([None] * 11)) == ERR_ARG
    assert L.hmme_select_dirs4_frame(None, 64, 64, f, s, d, *([None] * 10)) == ERR_ARG
    assert L.hmme_predict_bi4_device(None, None, None, 1, f, None, None, None, 64, None) == ERR_ARG
    assert L.hmme_predict_bi4_frame(None, None, None, f, None, None, None, 64) == ERR_ARG
    assert L.hmme_predict_chroma_bi4_device(None, None, None, 1, 64, 64, f, None, None, None, 32, None) == ERR_ARG
    assert L.hmme_predict_chroma_bi4_frame(None, None, None, 64, 64, f, None, None, None, 32) == ERR_ARG


# ---- the check function -------------------------------------------------------------------------------------------------------------------
def test_select_dirs4_check_follows_the_rule(api):
    ok = [api.DirParams((3, 3, 5), (2, 1))]
    S = api.SelectParams
    cases = [
        (S(256), 1, ok, 0), (S(256), 4, ok * 4, 0), (S(256, min_depth=3, max_depth=3), 1, ok, 0), (S(256, part_mask=0x07, max_depth=2), 2, ok * 2, 0),
        (S(256), 1, [api.DirParams((4096, 4096, 4096), (4096, 4096))], 0),
        (S(64), 1, ok, ERR_ARG),                                                       # the 64 layout belongs to hmme_select_dirs_check
        (S(128), 1, ok, ERR_ARG),
        (S(256, mv_unit=1), 1, ok, ERR_ARG), (S(256, price_mv=1), 1, ok, ERR_ARG),
        (S(256), 0, ok, ERR_ARG), (S(256), 5, ok * 5, ERR_ARG), (S(256), 1, None, ERR_ARG),
        (S(256), 1, [api.DirParams((4097, 0, 0), (0, 0))], ERR_ARG), (S(256), 1, [api.DirParams((0, 0, 4097), (0, 0))], ERR_ARG),
        (S(256), 1, [api.DirParams((0, 0, 0), (0, 4097))], ERR_ARG), (S(256), 2, ok + [api.DirParams((0, 0, 0), (4097, 0))], ERR_ARG),
        (S(256, part_mask=0xF6), 1, ok, ERR_ARG), (S(256, min_depth=2, max_depth=1), 1, ok, ERR_ARG), (S(256, cu_cost=(1 << 20) + 1), 1, ok, ERR_ARG),
    ]
    for sel, n, dirs, want in cases:
        assert api.select_dirs4_check(sel, n, dirs) == want, (sel.mv_per_ctu, sel.mv_unit, sel.price_mv, n, want)
    # and the two checks split the layouts between them
    assert api.select_dirs_check(S(64), 1, ok) == 0 and api.select_dirs_check(S(256), 1, ok) == ERR_ARG
    assert api.load().hmme_select_dirs4_check(None, 1, None) == ERR_ARG


# ---- the decision model --------------------------------------------------------------------------------------------------------------------
def test_the_restricted_slots_are_the_8x4_and_4x8_pus(api):
    rs = b4.restricted_slots()
    assert rs == frozenset(range(256))                                                  # the constant the kernel's merge compares with
    assert {api.slot_rect(s)[2:] for s in rs} == {(8, 4), (4, 8)}
    assert all(api.slot_rect(s)[2:] not in ((8, 4), (4, 8)) for s in range(593) if s not in rs)


@pytest.mark.parametrize("size", [(64, 64), (100, 70)])
def test_the_decision_on_replicated_input_is_the_64_models(api, size):
    """a sel that admits only 8-aligned shapes and a replicated uni field: every 4x4 output is the 64 model's output of its 8x8 block"""
    w, h = size
    n = sdm.n_ctus(w, h)
    pred = sdm.predictors(n, 11)
    tabs = sdm.random_dir_tables(n, n, 12, pred)
    seen = set()
    for kw in (dict(min_depth=2, max_depth=2, part_mask=0x07), dict(min_depth=1, max_depth=2, part_mask=0x03, cu_cost=9, pu_cost=4)):
        f64, d64, s64, c64 = sdm.select_dirs_picture(*tabs, api.SelectParams(64, **kw), w, h, sdm.HM_BITS, pred=pred)
        f, d, s, c, _ = b4.select_dirs4_picture(*tabs[:4], b4.replicate_lists(tabs[4]), api.SelectParams(256, **kw), w, h, sdm.HM_BITS, pred=pred)
        assert np.array_equal(f, b4.replicate_lists(f64)) and np.array_equal(d, p4.replicate(d64)) and np.array_equal(s, p4.replicate(s64)) and np.array_equal(c, c64)
        assert b4.mixed_blocks(f, d) == 0
        seen = seen | set(d.reshape(-1).tolist())
    assert {1, 2, 3} <= seen


def test_an_8x4_or_4x8_pu_is_never_bi_whatever_its_bi_tables_hold(api):
    """random tables in which every restricted slot's bi cost is 0 -- the cheapest candidate there could be: no block under such a slot has
    direction 3, and refilling those slots' bi entries leaves every output equal"""
    w, h = 128, 64
    n = sdm.n_ctus(w, h)
    lq, zero = b4.TABLE_LAMBDA_Q16, ((0, 0, 0), (0, 0))
    mv_uni, cost_uni, mv_bi, cost_bi, uni_field = b4.random_dir_tables4(n, n, 21, lambda_q16=lq)
    rs = sorted(b4.restricted_slots())
    cost_bi = cost_bi.copy(); mv_bi = mv_bi.copy()
    cost_bi[:, :, rs] = 0
    sel = api.SelectParams(256, min_depth=3, max_depth=3)
    f, d, s, c, leaves = b4.select_dirs4_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, sel, w, h, zero, lambda_q16=lq)
    under = np.isin(s, rs)
    assert under.any() and not (d[under] == 3).any() and set(d[under].tolist()) == {1, 2}
    assert (d[~under] == 3).any()                                                      # 8x8 PUs still go bi
    # without the restriction the same tables WOULD choose bi there: the test is not vacuous
    free = sdm.merge_ctu(mv_uni[:, 0], cost_uni[:, 0], mv_bi[:, 0], cost_bi[:, 0], [(0, 0), (0, 0)], zero, lq)
    assert sum(free[2][r] == 3 for r in rs) >= 200
    rng = np.random.default_rng(22)
    cost_bi[:, :, rs] = rng.integers(0, 1 << 32, size=cost_bi[:, :, rs].shape, dtype=np.uint64).astype(np.uint32)
    mv_bi[:, :, rs] = rng.integers(-32768, 32768, size=mv_bi[:, :, rs].shape).astype(np.int16)
    f2, d2, s2, c2, _ = b4.select_dirs4_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, sel, w, h, zero, lambda_q16=lq)
    assert np.array_equal(f, f2) and np.array_equal(d, d2) and np.array_equal(s, s2) and np.array_equal(c, c2)


def test_a_bi_block_takes_its_own_4x4_entry_of_the_other_list(api):
    w, h = 64, 64
    tabs = b4.random_dir_tables4(1, 1, 31)
    f, d, s, _, _ = b4.select_dirs4_picture(*tabs, api.SelectParams(256, max_depth=1), w, h, sdm.HM_BITS)
    bi = np.flatnonzero(d[0] == 3)
    assert len(bi) >= 64                                                                # large PUs: many 4x4 blocks under one bi slot
    for b in bi:
        own = [np.array_equal(f[l, 0, b], tabs[4][l, 0, b]) for l in range(2)]
        assert any(own)
    assert len({tuple(f[l, 0, b]) for b in bi for l in range(2)}) > len(bi)           # the entries differ from block to block


# ---- the end-to-end recipes ----------------------------------------------------------------------------------------------------------------
def check_coverage(depth, cov):
    if depth == 3:
        assert {1, 2} <= cov["sizes"], cov["sizes"]                                    # both 2NxN and Nx2N CUs occur ...
        for ps in (1, 2):
            assert set(cov["dirs_by_ps"][ps]) <= {1, 2} and len(cov["dirs_by_ps"][ps]) >= 2   # ... all of them with directions in {1, 2}
    else:
        for ps in (4, 5, 6, 7):
            assert 3 in cov["dirs_by_ps"].get(ps, []), (ps, cov["dirs_by_ps"].get(ps))   # each AMP PartSize with at least one bi PU
    assert cov["mixed"] >= 20, cov["mixed"]


@pytest.mark.parametrize("depth", [3, 2])
def test_the_table_recipe_chooses_the_small_shapes_and_every_direction(api, depth):
    """random_dir_tables4(2, 2, TABLE_SEED) at TABLE_LAMBDA_Q16 on 128 x 64 with the depth forced: the counts are recorded in DESIGN.md 7
    item 19"""
    w, h = b4.E2E_SIZE
    lq = b4.TABLE_LAMBDA_Q16
    tabs = b4.random_dir_tables4(2, 2, b4.TABLE_SEED, lambda_q16=lq)
    f, d, s, _, leaves = b4.select_dirs4_picture(*tabs, b4.e2e_sel(api, depth), w, h, sdm.HM_BITS, lambda_q16=lq)
    assert all(dep == depth for lv in leaves for dep, _ in lv)
    check_coverage(depth, b4.coverage(depth, s, d, f, leaves))


@pytest.mark.parametrize("depth", [3, 2])
def test_the_picture_recipe_chooses_the_small_shapes_and_every_direction(api, oracle_lib, hmo, depth):
    """the chain of tests/test_gpu_bi4.py's end-to-end test on its own picture (b_scene(128, 64, 8, 4100)), every step by its model: the GPU
    test cannot pass on a degenerate picture"""
    w, h = b4.E2E_SIZE
    cur, r0, r1 = b4.b_scene(w, h, 8, b4.E2E_SEED)
    c = b4.chain(oracle_lib, hmo, api, cur, (r0, r1), w, h, 8, depth, sdm.LAMBDA_Q16)
    check_coverage(depth, b4.coverage(depth, c["slot"], c["dirs"], c["field"], c["leaves"]))


# ---- the prediction model ------------------------------------------------------------------------------------------------------------------
def test_the_prediction_model_on_replicated_fields_is_the_64_models(hmo):
    w, h, bd = 130, 66, 10
    n = dims(w, h)[0] * dims(w, h)[1]
    luma = planes(w, h, bd, 40, 2)
    comps = [planes(w // 2, h // 2, bd, 50 + 5 * c, 2) for c in range(2)]
    field64 = np.stack([random_field(n, 64, 41 + l, max_pel=20) for l in range(2)])
    dirs64 = np.random.default_rng(42).choice(np.array([1, 2, 3, 3, 0xFF, 0], np.uint8), size=(n, 64))
    got = b4.luma_picture(hmo, luma, w, h, bd, b4.replicate_lists(field64), p4.replicate(dirs64), np.full((h, w), -1, np.int64))
    assert np.array_equal(got, pbm.pred_picture(hmo, luma, w, h, bd, field64, dirs64, np.full((h, w), -1, np.int64)))
    assert (got == -1).any() and (got != -1).any()
    fill = lambda: tuple(np.full((h // 2, w // 2), -1, np.int64) for _ in range(2))
    got_c = b4.chroma_picture(hmo, comps, w, h, bd, b4.replicate_lists(field64), p4.replicate(dirs64), fill())
    want_c = cm.bi_picture(hmo, comps, w, h, bd, field64, dirs64, fill())
    assert all(np.array_equal(got_c[c], want_c[c]) for c in range(2)) and not np.array_equal(got_c[0], got_c[1])


def test_quadrant_q_of_the_prediction_model_is_the_64_model_on_the_quadrant_field(hmo):
    w, h, bd = 100, 70, 8
    luma = planes(w, h, bd, 60, 2)
    comps = [planes(w // 2, h // 2, bd, 65 + 5 * c, 2) for c in range(2)]
    field, dirs = b4.random_field_bi4(w, h, 61)
    assert {1, 2, 3, 0, 0xFF} <= set(dirs.reshape(-1).tolist()) and all(len(s) == 16 for s in b4.phase_pairs(w, h, field, dirs))
    got = b4.luma_picture(hmo, luma, w, h, bd, field, dirs, np.full((h, w), -1, np.int64))
    fill = lambda: tuple(np.full((h // 2, w // 2), -1, np.int64) for _ in range(2))
    got_c = b4.chroma_picture(hmo, comps, w, h, bd, field, dirs, fill())
    for q, (fq, dq) in enumerate(b4.quadrant_fields(field, dirs)):
        m = p4.quadrant_mask(w, h, q)
        want = pbm.pred_picture(hmo, luma, w, h, bd, fq, dq, np.full((h, w), -1, np.int64))
        assert np.array_equal(got[m], want[m]), q
        want_c = cm.bi_picture(hmo, comps, w, h, bd, fq, dq, fill())
        mc = p4.quadrant_mask(w, h, q, 2)
        assert all(np.array_equal(got_c[c][mc], want_c[c][mc]) for c in range(2)), q
    assert (got == -1).any() and (got != -1).any()


def test_the_rotation_ctu_holds_every_rotation(hmo):
    field, dirs = b4.rotation_ctu(5)
    quads = {tuple(int(v) for v in q) for q in b4.block_of(dirs)[0]}
    assert len(quads) == 8 and all(sorted(min(v, 4) for v in q) == [0, 1, 2, 3] or sorted(q) == [1, 2, 3, 0xFF] for q in quads)


def test_the_origin_prediction_on_a_replicated_field_is_the_64_forms(hmo):
    from frame_helpers import oracle_prediction
    w, h, bd = 100, 70, 8
    n = dims(w, h)[0] * dims(w, h)[1]
    plane = planes(w, h, bd, 70, 1)[0]
    field64 = random_field(n, 64, 71, max_pel=20)
    assert np.array_equal(b4.origin_prediction(hmo, plane, w, h, bd, p4.replicate(field64)), oracle_prediction(hmo, plane, w, h, bd, field64))
