"""B pictures with several references per list from one MV per 4x4 block (the "bi_refs4" family of include/hmme.h), the part that needs no
GPU: the eleven names declared, exported and bound; a NULL context; hmme_select_dirs_refs4_check against cases taken from the rule; the model
tests/bi_refs4_model.py pinned three ways -- on replicated fields it is the 64-form models, with one reference per list it is bi4_model,
and on 4x4 fields it is four runs of the 64-form models composed quadrant by quadrant; and, on the model alone, that the content
tests/test_gpu_bi_refs4.py feeds covers what it must."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bi4_model as b4
import bi_refs4_model as br4
import predict4_model as p4
import predict_bi_refs_model as pbr
import predict_chroma_bi_refs_model as pcbr
import select_dirs_model as sdm
import select_dirs_refs_model as drm
import select_model as sm
from conftest import ROOT
from frame_helpers import bind_hmo, dims, random_field

ERR_ARG = -1
NAMES = ["hmme_search_frame_bi_refs4_device", "hmme_refine_frame_bi_refs4_device", "hmme_search_frame_bi_refs4", "hmme_refine_frame_bi_refs4",
         "hmme_select_dirs_refs4_check", "hmme_select_dirs_refs4_device", "hmme_select_dirs_refs4_frame", "hmme_predict_bi_refs4_device",
         "hmme_predict_bi_refs4_frame", "hmme_predict_chroma_bi_refs4_device", "hmme_predict_chroma_bi_refs4_frame"]
METHODS = ["search_frame_bi_refs4", "refine_frame_bi_refs4", "search_frame_bi_refs4_device", "refine_frame_bi_refs4_device", "select_dirs_refs4_device",
           "select_dirs_refs4_frame", "predict_bi_refs4_device", "predict_bi_refs4_frame", "predict_chroma_bi_refs4_device", "predict_chroma_bi_refs4_frame"]


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


def blank(w, h, sub=1):
    return np.full((h // sub, w // sub), -7, np.int64)


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
    assert callable(api.select_dirs_refs4_check)
    assert re.search(r"#define HMME_ABI_VERSION 6\b", header) and L.hmme_abi_version() == 6 and api.ABI_VERSION == 6   # new functions only
    assert "several references per list (hmme_select_dirs_refs_* at 4x4)" not in header   # the line of the bi4 text this family makes untrue


def test_a_null_context_is_refused_by_every_new_entry_point(api):
    """HMME_ERR_ARG before anything else is looked at: no device is touched (this test runs where there is none)"""
    L = api.load()
    fp, sel, dp = api.FrameParams(1, 0, 8, 0, -1), api.SelectParams(256), api.DirRefsParams()
    f, s, d = C.byref(fp), C.byref(sel), C.byref(dp)
    assert L.hmme_search_frame_bi_refs4_device(None, None, None, 1, None, 1, f, *([None] * 7)) == ERR_ARG
    assert L.hmme_refine_frame_bi_refs4_device(None, None, None, 1, None, 1, f, *([None] * 5), 1, None, None, None) == ERR_ARG
    assert L.hmme_search_frame_bi_refs4(None, None, None, 1, None, 1, f, *([None] * 6)) == ERR_ARG
    assert L.hmme_refine_frame_bi_refs4(None, None, None, 1, None, 1, f, *([None] * 5), 1, None, None) == ERR_ARG
    assert L.hmme_select_dirs_refs4_device(None, 64, 64, 1, 1, f, s, d, *([None] * 13)) == ERR_ARG
    assert L.hmme_select_dirs_refs4_frame(None, 64, 64, 1, f, s, d, *([None] * 12)) == ERR_ARG
    assert L.hmme_predict_bi_refs4_device(None, None, 1, None, 1, f, None, None, None, None, 64, None) == ERR_ARG
    assert L.hmme_predict_bi_refs4_frame(None, None, 1, None, 1, f, None, None, None, None, 64) == ERR_ARG
    assert L.hmme_predict_chroma_bi_refs4_device(None, None, 1, None, 1, 64, 64, f, None, None, None, None, None, 32, None) == ERR_ARG
    assert L.hmme_predict_chroma_bi_refs4_frame(None, None, 1, None, 1, 64, 64, f, None, None, None, None, 32) == ERR_ARG


def test_select_dirs_refs4_check_follows_the_rule(api):
    D, S = api.DirRefsParams, api.SelectParams
    ok = [D((3, 3, 5), (2, 2), ((1, 2), (1, 2)))]
    cases = [
        (S(256), 1, 2, ok, 0), (S(256), 4, 2, ok * 4, 0), (S(256), 1, 8, [D((3, 3, 5), (8, 3), ([1] * 8, [2] * 3), 0b101)], 0),
        (S(256, min_depth=3, max_depth=3), 1, 2, ok, 0), (S(256), 1, 2, [D((3, 3, 5), (2, 2), ((1, 2), (1, 2)), 0)], 0),
        (S(64), 1, 2, ok, ERR_ARG),                                                    # the 64 layout belongs to hmme_select_dirs_refs_check
        (S(128), 1, 2, ok, ERR_ARG), (S(256, mv_unit=1), 1, 2, ok, ERR_ARG), (S(256, price_mv=1), 1, 2, ok, ERR_ARG),
        (S(256), 0, 2, ok, ERR_ARG), (S(256), 5, 2, ok * 5, ERR_ARG), (S(256), 1, 2, None, ERR_ARG),
        (S(256), 1, 9, ok, ERR_ARG), (S(256), 1, 0, ok, ERR_ARG),                      # R outside 1..8
        (S(256), 1, 2, [D((3, 3, 5), (0, 2), ((), (1, 2)))], ERR_ARG), (S(256), 1, 2, [D((3, 3, 5), (2, 3), ((1, 2), (1, 2, 3)))], ERR_ARG),   # n_refs outside 1..R
        (S(256), 1, 2, [D((3, 3, 5), (2, 2), ((1, 2), (1, 2)), 0b100)], ERR_ARG),      # mask bits beyond n_refs[1]
        (S(256), 1, 2, [D((4097, 0, 0), (2, 2), ((1, 2), (1, 2)))], ERR_ARG), (S(256), 1, 2, [D((3, 3, 5), (2, 2), ((1, 4097), (1, 2)))], ERR_ARG),
    ]
    for sel, n, R, dirs, want in cases:
        assert api.select_dirs_refs4_check(sel, n, R, dirs) == want, (sel.mv_per_ctu, sel.mv_unit, sel.price_mv, n, R, want)
    # the two checks split the layouts between them
    assert api.select_dirs_refs_check(S(64), 1, 2, ok) == 0 and api.select_dirs_refs_check(S(256), 1, 2, ok) == ERR_ARG
    assert api.load().hmme_select_dirs_refs4_check(None, 1, 2, None) == ERR_ARG


# ---- the model: replicated input is the 64 models ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 64), (100, 70)])
def test_the_decision_on_replicated_input_is_the_64_model(api, size):
    """a sel that admits only 8-aligned shapes and replicated uni fields: every 4x4 output is the 64 model's output of its 8x8 block"""
    w, h = size
    n = sdm.n_ctus(w, h)
    R = 3
    pred = drm.predictors(R, n, 31)
    tabs = drm.random_tables(R, n, n, 32, pred)
    bits = drm.Bits((3, 3, 5), (3, 2), ((1, 2, 3), (2, 2, 0)), 0b10)
    seen = set()
    for kw in (dict(min_depth=2, max_depth=2, part_mask=0x07), dict(min_depth=1, max_depth=2, part_mask=0x03, cu_cost=9, pu_cost=4)):
        f64, r64, d64, s64, c64 = drm.select_dirs_refs_picture(*tabs, api.SelectParams(64, **kw), w, h, bits, pred=pred)
        f, r, d, s, c = br4.select_dirs_refs4_picture(*tabs[:4], b4.replicate_lists(tabs[4]), b4.replicate_lists(tabs[5]), api.SelectParams(256, **kw), w, h, bits, pred=pred)
        assert np.array_equal(f, b4.replicate_lists(f64)) and np.array_equal(r, b4.replicate_lists(r64)) and np.array_equal(d, p4.replicate(d64))
        assert np.array_equal(s, p4.replicate(s64)) and np.array_equal(c, c64)
        seen |= set(d.reshape(-1).tolist())
    assert {1, 2, 3} <= seen


@pytest.mark.parametrize("size,bd", [((64, 64), 8), ((100, 70), 10)])
def test_the_prediction_on_replicated_fields_is_the_64_models(hmo, size, bd):
    w, h = size
    n = dims(w, h)[0] * dims(w, h)[1]
    n0, n1 = 3, 2
    l0, l1 = planes(w, h, bd, 40, n0), planes(w, h, bd, 41, n1)
    rng = np.random.default_rng(42 + w)
    field64 = np.stack([random_field(n, 64, 43 + l + w, max_pel=20) for l in range(2)])
    dirs64 = rng.choice(np.array([1, 2, 3, 3, 0xFF, 0], np.uint8), size=(n, 64))
    refs64 = np.stack([rng.choice(np.array(list(range(k)) * 3 + [0xFF, k], np.uint8), size=(n, 64)) for k in (n0, n1)])
    field, dirs, refs = br4.replicate3(field64, dirs64, refs64)
    got = br4.luma_picture(hmo, l0, l1, w, h, bd, field, dirs, refs, blank(w, h))
    want = pbr.pred_picture(hmo, l0, l1, w, h, bd, field64, dirs64, refs64, blank(w, h))
    assert np.array_equal(got, want) and (got != -7).any() and (got == -7).any()
    if w % 2 == 0:
        c0 = [[planes(w // 2, h // 2, bd, 50 + 5 * c + l, (n0, n1)[l]) for l in range(2)] for c in range(2)]
        got_c = br4.chroma_picture(hmo, c0, w, h, bd, field, dirs, refs, (blank(w, h, 2), blank(w, h, 2)))
        want_c = pcbr.bi_refs_picture(hmo, c0, w, h, bd, field64, dirs64, refs64, (blank(w, h, 2), blank(w, h, 2)))
        assert all(np.array_equal(a, b) for a, b in zip(got_c, want_c)) and (got_c[0] != -7).any()


# ---- the model: one reference per list is bi4_model ----------------------------------------------------------------------------------------
def test_one_reference_per_list_is_bi4_model(api, hmo):
    w, h, bd = 100, 70, 10
    n = dims(w, h)[0] * dims(w, h)[1]
    field, dirs = b4.random_field_bi4(w, h, 60)
    refs = np.zeros((2, n, 256), np.uint8)
    l0, l1 = planes(w, h, bd, 61, 1), planes(w, h, bd, 62, 1)
    assert np.array_equal(br4.luma_picture(hmo, l0, l1, w, h, bd, field, dirs, refs, blank(w, h)), b4.luma_picture(hmo, (l0[0], l1[0]), w, h, bd, field, dirs, blank(w, h)))
    cp = [[planes(w // 2, h // 2, bd, 63 + 5 * c + l, 1) for l in range(2)] for c in range(2)]
    got_c = br4.chroma_picture(hmo, cp, w, h, bd, field, dirs, refs, (blank(w, h, 2), blank(w, h, 2)))
    want_c = b4.chroma_picture(hmo, [(cp[c][0][0], cp[c][1][0]) for c in range(2)], w, h, bd, field, dirs, (blank(w, h, 2), blank(w, h, 2)))
    assert all(np.array_equal(a, b) for a, b in zip(got_c, want_c))
    # the origin: any index reads the one plane
    anyref = np.random.default_rng(64).integers(0, 256, size=(n, 256)).astype(np.uint8)
    assert np.array_equal(br4.origin_prediction(hmo, l1, w, h, bd, field[1], anyref), b4.origin_prediction(hmo, l1[0], w, h, bd, field[1]))
    # the decision: R = 1, the reference bits folded into the direction bits
    pred = sdm.predictors(n, 65)
    mv_uni, cost_uni, mv_bi, cost_bi, uni_field = b4.random_dir_tables4(n, n, 66, pred)
    rb = (2, 1)
    folded = ((3 + rb[0], 3 + rb[1], 5 + rb[0] + rb[1]), (0, 0))
    seen = set()
    for sel in (api.SelectParams(256), api.SelectParams(256, min_depth=3, max_depth=3)):
        f4, d4, s4, c4, _ = b4.select_dirs4_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, sel, w, h, folded, pred=pred)
        f, r, d, s, c = br4.select_dirs_refs4_picture(mv_uni[:, None], cost_uni[:, None], mv_bi[:, None], cost_bi[:, None], uni_field, np.zeros((2, n, 256), np.uint8), sel, w, h,
                                                      drm.Bits((3, 3, 5), (1, 1), ((rb[0],), (rb[1],))), pred=pred[:, None])
        assert np.array_equal(f, f4) and np.array_equal(d, d4) and np.array_equal(s, s4) and np.array_equal(c, c4)
        seen |= set(d.reshape(-1).tolist())
        used = np.stack([(d & (1 << l)) != 0 for l in range(2)]) & (d != 0xFF)[None]
        assert (r[used] == 0).all() and (r[~used] == 0xFF).all()
    assert {1, 2, 3} <= seen


# ---- the model: quadrant by quadrant it is four runs of the 64 models --------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in br4.FIELD_CASES if c[0] in ((101, 71), (130, 66), (16, 16))], ids=str)
def test_quadrant_by_quadrant_the_prediction_is_four_runs_of_the_64_models(hmo, case):
    (w, h), bd, (n0, n1), seed = case
    field, dirs, refs = br4.random_field_bi_refs4(w, h, n0, n1, seed)
    l0, l1 = planes(w, h, bd, seed + 1, n0), planes(w, h, bd, seed + 2, n1)
    quads = br4.quadrant_fields(field, dirs, refs)
    got = br4.luma_picture(hmo, l0, l1, w, h, bd, field, dirs, refs, blank(w, h))
    images = [pbr.pred_picture(hmo, l0, l1, w, h, bd, fq, dq, rq, blank(w, h)) for fq, dq, rq in quads]
    assert np.array_equal(got, p4.compose(images, w, h)) and (got != -7).any()
    if w % 2 == 0:
        cp = [[planes(w // 2, h // 2, bd, seed + 3 + 5 * c + l, (n0, n1)[l]) for l in range(2)] for c in range(2)]
        got_c = br4.chroma_picture(hmo, cp, w, h, bd, field, dirs, refs, (blank(w, h, 2), blank(w, h, 2)))
        images = [pcbr.bi_refs_picture(hmo, cp, w, h, bd, fq, dq, rq, (blank(w, h, 2), blank(w, h, 2))) for fq, dq, rq in quads]
        for c in range(2):
            assert np.array_equal(got_c[c], p4.compose([im[c] for im in images], w, h, 2))


# ---- the restriction and the ties, on the model -----------------------------------------------------------------------------------------------
def test_a_restricted_slot_decides_between_its_uni_candidates_alone():
    bits = drm.hm_bits(3, 3, 0b110)
    mu = [[(4, 0)] * 3, [(0, 4)] * 3]
    cu, cb = [[900, 800, 700], [100, 650, 600]], [[0, 0, 0], [0, 0, 0]]
    pred = [[(0, 0)] * 3, [(0, 0)] * 3]
    free = br4.slot_decide4(mu, cu, mu, cb, pred, bits, 1 << 16, False)
    held = br4.slot_decide4(mu, cu, mu, cb, pred, bits, 1 << 16, True)
    assert free[0] == 3 and held[0] == 2 and held[4] == (0xFF, 2)                       # list 1's reference 0 is outside the mask
    none = drm.Bits(bits.dir_bits, bits.n_refs, bits.ref_bits, 0)
    assert br4.slot_decide4(mu, cu, mu, cb, pred, none, 1 << 16, True)[0] == 1           # an empty mask: direction 1


def test_the_tie_scenarios_sit_below_and_above_256(api):
    for bits in drm.tie_bits(drm.TIE_MASK) + drm.tie_bits(0):
        tabs, placed = br4.tie_tables4(bits)
        below, above = [k for k in placed if k[1] < 256], [k for k in placed if k[1] >= 384]
        assert len(below) == 32 and above and len(below) + len(above) == len(placed)
        names = {k for k, v in drm.tie_scenarios().items() if v[0] == bits.l1_valid_mask}
        assert {placed[k] for k in below} == names and {placed[k] for k in above} == names
        seen = set()
        for sel in (api.SelectParams(256), api.SelectParams(256, min_depth=3, max_depth=3)):
            f, r, d, s, c = br4.select_dirs_refs4_picture(*tabs, sel, 128, 64, bits, lambda_q16=drm.TIE_LAMBDA_Q16)
            for ctu in range(2):
                for b in range(256):
                    key = (ctu, int(s[ctu, b]))
                    if key not in placed:
                        continue
                    seen.add(key)
                    want_d, bl, mv, want_refs = drm.tie_want(bits.l1_valid_mask, drm.tie_scenarios()[placed[key]])
                    if key[1] >= 384:                                                    # the 64 form's statement of the scenario
                        l = bl if want_d == 3 else want_d - 1
                        assert d[ctu, b] == want_d and tuple(f[l, ctu, b]) == mv and r[l, ctu, b] == want_refs[l], (placed[key], key)
                    else:
                        assert d[ctu, b] in (1, 2), (placed[key], key)                  # never bi
        assert seen == set(placed)                                                      # every site is coded in one of the two runs


# ---- the content of the GPU tests covers what it must ---------------------------------------------------------------------------------------
def test_the_random_fields_cover_directions_indices_quadrants_phases_and_far_mvs():
    for (w, h), bd, (n0, n1), seed in br4.FIELD_CASES:
        field, dirs, refs = br4.random_field_bi_refs4(w, h, n0, n1, seed)
        cov = br4.field_coverage(w, h, field, dirs, refs, n0, n1)
        if w >= 64:
            assert {1, 2, 3, 0, 0xFF} <= cov["dirs"], (w, h)
            assert cov["live_refs"][0] == set(range(n0)) and cov["live_refs"][1] == set(range(n1)), (w, h, cov["live_refs"])
            assert cov["dead_by_used_index"] and cov["live_with_unused_index_beyond"], (w, h)
            assert cov["distinct_blocks"] >= 8, (w, h, cov["distinct_blocks"])
            assert cov["far_bi"], (w, h)
        if w >= 100:
            assert all(len(p) == 16 for p in cov["phases"]), (w, h)


def test_the_end_to_end_picture_needs_this_family(api, oracle_lib, hmo):
    """on the model: at least one decided PU has a slot < 384 AND a reference index != 0, and at least one 8x8 block mixes reference indices
    -- what the 64 form cannot express"""
    w, h = br4.E2E_SIZE
    cur, lists = br4.b_refs_scene(w, h, 8, br4.E2E_SEED)
    want = br4.chain(oracle_lib, hmo, api, cur, lists, w, h, 8, br4.E2E_LAMBDA_Q16, drm.hm_bits(2, 2))
    pus, mixed = br4.beyond_the_64_form(want["slot"], want["dirs"], want["ref"])
    assert pus >= 1 and mixed >= 1, (pus, mixed)
    assert {1, 2, 3} <= set(want["dirs"].reshape(-1).tolist())
    assert (want["slot"][want["dirs"] != 0xFF] < 384).any()
