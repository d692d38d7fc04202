"""Prediction from one MV per 4x4 block (hmme_predict_refs4_* / hmme_predict_chroma_refs4_*), the part that needs no GPU: the four names
declared, exported and bound; a NULL context; the model tests/predict4_model.py against the models of the 64 forms -- on replicated fields
the whole picture, on 4x4 fields quadrant by quadrant; and the proof that the table recipe of the end-to-end test in
tests/test_gpu_predict4.py really chooses the shapes only the 256 layout can hold."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bipred_wp_model as bwm
import predict4_model as p4
import predict_chroma_model as cm
import select_model as sm
from conftest import ROOT
from frame_helpers import bind_hmo, dims, random_field

ERR_ARG = -1
NAMES = ["hmme_predict_refs4_device", "hmme_predict_refs4_frame", "hmme_predict_chroma_refs4_device", "hmme_predict_chroma_refs4_frame"]


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


def test_the_new_names_are_declared_exported_and_bound(api):
    L = api.load()
    header = open(os.path.join(ROOT, "include", "hmme.h")).read()
    declared = set(re.findall(r"\b(hmme_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/hmme.h"
        assert hasattr(L, name), f"libhmme.so does not export {name}"
        assert name in api.SYMBOLS
        assert getattr(L, name).argtypes is not None, f"api.py binds no argument types for {name}"
    for method in ("predict_refs4_device", "predict_refs4_frame", "predict_chroma_refs4_device", "predict_chroma_refs4_frame"):
        assert callable(getattr(api.Engine, method))
    assert re.search(r"#define HMME_ABI_VERSION 6\b", header) and L.hmme_abi_version() == 6 and api.ABI_VERSION == 6   # new functions only


def test_a_null_context_is_refused_by_every_new_entry_point(api):
    """HMME_ERR_ARG before anything else is looked at: no device is touched (this test runs where there is none)"""
    L = api.load()
    fp = api.FrameParams(1, 0, 8, 0, -1)
    assert L.hmme_predict_refs4_device(None, None, 1, C.byref(fp), None, None, None, None, 64, None) == ERR_ARG
    assert L.hmme_predict_refs4_frame(None, None, 1, C.byref(fp), None, None, None, None, 64) == ERR_ARG
    assert L.hmme_predict_chroma_refs4_device(None, None, 1, 64, 64, C.byref(fp), None, None, None, None, None, 32, None) == ERR_ARG
    assert L.hmme_predict_chroma_refs4_frame(None, None, 1, 64, 64, C.byref(fp), None, None, None, None, 32) == ERR_ARG


def test_replicate_and_quadrant_fields_are_inverse():
    rng = np.random.default_rng(5)
    f64 = rng.integers(-99, 100, size=(3, 64, 2)).astype(np.int16)
    r64 = rng.integers(0, 4, size=(3, 64)).astype(np.uint8)
    f, r = p4.replicate(f64), p4.replicate(r64)
    assert f.shape == (3, 256, 2) and r.shape == (3, 256) and p4.mixed_blocks(f, r) == 0
    for b in range(256):
        x, y = p4.block_xy(b)
        assert np.array_equal(f[:, b], f64[:, (y // 8) * 8 + x // 8]) and np.array_equal(r[:, b], r64[:, (y // 8) * 8 + x // 8])
    for fq, rq in p4.quadrant_fields(f, r):
        assert np.array_equal(fq, f64) and np.array_equal(rq, r64)
    f4 = rng.integers(-99, 100, size=(3, 256, 2)).astype(np.int16)
    r4 = rng.integers(0, 4, size=(3, 256)).astype(np.uint8)
    for q, (fq, rq) in enumerate(p4.quadrant_fields(f4, r4)):
        for b8 in range(64):
            b = (2 * (b8 >> 3) + (q >> 1)) * 16 + 2 * (b8 & 7) + (q & 1)
            assert np.array_equal(fq[:, b8], f4[:, b]) and np.array_equal(rq[:, b8], r4[:, b])
    assert p4.mixed_blocks(f4, r4) == 3 * 64


def luma_64(hmo, refs, w, h, bd, field64, ref64, wps=None):
    """the luma picture of the 64 form with a reference per block, from bipred_wp_model.pred_picture reference by reference: int64 [h, w], -1
    where no reference writes"""
    cx_n, cy_n = dims(w, h)
    out = np.full((cy_n * 64, cx_n * 64), -1, np.int64)
    for r, ref in enumerate(refs):
        pic = bwm.pred_picture(hmo, ref, w, h, bd, field64, bwm.IDENT if wps is None else wps[r])
        for ctu in range(cx_n * cy_n):
            for b in np.flatnonzero(ref64[ctu] == r):
                x, y = (ctu % cx_n) * 64 + (b & 7) * 8, (ctu // cx_n) * 64 + (b >> 3) * 8
                out[y:y + 8, x:x + 8] = pic[y:y + 8, x:x + 8]
    return out[:h, :w]


def test_the_model_on_a_replicated_field_is_the_luma_model_of_the_64_form(hmo):
    w, h, bd = 101, 71, 8
    n = dims(w, h)[0] * dims(w, h)[1]
    refs = planes(w, h, bd, 40, 2)
    field64 = random_field(n, 64, 41, max_pel=20)
    ref64 = np.random.default_rng(42).choice(np.array([0, 1, 1, 0xFF, 2], np.uint8), size=(n, 64))
    for wps in (None, [(70, -3, 6, 32), bwm.IDENT]):
        got = p4.luma_picture(hmo, refs, w, h, bd, p4.replicate(field64), p4.replicate(ref64), np.full((h, w), -1, np.int64), wps)
        assert np.array_equal(got, luma_64(hmo, refs, w, h, bd, field64, ref64, wps))
    assert (got == -1).any() and (got != -1).any()
    one = p4.luma_picture(hmo, refs[:1], w, h, bd, p4.replicate(field64), None, np.full((h, w), -1, np.int64))      # no reference field: index 0
    assert np.array_equal(one, bwm.pred_picture(hmo, refs[0], w, h, bd, field64, bwm.IDENT)[:h, :w])


@pytest.mark.parametrize("size", [(130, 66), (100, 70)])
def test_the_model_on_a_replicated_field_is_the_chroma_model_of_the_64_form(hmo, size):
    w, h = size
    bd = 10
    n = dims(w, h)[0] * dims(w, h)[1]
    comps = [planes(w // 2, h // 2, bd, 50 + 5 * c, 2) for c in range(2)]
    field64 = random_field(n, 64, 51, max_pel=20)
    ref64 = np.random.default_rng(52).choice(np.array([0, 1, 1, 0xFF, 2], np.uint8), size=(n, 64))
    wps = [[(64 + 5 * r + 3 * c, 4 * (r - c), 6, 32) for r in range(2)] for c in range(2)]
    fill = lambda: tuple(np.full((h // 2, w // 2), -1, np.int64) for _ in range(2))
    for weights in (None, wps):
        got = p4.chroma_picture(hmo, comps, w, h, bd, p4.replicate(field64), p4.replicate(ref64), fill(), weights)
        want = cm.refs_picture(hmo, comps, w, h, bd, field64, ref64, fill(), weights)
        assert all(np.array_equal(got[c], want[c]) for c in range(2))
    assert (got[0] == -1).any() and (got[0] != -1).any() and not np.array_equal(got[0], got[1])


def test_quadrant_q_of_the_model_is_the_64_model_on_the_quadrant_field(hmo):
    w, h, bd = 100, 70, 8
    refs = planes(w, h, bd, 60, 2)
    comps = [planes(w // 2, h // 2, bd, 65 + 5 * c, 2) for c in range(2)]
    field, ref = p4.random_field4(w, h, 2, 61)
    got = p4.luma_picture(hmo, refs, w, h, bd, field, ref, np.full((h, w), -1, np.int64))
    got_c = p4.chroma_picture(hmo, comps, w, h, bd, field, ref, tuple(np.full((h // 2, w // 2), -1, np.int64) for _ in range(2)))
    for q, (fq, rq) in enumerate(p4.quadrant_fields(field, ref)):
        m = p4.quadrant_mask(w, h, q)
        want = luma_64(hmo, refs, w, h, bd, fq, rq)
        # a quadrant that starts outside the picture is dead in the 256 layout, while its 8x8 block may be live in the 64 form: only
        # quadrants inside the picture are compared, and those are all of a picture's samples
        assert np.array_equal(got[m], want[m]), q
        want_c = cm.refs_picture(hmo, comps, w, h, bd, fq, rq, tuple(np.full((h // 2, w // 2), -1, np.int64) for _ in range(2)))
        mc = p4.quadrant_mask(w, h, q, 2)
        assert all(np.array_equal(got_c[c][mc], want_c[c][mc]) for c in range(2)), q
    assert (got == -1).any() and (got != -1).any()


@pytest.mark.parametrize("depth", [3, 2])
def test_the_end_to_end_recipe_chooses_the_small_shapes(api, depth):
    """select_model.random_tables(2, 7) on 128 x 64 with mv_per_ctu = 256 and the depth forced: at depth 3 the 8x8 CUs split into 2NxN and
    Nx2N (8x4 / 4x8 PUs), at depth 2 all four AMP PartSizes occur (16x4, 16x12, 4x16, 12x16 PUs); either way at least 20 of the 128 8x8
    blocks hold 4x4 entries that differ -- what no 64-entry field can carry"""
    mv, cost = sm.random_tables(2, 7)
    field, slot, _, leaves = sm.select_picture(mv, cost, api.SelectParams(256, min_depth=depth, max_depth=depth), 128, 64)
    sizes = {ps for d, ps in leaves if d == depth}
    assert all(d == depth for d, _ in leaves)
    if depth == 3:
        assert {1, 2} <= sizes, sizes
    else:
        assert {4, 5, 6, 7} <= sizes, sizes
    assert p4.mixed_blocks(field, np.zeros(field.shape[:2], np.uint8)) >= 20
