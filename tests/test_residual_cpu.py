"""Residual and per-PU / per-CU distortion without a GPU: the two names are declared, exported and bound and refuse a null context; the model
of tests/residual_model.py agrees with the oracle's hmo_had / hmo_sad on every distinct PU shape of the 593 slots; its SSE takes xGetSSE's
per-sample shift; the overflow bound include/hmme.h states holds at the 12-bit extremes.  (The refusals that need a context need a device to
make one: tests/test_gpu_residual.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import residual_model as rm

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "include", "hmme.h")
NEW = ("hmme_residual_pairs_device", "hmme_residual_frame")
ERR_ARG = -1


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return oracle_lib.oracle()


def distinct_shapes():
    from hmme import api
    return sorted({api.slot_rect(s)[2:] for s in range(593)})


def test_names_are_declared_exported_and_bound():
    from hmme import api
    L = api.load()
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", text), name
        assert name in api.SYMBOLS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert L.hmme_abi_version() == 6 and api.ABI_VERSION == 6 and "#define HMME_ABI_VERSION 6" in text
    assert callable(api.Engine.residual_pairs_device) and callable(api.Engine.residual_frame)
    assert len(L.hmme_residual_pairs_device.argtypes) == 15 and len(L.hmme_residual_frame.argtypes) == 13


def test_a_null_context_is_refused():
    from hmme import api
    L = api.load()
    fp = api.FrameParams(1, 0, 8, 0, -1)
    a = C.c_void_p(256)   # never dereferenced
    pa = (C.c_void_p * 2)(256, 256)
    for per in (64, 256, 7):
        for had in (0, 1, 2):
            assert L.hmme_residual_pairs_device(None, pa, pa, 64, 1, C.byref(fp), a, per, had, pa, 128, a, a, a, None) == ERR_ARG
            assert L.hmme_residual_frame(None, a, C.byref(fp), a, 64, a, per, had, a, 64, a, a, a) == ERR_ARG
    assert L.hmme_residual_pairs_device(None, None, None, 0, 0, None, None, 64, 1, None, 0, None, None, None, None) == ERR_ARG
    assert L.hmme_residual_frame(None, None, None, None, 0, None, 64, 1, None, 0, None, None, None) == ERR_ARG


def test_the_593_slots_have_the_24_shapes_the_rule_speaks_of():
    shapes = distinct_shapes()
    assert len(shapes) == 24
    assert {(12, 16), (16, 4), (8, 4), (24, 32), (32, 8)} <= set(shapes)
    small = {s for s in shapes if s[0] % 8 or s[1] % 8}
    assert small == {(8, 4), (4, 8), (16, 4), (16, 12), (4, 16), (12, 16)}     # the shapes of slots 0..383 but the 8x8 2Nx2N: 4x4 Hadamards


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_model_agrees_with_the_oracle_on_every_pu_shape(hmo, bd):
    rng = np.random.default_rng(900 + bd)
    maxv = (1 << bd) - 1
    for w, h in distinct_shapes():
        for kind in ("noise", "binary"):
            if kind == "noise":
                cur, pred = rng.integers(0, maxv + 1, size=(2, 64, 64))
            else:
                cur, pred = (np.where(rng.integers(0, 2, size=(64, 64)) == 1, maxv, 0) for _ in range(2))
            c, p = rm.extended(cur, pred, 64, 64)
            x, y = int(rng.integers(0, (64 - w) // 4 + 1)) * 4, int(rng.integers(0, (64 - h) // 4 + 1)) * 4
            d = c[y:y + h, x:x + w].astype(np.int64) - p[y:y + h, x:x + w]
            assert rm.pu_error(hmo, c, p, x, y, w, h, bd, True) == rm.had_rule(d, bd), (w, h, kind)
            assert rm.pu_error(hmo, c, p, x, y, w, h, bd, False) == int(np.abs(d).sum()) >> (bd - 8), (w, h, kind)


def test_the_quadrant_butterfly_gives_the_8x8_sum():
    rng = np.random.default_rng(77)
    for k in range(50):
        d = rng.integers(-4095, 4096, size=(8, 8))
        if k % 5 == 0:
            d = np.where(d > 0, 4095, -4095)
        assert rm.had8_from_quadrants(d) == rm.had_abs_sum(d)


def test_the_difference_is_zero_outside_the_picture(hmo):
    rng = np.random.default_rng(5)
    w, h = 100, 70
    cur, pred = rng.integers(0, 256, size=(2, h, w))
    d = rm.difference(cur, pred, w, h)
    assert d.shape == (128, 128) and (d[h:] == 0).all() and (d[:, w:] == 0).all() and np.array_equal(d[:h, :w], cur - pred)
    # a PU that straddles the edge: only its part inside the picture counts
    c, p = rm.extended(cur, pred, w, h)
    inside = int(np.abs(cur[64:70, 96:100].astype(np.int64) - pred[64:70, 96:100]).sum())
    assert rm.pu_error(hmo, c, p, 96, 64, 8, 8, 8, False) == inside and inside > 0
    res, pu, cu, ctu = rm.residual_picture(hmo, cur, pred, w, h, 8, None, 64, False)
    assert np.array_equal(res, cur - pred) and pu[3, 8 * 0 + 4] == inside and (pu[3, 8:] == 0).all() and (cu[1, 5:8] == 0).all()
    assert ctu[3, 0] == pu[3].sum() and ctu[3, 1] == cu[3].sum() == rm.sse(d[64:, 64:], 8)


def test_sse_shifts_every_sample(hmo):
    """10-bit differences below 4 vanish one by one under xGetSSE's shift and would not if the total were shifted"""
    rng = np.random.default_rng(11)
    d = rng.integers(-3, 4, size=(16, 16))
    assert rm.sse(d, 10) == 0 and rm.sse_shifted_total(d, 10) > 0
    cur = rng.integers(0, 1024, size=(64, 64))
    pred = np.clip(cur + rng.integers(-9, 10, size=(64, 64)), 0, 1023)
    dd = cur - pred
    per_sample = sum((int(v) * int(v)) >> 4 for v in dd.reshape(-1))
    assert rm.sse(dd, 10) == per_sample != rm.sse_shifted_total(dd, 10)
    # ... and through the model's CU sums, with one 64x64 CU
    _, pu, cu, ctu = rm.residual_picture(hmo, cur, pred, 64, 64, 10, np.full((1, 64), 592, np.uint16), 64, True)
    assert (cu == per_sample).all() and ctu[0, 1] == per_sample and (pu == pu[0, 0]).all() and ctu[0, 0] == pu[0, 0]
    assert rm.sse(dd, 8) == int((dd.astype(np.int64) ** 2).sum())


def test_the_overflow_bound_holds_at_the_12_bit_extremes(hmo):
    maxv = 4095
    bound = 64 * ((64 * 64 * maxv + 2) >> 2)
    assert bound < 1 << 32 and 4096 * ((maxv * maxv) >> 8) < 1 << 32 and 4096 * 255 * 255 < 1 << 32
    rng = np.random.default_rng(12)
    ys, xs = np.mgrid[0:64, 0:64]
    patterns = [np.full((64, 64), maxv), np.where((xs + ys) & 1, maxv, -maxv), np.where(xs & 1, maxv, -maxv), np.where((xs >> 2 ^ ys >> 2) & 1, maxv, -maxv),
                np.where(rng.integers(0, 2, size=(64, 64)) == 1, maxv, -maxv)]
    for d in patterns:
        total, shifted = rm.had_rule(d, 12, wide=True)
        assert total <= bound and shifted == total >> 4
        cur, pred = np.where(d > 0, maxv, 0), np.where(d > 0, 0, maxv)
        c, p = rm.extended(cur, pred, 64, 64)
        assert rm.pu_error(hmo, c, p, 0, 0, 64, 64, 12, True) == shifted            # the oracle's uint32 did not wrap either
        assert rm.pu_error(hmo, c, p, 0, 0, 64, 64, 12, False) == (4096 * maxv) >> 4
        assert rm.sse(d, 12) == 4096 * ((maxv * maxv) >> 8)
    # every 8x8 block's sum stays below the per-block term of the bound (Parseval: sum |coef| <= 8 * 64 * maxv)
    assert all(rm.had_abs_sum(d[:8, :8]) <= 64 * 64 * maxv // 8 for d in patterns)
