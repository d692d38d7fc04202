"""The partition decision over the 593-slot tables (hmme_select_*), the part that needs no GPU: the new names declared, exported and bound;
every entry point with a context refusing a null one; hmme_select_check against the ranges include/hmme.h states; hmme_slot_key as the
inverse of hmme_slot_index; and the `select` argument of sequence.run_rank (plumbing only: nothing here touches a device)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import lambda_cases as lc
import select_model as sm
from conftest import ROOT

OK, ERR_ARG = 0, -1
NAMES = ["hmme_select_check", "hmme_select_pairs_device", "hmme_select_frame", "hmme_slot_key"]


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
    assert re.search(r"typedef struct hmme_select_params \{", header)
    for method in ("select_pairs_device", "select_frame"):
        assert callable(getattr(api.Engine, method))
    assert callable(api.select_check) and callable(api.slot_key)
    assert [f[0] for f in api.SelectParams._fields_] == ["mv_per_ctu", "mv_unit", "price_mv", "part_mask", "min_depth", "max_depth", "cu_cost", "pu_cost"]
    assert C.sizeof(api.SelectParams) == 32
    assert re.search(r"#define HMME_ABI_VERSION 6\b", header) and L.hmme_abi_version() == 6 and api.ABI_VERSION == 6   # new functions and one new struct only


def test_a_null_context_is_refused_by_every_new_entry_point(api):
    """HMME_ERR_ARG before anything else is looked at: no device is touched (this test runs where there is none)"""
    L = api.load()
    fp = api.FrameParams(1, 0, 8, 0, -1)
    sel = api.SelectParams(64)
    assert api.select_check(sel) == OK
    assert L.hmme_select_pairs_device(None, 64, 64, 1, C.byref(fp), C.byref(sel), None, None, None, None, None, None, None) == ERR_ARG
    assert L.hmme_select_frame(None, 64, 64, C.byref(fp), C.byref(sel), None, None, None, None, None, None) == ERR_ARG


def test_select_check_follows_the_stated_ranges(api):
    def check(**kw):
        return api.select_check(api.SelectParams(**kw))

    assert api.load().hmme_select_check(None) == ERR_ARG
    for per in (64, 256):
        assert check(mv_per_ctu=per) == OK
    for per in (1, 128, 0, -64, 63, 65, 512):
        assert check(mv_per_ctu=per) == ERR_ARG, per
    for unit, price in ((0, 0), (0, 1), (1, 0), (1, 1)):
        assert check(mv_unit=unit, price_mv=price) == OK
    for v in (-1, 2, 64):
        assert check(mv_unit=v) == ERR_ARG and check(price_mv=v) == ERR_ARG
    for mask in (0x01, 0x07, 0xF7, 0xF1, 0x11, 0x83):
        assert check(part_mask=mask) == OK, hex(mask)
    for mask in (0x00, 0x06, 0xF6, 0x80, 0x09, 0xFF, 0x101, 0x80000001):   # bit 0 missing; NxN (bit 3) or a bit above 7 set
        assert check(part_mask=mask) == ERR_ARG, hex(mask)
    for lo in range(4):
        for hi in range(4):
            assert check(min_depth=lo, max_depth=hi) == (OK if lo <= hi else ERR_ARG), (lo, hi)
    for lo, hi in ((-1, 3), (0, 4), (4, 4), (-2, -1)):
        assert check(min_depth=lo, max_depth=hi) == ERR_ARG, (lo, hi)
    for v in (0, 1, 1 << 20):
        assert check(cu_cost=v) == OK and check(pu_cost=v) == OK and check(cu_cost=v, pu_cost=v) == OK
    for v in ((1 << 20) + 1, 1 << 21, 0xFFFFFFFF):
        assert check(cu_cost=v) == ERR_ARG and check(pu_cost=v) == ERR_ARG, v


def test_slot_key_is_the_inverse_of_slot_index(api):
    L = api.load()
    seen = {}
    for ps in (0, 1, 2, 4, 5, 6, 7):
        for depth in range(4):
            for idx in range(2):
                for z in range(256):
                    s = api.slot_index(ps, depth, idx, z)
                    if s < 0:
                        continue
                    assert s not in seen, (s, seen[s], (ps, depth, idx, z))
                    seen[s] = (ps, depth, idx, z)
                    assert api.slot_key(s) == (ps, depth, idx, z)
    assert sorted(seen) == list(range(593))
    out = [C.c_int(-7) for _ in range(4)]
    for bad in (-1, 593, 1 << 20):
        assert L.hmme_slot_key(bad, *[C.byref(o) for o in out]) == ERR_ARG
        assert [o.value for o in out] == [-7] * 4   # nothing written
        with pytest.raises(api.HmmeError):
            api.slot_key(bad)
    assert L.hmme_slot_key(0, None, None, None, None) == ERR_ARG


def test_run_rank_select_defaults_to_none_and_is_checked_before_any_device(api):
    from hmme import sequence
    params = inspect.signature(sequence.run_rank).parameters
    # the signature as it was, then the one new keyword: callers that do not name it get what they got before
    assert list(params)[:7] == ["eng", "source", "pairs", "width", "height", "bit_depth", "search_range"]
    old_keywords = {"stream_mode": False, "pairs_per_launch": 1, "refine": False, "download": False, "n_slots": None, "device": None, "host_buffers": 4,
                    "resources": None, "weights": None}
    for name, default in old_keywords.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default, name
    assert params["select"].kind is inspect.Parameter.KEYWORD_ONLY and params["select"].default is None
    assert set(params) == set(list(params)[:7]) | set(old_keywords) | {"select"}
    # a SelectParams that does not fit the tables it would read is refused by argument checks alone (no engine, no source, no torch device)
    with pytest.raises(ValueError):   # the search's tables are pure SADs at integer MVs
        sequence.run_rank(None, None, [(1, 0)], 64, 64, 8, 8, refine=False, select=api.SelectParams(64, mv_unit=0, price_mv=0))
    with pytest.raises(ValueError):
        sequence.run_rank(None, None, [(1, 0)], 64, 64, 8, 8, refine=False, select=api.SelectParams(64, mv_unit=1, price_mv=0))
    with pytest.raises(ValueError):   # the refinement's MVs are quarter-pel
        sequence.run_rank(None, None, [(1, 0)], 64, 64, 8, 8, refine=True, select=api.SelectParams(64, mv_unit=1, price_mv=0))
    with pytest.raises(ValueError):   # outside hmme_select_check's ranges
        sequence.run_rank(None, None, [(1, 0)], 64, 64, 8, 8, refine=True, select=api.SelectParams(128))


# ---- the MV cost where its product wraps (tests/lambda_cases.py) -----------------------------------------------------------------------
def _wide(lq, x, y, px, py, scale):
    """the MV cost from a 64-bit product: what the rule does NOT say"""
    return lc.get_cost_64(lq, lc.mv_bits(x << scale, y << scale, px, py))


def _wrapped(lq, x, y, px, py, scale):
    return lc.get_cost(lq, lc.mv_bits(x << scale, y << scale, px, py))


@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("lq", lc.LAMBDA_Q16)
def test_the_model_prices_mvs_with_the_wrapping_product(api, oracle_lib, lq, unit):
    """select_model with the oracle's hmo_mv_cost == with tests/lambda_cases.py's Python restatement, at every lambda of the set, far predictors"""
    L = oracle_lib.oracle()
    mv, cost = sm.random_tables(2, seed=91, noise=64)
    pred = np.array([[-1900, 1733], [37, -1012]], np.int16)
    sel = api.SelectParams(64, mv_unit=unit, price_mv=1, cu_cost=40, pu_cost=12)
    a = sm.select_picture(mv, cost, sel, 128, 64, 0, pred, lq, lambda *v: L.hmo_mv_cost(*v))
    b = sm.select_picture(mv, cost, sel, 128, 64, 0, pred, lq, _wrapped)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    bits = [lc.mv_bits(int(v[0]) << (2 * unit), int(v[1]) << (2 * unit), *pred[k]) for k in range(2) for v in mv[k]]
    if lq in lc.WRAPPING:
        assert any(lc.wraps(lq, n) for n in bits)
        assert not np.array_equal(sm.select_picture(mv, cost, sel, 128, 64, 0, pred, lq, _wide)[2], a[2])


def test_the_wrap_changes_the_partition_by_hand(api):
    """one 64x64 CU, 2Nx2N or 2NxN, lambda_q16 = 178956971 = ceil(2^32 / 24).  2Nx2N: cost 1000 at MV (1024, 0) quarter pels -- 23 + 1 = 24 bits,
    24 * 178956971 = 2^32 + 8, wrapped >> 16 = 0: 1000 in all.  2NxN: 400 per PU at MV (0, 0) -- 2 bits, 357913942 >> 16 = 5461: 2 * (400 + 5461)
    = 11722.  HM's wrapping product codes 2Nx2N; a 64-bit product would price the 24 bits at 65536 and code 2NxN"""
    assert lc.mv_bits(1024, 0, 0, 0) == 24 and lc.get_cost(lc.WRAP24, 24) == 0 and lc.get_cost_64(lc.WRAP24, 24) == 65536 and lc.get_cost(lc.WRAP24, 2) == 5461
    whole, (top, bottom) = api.slot_index(0, 0, 0, 0), (api.slot_index(1, 0, i, 0) for i in range(2))
    mv, cost = np.zeros((593, 2), np.int16), np.full(593, 1 << 20, np.uint32)
    mv[whole], cost[whole], cost[top], cost[bottom] = (1024, 0), 1000, 400, 400
    sel = api.SelectParams(64, price_mv=1, part_mask=0x03, max_depth=0)
    _, slot, total, leaves = sm.select_ctu(mv, cost, sel, 0, 0, 64, 64, (0, 0), lc.WRAP24, _wrapped)
    assert (total, leaves) == (1000, [(0, 0)]) and set(slot.tolist()) == {whole}
    _, slot, total, leaves = sm.select_ctu(mv, cost, sel, 0, 0, 64, 64, (0, 0), lc.WRAP24, _wide)
    assert (total, leaves) == (11722, [(0, 1)]) and set(slot.tolist()) == {top, bottom}
