"""Weighted prediction on whole pictures, the part that needs no GPU: hmme_weight_check -- the refusal rule of
hmme_search_pairs_w_device / hmme_refine_pairs_w_device, a pure host function -- against a table computed here from the rule as
include/hmme.h states it, and the five new names declared, exported and bound."""
import os
import re

import pytest

from conftest import ROOT

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
INV_COST16 = 8000000   # the engine's cost field (me_kernels.hpp kInvCost16; "8 000 000" in include/hmme.h)


def expected(bit_depth, wp, refine):
    """the rule of include/hmme.h from the nominal range [0, 2^bitDepth - 1] of both pictures"""
    w0, offset, shift, rnd = wp
    if shift < 0 or shift > 15:
        return ERR_ARG
    maxv = (1 << bit_depth) - 1
    ends = [((w0 * v + rnd) >> shift) + offset for v in (0, maxv)]   # monotonic in v: the extremes are at the ends of the range
    wlo, whi = min(ends), max(ends)
    if wlo < -32768 or whi > 32767:
        return ERR_UNSUPPORTED
    bias = max(0, -wlo)
    if max(whi, maxv) + bias > 65535:
        return ERR_UNSUPPORTED
    span = max(maxv - wlo, whi - 0)   # largest |block - weighted sample|
    if ((4096 * span) >> (bit_depth - 8)) + 65535 >= INV_COST16:
        return ERR_UNSUPPORTED
    if refine and 4096 * span >= 1 << 24:
        return ERR_UNSUPPORTED
    return OK


def identity(shift):
    return (1 << shift, 0, shift, (1 << (shift - 1)) if shift else 0)


WEIGHTS = [identity(0), identity(6), identity(7),
           (40, 12, 6, 32),        # a fade
           (88, -20, 6, 32),       # a fade up with a negative offset
           (-24, 300, 5, 16),      # a negative weight
           (-64, 0, 6, 32),        # ... whose weighted samples all go negative (bias > 0)
           (3, -5, 0, 0),          # shift 0
           (1 << 15, 0, 15, 1 << 14),
           (1, 0, 16, 0), (64, 0, 16, 1 << 15), (64, 0, -1, 0),   # shift outside 0..15
           (300, 0, 0, 0),         # 300 * 255 > 32767: beyond int16 at every bit depth
           (100, 0, 0, 0),         # ... 100 * 255 is not, 100 * 1023 is
           (64, 30000, 6, 32),     # the offset alone carries it beyond int16 at 12 bit, beyond the cost field below
           (64, 100, 6, 32),       # 12 bit: passes for the search, too wide for the refinement (4096 * 4195 >= 2^24)
           (64, 2000, 6, 32),
           (-64, -100, 6, 32)]


@pytest.mark.parametrize("bit_depth", [8, 10, 12])
def test_weight_check_follows_the_stated_rule(bit_depth):
    from hmme import api
    api.build()
    seen = set()
    for wp in WEIGHTS:
        for refine in (0, 1):
            want = expected(bit_depth, wp, refine)
            got = api.weight_check(bit_depth, wp, refine)
            assert got == want, f"bit depth {bit_depth}, weight {wp}, refine {refine}: hmme_weight_check {got}, the rule says {want}"
            seen.add(want)
    assert seen == {OK, ERR_ARG, ERR_UNSUPPORTED}   # the table exercises every answer at every bit depth


def test_weight_check_named_cases():
    from hmme import api
    api.build()
    for bd in (8, 10, 12):
        for sh in (0, 6, 7, 15):
            assert api.weight_check(bd, identity(sh), 0) == OK and api.weight_check(bd, identity(sh), 1) == OK
        assert api.weight_check(bd, (40, 12, 6, 32), 1) == OK                    # the fade
        assert api.weight_check(bd, (-24, 300, 5, 16), 0) == OK                  # a negative weight is served
        assert api.weight_check(bd, (3, -5, 0, 0), 0) == OK                      # shift 0
        assert api.weight_check(bd, (64, 0, 16, 1 << 15), 0) == ERR_ARG          # shift 16
        assert api.weight_check(bd, (300, 0, 0, 0), 0) == ERR_UNSUPPORTED        # a weighted sample beyond int16
    # passes for the search and fails for the refinement
    assert api.weight_check(12, (64, 100, 6, 32), 0) == OK
    assert api.weight_check(12, (64, 100, 6, 32), 1) == ERR_UNSUPPORTED
    # the same weight on tame bit depths is refined
    assert api.weight_check(8, (64, 100, 6, 32), 1) == OK and api.weight_check(10, (64, 100, 6, 32), 1) == OK
    # the cost field: 10-bit samples against a prediction 7000 away
    assert expected(10, (64, 7000, 6, 32), 0) == ERR_UNSUPPORTED and api.weight_check(10, (64, 7000, 6, 32), 0) == ERR_UNSUPPORTED
    # beyond the stated rule, the engine's own exactness bound: the refinement weights in fp32, exact while |w0 * sample + round| < 2^24
    # (identity weights run the unweighted kernel and are exempt)
    assert expected(10, (1 << 15, 1, 15, 1 << 14), 1) == OK
    assert api.weight_check(10, (1 << 15, 1, 15, 1 << 14), 0) == OK
    assert api.weight_check(10, (1 << 15, 1, 15, 1 << 14), 1) == ERR_UNSUPPORTED
    assert api.weight_check(10, identity(15), 1) == OK
    # a null weight
    assert api.load().hmme_weight_check(8, None, 0) == ERR_ARG
    # bit depths the engine does not serve
    assert api.weight_check(7, identity(6), 0) == ERR_UNSUPPORTED and api.weight_check(13, identity(6), 0) == ERR_UNSUPPORTED


NAMES = ["hmme_weight_check", "hmme_search_pairs_w_device", "hmme_refine_pairs_w_device", "hmme_search_frame_w", "hmme_refine_frame_w"]


def test_the_five_names_are_declared_exported_and_bound():
    from hmme import api
    api.build()
    L = api.load()
    header = open(os.path.join(ROOT, "include", "hmme.h")).read()
    declared = set(re.findall(r"\b(hmme_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/hmme.h"
        assert hasattr(L, name), f"libhmme.so does not export {name}"
        assert name in api.SYMBOLS
        assert getattr(L, name).argtypes is not None, f"api.py binds no argument types for {name}"
    for method in ("search_frame_w", "refine_frame_w", "search_pairs_w_device", "refine_pairs_w_device"):
        assert callable(getattr(api.Engine, method))
    assert callable(api.weight_check)
    assert re.search(r"#define HMME_ABI_VERSION 6\b", header) and L.hmme_abi_version() == 6   # new functions only: the version stays


def test_run_rank_takes_weights():
    import inspect
    from hmme import sequence
    p = inspect.signature(sequence.run_rank).parameters["weights"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
