"""Bi-prediction on whole pictures, the part that needs no GPU: hmme_bipred_check -- the refusal rule of the *_bi_* and predict calls, a
pure host function -- against a table computed here from the bounds as include/hmme.h states them; the new names declared, exported
and bound; and every new entry point refusing a null context without touching a device."""
import os
import re

import pytest

from conftest import ROOT

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -5
INV_COST16 = 8000000   # the engine's cost field ("8 000 000" in include/hmme.h)

NAMES = ["hmme_bipred_check", "hmme_predict_pairs_device", "hmme_predict_frame", "hmme_search_pairs_bi_device", "hmme_refine_pairs_bi_device",
         "hmme_search_frame_bi", "hmme_refine_frame_bi"]


def expected(bit_depth, refine):
    """the rule of include/hmme.h: origin 2 * cur - pred in [-maxv, 2 maxv], staged with the bias maxv next to a reference in [0, maxv]"""
    if bit_depth < 8 or bit_depth > 12:
        return ERR_ARG
    maxv = (1 << bit_depth) - 1
    if 2 * maxv + maxv > 65535:                      # the 16-bit search's sample span
        return ERR_UNSUPPORTED
    span = max(2 * maxv - 0, maxv - (-maxv))         # largest |origin - reference sample|
    if ((4096 * span) >> (bit_depth - 8)) + 65535 >= INV_COST16:
        return ERR_UNSUPPORTED
    if refine and 4096 * span >= 1 << 24:            # the refinement's exact-sum bound (the one hmme_weight_check states)
        return ERR_UNSUPPORTED
    return OK


def test_bipred_check_follows_the_stated_bounds():
    from hmme import api
    api.build()
    for bd in (8, 10):
        for refine in (0, 1):
            assert expected(bd, refine) == OK and api.bipred_check(bd, refine) == OK   # must be served in both modes
    for bd in (7, 13, 0, -3, 16):
        for refine in (0, 1):
            assert api.bipred_check(bd, refine) == ERR_ARG
    for bd in (9, 11, 12):
        for refine in (0, 1):
            assert api.bipred_check(bd, refine) == expected(bd, refine), (bd, refine)
    # the one refusal the bounds produce: 12-bit refinement (sample differences up to 8190 >= 4096)
    assert expected(12, 0) == OK and expected(12, 1) == ERR_UNSUPPORTED and expected(11, 1) == OK


def test_the_header_table_is_the_rule():
    """the table written into include/hmme.h says what the bounds give"""
    header = open(os.path.join(ROOT, "include", "hmme.h")).read()
    depths = re.search(r"bit depth\s+8\s+9\s+10\s+11\s+12\s*\n", header)
    assert depths, "include/hmme.h carries no bit-depth table for hmme_bipred_check"
    rows = header[depths.end():].split("\n")[:2]
    for refine, row in enumerate(rows):
        assert re.search(r"refine = %d" % refine, row), row
        cells = re.findall(r"\b(ok|HMME_ERR_UNSUPPORTED|HMME_ERR_ARG)\b", row.split("refine = %d" % refine)[1])
        assert len(cells) == 5, row
        for bd, cell in zip((8, 9, 10, 11, 12), cells):
            assert {"ok": OK, "HMME_ERR_UNSUPPORTED": ERR_UNSUPPORTED, "HMME_ERR_ARG": ERR_ARG}[cell] == expected(bd, refine), (bd, refine, cell)


def test_the_new_names_are_declared_exported_and_bound():
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
    for method in ("predict_pairs_device", "predict_frame", "search_pairs_bi_device", "refine_pairs_bi_device", "search_frame_bi", "refine_frame_bi"):
        assert callable(getattr(api.Engine, method))
    assert callable(api.bipred_check)
    assert re.search(r"#define HMME_ABI_VERSION 6\b", header) and L.hmme_abi_version() == 6   # new functions only: the version stays


def test_a_null_context_is_refused_by_every_new_entry_point():
    """HMME_ERR_ARG before anything else is looked at: no device is touched (this test runs where there is none)"""
    import ctypes as C
    from hmme import api
    api.build()
    L = api.load()
    fp = api.FrameParams(4, 1, 8, 0, -1)
    one = (C.c_void_p * 1)(None)
    assert L.hmme_predict_pairs_device(None, one, 1, C.byref(fp), None, 1, one, 0, None) == ERR_ARG
    assert L.hmme_predict_frame(None, None, C.byref(fp), None, 1, None, 0) == ERR_ARG
    assert L.hmme_search_pairs_bi_device(None, one, one, one, 1, C.byref(fp), None, 1, None, None, None, None, None) == ERR_ARG
    assert L.hmme_refine_pairs_bi_device(None, one, one, one, 1, C.byref(fp), None, 1, None, None, None, 1, None, None, None) == ERR_ARG
    assert L.hmme_search_frame_bi(None, None, None, None, C.byref(fp), None, 1, None, None, None, None) == ERR_ARG
    assert L.hmme_refine_frame_bi(None, None, None, None, C.byref(fp), None, 1, None, None, None, 1, None, None) == ERR_ARG
