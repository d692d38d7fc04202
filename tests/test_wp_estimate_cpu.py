"""The weighted-prediction estimator without a GPU: the numpy model of HM's WeightPredAnalysis (tests/wp_estimate_model.py) on pictures whose
numbers can be checked by hand, and the host-only behaviour of the new ABI (symbols, struct layout, refusals that need no context)."""
import ctypes as C
import math

import numpy as np

import wp_estimate_model as model


pictures = model.pictures


def test_checkerboard_intermediates():
    cur, ref = pictures("checkerboard")
    n = cur.size
    assert n % 2 == 0
    (cs, cac), (rs, rac) = model.plane_stats(cur), model.plane_stats(ref)
    assert model.norm_dc(rs, n) == 125 and model.norm_dc(cs, n) == 118      # (117.5 N + N / 2) / N = 118
    assert 2 * rac == 10 * n and 2 * cac == 35 * n                          # AC per sample 5 and 17.5
    assert cac / rac == 3.5
    ok6, _ = model.update_parameters((cs, cac), [(rs, rac)], n, 8, 6)
    assert not ok6                                                          # weight 224: 64 - 224 = -160 < -128
    assert int(0.5 + 3.5 * 64) == 224
    ok5, p5 = model.update_parameters((cs, cac), [(rs, rac)], n, 8, 5)
    # offset = ((118 << 5) - 112 * 125 + 16) >> 5 = -10208 >> 5 = -319, clipped to -128
    assert ok5 and p5 == [(112, -128)]
    (e,) = model.estimate(cur, [ref], 8, 6)
    assert e["log2_denom"] == 5
    # with the offset clipped the weighted picture is far off: |(100 << 5) - (120 * 112 - 4096)| = |(135 << 5) - (130 * 112 - 4096)| = 6144 against
    # the unweighted (20 << 5 + 5 << 5) / 2 = 400, so xSelectWP switches the weight off again
    assert (e["sad_wp"], e["sad_nowp"]) == (6144, 400)
    assert e["present"] == 0 and e["wp"] == (32, 0, 5, 16)


def test_identical_pictures_keep_the_identity_weight_present():
    cur, ref = pictures("identical")
    (e,) = model.estimate(cur, [ref], 8, 6)
    assert e["sad_wp"] == 0 and e["sad_nowp"] == 0 and math.isnan(e["ratio"])
    assert e["present"] == 1 and e["wp"] == (64, 0, 6, 32)


def test_flat_reference_takes_weight_one():
    cur, ref = pictures("flat_reference")
    (e,) = model.estimate(cur, [ref], 8, 6)
    assert e["ref_ac"] == 0 and e["log2_denom"] == 6
    ok, p = model.update_parameters(model.plane_stats(cur), [model.plane_stats(ref)], cur.size, 8, 6)
    assert ok and p[0][0] == 64                                              # dWeight 1.0


def test_pure_offset_fade():
    cur, ref = pictures("offset_fade")
    (e,) = model.estimate(cur, [ref], 8, 6)
    assert e["cur_ac"] == e["ref_ac"]
    assert (e["weight"], e["offset"], e["log2_denom"], e["present"]) == (64, 20, 6, 1)
    assert e["sad_wp"] == 0 and e["ratio"] == 0.0
    assert e["wp"] == (64, 20, 6, 32)
    (e10,) = model.estimate(cur * 4, [ref * 4], 10, 6)                       # the same fade at 10 bits: offset in 8-bit units, handed out << 2
    assert (e10["weight"], e10["offset"], e10["present"]) == (64, 20, 1) and e10["wp"] == (64, 80, 6, 32)


def test_unrelated_noise_is_not_present():
    cur, ref = pictures("noise")
    (e,) = model.estimate(cur, [ref], 8, 6)
    assert e["sad_nowp"] > 0 and e["ratio"] >= 0.99
    assert e["present"] == 0 and e["wp"] == (1 << e["log2_denom"], 0, e["log2_denom"], 1 << (e["log2_denom"] - 1))


def test_positive_sad_over_zero_disables():
    assert model.ratio_disables(5, 0) == (math.inf, True)
    r, off = model.ratio_disables(0, 0)
    assert math.isnan(r) and not off


def test_shared_denominator_goes_down_for_every_reference():
    cur, ref = pictures("checkerboard")
    same = cur.copy()
    es = model.estimate(cur, [same, ref], 8, 6)
    assert [e["log2_denom"] for e in es] == [5, 5]
    assert es[0]["wp"] == (32, 0, 5, 16) and es[0]["present"] == 1          # identical pictures, at the denominator the other reference forced


# ---- the ABI, host side ----------------------------------------------------------------------------------------------------------------------

def test_new_symbols_and_struct_layout():
    from hmme import api
    L = api.load()
    for name in ("hmme_plane_stats", "hmme_wp_estimate"):
        assert hasattr(L, name), name
        assert name in api.SYMBOLS
    assert L.hmme_abi_version() == 6
    # hmme_wp_info: six int64, six int; hmme_weight unchanged
    assert C.sizeof(api.WpInfo) == 6 * 8 + 6 * 4 == 72 and C.alignment(api.WpInfo) == 8
    assert [f[0] for f in api.WpInfo._fields_] == ["cur_dc_sum", "cur_ac", "ref_dc_sum", "ref_ac", "sad_wp", "sad_nowp", "log2_denom", "weight", "offset",
                                                   "present", "served_search", "served_refine"]
    assert api.WpInfo.log2_denom.offset == 48 and api.WpInfo.served_refine.offset == 68
    assert C.sizeof(api.Weight) == 16
    # the header declares the struct the bindings mirror, field for field
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hmme.h")).read()
    body = re.search(r"typedef struct hmme_wp_info \{(.*?)\} hmme_wp_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("int64_t", "").replace("int", "").split(",")]
    assert names == [f[0] for f in api.WpInfo._fields_]


def test_refusals_that_need_no_context():
    from hmme import api
    L = api.load()
    ERR_ARG = -1
    dc, ac = C.c_int64(7), C.c_int64(7)
    assert L.hmme_plane_stats(None, C.byref(dc), C.byref(ac)) == ERR_ARG
    assert (dc.value, ac.value) == (7, 7)
    w, info = (api.Weight * 1)(api.Weight(1, 2, 3, 4)), (api.WpInfo * 1)()
    refs = (C.c_void_p * 1)(None)
    for n_refs, start in ((1, 6), (0, 6), (17, 6), (1, 2), (1, 8)):
        assert L.hmme_wp_estimate(None, None, refs, n_refs, start, w, info) == ERR_ARG
    assert (w[0].w0, w[0].offset, w[0].shift, w[0].round) == (1, 2, 3, 4)
