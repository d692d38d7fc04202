"""The 4:2:0 weighted-prediction estimator without a GPU: the numpy model of HM's joint estimator (tests/wp_estimate_420_model.py) on pictures
whose numbers can be checked by hand, its reduction to the luma model, and the host-only behaviour of the new entry point (symbol, refusals
that need no context)."""
import ctypes as C
import os
import re

import numpy as np

import wp_estimate_420_model as model
import wp_estimate_model as luma_model


def stats3(pic3):
    return [luma_model.plane_stats(p) for p in pic3]


SIZES = [32 * 16, 16 * 8, 16 * 8]


def test_case_1_one_chroma_plane_lowers_the_denominator_luma_uses():
    cur, ref = model.pictures(1)
    assert np.array_equal(cur[0], ref[0])
    (alone,) = luma_model.estimate(cur[0], [ref[0]], 8, 6)
    assert alone["wp"] == (64, 0, 6, 32)
    # Cb: AC 10 over 2 per sample -> dWeight 5: 320 at d = 6 (64 - 320 < -128), 160 at d = 5 (32 - 160 = -128: just inside)
    ok6, _ = model.update_parameters(stats3(cur), [stats3(ref)], SIZES, 8, 6)
    ok5, p5 = model.update_parameters(stats3(cur), [stats3(ref)], SIZES, 8, 5)
    assert not ok6 and ok5
    # Cb offset: ((200 << 5) - 160 * 20 + 16) >> 5 = 100; pred = 128 - ((128 * 160) >> 5) = -512; delta = Clip3(-512, 511, 612) = 511; 511 - 512 = -1
    assert model.raw_parameters(stats3(cur)[1], stats3(ref)[1], 128, 8, 5) == (160, 100)
    assert model.chroma_offset(100, 160, 5) == (-512, -1)
    assert p5 == [[(32, 0), (160, -1), (32, 0)]]
    (e,) = model.estimate(cur, [ref], 8, 6)
    assert [x["log2_denom"] for x in e] == [5, 5, 5]
    assert e[0]["wp"] == (32, 0, 5, 16) and e[1]["wp"] == (160, -1, 5, 16) and e[2]["wp"] == (32, 0, 5, 16)
    # |(190 << 5) - (18 * 160 - 32)| = |(210 << 5) - (22 * 160 - 32)| = 3232 against (172 << 5 + 188 << 5) / 2 = 5760; luma and Cr add 0 to both
    assert (sum(x["sad_wp"] for x in e), sum(x["sad_nowp"] for x in e)) == (3232, 5760)
    assert [x["present"] for x in e] == [1, 1, 1]


def test_case_2_chroma_keeps_a_luma_weight_that_luma_alone_would_lose():
    cur, ref = model.pictures(2)
    (alone,) = luma_model.estimate(cur[0], [ref[0]], 8, 6)
    assert round(alone["ratio"], 3) == 1.014 and alone["present"] == 0 and alone["wp"] == (64, 0, 6, 32)
    (e,) = model.estimate(cur, [ref], 8, 6)
    assert round(e[0]["ratio"], 2) == 0.42 and [x["present"] for x in e] == [1, 1, 1]
    assert e[0]["weight"] == 66 and e[0]["log2_denom"] == 6
    assert [(x["weight"], x["offset"], x["sad_wp"]) for x in e[1:]] == [(64, 60, 0), (64, 60, 0)]


def test_case_3_chroma_switches_a_good_luma_offset_off():
    cur, ref = model.pictures(3)
    (alone,) = luma_model.estimate(cur[0], [ref[0]], 8, 6)
    assert alone["wp"] == (64, 2, 6, 32) and alone["present"] == 1
    # chroma weight 224 is out of range at d = 6, so d = 5
    assert model.raw_parameters(stats3(cur)[1], stats3(ref)[1], 128, 8, 6)[0] == 224 and 64 - 224 < -128
    ok6, p6 = model.update_parameters(stats3(cur), [stats3(ref)], SIZES, 8, 6)
    assert not ok6 and p6 == [[(64, 2)]]                                      # luma passed, Cb ended the pass
    ok5, p5 = model.update_parameters(stats3(cur), [stats3(ref)], SIZES, 8, 5)
    # pred = 128 - ((128 * 112) >> 5) = -320; the raw offset -319 is within 512 of it, so only the last clip acts: -128
    assert model.raw_parameters(stats3(cur)[1], stats3(ref)[1], 128, 8, 5) == (112, -319)
    assert model.chroma_offset(-319, 112, 5) == (-320, -128)
    assert ok5 and p5 == [[(32, 2), (112, -128), (112, -128)]]
    (e,) = model.estimate(cur, [ref], 8, 6)
    assert [(x["sad_wp"], x["sad_nowp"]) for x in e] == [(0, 64), (6144, 400), (6144, 400)]      # 12288 / 864
    assert e[0]["ratio"] == 12288 / 864
    assert [x["present"] for x in e] == [0, 0, 0] and all(x["wp"] == (32, 0, 5, 16) for x in e)


def test_chroma_offset_rule_differs_from_a_plain_clip():
    # weight 160 at d = 5: pred = -512, so any raw offset of 0 or more ends at Clip3(-128, 127, 511 - 512) = -1; a plain clip would keep 0 .. 127
    for raw in (0, 50, 100, 127, 400):
        assert model.chroma_offset(raw, 160, 5) == (-512, -1)
        assert model.clip3(-128, 127, raw) != -1
    # at the default weight pred is 0 and the two rules agree
    for raw in (-600, -128, -5, 0, 127, 600):
        assert model.chroma_offset(raw, 64, 6) == (0, model.clip3(-128, 127, raw))


def test_reduces_to_the_luma_model_when_chroma_is_flat_and_equal():
    rng = np.random.default_rng(5)
    ref_y = rng.integers(20, 120, (16, 32)).astype(np.int64)
    cases = {"fade": np.rint(ref_y * 1.5 + 10).astype(np.int64), "noise": rng.integers(0, 256, (16, 32)).astype(np.int64), "identical": ref_y.copy(),
             "steep": ref_y * 4}
    kept = 0
    for name, cur_y in cases.items():
        for start in (6, 7):
            cb, cr = model.flat(16, 8, 90), model.flat(16, 8, 200)
            es = model.estimate((cur_y, cb, cr), [(ref_y, cb.copy(), cr.copy()), (cur_y.copy(), cb, cr)], 8, start)
            want = luma_model.estimate(cur_y, [ref_y, cur_y], 8, start)
            for e, l in zip(es, want):
                # flat chroma equal to its reference: weight 1 << d, offset 0, both SADs 0 -- it moves neither the denominator nor the ratio
                assert {k: e[0][k] for k in luma_model.INFO_FIELDS} == {k: l[k] for k in luma_model.INFO_FIELDS}, (name, start)
                assert e[0]["wp"] == l["wp"]
                assert all((x["sad_wp"], x["sad_nowp"]) == (0, 0) for x in e[1:])
                kept += l["present"]
    assert 0 < kept < 16


# ---- the ABI, host side ----------------------------------------------------------------------------------------------------------------------

def test_symbol_is_declared_and_bound():
    from hmme import api
    L = api.load()
    assert hasattr(L, "hmme_wp_estimate_420") and "hmme_wp_estimate_420" in api.SYMBOLS
    assert L.hmme_abi_version() == 6 == api.ABI_VERSION
    assert hasattr(api.Engine, "wp_estimate_420")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hmme.h")).read()
    decl = re.search(r"^int hmme_wp_estimate_420\((.*?)\);", hdr, re.S | re.M).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == ["ctx", "cur", "refs", "n_refs", "log2_denom_start", "out_wp_luma", "out_wp_chroma", "out_info"]
    assert C.sizeof(api.WpInfo) == 72 and C.sizeof(api.Weight) == 16         # no new or changed struct


def test_refusals_that_need_no_context():
    from hmme import api
    L = api.load()
    ERR_ARG = -1
    wl, wc, info = (api.Weight * 1)(api.Weight(1, 2, 3, 4)), (api.Weight * 2)(api.Weight(5, 6, 7, 8), api.Weight(5, 6, 7, 8)), (api.WpInfo * 3)()
    C.memset(info, 0x5a, C.sizeof(info))
    cur, refs = (C.c_void_p * 3)(None, None, None), (C.c_void_p * 3)(None, None, None)
    for n_refs, start in ((1, 6), (0, 6), (17, 6), (1, 2), (1, 8)):
        assert L.hmme_wp_estimate_420(None, cur, refs, n_refs, start, wl, wc, info) == ERR_ARG
    assert (wl[0].w0, wl[0].offset, wl[0].shift, wl[0].round) == (1, 2, 3, 4)
    assert all((w.w0, w.offset, w.shift, w.round) == (5, 6, 7, 8) for w in wc)
    assert bytes(info) == b"\x5a" * C.sizeof(info)
