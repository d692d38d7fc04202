"""The plan of a per-CTU call, through hmme_test_ctu_plan (include/hmme_test.h): the host arithmetic hmme_search_ctu(_w),
hmme_search_refine_ctu(_w) and hmme_refine_ctu(_w) run before they pack and launch -- sample width and bias, the window's geometry, the deal
of the window to up to 64 workgroups, and the refusals in their order.  Needs no GPU.

The deal decides latency only: results do not depend on it, so no result-based test would notice a change.  PARENT_DEAL8 / PARENT_DEAL16
were recorded by running the dealing lines of the library as it was before the per-CTU body was split (one function, ctu_call) on the CPU."""
import ctypes as C

import numpy as np
import pytest

import ctu_refusal_cases as crc
import range_content as rc
from test_wp_frame_cpu import WEIGHTS

SEARCH, REFINE, HADAMARD = 1, 2, 4                # HMME_TEST_CTU_*
LDS_BUDGET16, PITCHES = 78 * 1024, (65, 130, 131, 161)
WINDOWS8 = [(1, 1), (5, 3), (129, 129), (130, 129), (129, 130), (130, 130), (257, 1), (257, 257)]
WINDOWS16 = [(wx, wy) for wx in (1, 129, 257) for wy in (1, 4, 5, 53, 54, 129, 257)]
# (wx, wy) -> (n_wg, pdw, smax, first [y0, y1), last [y0, y1))
PARENT_DEAL8 = {
    (1, 1): (1, 0, 0, (0, 1), (0, 1)), (5, 3): (1, 0, 0, (0, 1), (0, 1)), (129, 129): (17, 0, 0, (0, 3), (63, 67)), (130, 129): (18, 0, 0, (0, 3), (0, 3)),
    (129, 130): (18, 0, 0, (0, 3), (0, 1)), (130, 130): (19, 0, 0, (0, 4), (0, 1)), (257, 1): (2, 0, 0, (0, 1), (0, 1)), (257, 257): (64, 0, 0, (0, 4), (60, 64))}
PARENT_DEAL16 = {
    (1, 1): (1, 131, 1, (0, 1), (0, 1)), (1, 4): (1, 131, 4, (0, 4), (0, 4)), (1, 5): (2, 131, 3, (0, 2), (2, 5)), (1, 53): (14, 131, 4, (0, 3), (49, 53)),
    (1, 54): (14, 131, 4, (0, 3), (50, 54)), (1, 129): (33, 131, 4, (0, 3), (125, 129)), (1, 257): (64, 131, 5, (0, 4), (252, 257)),
    (129, 1): (1, 130, 1, (0, 1), (0, 1)), (129, 4): (1, 130, 4, (0, 4), (0, 4)), (129, 5): (2, 130, 3, (0, 2), (2, 5)), (129, 53): (14, 130, 4, (0, 3), (49, 53)),
    (129, 54): (14, 130, 4, (0, 3), (50, 54)), (129, 129): (33, 130, 4, (0, 3), (125, 129)), (129, 257): (64, 130, 5, (0, 4), (252, 257)),
    (257, 1): (1, 161, 1, (0, 1), (0, 1)), (257, 4): (1, 161, 4, (0, 4), (0, 4)), (257, 5): (2, 161, 3, (0, 2), (2, 5)), (257, 53): (14, 161, 4, (0, 3), (49, 53)),
    (257, 54): (14, 161, 4, (0, 3), (50, 54)), (257, 129): (33, 161, 4, (0, 3), (125, 129)), (257, 257): (64, 161, 5, (0, 4), (252, 257))}
SCALARS = ("wide", "bias", "origin", "shift_bd", "halo", "rows", "cols", "n_wg", "pdw", "smax", "build_wide", "build_had", "build_wp")


def plan(p, mode, wp, ranges, sr_max=128):
    """-> (return code, message, dict of the plan's scalars + tile_tasks + fw + wg: per workgroup (lt_x, lt_y, rb_x, rb_y, tx, ty, y0, y1))"""
    from hmme import api
    api.build()
    L = api.load()
    L.hmme_test_ctu_plan.argtypes = [C.c_int, C.POINTER(api.SearchParams), C.c_int, C.POINTER(api.Weight), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                     C.POINTER(C.c_float), C.POINTER(C.c_int16), C.c_char_p, C.c_int]
    out, fw, wg, msg = (C.c_int * 17)(), (C.c_float * 3)(), (C.c_int16 * (64 * 8))(*([-1] * 512)), C.create_string_buffer(256)
    w = None if wp is None else C.byref(api.Weight(*wp))
    code = L.hmme_test_ctu_plan(sr_max, C.byref(api.SearchParams(*p)), mode, w, (C.c_int * 4)(*ranges), out, fw, wg, msg, 256)
    d = dict(zip(SCALARS, out[:13]), tile_tasks=tuple(out[13:17]), fw=tuple(fw))
    d["wg"] = [tuple(wg[8 * i:8 * i + 8]) for i in range(d["n_wg"])] if code == 0 else []
    assert all(v == -1 for v in wg[8 * len(d["wg"]):])            # nothing written beyond the workgroups of the deal
    return code, msg.value, d


def params(wx, wy, bd, lt=(-7, 11), shift_free=0):
    """a window of wx x wy candidates that does not start at the origin"""
    return (lt[0], lt[1], lt[0] + wx - 1, lt[1] + wy - 1, 3, -5, 1, bd, shift_free)


@pytest.mark.parametrize("wx,wy", WINDOWS8)
def test_8bit_deal_tiles_partition_the_window_and_ranges_the_tasks(wx, wy):
    p = params(wx, wy, 8)
    code, msg, d = plan(p, SEARCH, None, (0, 255, 0, 255))
    assert code == 0 and not d["wide"] and (d["pdw"], d["smax"]) == (0, 0), msg
    assert 1 <= d["n_wg"] <= 64
    tiles = {}
    for lt_x, lt_y, rb_x, rb_y, tx, ty, y0, y1 in d["wg"]:
        tiles.setdefault((tx, ty), []).append((lt_x, lt_y, rb_x, rb_y, y0, y1))
    assert d["wg"][0][4:6] == (0, 0)                                # tile (0,0) first: finalize decodes against its top-left
    assert set(tiles) == {(tx, ty) for tx in range((wx + 128) // 129) for ty in range((wy + 128) // 129)}
    covered = np.zeros((wy, wx), np.int32)                          # how many tiles hold each candidate
    for (tx, ty), wgs in tiles.items():
        assert len({w[:4] for w in wgs}) == 1                       # one window per tile
        lt_x, lt_y, rb_x, rb_y = wgs[0][:4]
        assert (lt_x, lt_y) == (p[0] + 129 * tx, p[1] + 129 * ty) and lt_x <= rb_x <= p[2] and lt_y <= rb_y <= p[3]
        covered[lt_y - p[1]:rb_y - p[1] + 1, lt_x - p[0]:rb_x - p[0] + 1] += 1
        tasks = d["tile_tasks"][ty * 2 + tx]
        assert tasks >= 1 and wgs[0][4] == 0 and wgs[-1][5] == tasks
        assert all(a[5] == b[4] for a, b in zip(wgs, wgs[1:])) and all(w[4] < w[5] for w in wgs)   # non-empty, contiguous
    assert (covered == 1).all()
    want = PARENT_DEAL8[(wx, wy)]
    assert (d["n_wg"], d["pdw"], d["smax"], d["wg"][0][6:], d["wg"][-1][6:]) == want


@pytest.mark.parametrize("wx,wy", WINDOWS16)
@pytest.mark.parametrize("weighted", [False, True])
def test_16bit_deal_strips_partition_the_rows_within_the_lds_budget(wx, wy, weighted):
    """bit depth 10, and a weighted 8-bit call (which runs the 16-bit kernels as well)"""
    p = params(wx, wy, 8 if weighted else 10)
    code, msg, d = plan(p, SEARCH, (70, 9, 6, 32) if weighted else None, (0, 255, 0, 255))
    assert code == 0 and d["wide"], msg
    assert 1 <= d["n_wg"] <= 64
    strips = [w[6:] for w in d["wg"]]
    assert all(w[:6] == (p[0], p[1], p[2], p[3], 0, 0) for w in d["wg"])         # every strip searches the whole window's columns
    assert strips[0][0] == 0 and strips[-1][1] == wy and all(a[1] == b[0] for a, b in zip(strips, strips[1:])) and all(a < b for a, b in strips)
    assert d["smax"] == max(b - a for a, b in strips)
    lanes = ((wx + 1) // 2 + 2) // 3
    assert d["pdw"] in PITCHES and d["pdw"] >= 3 * (lanes - 1) + 34              # a lane reads dwords 3 * lane + 0..33 of its row
    assert (2 * 594 + 4 + (d["smax"] + 63) * d["pdw"]) * 4 <= LDS_BUDGET16       # lds_bytes16(pdw, smax)
    assert (d["n_wg"], d["pdw"], d["smax"], strips[0], strips[-1]) == PARENT_DEAL16[(wx, wy)]


def test_refinement_alone_is_dealt_no_search():
    code, _, d = plan(params(17, 17, 8), REFINE | HADAMARD, None, (0, 255, 0, 255))
    assert code == 0 and d["n_wg"] == 0 and d["wg"] == [] and d["tile_tasks"] == (0, 0, 0, 0)


def test_format_width_bias_origin_and_geometry():
    p8, p10 = params(33, 17, 8), params(33, 17, 10)
    code, _, d = plan(p8, SEARCH, None, (0, 255, 0, 255))                        # 8 bit plain: the 8-bit kernels, no halo
    assert code == 0 and (d["wide"], d["bias"], d["origin"], d["shift_bd"], d["halo"], d["rows"], d["cols"]) == (0, 0, 0, 8, 0, 17 + 63, 33 + 63)
    assert d["fw"] == (0.0, 0.0, 0.0)
    code, _, d = plan(p8, SEARCH | REFINE | HADAMARD, None, (-1, 255, 0, 255))   # a block minimum of -1: a bi-prediction origin, biased by 2^8
    assert code == 0 and (d["wide"], d["bias"], d["origin"], d["shift_bd"], d["halo"], d["rows"], d["cols"]) == (1, 256, 1, 8, 4, 17 + 71, 33 + 71)
    assert (d["build_wide"], d["build_had"], d["build_wp"]) == (1, 1, 0)
    code, _, d = plan(p8, REFINE, None, (0, 256, 0, 255))                        # ... and a maximum above maxv; SAD refinement
    assert code == 0 and (d["wide"], d["bias"], d["origin"], d["build_had"]) == (1, 256, 1, 0)
    code, _, d = plan(p10, SEARCH, None, (0, 1023, 0, 1023))                     # 10 bit: wide, unbiased
    assert code == 0 and (d["wide"], d["bias"], d["origin"], d["shift_bd"]) == (1, 0, 0, 10)
    code, _, d = plan(params(33, 17, 10, shift_free=1), SEARCH, None, (0, 1023, 0, 1023))
    assert code == 0 and d["shift_bd"] == 8                                      # shift-free: the sums are not shifted
    # a weight whose weighted minimum is negative: ((-64 * 255 + 32) >> 6) + 10 = -245 -> bias 245, FracWp takes bias + offset off again
    code, _, d = plan(p8, SEARCH | REFINE | HADAMARD, (-64, 10, 6, 32), (0, 255, 0, 255))
    assert code == 0 and (d["wide"], d["bias"], d["origin"]) == (1, 245, 0) and (d["build_wide"], d["build_had"], d["build_wp"]) == (1, 1, 1)
    assert d["fw"] == (-1.0, 0.5, 255.0)
    code, _, d = plan(p8, SEARCH, (-64, 10, 6, 32), (-250, 255, 0, 255))         # ... under an origin block that reaches lower still: the block's minimum
    assert code == 0 and (d["bias"], d["origin"]) == (250, 1)
    code, _, d = plan(p8, SEARCH, (-64, 10, 6, 32), (0, 255, 100, 200))          # the scanned range, not the nominal one: ((-64 * 200 + 32) >> 6) + 10
    assert code == 0 and d["bias"] == 190


def test_entry_refuses_what_is_no_call():
    from hmme import api
    api.build()
    assert plan(params(5, 5, 8), 0, None, (0, 255, 0, 255))[0] == crc.ERR_ARG            # neither search nor refinement
    assert plan(params(5, 5, 8), SEARCH | HADAMARD, None, (0, 255, 0, 255))[0] == crc.ERR_ARG
    assert plan(params(5, 5, 8), SEARCH, None, (0, 255, 0, 255), sr_max=129)[0] == crc.ERR_ARG
    assert api.load().hmme_test_ctu_plan(64, None, SEARCH, None, None, None, None, None, None, 0) == crc.ERR_ARG


def ranges_case(entry, faults):
    """a case of ctu_refusal_cases as hmme_test_ctu_plan takes it: (params, mode, weight, ranges)"""
    c = crc.case(entry, faults)
    _, searches, refines = crc.ENTRIES[entry]
    mode = (SEARCH if searches else 0) | (REFINE | HADAMARD if refines else 0)
    return (*c["window"], c["pred_x"], 0, 1, c["bit_depth"], c["shift_free"]), mode, c["weight"], (*c["cur"], *c["ref"])


def test_refusal_order_is_the_calls_own():
    """the ORDER table the GPU test holds the six entries to (tests/test_gpu_ctu_refusal_order.py), through the plan with the faults expressed
    as ranges; the null-pointer faults exist in a call only"""
    n = 0
    for entry in crc.ENTRIES:
        for faults in [(f,) for f in crc.faults_of(entry)] + crc.pairs_of(entry):
            if crc.NULLW in faults or crc.NULLOUT in faults:
                continue
            first = min(faults, key=crc.ORDER.index)
            code, msg, _ = plan(*ranges_case(entry, faults), sr_max=crc.SR_MAX)
            assert code == crc.CODE[first] and all(f in msg for f in crc.FRAGMENT[first]), (entry, faults, first, code, msg)
            n += 1
        assert plan(*ranges_case(entry, ()), sr_max=crc.SR_MAX)[0] == 0, entry      # the case without a fault is served
    assert n == 3 * (6 + 15) + (9 + 36) + 2 * (10 + 44)


def rule_weights():
    """the weights of the refusal suite (tests/test_wp_frame_cpu.py) and of the edge suite: per family of tests/range_content.py the last
    weight hmme_weight_check accepts and the first it refuses"""
    out = [(bd, wp, refine) for bd in (8, 10, 12) for wp in WEIGHTS for refine in (0, 1)]
    for bd in (8, 10, 12):
        for refine in (0, 1):
            for b in rc.boundary_weights(bd, refine):
                out += [(bd, b["wp"], refine), (bd, b["next"], refine)]
    return out


def test_one_weight_rule_for_per_ctu_and_picture_calls():
    """hmme_weight_check (the picture-level calls) and the per-CTU plan on the nominal ranges [0, maxv] of block and reference answer alike,
    except where hmme_weight_check refuses for one of the two checks only it makes: w0 * sample + round beyond 32 bits, and, for a refinement
    with a weight that is not the identity, beyond the 2^24 that fp32 holds exactly ("fp32" in tests/range_content.py).  The per-CTU calls
    serve such a weight (open points)."""
    from hmme import api
    api.build()
    differ = {"32 bits": 0, "fp32": 0}
    for bd, wp, refine in rule_weights():
        maxv = (1 << bd) - 1
        mode = SEARCH | (REFINE | HADAMARD if refine else 0)
        got, msg, _ = plan(params(5, 5, bd), mode, wp, (0, maxv, 0, maxv))
        want = api.weight_check(bd, wp, refine)
        if got == want:
            continue
        assert (got, want) == (0, crc.ERR_UNSUPPORTED), (bd, wp, refine, got, want, msg)
        ends = (wp[3], wp[0] * maxv + wp[3])
        if min(ends) < -(1 << 31) or max(ends) > (1 << 31) - 1:
            differ["32 bits"] += 1
        else:
            assert rc.failing(bd, wp, refine) == ("fp32",), (bd, wp, refine)
            differ["fp32"] += 1
    assert differ["fp32"] > 0                                       # the edge suite's large-gain families sit next to it
