"""The sizes of tests/geometry_cases.py without a device: the models give at these sizes what tests/test_gpu_geometry.py relies on (blocks
without a CU, CUs that straddle the edge, a difference of 0 outside the picture, clipped windows), and the library's host arithmetic --
hmme_set_search_range, me_picture_job, hmme_num_ctus, the launch plans -- equals its restatement for every CTU."""
import ctypes as C

import numpy as np
import pytest

import geometry_cases as gc
import residual_model as rm
import select_dirs_model as sdm
import select_model as sm
import select_refs_model as srm


@pytest.fixture(scope="module")
def api():
    from hmme import api
    api.load()
    return api


def test_the_table_says_what_the_sizes_are():
    for size in (gc.ODD, gc.NARROW, gc.EVEN, gc.MIN1):
        assert gc.last_ctu(*size) == gc.LAST_CTU[size]
        assert size[0] % 8 and size[1] % 8
    assert gc.ODD[0] % 4 == 1 and gc.ODD[1] % 4 == 3 and gc.EVEN[0] % 4 == 2 and gc.EVEN[0] % 2 == gc.EVEN[1] % 2 == 0
    assert (gc.EVEN[0] // 2) % 2 == (gc.EVEN[1] // 2) % 2 == 1                    # an odd chroma size
    assert [gc.n_ctus(*s) for s in gc.TABLE] == [4, 4, 6, 1, 256, 256]
    assert sorted({(w % 16) for w, _ in gc.STATS_SIZES}) == list(range(1, 16))
    sizes = [gc.fuzz_size(s) for s in gc.FUZZ_SEEDS]
    assert len(set(sizes)) == 10 and all(8 <= v <= 200 for s in sizes for v in s)
    assert sum(1 for w, h in sizes if w % 2 or h % 2) >= 5 and sum(1 for w, h in sizes if w % 8 or h % 8) >= 8


def test_the_plane_set_launches_take_the_rounds_the_cases_claim():
    """geometry_cases.stat_grid restates stat_grid of hmme.hip: the 2048 x 50 case with 16 references needs two rounds for luma in both set
    launches while chroma's workgroups beyond its seventh row block leave; every size of tests/test_gpu_wp_estimate_420.py and the row-tail
    sizes need one"""
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "hm-opencl_amd", "csrc", "hmme.hip")).read()
    assert int(re.search(r"constexpr int kWpStatBlocks = (\d+);", src).group(1)) == gc.STAT_BLOCKS
    assert "cap = std::max(1, kWpStatBlocks / n_y)" in src and "rounds = (row_blocks + cap - 1) / cap" in src
    w, h, n_refs = gc.ROUNDS_420
    for name, grids in gc.stat_grids_420(w, h, 1, n_refs).items():
        luma, chroma = grids
        assert (luma["lpr_log2"], luma["rows_per_block"], luma["row_blocks"], luma["rounds"], luma["blocks"]) == (7, 2, 25, 2, 13), name
        assert luma["cap"] == (20 if name == "stats" else 21) and luma["row_blocks"] > luma["cap"]
        assert luma["blocks"] * luma["rows_per_block"] < h                       # a second iteration of the row loop has rows to read
        assert (chroma["lpr_log2"], chroma["rows_per_block"], chroma["row_blocks"], chroma["rounds"], chroma["blocks"]) == (6, 4, 7, 1, 7), name
        assert chroma["blocks"] < luma["blocks"] and chroma["blocks"] * chroma["rows_per_block"] >= h // 2   # workgroups 7..12 of a chroma plane: no row
    # one round everywhere else: the family's own sizes with the most references each is run with, and the row tails
    from_family = [(16, 16, 2), (32, 16, 16), (48, 18, 4), (130, 66, 3), (8200, 16, 2), (512, 128, 1), (128, 128, 1)]
    for w, h, n_refs in from_family + [s + (1,) for s in gc.STATS_SIZES_420]:
        for bytes_ in (1, 2):
            assert all(g["rounds"] == 1 for grids in gc.stat_grids_420(w, h, bytes_, n_refs).values() for g in grids), (w, h, n_refs)
    assert sorted({(w // 2) % 16 for w, _ in gc.STATS_SIZES_420}) == list(range(1, 16)) and all(h == 18 and w % 16 == 2 * k % 16
                                                                                                  for k, (w, h) in enumerate(gc.STATS_SIZES_420, 1))


def test_the_luma_set_launches_take_the_rounds_the_case_claims():
    """hmme_wp_estimate on 1033 x 66 at 10 bit with 16 distinct references: the statistics of 17 planes and the SADs of 16 pairs share a launch
    each, both capped below the picture's 66 row blocks -- two rounds of 33 workgroups, so both row loops iterate twice -- and a row's last
    vector holds 2 of 16 bytes"""
    w, h, n_refs = gc.ROUNDS_LUMA
    for n_y, cap in ((1 + n_refs, 60), (n_refs, 64)):
        g = gc.stat_grid(w, h, 2, n_y)
        assert (g["lpr_log2"], g["rows_per_block"], g["row_blocks"], g["cap"], g["rounds"], g["blocks"]) == (8, 1, 66, cap, 2, 33), n_y
        assert g["blocks"] * g["rows_per_block"] < h                              # a second iteration of the row loop has rows to read
    assert (2 * w + 15) // 16 == 130 and 2 * w - 16 * 129 == 2
    assert gc.stat_grid(w, h, 2, 1)["rounds"] == 1                              # a plane on its own (hmme_plane_stats) needs one


def test_windows_are_clipped_as_the_table_states(api, oracle_lib):
    hmo = oracle_lib.oracle()
    win = [C.c_int() for _ in range(4)]
    for size, want in gc.LAST_WINDOW.items():
        w, h = size
        sr = gc.SEARCH_RANGE[size]
        x, y = gc.ctu_origin(gc.n_ctus(w, h) - 1, w)
        assert gc.window(0, 0, sr, x, y, w, h) == want and gc.is_clipped(want, sr)
        assert api.set_search_range(0, 0, sr, x, y, w, h) == want
        hmo.hmo_set_search_range(0, 0, sr, x, y, w, h, 64, *[C.byref(v) for v in win])
        assert tuple(v.value for v in win) == want
    # the predictors the GPU search cases use leave the last window clipped, at 9 x 9 too (its window reaches 16 samples to the right)
    for size, sr in gc.SEARCH_RANGE.items():
        w, h = size
        pred = gc.predictors(w, h, seed=3, max_pel=16 if size == gc.MIN1 else 5)
        last = gc.n_ctus(w, h) - 1
        x, y = gc.ctu_origin(last, w)
        assert gc.is_clipped(api.set_search_range(int(pred[last, 0]), int(pred[last, 1]), sr, x, y, w, h), sr), size


def test_search_range_and_picture_job_equal_the_restatement_for_every_ctu(api):
    L = api.load()
    i16p = C.POINTER(C.c_int16)
    L.hmme_test_picture_job.restype = C.c_int
    L.hmme_test_picture_job.argtypes = [C.c_int] * 6 + [i16p, i16p, i16p]
    out = np.zeros(8, np.int16)
    checked = 0
    for w, h in gc.TABLE:
        n = gc.n_ctus(w, h)
        assert L.hmme_num_ctus(w, h) == n
        for sr in ((4,) if (w, h) in gc.SLIVERS else (8, 16, 64)):
            for pred in (None, gc.predictors(w, h, seed=w + sr, max_pel=40), gc.predictors(w, h, seed=h + sr, max_pel=2000)):
                for ctu in range(n):
                    x, y = gc.ctu_origin(ctu, w)
                    px, py = (0, 0) if pred is None else (int(pred[ctu, 0]), int(pred[ctu, 1]))
                    want = gc.window(px, py, sr, x, y, w, h)
                    assert api.set_search_range(px, py, sr, x, y, w, h) == want, (w, h, sr, ctu)
                    assert L.hmme_test_picture_job(ctu, 0, n, w, h, sr, None if pred is None else pred.ctypes.data_as(i16p), None, out.ctypes.data_as(i16p)) == 0
                    assert (int(out[0]), int(out[1])) == (x, y) and tuple(int(v) for v in out[2:6]) == want and (int(out[6]), int(out[7])) == (px, py), (w, h, sr, ctu)
                    assert want[0] <= want[2] and want[1] <= want[3]
                    checked += 1
    assert checked == 3 * (3 * (4 + 4 + 6 + 1) + 2 * 256)


def test_num_ctus_and_the_launch_plans_take_these_sizes(api):
    """hmme_num_ctus and the pure-host plans that take a picture size (none of the hmme_*_check functions does: they take bit depths, weights
    and decision parameters) accept every size of the table; the refinement deal is a permutation of the picture's CTUs"""
    L = api.load()
    assert L.hmme_num_ctus(16384, 8) == 256 and L.hmme_num_ctus(8, 16384) == 256 and L.hmme_num_ctus(16384, 16384) == 65536
    assert L.hmme_num_ctus(9, 9) == 1 and L.hmme_num_ctus(65, 67) == 4 and L.hmme_num_ctus(130, 66) == 6
    L.hmme_test_tail_plan.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)]
    plan = (C.c_int * 4)()
    for w, h in gc.TABLE:
        n = gc.n_ctus(w, h)
        for sr in (4, 64):
            assert L.hmme_test_tail_plan(w, h, sr, 1, 512, plan) == 0
            assert plan[0] == n and 0 <= plan[1] <= n
        assert sorted(L.hmme_test_frac_deal(k, 1, w, h) for k in range(n)) == list(range(n))
        assert L.hmme_test_frac_deal(n, 1, w, h) == -1
    for w, h in gc.REFUSED_PLANES:
        assert L.hmme_test_tail_plan(w, h, 4, 1, 512, plan) != 0 and L.hmme_test_frac_deal(0, 1, w, h) == -1


@pytest.mark.parametrize("size", [gc.ODD, gc.NARROW, gc.MIN1])
def test_the_decision_models_leave_blocks_without_a_cu_and_cus_that_straddle(api, size):
    w, h = size
    n = gc.n_ctus(w, h)
    mv, cost = sm.random_tables(n, seed=500 + w)
    for per in (64, 256):
        _, slot, _, _ = sm.select_picture(mv, cost, api.SelectParams(per), w, h)
        assert (slot == sm.NO_SLOT).sum() > 0 and (slot != sm.NO_SLOT).sum() > 0
        _, slot1, _, leaves = sm.select_picture(mv, cost, api.SelectParams(per, max_depth=1), w, h)
        assert (slot1 == sm.NO_SLOT).sum() > 0 and gc.straddling_leaves(slot1, w, h, per) >= 1 and all(d <= 1 for d, _ in leaves)
        # a CU at max_depth exists iff its origin is inside the picture: block by block
        g, nb = (8, 8) if per == 64 else (4, 16)
        for c in range(n):
            x0, y0 = gc.ctu_origin(c, w)
            for b in range(per):
                bx, by = x0 + (b % nb) * g, y0 + (b // nb) * g
                assert (slot[c, b] != sm.NO_SLOT) == (bx // 8 * 8 < w and by // 8 * 8 < h), (c, b)
    rmv, rcost = srm.random_ref_tables(3, n, seed=510 + w)
    _, ref, rslot, _, _ = srm.select_refs_picture(rmv, rcost, api.SelectParams(64, max_depth=1), w, h)
    assert (rslot == sm.NO_SLOT).sum() > 0 and ((ref == srm.NO_REF) == (rslot == sm.NO_SLOT)).all() and gc.straddling_leaves(rslot, w, h, 64) >= 1
    tabs = sdm.random_dir_tables(n, n, seed=520 + w)
    _, dirs, dslot, _ = sdm.select_dirs_picture(*tabs, api.SelectParams(64, max_depth=1), w, h, sdm.HM_BITS)
    assert (dslot == sm.NO_SLOT).sum() > 0 and ((dirs == sdm.NO_DIR) == (dslot == sm.NO_SLOT)).all() and gc.straddling_leaves(dslot, w, h, 64) >= 1


@pytest.mark.parametrize("size", [gc.ODD, gc.NARROW, gc.MIN1, gc.EVEN])
def test_the_residual_model_is_zero_outside_the_picture(api, oracle_lib, size):
    w, h = size
    hmo = oracle_lib.oracle()
    rng = np.random.default_rng(w)
    for bd in (8, 12):
        cur, pred = (rng.integers(0, 1 << bd, size=(h, w)).astype(np.int16) for _ in range(2))
        d = rm.difference(cur, pred, w, h)
        assert d.shape == tuple(64 * v for v in gc.dims(w, h)[::-1])
        assert d[:h, :w].any() and not d[h:].any() and not d[:, w:].any()
        assert np.array_equal(d[:h, :w], cur.astype(np.int32) - pred)
        # blocks wholly outside the picture cost nothing; one that holds a single sample column costs that column's
        res, pu, cu, ctu = rm.residual_picture(hmo, cur, pred, w, h, bd, None, 256, 0)
        last = gc.n_ctus(w, h) - 1
        x0, y0 = gc.ctu_origin(last, w)
        for b in range(256):
            bx, by = x0 + (b % 16) * 4, y0 + (b // 16) * 4
            if bx >= w or by >= h:
                assert pu[last, b] == 0 and cu[last, b] == 0
            else:
                blk = d[by:by + 4, bx:bx + 4].astype(np.int64)
                assert pu[last, b] == np.abs(blk).sum() >> (bd - 8) and cu[last, b] == rm.sse(blk, bd)
        assert np.array_equal(res, d[:h, :w])
