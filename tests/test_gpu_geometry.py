"""Every call family at picture sizes that are no multiple of 8 (tests/geometry_cases.py names the sizes and what each reaches): odd widths and
heights, a last CTU column one sample wide, an odd chroma size, the minimum plus one and the largest sizes a plane accepts.  Every comparison is
bit-exact against the CPU oracle or the numpy models of the suite; the one comparison between results of the library -- the four upload
forms give one image -- also compares each of them with the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import bipred_wp_model as bwm
import frame_helpers as fh
import geometry_cases as gc
import predict_bi_model as pbm
import predict_bi_w_model as pbw
import predict_chroma_model as cm
import residual_model as rm
import select_dirs_model as sdm
import select_model as sm
import select_refs_model as srm
import wp_estimate_model as wpm

pytestmark = pytest.mark.gpu

ERR_ARG = -1
FADE, FADE_OTHER = (40, -12, 5, 16), (48, 9, 5, 16)      # written for 8 bits: 40 / 32 - 12 and 48 / 32 + 9, one shift (a slice has one denominator)
BDS = [8, 10]


def at(wp, bd):
    return (wp[0], wp[1] << (bd - 8), wp[2], wp[3])


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 128)
    e.set_lambda(57.9)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return fh.bind_hmo(oracle_lib)


@pytest.fixture(scope="module")
def mv_cost(oracle_lib):
    L = oracle_lib.oracle()
    return lambda lq, x, y, px, py, scale: L.hmo_mv_cost(lq, x, y, px, py, scale)


def margin():
    from hmme import synth
    return synth.MARGIN


def pictures(w, h, bd, seed, n=1):
    """n + 1 padded int16 pictures: cur, and n references of the same scene moved differently"""
    from hmme import synth
    cur, ref, _ = synth.make_pair(w, h, seed=seed, bit_depth=bd, max_mv=min(4, w // 2), region=32)
    more = [synth.make_pair(w, h, seed=seed + 1000 * k, bit_depth=bd, max_mv=min(4, w // 2), region=32)[1] for k in range(1, n)]
    return [cur, ref] + more


def area(padded, w, h):
    m = margin()
    return padded[m:m + h, m:m + w]


def sentinel(bd):
    return (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0xA5A5)


def oracle_search(oracle_lib, cur, ref, w, h, sr, pred, lq, fen, bd, first=0, count=-1):
    m = margin()
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pred, lq, fen, bd, ctu_first=first, ctu_count=count, n_threads=8)
    return np.stack([ox, oy], axis=-1).astype(np.int16), osad


def same_tables(got, want, what):
    for g, o, name in zip(got, want, ("mv", "cost")):
        assert np.array_equal(g, o), (what, name, np.argwhere(np.asarray(g) != np.asarray(o))[:4])


# ---- 1: planes and the four upload forms --------------------------------------------------------------------------------------------------------
def test_plane_sizes_accepted_and_refused(engine):
    L = engine.L
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        for w, h in gc.REFUSED_PLANES:
            for bd in BDS:
                p = C.c_void_p()
                assert L.hmme_plane_create_ex(engine.h, w, h, bd, C.byref(p)) == ERR_ARG and not p.value, (w, h, bd)
                assert b"hmme_plane_create" in L.hmme_last_error(engine.h)
    finally:
        L.hmme_set_error_printing(engine.h, prev)
    for w, h in ((gc.PLANE_MIN, gc.PLANE_MIN),) + gc.SLIVERS:
        for bd in BDS:
            with engine.plane(w, h, bd) as p:
                assert (L.hmme_plane_width(p.h), L.hmme_plane_height(p.h), L.hmme_plane_bit_depth(p.h)) == (w, h, bd)


@pytest.mark.parametrize("bd", BDS)
@pytest.mark.parametrize("size", [gc.ODD, gc.NARROW, gc.EVEN, gc.MIN1])
def test_upload_forms_give_the_picture_and_its_replicated_border(engine, hmo, size, bd):
    """The device plane is read through predict_frame: a zero field returns the picture, one far MV per CTU in each of the eight directions
    returns the border as numpy's edge replication holds it.  set_device_u8 carries bytes: into a 10-bit plane it uploads the picture >> 2"""
    import torch
    from hmme import synth
    w, h = size
    m, dev = margin(), torch.device("cuda", 0)
    cur = pictures(w, h, bd, seed=4100 + w + bd)[0]
    img = np.ascontiguousarray(area(cur, w, h))
    low = img if bd == 8 else img >> 2
    low_padded = synth.pad_plane(low)
    img8 = np.ascontiguousarray(low.astype(np.uint8))
    dt = sentinel(bd)[0]
    fields = [np.zeros((gc.n_ctus(w, h), 1, 2), np.int16)] + gc.far_fields(w, h)
    for f in fields[1:]:                                                            # beyond the clip range in the direction they point
        clipped = gc.clip_mv(int(f[0, 0, 0]), int(f[0, 0, 1]), 0, 0, w, h)
        assert all(clipped[k] != f[0, 0, k] for k in range(2) if abs(int(f[0, 0, k])) == gc.FAR)

    def want_of(padded):
        out = [fh.oracle_prediction(hmo, padded, w, h, bd, f)[:h, :w].astype(dt) for f in fields]
        assert np.array_equal(out[0], area(padded, w, h)) and len({o.tobytes() for o in out}) == len(out)
        return out

    want, want_low = want_of(cur), want_of(low_padded)
    stream = torch.cuda.Stream()
    wide = torch.full((h, w + 3), 0xEE, dtype=torch.uint8, device=dev)
    wide[:, :w] = torch.from_numpy(img8).to(dev)
    packed = torch.from_numpy(img8).to(dev)
    torch.cuda.synchronize()
    packed16 = np.ascontiguousarray(img)                                            # rows of w samples: an odd stride

    def registered(pl, buf, ptr, stride, sample_bytes):
        engine.host_register(buf)
        try:
            pl.upload_async(ptr, stride, sample_bytes, stream.cuda_stream)
            engine.upload_status(stream.cuda_stream)
        finally:
            engine.host_unregister(buf)

    forms = {"pel_padded": (lambda pl: pl.upload_pel(cur, (m, m)), want),
             "packed": (lambda pl: pl.upload_u8(img8) if bd == 8 else pl.upload_pel(packed16, (0, 0)), want),
             "async_registered": (lambda pl: registered(pl, img8, img8.ctypes.data, w, 1) if bd == 8 else
                                  registered(pl, cur, cur.ctypes.data + 2 * (m * cur.shape[1] + m), cur.shape[1], 2), want),
             "async_registered_u8": (lambda pl: registered(pl, img8, img8.ctypes.data, w, 1), want_low),
             "device_u8_pitch_w": (lambda pl: pl.set_device_u8(packed.data_ptr(), w, 0), want_low),
             "device_u8_pitch_w_3": (lambda pl: pl.set_device_u8(wide.data_ptr(), w + 3, 0), want_low)}
    images = {}
    with engine.plane(w, h, bd) as pl:
        for name, (upload, expect) in forms.items():
            upload(pl)
            torch.cuda.synchronize()
            got = [engine.predict_frame(pl, f) for f in fields]
            for k, (g, o) in enumerate(zip(got, expect)):
                assert np.array_equal(g, o), (name, k, np.argwhere(g != o)[:4])
            images[name] = got
            pl.upload_pel(np.zeros_like(cur), (m, m))                               # the next form starts from another content
    for group in (("pel_padded", "packed", "async_registered"), ("async_registered_u8", "device_u8_pitch_w", "device_u8_pitch_w_3")):
        for name in group[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(images[group[0]], images[name])), name
    assert (wide[:, w:] == 0xEE).all()


# ---- 2: integer search and refinement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", BDS)
@pytest.mark.parametrize("size", [gc.ODD, gc.NARROW, gc.MIN1])
def test_search_and_refinement(engine, oracle_lib, size, bd):
    import torch
    from hmme import api
    w, h = size
    sr, n, m = gc.SEARCH_RANGE[size], gc.n_ctus(w, h), margin()
    cur, ref, ref2 = pictures(w, h, bd, seed=4200 + w + bd, n=2)
    pred = gc.predictors(w, h, seed=3, max_pel=16 if size == gc.MIN1 else 5)
    x, y = gc.ctu_origin(n - 1, w)
    assert gc.is_clipped(api.set_search_range(int(pred[n - 1, 0]), int(pred[n - 1, 1]), sr, x, y, w, h), sr)
    if size in gc.LAST_WINDOW:
        assert api.set_search_range(0, 0, sr, x, y, w, h) == gc.LAST_WINDOW[size]
    engine.set_lambda(57.9)
    lq = engine.lambda_q16
    with fh.mkplane(engine, cur, w, h, bd) as pc, fh.mkplane(engine, ref, w, h, bd) as pr, fh.mkplane(engine, ref2, w, h, bd) as pr2:
        for fen in (0, 1):
            mv, sad = engine.search_frame(pc, pr, sr, pred, fen=fen)
            same_tables((mv, sad), oracle_search(oracle_lib, cur, ref, w, h, sr, pred, lq, fen, bd), ("search", fen))
        for had in (1, 0):
            got = engine.refine_frame(pc, pr, sr, mv, pred, use_hadamard=bool(had))
            same_tables(got, oracle_lib.refine_frame(cur, ref, (m, m), w, h, mv, pred, lq, had, bd, n_threads=8), ("refine", had))
        if size != gc.ODD:
            return
        dev = torch.device("cuda", 0)
        # two different pairs in one launch: (cur, ref) and (ref, ref2), each with its own predictors
        preds = np.stack([pred, gc.predictors(w, h, seed=5)])
        d_pred = torch.from_numpy(preds).to(dev)
        d_mv, d_sad = fh.device_tables(2, n, dev)
        torch.cuda.synchronize()
        fp = api.FrameParams(sr, 1, bd, 0, n)
        engine.search_pairs_device([pc, pr], [pr, pr2], fp, d_pred.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), 0)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(((cur, ref), (ref, ref2))):
            same_tables((d_mv[i].cpu().numpy(), d_sad[i].cpu().numpy().view(np.uint32)), oracle_search(oracle_lib, a, b, w, h, sr, preds[i], lq, 1, bd), ("pairs", i))
        # two references of one picture in one launch
        d_mv.zero_(); d_sad.zero_()
        torch.cuda.synchronize()
        engine.search_frame_multi_device(pc, [pr, pr2], fp, d_pred.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), 0)
        torch.cuda.synchronize()
        for i, b in enumerate((ref, ref2)):
            same_tables((d_mv[i].cpu().numpy(), d_sad[i].cpu().numpy().view(np.uint32)), oracle_search(oracle_lib, cur, b, w, h, sr, preds[i], lq, 1, bd), ("multi", i))
        # a CTU sub-range of the frame form: the bottom-left and the corner CTU
        sub = engine.search_frame(pc, pr2, sr, preds[1], fen=0, ctu_first=2, ctu_count=2)
        same_tables(sub, oracle_search(oracle_lib, cur, ref2, w, h, sr, preds[1], lq, 0, bd, 2, 2), "sub-range")
        qsub = engine.refine_frame(pc, pr2, sr, sub[0], preds[1], ctu_first=2, ctu_count=2)
        same_tables(qsub, oracle_lib.refine_frame(cur, ref2, (m, m), w, h, sub[0], preds[1], lq, 1, bd, ctu_first=2, ctu_count=2), "refined sub-range")


# ---- 3: weighted, bi and weighted bi-directional search and refinement -------------------------------------------------------------------------
@pytest.mark.parametrize("bd", BDS)
@pytest.mark.parametrize("size", [gc.ODD, gc.NARROW])
def test_weighted_search_and_refinement(engine, oracle_lib, size, bd):
    from hmme import api
    w, h = size
    sr, n, m = gc.SEARCH_RANGE[size], gc.n_ctus(w, h), margin()
    cx_n, cy_n = gc.dims(w, h)
    wp = at(FADE, bd)
    assert api.weight_check(bd, wp, True) == 0
    cur, ref = pictures(w, h, bd, seed=4300 + w + bd)
    pred = gc.predictors(w, h, seed=7)
    engine.set_lambda(57.9)
    lq = engine.lambda_q16
    with fh.mkplane(engine, cur, w, h, bd) as pc, fh.mkplane(engine, ref, w, h, bd) as pr:
        mv, sad = engine.search_frame_w(pc, pr, sr, wp, pred)
        same_tables((mv, sad), fh.oracle_search_w(oracle_lib, cur, ref, w, h, sr, pred, lq, bd, wp, range(n)), "search_w")
        blocks = np.ascontiguousarray(cur[m:m + 64 * cy_n, m:m + 64 * cx_n])        # the CTU blocks, partial ones completed by the replicated border
        for had in (1, 0):
            got = engine.refine_frame_w(pc, pr, sr, wp, mv, pred, use_hadamard=bool(had))
            same_tables(got, fh.oracle_origin_refine_w(oracle_lib, blocks, ref, w, h, mv, pred, lq, had, bd, wp, range(n)), ("refine_w", had))


@pytest.mark.parametrize("bd", BDS)
@pytest.mark.parametrize("size", [gc.ODD, gc.NARROW])
def test_bi_search_and_refinement(engine, oracle_lib, hmo, size, bd):
    w, h = size
    sr, m = gc.SEARCH_RANGE[size], margin()
    engine.set_lambda(57.9)
    r = fh.run_bi_search(engine, oracle_lib, hmo, w, h, bd, sr, 1, 64, seed=4400 + w + bd)          # asserts the search against the oracle on the origin
    assert (r["field"] & 3).any()                                                                    # fractional MVs in the other prediction
    org_padded = np.ascontiguousarray(np.pad(r["org"], m))
    with fh.mkplane(engine, r["cur"], w, h, bd) as pc, fh.mkplane(engine, r["ref"], w, h, bd) as pr, fh.mkplane(engine, r["other"], w, h, bd) as po:
        for had in (1, 0):
            got = engine.refine_frame_bi(pc, pr, po, sr, r["field"], r["mv"], center_q=r["center"], pred_q=r["pred"], use_hadamard=bool(had))
            want = oracle_lib.refine_frame(org_padded, r["ref"], (m, m), w, h, r["mv"], r["pred"], engine.lambda_q16, had, bd, n_threads=8)
            same_tables(got, want, ("refine_bi", had))


@pytest.mark.parametrize("bd", BDS)
@pytest.mark.parametrize("size", [gc.ODD, gc.NARROW])
def test_weighted_bi_search_and_refinement(engine, oracle_lib, hmo, size, bd):
    from test_gpu_bipred_wp import run_case
    w, h = size
    engine.set_lambda(57.9)
    r = run_case(engine, oracle_lib, hmo, w, h, bd, gc.SEARCH_RANGE[size], at(FADE, bd), at(FADE_OTHER, bd), 64, seed=4500 + w + bd, had=(1, 0))
    assert (r["field"] & 3).any() and "cost" in r
    unweighted = bwm.pred_picture(hmo, r["other"], w, h, bd, r["field"], bwm.IDENT)
    assert not np.array_equal(r["org"], bwm.origin(r["cur"], unweighted, w, h))     # the other list's weight acts on the origin


@pytest.mark.parametrize("size,bd,per", [(gc.ODD, 8, 64), (gc.ODD, 10, 64), (gc.NARROW, 8, 64), (gc.NARROW, 10, 64), (gc.ODD, 8, 1), (gc.MIN1, 8, 64)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_bi_search_and_refinement_over_several_references(engine, hmo, size, bd, per):
    """hmme_search / refine_frame_bi_refs: two references in the searched list against two planes of DIFFERENT content in the other list, whose
    index changes from 8x8 block to 8x8 block -- the blocks that straddle the picture edge read different planes -- every CTU against the
    per-CTU calls on the origin; 9 x 9 with one reference"""
    from test_gpu_bipred_refs import check_against_the_per_ctu_calls, checkerboard, unrelated
    w, h = size
    n = gc.n_ctus(w, h)
    n_refs = 1 if size == gc.MIN1 else 2
    engine.set_lambda(57.9)
    pics = pictures(w, h, bd, seed=4550 + w + bd + per, n=n_refs) + unrelated(w, h, bd, 4560 + w + bd, 2)
    field = fh.random_field(n, per, 4570 + w + bd)
    ref_field = checkerboard(n, per, 2, w)
    assert set(ref_field.reshape(-1).tolist()) == ({0, 1} if per == 64 or n > 1 else {0})
    if per == 64:                                                                   # the blocks that begin inside the picture and end beyond it name both planes
        straddle = set()
        for c in range(n):
            x0, y0 = gc.ctu_origin(c, w)
            straddle |= {int(ref_field[c, b]) for b in range(64) if x0 + (b % 8) * 8 < w and y0 + (b // 8) * 8 < h
                         and (x0 + (b % 8) * 8 + 8 > w or y0 + (b // 8) * 8 + 8 > h)}
        assert straddle == {0, 1}
    refs_i, others_i = list(range(1, 1 + n_refs)), [1 + n_refs, 2 + n_refs]
    for had in ((True, False) if size == gc.NARROW else (True,)):
        mv, sad, qmv, cost = check_against_the_per_ctu_calls(engine, hmo, w, h, bd, pics, refs_i, others_i, field, ref_field, 4580 + w, fen=int(bd == 8), had=had,
                                                             sr=gc.SEARCH_RANGE[size])
    assert mv.shape == (n_refs, n, 593, 2) and (n_refs == 1 or not np.array_equal(mv[0], mv[1]))
    # the index matters at the edge: the last CTU read from plane 0 alone gives another table
    planes = [fh.mkplane(engine, p, w, h, bd) for p in pics]
    try:
        flat, _ = engine.search_frame_bi_refs(planes[0], [planes[i] for i in refs_i], [planes[i] for i in others_i], gc.SEARCH_RANGE[size], field, np.zeros_like(ref_field),
                                              fen=int(bd == 8), ctu_first=n - 1, ctu_count=1)
        again, _ = engine.search_frame_bi_refs(planes[0], [planes[i] for i in refs_i], [planes[i] for i in others_i], gc.SEARCH_RANGE[size], field, ref_field,
                                               fen=int(bd == 8), ctu_first=n - 1, ctu_count=1)
        assert not np.array_equal(flat, again)
    finally:
        for p in planes:
            p.close()


# ---- 4: decisions --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [gc.ODD, gc.NARROW, gc.MIN1])
def test_decisions(engine, mv_cost, size):
    from hmme import api
    w, h = size
    n = gc.n_ctus(w, h)
    engine.set_lambda_q16(srm.LAMBDA_Q16)
    lq = engine.lambda_q16
    straddle = 0
    # the partition decision: both field layouts, both MV units, with and without the MV cost, CUs of 32 x 32 at least (they straddle the edge)
    mv, cost = sm.random_tables(n, seed=4600 + w, noise=16)
    pred = gc.predictors(w, h, seed=11, max_pel=10)
    for per in (64, 256):
        for unit in (0, 1):
            for price in (0, 1):
                for max_depth in (3, 1):
                    sel = api.SelectParams(per, mv_unit=unit, price_mv=price, max_depth=max_depth, cu_cost=40, pu_cost=12)
                    got = engine.select_frame(w, h, sel, mv, cost, pred)
                    mf, ms, mc, _ = sm.select_picture(mv, cost, sel, w, h, 0, pred, lq, mv_cost)
                    for g, o, name in zip(got, (mf, ms, mc), ("field", "slot", "cost")):
                        assert np.array_equal(g, o), (per, unit, price, max_depth, name)
                    assert (ms == sm.NO_SLOT).any() and (ms != sm.NO_SLOT).any()
                    if max_depth == 1:
                        straddle += gc.straddling_leaves(ms, w, h, per)
    assert straddle >= 8
    # a sub-range into the caller's arrays: the other CTUs keep their values
    if n > 1:
        sel = api.SelectParams(64, max_depth=1)
        f0, s0, c0 = np.full((n, 64, 2), 0x5A5A, np.int16), np.full((n, 64), 0x1234, np.uint16), np.full(n, 0x0BADBEEF, np.uint32)
        engine.select_frame(w, h, sel, mv[1:3], cost[1:3], None, ctu_first=1, ctu_count=2, field=f0, slot=s0, ctu_cost=c0)
        mf, ms, mc, _ = sm.select_picture(mv[1:3], cost[1:3], sel, w, h, 1)
        assert np.array_equal(f0[1:3], mf) and np.array_equal(s0[1:3], ms) and np.array_equal(c0[1:3], mc)
        assert (f0[[0, 3]] == 0x5A5A).all() and (s0[[0, 3]] == 0x1234).all() and (c0[[0, 3]] == 0x0BADBEEF).all()
    # the reference per PU, three references
    rmv, rcost = srm.random_ref_tables(3, n, seed=4610 + w)
    rpred = srm.ref_predictors(3, n, seed=4611 + w)
    ref_cost = srm.hm_ref_cost(3, lq)
    for per, unit, price, max_depth in ((64, 0, 0, 3), (256, 1, 1, 3), (64, 0, 1, 1), (256, 0, 0, 1)):
        sel = api.SelectParams(per, mv_unit=unit, price_mv=price, max_depth=max_depth)
        got = engine.select_refs_frame(w, h, sel, rmv, rcost, ref_cost, rpred)
        want = srm.select_refs_picture(rmv, rcost, sel, w, h, ref_cost, 0, rpred, lq, mv_cost)
        for g, o, name in zip(got, want[:4], ("field", "ref", "slot", "cost")):
            assert np.array_equal(g, o), ("refs", per, unit, price, max_depth, name)
        assert (want[2] == sm.NO_SLOT).any() and ((want[1] == srm.NO_REF) == (want[2] == sm.NO_SLOT)).all()
        assert n == 1 or len(set(want[1][want[2] != sm.NO_SLOT].tolist())) >= 2                # (a single CTU of 9 x 9 holds four CUs at most)
        assert max_depth != 1 or gc.straddling_leaves(want[2], w, h, per) >= 1
    # L0, L1 or bi per PU
    dpred = sdm.predictors(n, seed=4620 + w)
    tabs = sdm.random_dir_tables(n, n, 4621 + w, dpred, lambda_q16=lq)
    for max_depth in (3, 1):
        sel = api.SelectParams(64, max_depth=max_depth, cu_cost=40, pu_cost=12)
        got = engine.select_dirs_frame(w, h, sel, api.DirParams(*sdm.HM_BITS), *tabs, dpred)
        want = sdm.select_dirs_picture(*tabs, sel, w, h, sdm.HM_BITS, 0, dpred, lq)
        for g, o, name in zip(got, want, ("field", "dir", "slot", "cost")):
            assert np.array_equal(g, o), ("dirs", max_depth, name)
        assert (want[2] == sm.NO_SLOT).any() and ((want[1] == sdm.NO_DIR) == (want[2] == sm.NO_SLOT)).all()
        assert n == 1 or len(set(want[1][want[2] != sm.NO_SLOT].tolist())) >= 2
        assert max_depth != 1 or gc.straddling_leaves(want[2], w, h, 64) >= 1


@pytest.mark.parametrize("size", [gc.ODD, gc.NARROW, gc.MIN1])
def test_direction_and_reference_decision(engine, size):
    """hmme_select_dirs_refs_device, two references per list and list 1's reference 0 masked out, against select_dirs_refs_model: blocks of
    CUs whose origin lies outside the picture carry no direction and no reference; a CU at the picture edge is decided bi"""
    import select_dirs_refs_model as drm
    from hmme import api
    from test_gpu_select_dirs_refs import compare, one_picture
    w, h = size
    n = gc.n_ctus(w, h)
    engine.set_lambda_q16(drm.LAMBDA_Q16)
    pred = drm.predictors(2, n, seed=4650 + w)
    tabs = one_picture(2, w, h, 4651 + w, pred)
    edge_bi = 0
    for max_depth in (3, 1):
        sel = api.SelectParams(64, max_depth=max_depth, cu_cost=40, pu_cost=12)
        mf, mr, md, ms, _ = compare(engine, w, h, tabs, sel, [drm.hm_bits(2, 2, 0b10)], pred[None])
        gone = ms[0] == sm.NO_SLOT
        assert gone.any() and (md[0][gone] == drm.NO_DIR).all() and (mr[0][:, gone] == drm.NO_REF).all() and (mf[0][:, gone] == 0).all()
        assert (md[0][~gone] != drm.NO_DIR).all() and 0 not in set(mr[0, 1][md[0] == 2].tolist())
        for c in range(n):
            x0, y0 = gc.ctu_origin(c, w)
            for v in np.unique(ms[0, c][~gone[c]]):
                _, (qx, qy, qs) = rm.slot_geometry(int(v))
                at_edge = x0 + qx < w <= x0 + qx + qs or y0 + qy < h <= y0 + qy + qs
                edge_bi += int(at_edge and (md[0, c][ms[0, c] == v] == 3).all())
        assert max_depth != 1 or gc.straddling_leaves(ms[0], w, h, 64) >= 1
    assert edge_bi >= 1


# ---- 5: luma prediction --------------------------------------------------------------------------------------------------------------------------
def luma_field(w, h, per, seed):
    """random MVs within a few pels, all 16 phases; the first and the last block of every CTU far away, in another direction per CTU"""
    n = gc.n_ctus(w, h)
    f = fh.random_field(n, per, seed)
    for c in range(n):
        if per == 64 or c % 2 == 0:                      # one MV per CTU: every other CTU keeps its near MV
            f[c, 0] = [v * gc.FAR for v in gc.DIRECTIONS[c % 8]]
            f[c, per - 1] = [v * gc.FAR + 1 for v in gc.DIRECTIONS[(c + 5) % 8]]
    return f


def check_image_forms(w, h, bd, entry, model, what):
    """the C entry of a _frame prediction form into sentinel-filled images of stride w (packed) and w + 3, over the whole picture and over
    CTUs 1 and 2: the picture columns equal `model` (an [h, w] array that holds the sentinel where the form writes nothing), the spare
    columns and the samples outside the CTU range keep the sentinel.  entry(fp, address, stride in samples) -> the return code"""
    from hmme import api
    dt, fill = sentinel(bd)
    for spare in (0, 3):
        for first, count in ((0, -1), (1, 2)):
            inside = rm.range_mask(w, h, first, count)
            img = np.full((h, w + spare), fill, dt)
            assert entry(api.FrameParams(1, 0, bd, first, count), img.ctypes.data, w + spare) == 0, what
            want = np.where(inside, model, fill)
            assert np.array_equal(img[:, :w], want), (what, spare, first, np.argwhere(img[:, :w] != want)[:4])
            assert (img[:, w:] == fill).all() and (want != fill).any()


@pytest.mark.parametrize("per", [1, 64])
@pytest.mark.parametrize("bd", BDS)
@pytest.mark.parametrize("size", [gc.ODD, gc.NARROW, gc.EVEN])
def test_luma_prediction(engine, hmo, size, bd, per):
    import torch
    from hmme import api
    w, h = size
    n, L, dev = gc.n_ctus(w, h), engine.L, torch.device("cuda", 0)
    dt, fill = sentinel(bd)
    arrays = pictures(w, h, bd, seed=4700 + w + bd, n=3)[1:]
    wps = [at(FADE, bd), at(FADE_OTHER, bd), at((-20, 200, 5, 16), bd)]
    assert api.predict_bi_weight_check(bd, wps[0], wps[1]) == 0
    rng = np.random.default_rng(4701 + w + bd + per)
    field = np.stack([luma_field(w, h, per, 4702 + w + bd + 10 * l) for l in range(2)])
    ref_field = rng.choice(np.array([0, 1, 2, 3, 0xFF], np.uint8), size=(n, per))
    dirs = rng.choice(np.array([1, 2, 3, 3, 0, 0xFF], np.uint8), size=(n, per))
    if per == 64:
        ref_field[0, :5], dirs[0, :5] = (0, 1, 2, 3, 0xFF), (1, 2, 3, 0, 0xFF)
    else:
        ref_field[:4, 0], dirs[:4, 0] = (1, 0, 2, 0xFF), (3, 1, 2, 0xFF)
    new = lambda: np.full((h, w), fill, np.int64)
    uni = [fh.oracle_prediction(hmo, a, w, h, bd, field[0])[:h, :w] for a in arrays]
    g = 64 if per == 1 else 8
    block_ref = np.full((64 * gc.dims(w, h)[1], 64 * gc.dims(w, h)[0]), 0xFF, np.uint8)
    for c in range(n):
        x0, y0 = gc.ctu_origin(c, w)
        for b in range(per):
            block_ref[y0 + (b // 8) * g:y0 + (b // 8) * g + g, x0 + (b % 8) * g:x0 + (b % 8) * g + g] = ref_field[c, b]
    block_ref = block_ref[:h, :w]
    refs_model = new()
    for r in range(3):
        refs_model[block_ref == r] = uni[r][block_ref == r]
    models = {"pairs": uni[0].astype(np.int64),
              "pairs_w": bwm.pred_picture(hmo, arrays[0], w, h, bd, field[0], wps[0])[:h, :w],
              "refs": refs_model,
              "refs_w": pbw.refs_picture(hmo, arrays, w, h, bd, field[0], ref_field, wps, new()),
              "bi": pbm.pred_picture(hmo, arrays[:2], w, h, bd, field, dirs, new()),
              "bi_w": pbw.pred_picture(hmo, arrays[:2], w, h, bd, field, dirs, wps[:2], new())}
    assert all((m != fill).any() for m in models.values()) and (models["refs"] == fill).any() and (models["bi"] == fill).any()
    assert len({m.tobytes() for m in models.values()}) == 6
    planes = [fh.mkplane(engine, a, w, h, bd) for a in arrays]
    try:
        hs = api._handles(planes)
        f0, f2, rf, df = (np.ascontiguousarray(a) for a in (field[0], field, ref_field, dirs))
        wa = engine._weights(wps)
        w0, w1 = (api.Weight(*v) for v in wps[:2])
        fptr = lambda fp: C.byref(fp)
        entries = {"pairs": lambda fp, out, s: L.hmme_predict_frame(engine.h, planes[0].h, fptr(fp), f0.ctypes.data, per, out, s),
                   "pairs_w": lambda fp, out, s: L.hmme_predict_frame_w(engine.h, planes[0].h, fptr(fp), C.byref(w0), f0.ctypes.data, per, out, s),
                   "refs": lambda fp, out, s: L.hmme_predict_refs_frame(engine.h, hs, 3, fptr(fp), f0.ctypes.data, rf.ctypes.data, per, out, s),
                   "refs_w": lambda fp, out, s: L.hmme_predict_refs_w_frame(engine.h, hs, 3, fptr(fp), wa, f0.ctypes.data, rf.ctypes.data, per, out, s),
                   "bi": lambda fp, out, s: L.hmme_predict_bi_frame(engine.h, planes[0].h, planes[1].h, fptr(fp), f2.ctypes.data, df.ctypes.data, per, out, s),
                   "bi_w": lambda fp, out, s: L.hmme_predict_bi_w_frame(engine.h, planes[0].h, planes[1].h, fptr(fp), C.byref(w0), C.byref(w1), f2.ctypes.data,
                                                                         df.ctypes.data, per, out, s)}
        for name, entry in entries.items():
            check_image_forms(w, h, bd, entry, models[name], (name, per))
        # the Python methods, packed images of their own
        assert np.array_equal(engine.predict_frame(planes[0], field[0]), models["pairs"])
        assert np.array_equal(engine.predict_frame_w(planes[0], wps[0], field[0]), models["pairs_w"])
        # the device forms once, CTUs 1.., at a byte pitch that is odd where samples are bytes
        pitch = ((w + 3) | 1) if bd == 8 else 2 * (w + 3)
        cols = pitch // (1 if bd == 8 else 2)
        first, count = 1, n - 1
        fp = api.FrameParams(1, 0, bd, first, count)
        inside = rm.range_mask(w, h, first, count)
        d_f2 = torch.from_numpy(f2).to(dev)
        d_rf, d_df = torch.from_numpy(rf).to(dev), torch.from_numpy(df).to(dev)
        image = lambda: torch.full((h, cols), fill if bd == 8 else fill - 0x10000, dtype=torch.uint8 if bd == 8 else torch.int16, device=dev)
        imgs = {k: image() for k in ("pairs", "pairs_w", "refs", "refs_w", "bi", "bi_w")}
        torch.cuda.synchronize()
        engine.predict_pairs_device([planes[0]], fp, d_f2.data_ptr(), per, [imgs["pairs"].data_ptr()], pitch)
        engine.predict_pairs_w_device([planes[0]], fp, [wps[0]], d_f2.data_ptr(), per, [imgs["pairs_w"].data_ptr()], pitch)
        engine.predict_refs_device(planes, fp, d_f2.data_ptr(), d_rf.data_ptr(), per, imgs["refs"].data_ptr(), pitch)
        engine.predict_refs_w_device(planes, fp, wps, d_f2.data_ptr(), d_rf.data_ptr(), per, imgs["refs_w"].data_ptr(), pitch)
        engine.predict_bi_device([planes[0]], [planes[1]], fp, d_f2.data_ptr(), d_df.data_ptr(), per, [imgs["bi"].data_ptr()], pitch)
        engine.predict_bi_w_device([planes[0]], [planes[1]], fp, [wps[0]], [wps[1]], d_f2.data_ptr(), d_df.data_ptr(), per, [imgs["bi_w"].data_ptr()], pitch)
        torch.cuda.synchronize()
        for name, t in imgs.items():
            got = t.cpu().numpy().view(dt)
            want = np.where(inside, models[name], fill)
            assert np.array_equal(got[:, :w], want), ("device", name, per, np.argwhere(got[:, :w] != want)[:4])
            assert (got[:, w:] == fill).all()
    finally:
        for p in planes:
            p.close()


@pytest.mark.parametrize("bd", BDS)
@pytest.mark.parametrize("size", [gc.ODD, gc.NARROW, gc.EVEN])
def test_luma_prediction_of_a_b_picture_with_several_references(engine, hmo, size, bd):
    """hmme_predict_bi_refs_frame with two planes per list against predict_bi_refs_model, into images whose stride exceeds the width: one MV
    per block with all three directions and every plane named; one far MV per CTU in each of the eight directions, every CTU bi from another
    pair of planes, so that a block averages the replicated borders of two different planes"""
    import predict_bi_refs_model as pbrm
    from hmme import api
    from test_gpu_predict_bi_refs import inputs, textures
    w, h = size
    n, L = gc.n_ctus(w, h), engine.L
    dt, fill = sentinel(bd)
    pics = textures(w, h, bd, 4750 + w + bd, 4)
    planes = [fh.mkplane(engine, a, w, h, bd) for a in pics]
    try:
        h0, h1 = api._handles(planes[:2]), api._handles(planes[2:])
        new = lambda: np.full((h, w), fill, np.int64)

        def run(field, dirs, refs, per, what):
            f, d, r = (np.ascontiguousarray(a) for a in (field, dirs, refs))
            model = pbrm.pred_picture(hmo, pics[:2], pics[2:], w, h, bd, f, d, r, new())
            check_image_forms(w, h, bd, lambda fp, out, s: L.hmme_predict_bi_refs_frame(engine.h, h0, 2, h1, 2, C.byref(fp), f.ctypes.data, d.ctypes.data, r.ctypes.data,
                                                                                         per, out, s), model, what)
            return model

        field, dirs, refs = inputs(w, h, 64, 4751 + w + bd, 2, 2)
        model = run(field, dirs, refs, 64, "blocks")
        live = [(c, b) for c in range(n) for b in range(64) if dirs[c, b] in (1, 2, 3) and gc.ctu_origin(c, w)[0] + (b % 8) * 8 < w and gc.ctu_origin(c, w)[1] + (b // 8) * 8 < h
                and all(not (dirs[c, b] >> l) & 1 or refs[l, c, b] < 2 for l in range(2))]
        assert {int(dirs[c, b]) for c, b in live} == {1, 2, 3} and (model == fill).any()
        assert all({int(refs[l, c, b]) for c, b in live if (dirs[c, b] >> l) & 1} == {0, 1} for l in range(2))
        # the border: list 0 and list 1 far away in the same direction, the pair of planes changing from CTU to CTU
        c = np.arange(n)
        far_refs = np.stack([c % 2, (c // 2 + 1) % 2]).astype(np.uint8).reshape(2, n, 1)
        far_dirs = np.full((n, 1), 3, np.uint8)
        seen = set()
        for k, f in enumerate(gc.far_fields(w, h)):
            both = np.stack([f, f + np.array([3, 2], np.int16)])                  # another phase in list 1
            model = run(both, far_dirs, far_refs, 1, ("far", k))
            alone = [pbrm.pred_picture(hmo, pics[:2], pics[2:], w, h, bd, both, np.full((n, 1), l + 1, np.uint8), far_refs, new()) for l in range(2)]
            assert not np.array_equal(alone[0], alone[1]) and not np.array_equal(model, alone[0]) and not np.array_equal(model, alone[1])
            seen.add(model.tobytes())
        assert len(seen) == 8 and (n == 1 or len(set(map(tuple, far_refs[:, :, 0].T.tolist()))) >= 2)
    finally:
        for p in planes:
            p.close()


# ---- 6: chroma -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [1, 64])
@pytest.mark.parametrize("bd", BDS)
@pytest.mark.parametrize("size", [gc.EVEN, gc.EVEN[::-1]])
def test_chroma_prediction(engine, hmo, size, bd, per):
    from hmme import api
    from test_gpu_predict_chroma import Chroma, make_dirs, make_field, wset
    w, h = size
    cw, chh, L = w // 2, h // 2, engine.L
    assert cw % 2 == 1 and chh % 2 == 1
    dt, fill = sentinel(bd)
    ch = Chroma(engine, w, h, bd, seed=4800 + w + bd, n=2)
    try:
        field = np.ascontiguousarray(np.stack([make_field(w, h, per, 4801 + w + bd + 50 * l, rot=23 * l) for l in range(2)]))
        dirs = np.ascontiguousarray(make_dirs(w, h, per, 4803 + w + bd))
        ref_field = np.ascontiguousarray((dirs & 1).astype(np.uint8))
        ref_field[dirs == 0xFF] = 0xFF
        f0 = np.ascontiguousarray(field[0])
        hw = wset("hm_like", bd)                                                    # hw[component] = (list 0, list 1)
        new = lambda: tuple(np.full((chh, cw), fill, np.int64) for _ in range(2))
        hs = lambda planes: api._handles(planes)
        wts = lambda ws: engine._weights(ws)
        for weighted in (False, True):
            pw = [hw[0][0], hw[1][0]] if weighted else None                         # Cb, Cr of list 0
            rw = [hw[0][0], hw[1][0], hw[0][1], hw[1][1]] if weighted else None     # cb0, cr0, cb1, cr1
            b0, b1 = ([hw[0][l], hw[1][l]] if weighted else None for l in range(2))
            models = {"pairs": cm.pairs_picture(hmo, ch.arrays[0], w, h, bd, f0, new(), pw),
                      "refs": cm.refs_picture(hmo, ch.comps((0, 1)), w, h, bd, f0, ref_field, new(), hw if weighted else None),
                      "bi": cm.bi_picture(hmo, ch.comps((0, 1)), w, h, bd, field, dirs, new(), hw if weighted else None)}
            opt = lambda ws: None if ws is None else wts(ws)
            entries = {"pairs": lambda fp, outs, s: L.hmme_predict_chroma_frame(engine.h, hs(ch.planes[0]), w, h, C.byref(fp), opt(pw), f0.ctypes.data, per, outs, s),
                       "refs": lambda fp, outs, s: L.hmme_predict_chroma_refs_frame(engine.h, hs(ch.flat((0, 1))), 2, w, h, C.byref(fp), opt(rw), f0.ctypes.data,
                                                                                    ref_field.ctypes.data, per, outs, s),
                       "bi": lambda fp, outs, s: L.hmme_predict_chroma_bi_frame(engine.h, hs(ch.planes[0]), hs(ch.planes[1]), w, h, C.byref(fp), opt(b0), opt(b1),
                                                                                field.ctypes.data, dirs.ctypes.data, per, outs, s)}
            for name, entry in entries.items():
                assert all((m != fill).any() for m in models[name]) and not np.array_equal(*models[name])
                for stride in (65, 68):
                    for first, count in ((0, -1), (1, 2)):
                        inside = rm.range_mask(w, h, first, count)[::2, ::2]        # the chroma samples of the luma CTUs
                        imgs = [np.full((chh, stride), fill, dt) for _ in range(2)]
                        outs = (C.c_void_p * 2)(*[i.ctypes.data for i in imgs])
                        assert entry(api.FrameParams(1, 0, bd, first, count), outs, stride) == 0, (name, weighted, stride)
                        for c in range(2):
                            want = np.where(inside, models[name][c], fill)
                            assert np.array_equal(imgs[c][:, :cw], want), (name, weighted, stride, first, c, np.argwhere(imgs[c][:, :cw] != want)[:4])
                            assert (imgs[c][:, cw:] == fill).all()
    finally:
        ch.close()


def test_chroma_refuses_odd_luma_sizes(engine):
    """101 x 71 and 16 x 15: 4:2:0 needs an even luma size; nothing is written"""
    from hmme import api
    L = engine.L
    prev = L.hmme_set_error_printing(engine.h, 0)
    planes = {(101, 71): [engine.plane(50, 35) for _ in range(4)], (16, 15): [engine.plane(8, 8) for _ in range(4)]}
    try:
        for (w, h), ps in planes.items():
            n = gc.n_ctus(w, h)
            field, dirs = np.zeros((2, n, 64, 2), np.int16), np.full((n, 64), 3, np.uint8)
            imgs = [np.full((ps[0].height, ps[0].width), 0x5C, np.uint8) for _ in range(2)]
            outs = (C.c_void_p * 2)(*[i.ctypes.data for i in imgs])
            fp = api.FrameParams(1, 0, 8, 0, -1)
            cw = ps[0].width
            assert L.hmme_predict_chroma_frame(engine.h, api._handles(ps[:2]), w, h, C.byref(fp), None, field.ctypes.data, 64, outs, cw) == ERR_ARG
            assert b"hmme_predict_chroma_frame" in L.hmme_last_error(engine.h)
            assert L.hmme_predict_chroma_refs_frame(engine.h, api._handles(ps), 2, w, h, C.byref(fp), None, field.ctypes.data, dirs.ctypes.data, 64, outs, cw) == ERR_ARG
            assert L.hmme_predict_chroma_bi_frame(engine.h, api._handles(ps[:2]), api._handles(ps[2:]), w, h, C.byref(fp), None, None, field.ctypes.data,
                                                  dirs.ctypes.data, 64, outs, cw) == ERR_ARG
            assert b"hmme_predict_chroma_bi_frame" in L.hmme_last_error(engine.h)
            assert all((i == 0x5C).all() for i in imgs)
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for ps in planes.values():
            for p in ps:
                p.close()


# ---- 7: residual ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("size", [gc.ODD, gc.NARROW, gc.MIN1])
def test_residual(engine, hmo, size, bd):
    from hmme import api
    from test_gpu_residual import compare
    w, h = size
    n = gc.n_ctus(w, h)
    engine.set_lambda(57.9)
    cur, ref = pictures(w, h, bd, seed=4900 + w + bd)
    cur_img = np.ascontiguousarray(area(cur, w, h))
    with fh.mkplane(engine, cur, w, h, bd) as pc, fh.mkplane(engine, ref, w, h, bd) as pr:
        # a real chain on the device: search, refinement, decision, prediction
        mv, _ = engine.search_frame(pc, pr, 8)
        qmv, cost = engine.refine_frame(pc, pr, 8, mv)
        field, _, _ = engine.select_frame(w, h, api.SelectParams(64), qmv, cost)
        pred = engine.predict_frame(pr, field)
        assert (pred != cur_img).any()
        for per, max_depth in ((64, 3), (256, 3), (64, 1), (256, 1)):
            _, slot, _ = engine.select_frame(w, h, api.SelectParams(per, max_depth=max_depth), qmv, cost)
            assert (slot == rm.NO_SLOT).any() and (slot != rm.NO_SLOT).any()
            assert max_depth != 1 or gc.straddling_leaves(slot, w, h, per) >= 1
            for had in (1, 0):
                (mpu, mcu, mctu), = compare(engine, hmo, [pc], [cur_img], [pred], bd, slot[None], per, had)      # hmme_residual_pairs_device, sentinels everywhere
                assert mctu[0].all() and (mpu[slot == rm.NO_SLOT] == 0).all() and (mcu[slot == rm.NO_SLOT] == 0).all()
                # hmme_residual_frame: packed rows of w samples in and out
                want = rm.residual_picture(hmo, cur_img, pred, w, h, bd, slot, per, had)
                got = engine.residual_frame(pc, pred, slot, per, bool(had))
                for g, o, name in zip(got, want, ("resid", "pu", "cu", "ctu")):
                    assert np.array_equal(g, o), ("frame", per, max_depth, had, name)
            if size == gc.NARROW:
                # CTU 1 holds one sample column: its blocks beyond column 0 lie outside the picture and still carry their CU's totals
                g = 8 if per == 64 else 4
                assert 64 + g > w and slot[1, 0] != rm.NO_SLOT
                if per == 256 or max_depth == 1:                     # (8 x 8 CUs in 8 x 8 blocks: block 1 is a CU of its own, which does not exist)
                    _, (qx, qy, qs) = rm.slot_geometry(int(slot[1, 1]))
                    assert (qx, qy) == (0, 0) and rm.slot_geometry(int(slot[1, 0]))[1] == (qx, qy, qs)
                    column = cur_img[:qs, 64:65].astype(np.int64) - pred[:qs, 64:65]
                    assert mcu[1, 1] == mcu[1, 0] == rm.sse(column, bd) and (mcu[1, 0] != 0 or bd > 8)
        # without a slot map: every block its own PU and CU
        for per in (64, 256):
            for had in (1, 0):
                compare(engine, hmo, [pc], [cur_img], [pred], bd, None, per, had)
            want = rm.residual_picture(hmo, cur_img, pred, w, h, bd, None, per, 1)
            got = engine.residual_frame(pc, pred, None, per, True)
            for g, o, name in zip(got, want, ("resid", "pu", "cu", "ctu")):
                assert np.array_equal(g, o), ("frame without a map", per, name)
        # a sub-range of the frame form and strides beyond the width, through the C entry
        if n > 1:
            dt, fill = sentinel(bd)
            wide = np.full((h, w + 3), fill, dt); wide[:, :w] = pred
            r1 = np.full((h, w + 5), 0x1111, np.int16); p1 = np.full((n, 64), 7, np.uint32); c1 = p1.copy(); t1 = np.full((n, 2), 7, np.uint32)
            fp = api.FrameParams(1, 0, bd, 1, 2)
            assert engine.L.hmme_residual_frame(engine.h, pc.h, C.byref(fp), wide.ctypes.data, w + 3, None, 64, 1, r1.ctypes.data, w + 5, p1.ctypes.data,
                                                c1.ctypes.data, t1.ctypes.data) == 0
            md, mpu, mcu, mctu = rm.residual_picture(hmo, cur_img, pred, w, h, bd, None, 64, 1, 1, 2)
            inside = rm.range_mask(w, h, 1, 2)
            assert np.array_equal(r1[:, :w][inside], md[inside]) and (r1[:, :w][~inside] == 0x1111).all() and (r1[:, w:] == 0x1111).all()
            assert np.array_equal(p1[1:3], mpu) and np.array_equal(c1[1:3], mcu) and np.array_equal(t1[1:3], mctu)
            assert (p1[[0, 3]] == 7).all() and (c1[[0, 3]] == 7).all() and (t1[[0, 3]] == 7).all()


# ---- 8: plane statistics and WP estimation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", BDS)
def test_plane_stats_at_every_row_tail(engine, bd):
    """(64 + k) x 9 for k = 1..15: a row ends 1..15 samples into a 16-byte (8-sample) vector -- every partial vector, every partial dword"""
    from test_gpu_wp_estimate import make_plane
    for w, h in gc.STATS_SIZES:
        img = np.random.default_rng(5000 + w + bd).integers(0, 1 << bd, (h, w)).astype(np.int64)
        img[:, -1] = (1 << bd) - 1                          # the replicated border beyond the last column is as far from the mean as a sample gets
        want = wpm.plane_stats(img)
        with make_plane(engine, img, bd) as pl:
            assert engine.plane_stats(pl) == want, (w, h, bd)


@pytest.mark.parametrize("w,h,bd", [gc.ODD + (8,), gc.NARROW + (10,), (67, 9, 8)])
def test_wp_estimate_on_a_fade(engine, w, h, bd):
    from test_gpu_wp_estimate import check_estimate, fade, smooth
    ref = smooth(w, h, bd, seed=5100 + w)
    other = smooth(w, h, bd, seed=5101 + w)
    cur = fade(ref, 0.75, 20, bd)
    want = check_estimate(engine, cur, [ref, other], bd)                            # every sum, intermediate and weight against the model
    assert want[0]["present"] == 1 and want[0]["weight"] != 1 << want[0]["log2_denom"] and want[0]["sad_wp"] < want[0]["sad_nowp"]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_wp_estimate_420_at_every_row_tail(engine, bd):
    """the plane-set kernels' own masked last vector: luma (128 + 2k) x 18 for k = 1..15 puts chroma at (64 + k) x 9 -- every partial vector,
    every partial dword -- while luma ends 2k samples past a vector boundary in the same launch; the last column of every plane at the
    nominal maximum, as in test_plane_stats_at_every_row_tail.  Every sum, intermediate and weight against the model"""
    from test_gpu_wp_estimate import fade
    from test_gpu_wp_estimate_420 import check, picture
    top = (1 << bd) - 1
    for w, h in gc.STATS_SIZES_420:
        ref = picture(w, h, bd, seed=5150 + w + bd)
        cur = tuple(fade(p, 0.75, 12, bd) for p in ref)
        for p in cur + ref:
            p[:, -1] = top
        (e,) = check(engine, cur, [ref], bd)
        assert all(x["cur_ac"] > 0 and x["ref_ac"] > 0 and x["sad_nowp"] > 0 for x in e), (w, h)
        assert (cur[0].shape[1] - 128, cur[1].shape[1] - 64) == (w - 128, (w - 128) // 2) and all((p[:, -1] == top).all() for p in cur + ref)


def test_wp_estimate_420_over_two_rounds_of_workgroups(engine):
    """16 references of 2048 x 50 at 8 bit: 51 planes / 48 pairs side by side cap a launch at 20 / 21 row blocks per plane; luma has 25 -- its
    row loop iterates twice -- and chroma (1024 x 25) 7, so that the workgroups beyond its block 6 leave at once in the same launch
    (tests/test_geometry_cpu.py asserts this arithmetic against geometry_cases.stat_grid)"""
    from test_gpu_wp_estimate import fade
    from test_gpu_wp_estimate_420 import check, picture
    w, h, n_refs = gc.ROUNDS_420
    grids = gc.stat_grids_420(w, h, 1, n_refs)
    assert all(g[0]["rounds"] == 2 and g[1]["rounds"] == 1 and g[1]["blocks"] < g[0]["blocks"] for g in grids.values())
    cur = picture(w, h, 8, seed=5160)
    rows = np.arange(h)[:, None]
    refs = []
    for i in range(n_refs):                                                      # the fade of reference i acts on the rows of the second round alone, or of the first
        ref = tuple(fade(p, 0.6 + 0.05 * i, 2 * i - 10, 8) for p in cur)
        second = rows >= grids["stats"][0]["blocks"] * grids["stats"][0]["rows_per_block"]
        ref[0][:] = np.where(second if i % 2 else ~second, ref[0], cur[0])
        refs.append(ref)
    es = check(engine, cur, refs, 8, 7)
    assert len({(r[0]["ref_ac"], r[0]["sad_nowp"]) for r in es}) == n_refs and all(x["sad_nowp"] > 0 for r in es for x in r)


def test_wp_estimate_over_two_rounds_of_workgroups(engine):
    """16 distinct references of 1033 x 66 at 10 bit: the luma call's 17 planes / 16 pairs side by side cap a launch at 60 / 64 row blocks, the
    picture has 66 -- both row loops iterate twice -- and a row's last vector holds 2 of 16 bytes (tests/test_geometry_cpu.py asserts this
    arithmetic against geometry_cases.stat_grid).  Every sum, intermediate and weight against the model"""
    from test_gpu_wp_estimate import check_estimate, fade, smooth
    w, h, n_refs = gc.ROUNDS_LUMA
    stats, sad = gc.stat_grid(w, h, 2, 1 + n_refs), gc.stat_grid(w, h, 2, n_refs)
    assert stats["rounds"] == sad["rounds"] == 2 and stats["blocks"] == sad["blocks"] and stats["rows_per_block"] == 1
    cur = smooth(w, h, 10, seed=5170)
    second = np.arange(h)[:, None] >= stats["blocks"]
    refs = []
    for i in range(n_refs):                                                      # the fade of reference i acts on the rows of the second round alone, or of the first
        refs.append(np.where(second if i % 2 else ~second, fade(cur, 0.6 + 0.05 * i, 2 * i - 10, 10), cur))
    want = check_estimate(engine, cur, refs, 10, 7)
    assert len({(e["ref_ac"], e["sad_nowp"]) for e in want}) == n_refs and all(e["sad_nowp"] > 0 for e in want)


# ---- 9: the largest sizes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,bd", [gc.SLIVERS[0] + (8,), gc.SLIVERS[1] + (10,)])
def test_the_largest_sizes(engine, oracle_lib, hmo, w, h, bd):
    from hmme import synth
    sr, n, m = 4, 256, margin()
    assert gc.n_ctus(w, h) == n
    cur, ref, _ = synth.make_pair(w, h, seed=5200 + bd, bit_depth=bd, max_mv=3, region=64)
    cur_img = np.ascontiguousarray(area(cur, w, h))
    pred = gc.predictors(w, h, seed=13, max_pel=3)
    engine.set_lambda(57.9)
    lq = engine.lambda_q16
    table = oracle_lib.slot_table()
    rng = np.random.default_rng(5201 + bd)
    dt = sentinel(bd)[0]
    with fh.mkplane(engine, cur, w, h, bd) as pc, fh.mkplane(engine, ref, w, h, bd) as pr:
        mv, sad = engine.search_frame(pc, pr, sr, pred)
        same_tables((mv, sad), oracle_search(oracle_lib, cur, ref, w, h, sr, pred, lq, 1, bd), "search")
        qmv, cost = engine.refine_frame(pc, pr, sr, mv, pred)
        for ctu in (0, 128, 255):
            cx, cy = gc.ctu_origin(ctu, w)
            for s in rng.integers(0, 593, size=12):
                x, y, bw, bh = (int(v) for v in table[s])
                imv = (int(mv[ctu, s, 0]), int(mv[ctu, s, 1]))
                hx, hy, qx, qy, c = oracle_lib.frac_refine(cur, (m + cx + x, m + cy + y), ref, (m + cx + x, m + cy + y), bw, bh, imv,
                                                           (int(pred[ctu, 0]), int(pred[ctu, 1])), lq, 1, bd)
                assert (int(qmv[ctu, s, 0]), int(qmv[ctu, s, 1]), int(cost[ctu, s])) == (4 * imv[0] + 2 * hx + qx, 4 * imv[1] + 2 * hy + qy, c), (ctu, s)
        assert np.array_equal(engine.predict_frame(pc, np.zeros((n, 2), np.int16)), cur_img)
        field = fh.random_field(n, 64, 5202 + bd)
        got = engine.predict_frame(pr, field)
        assert np.array_equal(got, fh.oracle_prediction(hmo, ref, w, h, bd, field)[:h, :w].astype(dt))
        want = rm.residual_picture(hmo, cur_img, got, w, h, bd, None, 64, 1)
        for g, o, name in zip(engine.residual_frame(pc, got, None, 64, True), want, ("resid", "pu", "cu", "ctu")):
            assert np.array_equal(g, o), name
        assert want[0].any() and engine.plane_stats(pc) == wpm.plane_stats(cur_img)


# ---- 10: a fuzz over any size --------------------------------------------------------------------------------------------------------------------
def _fuzz_case_of_any_size(engine, oracle_lib, seed):
    """the body of test_gpu_parity._fuzz_case at a size from geometry_cases.fuzz_size: 8..200 each way, no factor 8"""
    from hmme import synth
    rng = np.random.default_rng(seed)
    w, h = gc.fuzz_size(seed)
    bd = int(rng.choice([8, 8, 10, 12, 9]))
    sr = int(rng.choice([1, 2, 3, 7, 16, 31, 64, 65, 90, 128]))
    fen = int(rng.integers(0, 2))
    n = gc.n_ctus(w, h)
    if n * (2 * sr + 1) ** 2 > 6 * 129 * 129:     # keep the oracle's share of the run in seconds
        sr = 16
    max_pel = int(rng.choice([0, 4, 40, 300]))    # far predictors: windows clipped to slivers at the picture border
    pred = synth.random_predictors(n, seed=seed, max_pel=max_pel) if max_pel else None
    cur, ref, _ = synth.make_pair(w, h, seed=seed, bit_depth=bd, max_mv=min(sr, 10), region=32, noise_sigma=float(rng.choice([0.0, 2.0])))
    lam = float(rng.choice([0.0, 3.3, 57.9, 4000.0]))
    engine.set_lambda(lam)
    m = margin()
    with engine.plane(w, h, bd) as pc, engine.plane(w, h, bd) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        mv, sad = engine.search_frame(pc, pr, sr, pred, fen=fen)
        use_had = int(rng.integers(0, 2))
        qmv, cost = engine.refine_frame(pc, pr, sr, mv, pred, use_hadamard=bool(use_had))
    tag = dict(seed=seed, w=w, h=h, bd=bd, sr=sr, fen=fen, max_pel=max_pel, lam=lam)
    omv, osad = oracle_search(oracle_lib, cur, ref, w, h, sr, pred, engine.lambda_q16, fen, bd)
    assert np.array_equal(mv, omv) and np.array_equal(sad, osad), tag
    table = oracle_lib.slot_table()
    for k in range(int(os.environ.get("HMME_FUZZ_SLOTS", "12"))):
        ctu, s = int(rng.integers(0, n)), int(rng.integers(0, 593))
        cx, cy = gc.ctu_origin(ctu, w)
        x, y, bw, bh = (int(v) for v in table[s])
        imv = (int(mv[ctu, s, 0]), int(mv[ctu, s, 1]))
        p = (int(pred[ctu, 0]), int(pred[ctu, 1])) if pred is not None else (0, 0)
        hx, hy, qx, qy, c = oracle_lib.frac_refine(cur, (m + cx + x, m + cy + y), ref, (m + cx + x, m + cy + y), bw, bh, imv, p, engine.lambda_q16, use_had, bd)
        got = (int(qmv[ctu, s, 0]), int(qmv[ctu, s, 1]), int(cost[ctu, s]))
        assert got == (4 * imv[0] + 2 * hx + qx, 4 * imv[1] + 2 * hy + qy, c), (tag, ctu, s, use_had)


def test_fuzz_frames_of_any_size_vs_oracle(engine, oracle_lib):
    """random picture sizes of 8..200 samples each way (no factor 8; at least half with an odd dimension), bit depths, search ranges 1..128, FEN,
    lambdas and predictors up to 300 pel away: integer search of every CTU and spot-checked refinement against the oracle"""
    for seed in gc.FUZZ_SEEDS:
        _fuzz_case_of_any_size(engine, oracle_lib, seed)
