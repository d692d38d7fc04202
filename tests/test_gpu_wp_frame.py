"""Explicit weighted prediction on whole pictures and picture pairs (hmme_search_pairs_w_device, hmme_refine_pairs_w_device,
hmme_search_frame_w, hmme_refine_frame_w) against the CPU oracle's per-CTU weighted search (hmo_search_ctu_w, pinned to the compiled
reference by tests/golden/wp.npz) and weighted refinement (hmo_frac_refine_w, tests/golden/frac_wp.npz).  Every comparison is
bit-exact, MVs and costs.  Pictures are sized so that no case needs more than about a minute of oracle time."""
import numpy as np
import pytest

from frame_helpers import ctu_origin, oracle_search_w

pytestmark = pytest.mark.gpu

FADE = (40, 12, 6, 32)          # w0, offset, shift, round
IDENT = (64, 0, 6, 32)


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 128)
    e.set_lambda(57.9)
    yield e
    e.close()


def weigh(a, wp):
    return ((wp[0] * a.astype(np.int64) + wp[3]) >> wp[2]) + wp[1]


def fade_pair(w, h, bd, wp, seed, max_mv=9, clip=True):
    """padded int16 planes: ref a texture, cur its moved copy seen through the weight (what the weighted search should undo)"""
    from hmme import synth
    cur, ref, _ = synth.make_pair(w, h, seed=seed, bit_depth=bd, max_mv=max_mv, region=64)
    maxv = (1 << bd) - 1
    cur = np.clip(weigh(cur, wp), 0, maxv).astype(np.int16) if clip else cur   # weighting commutes with the edge replication
    return np.ascontiguousarray(cur), ref


def planes(engine, cur, ref, w, h, bd):
    from hmme import synth
    m = synth.MARGIN
    pc, pr = engine.plane(w, h, bd), engine.plane(w, h, bd)
    if bd == 8:
        pc.upload_u8(cur[m:m + h, m:m + w].astype(np.uint8))
        pr.upload_u8(ref[m:m + h, m:m + w].astype(np.uint8))
    else:
        pc.upload_pel(cur, (m, m))
        pr.upload_pel(ref, (m, m))
    return pc, pr


def check_search(engine, oracle_lib, w, h, bd, wp, sr, seed, fen=0, cur_ref=None):
    from hmme import synth
    cur, ref = cur_ref if cur_ref is not None else fade_pair(w, h, bd, wp, seed, max_mv=min(sr, 9))
    n_ctu = ((w + 63) // 64) * ((h + 63) // 64)
    pred = synth.random_predictors(n_ctu, seed=seed + 1, max_pel=min(sr, 16))
    pc, pr = planes(engine, cur, ref, w, h, bd)
    try:
        mv, sad = engine.search_frame_w(pc, pr, sr, wp, pred, fen=fen)
    finally:
        pc.close(); pr.close()
    omv, osad = oracle_search_w(oracle_lib, cur, ref, w, h, sr, pred, engine.lambda_q16, bd, wp, range(n_ctu))
    assert np.array_equal(mv, omv), (bd, wp, sr, np.argwhere(mv != omv)[:4])
    assert np.array_equal(sad, osad), (bd, wp, sr, np.argwhere(sad != osad)[:4])
    return cur, ref, pred, mv


# 1, 2: a fade on pictures whose size is no multiple of 64 in either direction (partial CTUs on two edges and in the corner), random
# quarter-pel predictors, a search range <= 16 and one of 64 (on a smaller picture: the oracle leg)
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h,sr", [(296, 200, 12), (168, 136, 64)])
def test_fade_search_vs_oracle(engine, oracle_lib, bd, w, h, sr):
    wp = (FADE[0], FADE[1] << (bd - 8), FADE[2], FADE[3])
    check_search(engine, oracle_lib, w, h, bd, wp, sr, seed=100 + bd + sr)


# 3: weighted samples below zero (bias > 0) and a negative w0
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("wp", [(50, -90, 6, 32), (-40, 200, 6, 32), (-64, 0, 6, 32), (3, -5, 0, 0)])
def test_negative_weighted_samples_and_negative_weights(engine, oracle_lib, bd, wp):
    from hmme import api
    wp = (wp[0], wp[1] << (bd - 8), wp[2], wp[3])
    assert api.weight_check(bd, wp, 0) == 0
    lo = min(((wp[0] * v + wp[3]) >> wp[2]) + wp[1] for v in (0, (1 << bd) - 1))
    assert lo < 0 or wp[0] < 0
    check_search(engine, oracle_lib, 200, 150, bd, wp, 10, seed=300 + bd + abs(wp[0]))


def _device_tables(n_pairs, count, dev):
    import torch
    return (torch.zeros((n_pairs, count, 593, 2), dtype=torch.int16, device=dev), torch.zeros((n_pairs, count, 593), dtype=torch.int32, device=dev))


# 4: three pairs, three weights (one the identity) in one launch == three single-pair calls == the oracle; and a CTU sub-range
@pytest.mark.parametrize("bd", [8, 10])
def test_three_pairs_three_weights_in_one_launch(engine, oracle_lib, bd):
    import torch
    from hmme import api, synth
    w, h, sr = 232, 170, 14
    n_ctu = 4 * 3
    dev = torch.device("cuda", 0)
    wps = [(40, 12 << (bd - 8), 6, 32), IDENT, (-30, 180 << (bd - 8), 5, 16)]
    pics = [fade_pair(w, h, bd, wp, seed=400 + i + bd) for i, wp in enumerate(wps)]
    pred = np.stack([synth.random_predictors(n_ctu, seed=40 + i, max_pel=12) for i in range(3)])
    pl = [planes(engine, c, r, w, h, bd) for c, r in pics]
    try:
        curs, refs = [p[0] for p in pl], [p[1] for p in pl]
        d_pred = torch.from_numpy(pred).to(dev)
        for first, count in ((0, n_ctu), (5, 6)):
            fp = api.FrameParams(sr, 1, bd, first, count)
            d_mv, d_sad = _device_tables(3, count, dev)
            engine.search_pairs_w_device(curs, refs, fp, wps, d_pred.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), 0)
            torch.cuda.synchronize()
            mv, sad = d_mv.cpu().numpy(), d_sad.cpu().numpy().astype(np.uint32)
            for i in range(3):
                smv, ssad = engine.search_frame_w(curs[i], refs[i], sr, wps[i], pred[i], ctu_first=first, ctu_count=count)
                assert np.array_equal(mv[i], smv) and np.array_equal(sad[i], ssad), (first, i)
                omv, osad = oracle_search_w(oracle_lib, pics[i][0], pics[i][1], w, h, sr, pred[i], engine.lambda_q16, bd, wps[i], range(first, first + count))
                assert np.array_equal(mv[i], omv) and np.array_equal(sad[i], osad), (first, i)
    finally:
        for a, b in pl:
            a.close(); b.close()


# 5: identity weights, fp->fen 0 and 1 on the weighted call: both are hmme_search_pairs_device with fen = 0 ("FEN is not consulted")
@pytest.mark.parametrize("bd", [8, 10])
def test_identity_weights_equal_the_unweighted_search_without_fen(engine, bd):
    import torch
    from hmme import api, synth
    w, h, sr = 296, 200, 16
    n_ctu = 5 * 4
    dev = torch.device("cuda", 0)
    pics = [synth.make_pair(w, h, seed=500 + i, bit_depth=bd, max_mv=9, region=64)[:2] for i in range(2)]
    pl = [planes(engine, c, r, w, h, bd) for c, r in pics]
    try:
        curs, refs = [p[0] for p in pl], [p[1] for p in pl]
        d_mv0, d_sad0 = _device_tables(2, n_ctu, dev)
        engine.search_pairs_device(curs, refs, api.FrameParams(sr, 0, bd, 0, n_ctu), None, d_mv0.data_ptr(), d_sad0.data_ptr(), 0)
        d_mvf, d_sadf = _device_tables(2, n_ctu, dev)
        engine.search_pairs_device(curs, refs, api.FrameParams(sr, 1, bd, 0, n_ctu), None, d_mvf.data_ptr(), d_sadf.data_ptr(), 0)
        torch.cuda.synchronize()
        assert not torch.equal(d_sad0, d_sadf)   # FEN does change the unweighted search of these pictures
        for ident in (IDENT, (1, 0, 0, 0)):
            for fen in (0, 1):
                d_mv, d_sad = _device_tables(2, n_ctu, dev)
                engine.search_pairs_w_device(curs, refs, api.FrameParams(sr, fen, bd, 0, n_ctu), [ident, ident], None, d_mv.data_ptr(), d_sad.data_ptr(), 0)
                torch.cuda.synchronize()
                assert torch.equal(d_mv, d_mv0) and torch.equal(d_sad, d_sad0), (ident, fen)
        # one identity pair beside a weighted one takes the weighted path: the same tables for it
        for fen in (0, 1):
            d_mv, d_sad = _device_tables(2, n_ctu, dev)
            engine.search_pairs_w_device(curs, refs, api.FrameParams(sr, fen, bd, 0, n_ctu), [IDENT, FADE], None, d_mv.data_ptr(), d_sad.data_ptr(), 0)
            torch.cuda.synchronize()
            assert torch.equal(d_mv[0], d_mv0[0]) and torch.equal(d_sad[0], d_sad0[0]), fen
    finally:
        for a, b in pl:
            a.close(); b.close()


# 6: refinement of the weighted winners, Hadamard and SAD, 8 and 10 bit: all 593 slots of the corner CTU, one partial CTU of each edge
# and two interior CTUs (a choice of inputs for oracle time, not a tolerance)
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("had", [1, 0])
def test_weighted_refinement_vs_oracle(engine, oracle_lib, bd, had):
    import torch
    from hmme import api, synth
    w, h, sr = 296, 200, 12          # 5 x 4 CTUs, the last column and the last row partial
    n_ctu = 20
    m = synth.MARGIN
    dev = torch.device("cuda", 0)
    wps = [(40, 12 << (bd - 8), 6, 32), (-30, 180 << (bd - 8), 5, 16)]   # the second: negative weight; both in one launch (two runs)
    pics = [fade_pair(w, h, bd, wp, seed=600 + i + bd) for i, wp in enumerate(wps)]
    pred = np.stack([synth.random_predictors(n_ctu, seed=60 + i, max_pel=10) for i in range(2)])
    pl = [planes(engine, c, r, w, h, bd) for c, r in pics]
    table = oracle_lib.slot_table()
    try:
        curs, refs = [p[0] for p in pl], [p[1] for p in pl]
        fp = api.FrameParams(sr, 1, bd, 0, n_ctu)
        d_pred = torch.from_numpy(pred).to(dev)
        d_mv, d_sad = _device_tables(2, n_ctu, dev)
        d_q, d_c = _device_tables(2, n_ctu, dev)
        engine.search_pairs_w_device(curs, refs, fp, wps, d_pred.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), 0)
        engine.refine_pairs_w_device(curs, refs, fp, wps, d_pred.data_ptr(), d_mv.data_ptr(), had, d_q.data_ptr(), d_c.data_ptr(), 0)
        torch.cuda.synchronize()
        mv, qmv, cost = d_mv.cpu().numpy(), d_q.cpu().numpy(), d_c.cpu().numpy().astype(np.uint32)
        # the synchronous single-pair call gives the same tables
        for i in range(2):
            q1, c1 = engine.refine_frame_w(curs[i], refs[i], sr, wps[i], mv[i], pred[i], use_hadamard=bool(had))
            assert np.array_equal(q1, qmv[i]) and np.array_equal(c1, cost[i]), i
        checked = 0
        for i, ctus in ((0, (19, 4, 17, 6, 12)), (1, (19, 9, 16, 7))):   # corner 19; right edge 4 / 9; bottom edge 17 / 16; interior 6, 12, 7
            cur, ref = pics[i]
            for ctu in ctus:
                cx, cy = ctu_origin(ctu, w)
                pq = (int(pred[i, ctu, 0]), int(pred[i, ctu, 1]))
                for s in range(593):
                    x, y, bw, bh = (int(v) for v in table[s])
                    imv = (int(mv[i, ctu, s, 0]), int(mv[i, ctu, s, 1]))
                    hx, hy, qx, qy, c = oracle_lib.frac_refine_w(cur, (m + cx + x, m + cy + y), ref, (m + cx + x, m + cy + y), bw, bh, imv, pq,
                                                                 engine.lambda_q16, had, bd, wps[i])
                    got = (int(qmv[i, ctu, s, 0]), int(qmv[i, ctu, s, 1]), int(cost[i, ctu, s]))
                    assert got == (4 * imv[0] + 2 * hx + qx, 4 * imv[1] + 2 * hy + qy, c), (i, ctu, s, wps[i])
                    checked += 1
        assert checked == 9 * 593
    finally:
        for a, b in pl:
            a.close(); b.close()


def test_identity_refinement_equals_the_unweighted_refinement(engine):
    from hmme import synth
    w, h, sr = 200, 150, 10
    for bd in (8, 10):
        cur, ref, _ = synth.make_pair(w, h, seed=650 + bd, bit_depth=bd, max_mv=8, region=64)
        pc, pr = planes(engine, cur, ref, w, h, bd)
        try:
            mv, _ = engine.search_frame(pc, pr, sr, fen=0)
            a = engine.refine_frame(pc, pr, sr, mv)
            b = engine.refine_frame_w(pc, pr, sr, IDENT, mv)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        finally:
            pc.close(); pr.close()


# 7: two back-to-back weighted calls with different weights on two streams, each followed only by its own stream's sync: the scratch
# planes of the first call must not be overwritten by the second while the first still reads them
def test_two_weighted_calls_on_two_streams(engine, oracle_lib):
    import torch
    from hmme import api
    w, h, sr, bd = 360, 250, 16, 8
    n_ctu = 6 * 4
    dev = torch.device("cuda", 0)
    wps = [FADE, (-40, 200, 6, 32)]
    pics = [fade_pair(w, h, bd, wp, seed=700 + i) for i, wp in enumerate(wps)]
    want = [oracle_search_w(oracle_lib, c, r, w, h, sr, None, engine.lambda_q16, bd, wp, range(n_ctu)) for (c, r), wp in zip(pics, wps)]
    pl = [planes(engine, c, r, w, h, bd) for c, r in pics]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    fp = api.FrameParams(sr, 0, bd, 0, n_ctu)
    try:
        torch.cuda.synchronize()
        for it in range(6):
            tabs = [_device_tables(1, n_ctu, dev) for _ in range(2)]
            torch.cuda.synchronize()
            for k in range(2):
                engine.search_pairs_w_device([pl[k][0]], [pl[k][1]], fp, [wps[k]], None, tabs[k][0].data_ptr(), tabs[k][1].data_ptr(), streams[k].cuda_stream)
            for k in range(2):
                streams[k].synchronize()
                mv, sad = tabs[k][0].cpu().numpy()[0], tabs[k][1].cpu().numpy().astype(np.uint32)[0]
                assert np.array_equal(mv, want[k][0]) and np.array_equal(sad, want[k][1]), (it, k)
    finally:
        torch.cuda.synchronize()
        for a, b in pl:
            a.close(); b.close()


# 8: refusals -- the code of hmme_weight_check, nothing launched (the output buffers keep their contents), a following valid call works
def test_refusals(engine, oracle_lib):
    import ctypes as C
    import torch
    from hmme import api
    w, h, sr, bd = 200, 150, 8, 10
    n_ctu = 4 * 3
    dev = torch.device("cuda", 0)
    cur, ref = fade_pair(w, h, bd, FADE, seed=800)
    pl = [planes(engine, cur, ref, w, h, bd) for _ in range(2)]
    curs, refs = [p[0] for p in pl], [p[1] for p in pl]
    ca = (C.c_void_p * 2)(*[c.h for c in curs])
    ra = (C.c_void_p * 2)(*[r.h for r in refs])
    fp = api.FrameParams(sr, 0, bd, 0, n_ctu)
    L = engine.L
    was = L.hmme_set_error_printing(engine.h, 0)
    try:
        for bad, refine_only in (((64, 0, 16, 0), False), ((300, 0, 0, 0), False), ((64, 7000, 6, 32), False), ((1 << 15, 1, 15, 1 << 14), True)):
            code = api.weight_check(bd, bad, 1 if refine_only else 0)
            assert code in (-1, -5)
            d_mv, d_sad = _device_tables(2, n_ctu, dev)
            d_mv.fill_(-7); d_sad.fill_(-7)
            d_q, d_c = _device_tables(2, n_ctu, dev)
            d_q.fill_(-7); d_c.fill_(-7)
            wa = (api.Weight * 2)(api.Weight(*FADE), api.Weight(*bad))     # the SECOND pair's weight is the bad one
            torch.cuda.synchronize()
            if not refine_only:
                assert L.hmme_search_pairs_w_device(engine.h, ca, ra, 2, C.byref(fp), wa, None, d_mv.data_ptr(), d_sad.data_ptr(), None) == code
                assert "pair 1" in L.hmme_last_error(engine.h).decode()
            else:
                assert api.weight_check(bd, bad, 0) == 0
            assert L.hmme_refine_pairs_w_device(engine.h, ca, ra, 2, C.byref(fp), wa, None, d_mv.data_ptr(), 1, d_q.data_ptr(), d_c.data_ptr(), None) == code
            assert "pair 1" in L.hmme_last_error(engine.h).decode()
            torch.cuda.synchronize()
            for t in (d_mv, d_sad, d_q, d_c):
                assert bool((t == -7).all())     # nothing ran, not even for the valid first pair
            with pytest.raises(api.HmmeError):
                engine.search_frame_w(curs[0], refs[0], sr, bad) if not refine_only else engine.refine_frame_w(curs[0], refs[0], sr, bad, np.zeros((n_ctu, 593, 2), np.int16))
        # null weights
        d_mv, d_sad = _device_tables(2, n_ctu, dev)
        assert L.hmme_search_pairs_w_device(engine.h, ca, ra, 2, C.byref(fp), None, None, d_mv.data_ptr(), d_sad.data_ptr(), None) == -1
        assert L.hmme_refine_pairs_w_device(engine.h, ca, ra, 2, C.byref(fp), None, None, d_mv.data_ptr(), 1, d_mv.data_ptr(), d_sad.data_ptr(), None) == -1
        mvh, sadh = np.zeros((n_ctu, 593, 2), np.int16), np.zeros((n_ctu, 593), np.uint32)
        assert L.hmme_search_frame_w(engine.h, curs[0].h, refs[0].h, C.byref(fp), None, None, mvh.ctypes.data, sadh.ctypes.data) == -1
        assert L.hmme_refine_frame_w(engine.h, curs[0].h, refs[0].h, C.byref(fp), None, None, mvh.ctypes.data, 1, mvh.ctypes.data, sadh.ctypes.data) == -1
    finally:
        L.hmme_set_error_printing(engine.h, was)
    try:
        # ... and a valid call right behind them works
        mv, sad = engine.search_frame_w(curs[0], refs[0], sr, FADE)
        omv, osad = oracle_search_w(oracle_lib, cur, ref, w, h, sr, None, engine.lambda_q16, bd, FADE, range(n_ctu))
        assert np.array_equal(mv, omv) and np.array_equal(sad, osad)
    finally:
        for a, b in pl:
            a.close(); b.close()


class _FadingSequence:
    """a synthetic sequence that fades to black: picture t = (texture moved by t * step) * (64 - 6 t) / 64"""

    def __init__(self, w, h, n, bd):
        from hmme import synth
        self.seq = synth.Sequence(w, h, n, seed=31, bit_depth=bd)

    def read_into(self, t, out):
        self.seq.read_into(t, out)
        np.copyto(out, ((out.astype(np.int64) * (64 - 6 * t) + 32) >> 6).astype(out.dtype))


# 9: the sequence driver passes one weight per pair through (resident mode); weights=None is the run without the argument
@pytest.mark.parametrize("bd", [8, 10])
def test_run_rank_with_weights(engine, bd):
    import torch
    from hmme import sequence
    w, h, sr = 296, 200, 16
    pairs = [(1, 0), (2, 1), (3, 2), (4, 0), (4, 3)]
    src = _FadingSequence(w, h, 5, bd)
    # the reference picture r seen at the brightness of picture c: w0 / 64 = (64 - 6 c) / (64 - 6 r)
    weights = [(int(round(64 * (64 - 6 * c) / (64 - 6 * r))), 0, 6, 32) for c, r in pairs]
    assert len(set(weights)) >= 3
    res = sequence.run_rank(engine, src, pairs, w, h, bd, sr, pairs_per_launch=2, refine=True, weights=weights)
    mv, sad = res["mv"].cpu().numpy(), res["sad"].cpu().numpy().astype(np.uint32)
    qmv, cost = res["qmv"].cpu().numpy(), res["cost"].cpu().numpy().astype(np.uint32)
    host = np.empty((h, w), np.uint8 if bd == 8 else np.uint16)
    for i, (c, r) in enumerate(pairs):
        pc, pr = engine.plane(w, h, bd), engine.plane(w, h, bd)
        try:
            for pl, t in ((pc, c), (pr, r)):
                src.read_into(t, host)
                if bd == 8:
                    pl.upload_u8(host)
                else:
                    engine._check(engine.L.hmme_plane_upload_pel(pl.h, host.ctypes.data, w))
            smv, ssad = engine.search_frame_w(pc, pr, sr, weights[i])
            sq, sc = engine.refine_frame_w(pc, pr, sr, weights[i], smv)
        finally:
            pc.close(); pr.close()
        assert np.array_equal(mv[i], smv) and np.array_equal(sad[i], ssad), i
        assert np.array_equal(qmv[i], sq) and np.array_equal(cost[i], sc), i
    # the weighted search sees through the fade: picture t is the texture at offset t * (3, 2), so cur(x, y) = ref(x + 3, y + 2) for the pair
    # (1, 0), and (58 * ref + 32) >> 6 IS the faded current picture there -- the 64x64 slot of an interior CTU finds that MV at SAD 0
    assert (int(mv[0, 6, 592, 0]), int(mv[0, 6, 592, 1]), int(sad[0, 6, 592])) == (3, 2, 0)
    a = sequence.run_rank(engine, src, pairs, w, h, bd, sr, pairs_per_launch=2, refine=True, weights=None)
    b = sequence.run_rank(engine, src, pairs, w, h, bd, sr, pairs_per_launch=2, refine=True)
    for k in ("mv", "sad", "qmv", "cost"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["sad"], res["sad"])
    with pytest.raises(ValueError):
        sequence.run_rank(engine, src, pairs, w, h, bd, sr, weights=weights[:2])
