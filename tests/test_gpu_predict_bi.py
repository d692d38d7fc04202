"""The prediction of a picture whose blocks are L0, L1 or bi (hmme_predict_bi_device / _frame) against tests/predict_bi_model.py --
TComYuv::addAvg over the two 14-bit intermediates, restated in numpy -- and, for blocks of one list, against Engine.predict_frame (that
call is pinned to the oracle elsewhere); and the whole chain on pictures: search, refinement, the partition per list, the bi pass in both
directions, hmme_select_dirs_device, hmme_predict_bi_device.  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import predict_bi_model as pbm
import select_dirs_model as sdm
from frame_helpers import bind_hmo, check_strided_image, mkplane

pytestmark = pytest.mark.gpu

W, H = 136, 72                                                # 3 x 2 CTUs, the right column and the bottom row partial
N, CTUS_X = 6, 3


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    e.set_lambda_q16(sdm.LAMBDA_Q16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


def textures(bd, seed):
    """two unrelated padded pictures"""
    from hmme import synth
    return [synth.make_pair(W, H, seed=seed + 7 * k, bit_depth=bd, max_mv=2)[1] for k in range(2)]


IN_PICTURE = [(c, b) for c in range(N) for b in range(64) if (c % CTUS_X) * 64 + (b % 8) * 8 < W and (c // CTUS_X) * 64 + (b // 8) * 8 < H]
BI_PER_ROUND, ROUNDS = 110, 3                                  # of the 153 blocks inside the picture; 330 >= the 256 pairs of phases


def inputs(per, seed, rnd=0):
    """(field int16[2, N, per, 2], dirs uint8[N, per]).  One MV per 8x8 block: the first BI_PER_ROUND blocks inside the picture are bi and
    take the pairs of quarter-pel phases of the two lists number rnd * BI_PER_ROUND onward (16 x 16 pairs: all of them over ROUNDS rounds),
    the rest are drawn from 1, 2, 3, 0xFF, 0 and 4; MVs reach beyond TComDataCU::clipMv's range on both axes in both lists.  One MV per
    CTU: six hand-picked CTUs"""
    rng = np.random.default_rng(seed + 1000 * rnd)
    field = (4 * rng.integers(-200, 201, size=(2, N, per, 2))).astype(np.int16)
    if per == 1:
        field[0, :, 0] = [(-700, 650), (5, -3), (-18, 7), (33, 2), (-1, -1), (14, 12)]
        field[1, :, 0] = [(700, -650), (6, 9), (3, 3), (-33, -2), (-5, -7), (-14, 11)]
        dirs = np.array([3, 3, 1, 2, 0xFF, 3], np.uint8).reshape(N, 1)
        return field, dirs
    dirs = rng.choice(np.array([1, 2, 3, 0xFF, 0, 4], np.uint8), size=(N, per))
    dirs[0, :2], dirs[1, :2] = (1, 2), (0xFF, 4)                 # every kind inside the picture, whatever was drawn
    for j, (c, b) in enumerate(IN_PICTURE):
        k = rnd * BI_PER_ROUND + j
        field[0, c, b] += (k & 3, (k >> 2) & 3)
        field[1, c, b] += ((k >> 4) & 3, (k >> 6) & 3)
        if 2 <= j < BI_PER_ROUND + 2:
            dirs[c, b] = 3
    for l in range(2):
        assert (field[l, 0, :, 0] < -4 * (64 + 8)).any() and (field[l, 0, :, 1] > 4 * (H + 8)).any()   # beyond the clip range at CTU 0
    return field, dirs


def phase_pairs(field, dirs):
    """the (list 0, list 1) phase pairs of the bi blocks inside the picture"""
    return {(int(field[0, c, b, 0]) & 3, int(field[0, c, b, 1]) & 3, int(field[1, c, b, 0]) & 3, int(field[1, c, b, 1]) & 3)
            for c, b in IN_PICTURE if b < dirs.shape[1] and dirs[c, b] == 3}


def blocks_of(dirs, per, want):
    """boolean [H, W]: the samples of the blocks whose direction is in `want`"""
    g = 64 if per == 1 else 8
    mask = np.zeros((H, W), bool)
    for c in range(N):
        for b in range(per):
            if int(dirs[c, b]) in want:
                x0, y0 = (c % CTUS_X) * 64 + (b % 8) * g, (c // CTUS_X) * 64 + (b // 8) * g
                mask[y0:y0 + g, x0:x0 + g] = True
    return mask


@pytest.mark.parametrize("per", [1, 64])
@pytest.mark.parametrize("bd", [8, 10])
def test_directions_against_the_model_and_predict_frame(engine, hmo, bd, per):
    refs = textures(bd, seed=800 + bd)
    planes = [mkplane(engine, r, W, H, bd) for r in refs]
    try:
        dt, fill = (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0x2A5)
        seen = set()
        for rnd in range(ROUNDS if per == 64 else 1):
            field, dirs = inputs(per, 810 + bd + per, rnd)
            seen |= phase_pairs(field, dirs)
            got = engine.predict_bi_frame(planes[0], planes[1], field, dirs, out=np.full((H, W), fill, dt))
            want = pbm.pred_picture(hmo, refs, W, H, bd, field, dirs, np.full((H, W), fill, np.int64))
            assert np.array_equal(got, want), rnd
            # blocks of one list are predict_frame of that plane, blocks of no direction keep the sentinel
            for l in range(2):
                m = blocks_of(dirs, per, {l + 1})
                assert m.any() and np.array_equal(got[m], engine.predict_frame(planes[l], field[l])[m])
            dead = blocks_of(dirs, per, {0, 4, 0xFF})
            assert dead.any() and (got[dead] == fill).all()
            bi = blocks_of(dirs, per, {3})
            assert bi.any() and not np.array_equal(got[bi], engine.predict_frame(planes[0], field[0])[bi])
        assert len(seen) == (256 if per == 64 else 3)               # every pair of phases of the two lists
        # a CTU sub-range: the rest of the caller's image keeps its samples
        part = engine.predict_bi_frame(planes[0], planes[1], field, dirs, out=np.full((H, W), fill, dt), ctu_first=1, ctu_count=1)
        assert np.array_equal(part[:64, 64:128], got[:64, 64:128])
        part[:64, 64:128] = fill
        assert (part == fill).all()
        # ... and into an image whose stride exceeds the width
        f = np.ascontiguousarray(field)
        check_strided_image(W, H, bd, lambda out, first, count: engine.predict_bi_frame(planes[0], planes[1], field, dirs, out=out, ctu_first=first, ctu_count=count),
                            lambda fp, out, stride: engine.L.hmme_predict_bi_frame(engine.h, planes[0].h, planes[1].h, C.byref(fp), f.ctypes.data, dirs.ctypes.data, per, out, stride))
    finally:
        for p in planes:
            p.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_both_lists_on_one_plane_and_mv_is_predict_frame(engine, bd):
    ref = textures(bd, seed=820 + bd)[0]
    plane = mkplane(engine, ref, W, H, bd)
    try:
        for per in (1, 64):
            one = inputs(per, seed=830 + per)[0][0]
            got = engine.predict_bi_frame(plane, plane, np.stack([one, one]), np.full((N, per), 3, np.uint8))
            assert np.array_equal(got, engine.predict_frame(plane, one))
    finally:
        plane.close()


def test_two_pictures_in_one_launch(engine, hmo):
    import torch
    from hmme import api
    dev = torch.device("cuda", 0)
    refs = textures(8, seed=840) + textures(8, seed=850)                        # picture 0: lists (0, 1); picture 1: lists (2, 3)
    planes = [mkplane(engine, r, W, H, 8) for r in refs]
    try:
        f0, d0 = inputs(64, seed=860)
        f1, d1 = inputs(64, seed=861)
        d_field = torch.from_numpy(np.stack([f0, f1])).to(dev)
        d_dirs = torch.from_numpy(np.stack([d0, d1])).to(dev)
        imgs = [torch.full((H, W + 24), 0xA5, dtype=torch.uint8, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        fp = api.FrameParams(1, 0, 8, 1, 4)                                     # CTUs 1..4 of both
        engine.predict_bi_device([planes[0], planes[2]], [planes[1], planes[3]], fp, d_field.data_ptr(), d_dirs.data_ptr(), 64, [i.data_ptr() for i in imgs], W + 24, 0)
        torch.cuda.synchronize()
        for i, (f, d) in enumerate(((f0, d0), (f1, d1))):
            want = pbm.pred_picture(hmo, refs[2 * i:2 * i + 2], W, H, 8, f, d, np.full((H, W), 0xA5, np.int64), ctus=range(1, 5))
            got = imgs[i].cpu().numpy()
            assert np.array_equal(got[:, :W], want) and (got[:, W:] == 0xA5).all()
            assert (want[:64, :64] == 0xA5).all() and (want[64:, 128:] == 0xA5).all() and (want != 0xA5).any()
    finally:
        for p in planes:
            p.close()


def test_refusals(engine):
    from hmme import api
    field, dirs = np.zeros((2, N, 64, 2), np.int16), np.full((N, 64), 3, np.uint8)
    other_engine = api.Engine(0, 64)
    a, b, small, deep, foreign = engine.plane(W, H), engine.plane(W, H), engine.plane(64, 64), engine.plane(W, H, 10), other_engine.plane(W, H)
    L = api.load()
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        img = np.full((H, W), 0x5C, np.uint8)
        fp8 = api.FrameParams(1, 0, 8, 0, -1)
        frame = lambda r0, r1: L.hmme_predict_bi_frame(engine.h, r0.h, r1.h, C.byref(fp8), field.ctypes.data, dirs.ctypes.data, 64, img.ctypes.data, W)
        for r0, r1 in ((a, small), (small, a), (a, deep), (a, foreign), (foreign, a)):
            assert frame(r0, r1) == -1
        with pytest.raises(api.HmmeError):
            engine.predict_bi_frame(a, deep, field, dirs, out=img)
        assert frame(a, b) == 0 and (img != 0x5C).any()                         # the accepted neighbour does run
        img[...] = 0x5C
        one = C.c_void_p(256)     # never dereferenced: refused before anything is launched
        ra = (C.c_void_p * 9)(*([a.h] * 9))
        outs = (C.c_void_p * 9)(*([256] * 9))
        call = lambda n, fp, f=one, d=one, per=64, o=outs, pitch=W: L.hmme_predict_bi_device(engine.h, ra, ra, n, C.byref(fp), f, d, per, o, pitch, None)
        ok = api.FrameParams(1, 0, 8, 0, -1)
        assert call(9, ok) == -1 and call(0, ok) == -1 and call(1, ok, per=256) == -1 and call(1, ok, f=None) == -1 and call(1, ok, d=None) == -1
        assert call(1, ok, o=None) == -1 and call(1, ok, pitch=W - 1) == -1
        assert call(1, api.FrameParams(1, 0, 7, 0, -1)) == -1 and call(1, api.FrameParams(1, 0, 13, 0, -1)) == -1
        assert call(1, api.FrameParams(1, 0, 10, 0, -1)) == -1                  # 8-bit planes, a 10-bit call
        assert (img == 0x5C).all()
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in (a, b, small, deep, foreign):
            p.close()
        other_engine.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_three_bands(engine, hmo):
    """cur: the left band moved out of list 0's picture, the right band out of list 1's, the middle band the rounded average of both"""
    import torch
    from hmme import api, synth
    sr, m, n = 8, synth.MARGIN, N
    dev = torch.device("cuda", 0)
    ref = textures(8, seed=900)
    moved = [r[m + dy:m + dy + H, m + dx:m + dx + W].astype(np.int32) for r, (dx, dy) in zip(ref, ((3, -2), (-2, 1)))]
    cur_img = moved[0].copy()
    cur_img[:, 48:96] = (moved[0][:, 48:96] + moved[1][:, 48:96] + 1) >> 1
    cur_img[:, 96:] = moved[1][:, 96:]
    planes = [mkplane(engine, synth.pad_plane(cur_img), W, H, 8)] + [mkplane(engine, r, W, H, 8) for r in ref]
    cur, refs = planes[0], planes[1:]
    try:
        fp, sel, bits = api.FrameParams(sr, 1, 8, 0, n), api.SelectParams(64), sdm.HM_BITS
        tab = lambda: (torch.zeros((2, n, 593, 2), dtype=torch.int16, device=dev), torch.zeros((2, n, 593), dtype=torch.int32, device=dev))
        (d_mv, d_sad), (d_q, d_c), (d_bmv, d_bsad), (d_bq, d_bc) = tab(), tab(), tab(), tab()
        d_uni = torch.zeros((2, n, 64, 2), dtype=torch.int16, device=dev)
        d_field = torch.full((1, 2, n, 64, 2), 0x5A5A, dtype=torch.int16, device=dev)
        d_dir = torch.full((1, n, 64), 0xA7, dtype=torch.uint8, device=dev)
        d_slot = torch.zeros((1, n, 64), dtype=torch.int16, device=dev)
        d_cc = torch.zeros((1, n), dtype=torch.int32, device=dev)
        d_img = torch.full((H, W), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        curs, others = [cur, cur], [refs[1], refs[0]]
        engine.search_pairs_device(curs, refs, fp, None, d_mv.data_ptr(), d_sad.data_ptr(), 0)
        engine.refine_pairs_device(curs, refs, fp, None, d_mv.data_ptr(), 1, d_q.data_ptr(), d_c.data_ptr(), 0)
        engine.select_pairs_device(W, H, 2, fp, sel, d_q.data_ptr(), d_c.data_ptr(), None, d_uni.data_ptr(), None, None, 0)
        torch.cuda.synchronize()
        d_other = d_uni.flip(0).contiguous()                                    # list l is searched against the origin built from list 1-l's field
        torch.cuda.synchronize()
        engine.search_pairs_bi_device(curs, refs, others, fp, d_other.data_ptr(), 64, None, None, d_bmv.data_ptr(), d_bsad.data_ptr(), 0)
        engine.refine_pairs_bi_device(curs, refs, others, fp, d_other.data_ptr(), 64, None, None, d_bmv.data_ptr(), 1, d_bq.data_ptr(), d_bc.data_ptr(), 0)
        engine.select_dirs_device(W, H, 1, fp, sel, [api.DirParams(*bits)], d_q.data_ptr(), d_c.data_ptr(), d_bq.data_ptr(), d_bc.data_ptr(), d_uni.data_ptr(), None,
                                  d_field.data_ptr(), d_dir.data_ptr(), d_slot.data_ptr(), d_cc.data_ptr(), 0)
        engine.predict_bi_device([refs[0]], [refs[1]], fp, d_field.data_ptr(), d_dir.data_ptr(), 64, [d_img.data_ptr()], W, 0)
        torch.cuda.synchronize()
        host = lambda t: t.cpu().numpy()
        mv_uni, cost_uni, mv_bi, cost_bi = host(d_q), host(d_c).view(np.uint32), host(d_bq), host(d_bc).view(np.uint32)
        uni_field = host(d_uni)
        mf, md, ms, mc = sdm.select_dirs_picture(mv_uni, cost_uni, mv_bi, cost_bi, uni_field, sel, W, H, bits)
        assert np.array_equal(host(d_field)[0], mf) and np.array_equal(host(d_dir)[0], md)
        assert np.array_equal(host(d_slot)[0].view(np.uint16), ms) and np.array_equal(host(d_cc)[0].view(np.uint32), mc)
        assert {1, 2, 3} <= set(md.reshape(-1).tolist()), np.bincount(md.reshape(-1))   # about the recipe: every direction is chosen somewhere
        # the directions follow the bands: counted on the model's output, block by block
        counts = np.zeros((3, 4), int)
        for c in range(n):
            for b in range(64):
                x0 = (c % CTUS_X) * 64 + (b % 8) * 8
                if md[c, b] != sdm.NO_DIR:
                    counts[0 if x0 < 48 else 1 if x0 < 96 else 2, md[c, b]] += 1
        assert counts[0].argmax() == 1 and counts[1].argmax() == 3 and counts[2].argmax() == 2, counts
        # the prediction: the model's field through the host call gives the same picture, and it beats either list alone
        pred = host(d_img)
        assert np.array_equal(pred, engine.predict_bi_frame(refs[0], refs[1], mf, md, out=np.full((H, W), 0xEE, np.uint8)))
        assert np.array_equal(pred, pbm.pred_picture(hmo, ref, W, H, 8, mf, md, np.full((H, W), 0xEE, np.int64)))
        sad = lambda p: int(np.abs(p.astype(np.int32) - cur_img).sum())
        for l in range(2):
            assert sad(pred) < sad(engine.predict_frame(refs[l], uni_field[l]))
    finally:
        for p in planes:
            p.close()
