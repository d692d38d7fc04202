"""The prediction of a picture whose blocks each name a reference picture, with one explicit weight per reference (hmme_predict_refs_w_device
/ _frame), against tests/predict_bi_w_model.py (refs_picture: TComWeightPrediction::addWeightUni over the 14-bit intermediate of the plane a
block names), against Engine.predict_refs_frame for identity weights and against Engine.predict_frame_w for one reference.  Every comparison
is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import predict_bi_w_model as pm
from frame_helpers import bind_hmo, check_strided_image, mkplane

pytestmark = pytest.mark.gpu

W, H, N = 136, 72, 6                                          # 3 x 2 CTUs, the right column and the bottom row partial
# four references, four weights as (w0, offset in 8-bit units, shift): the second the identity, the third negative, the fourth of another shift
WEIGHTS = ((70, 9, 6), (64, 0, 6), (-37, 150, 5), (300, -20, 8))


def weights(bd):
    return [(w, o * (1 << (bd - 8)), d, 1 << (d - 1)) for w, o, d in WEIGHTS]


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


def textures(bd, seed, k):
    from hmme import synth
    return [synth.make_pair(W, H, seed=seed + 7 * i, bit_depth=bd, max_mv=2)[1] for i in range(k)]


def inputs(per, seed, n_refs=4):
    """(field int16[N, per, 2], ref_field uint8[N, per]): all 16 phases, MVs beyond the clip range, every index 0..n_refs-1 and the indices
    n_refs, 9 and 0xFF that name no plane"""
    rng = np.random.default_rng(seed)
    field = (4 * rng.integers(-200, 201, size=(N, per, 2)) + rng.integers(0, 4, size=(N, per, 2))).astype(np.int16)
    if per == 1:
        return field, np.array([0, 1, 2, 3, 0xFF, 0], np.uint8).reshape(N, 1)
    refs = rng.choice(np.array(list(range(n_refs)) * 3 + [n_refs, 9, 0xFF], np.uint8), size=(N, per))
    refs[0, :n_refs + 3] = list(range(n_refs)) + [n_refs, 9, 0xFF]
    assert len({(int(x) & 3, int(y) & 3) for x, y in field[refs < n_refs]}) == 16
    return field, refs


def blocks_of(ref_field, per, want):
    g = 64 if per == 1 else 8
    mask = np.zeros((128, 192), bool)
    for c in range(N):
        for b in range(per):
            if want(int(ref_field[c, b])):
                x0, y0 = (c % 3) * 64 + (b % 8) * g, (c // 3) * 64 + (b // 8) * g
                mask[y0:y0 + g, x0:x0 + g] = True
    return mask[:H, :W]


@pytest.mark.parametrize("per", [1, 64])
@pytest.mark.parametrize("bd", [8, 10])
def test_four_references_four_weights(engine, hmo, bd, per):
    refs = textures(bd, 2800 + bd, 4)
    planes = [mkplane(engine, r, W, H, bd) for r in refs]
    try:
        dt, fill = (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0x2A5)
        field, rf = inputs(per, 2810 + bd + per)
        wps = weights(bd)
        got = engine.predict_refs_w_frame(planes, wps, field, rf, out=np.full((H, W), fill, dt))
        want = pm.refs_picture(hmo, refs, W, H, bd, field, rf, wps, np.full((H, W), fill, np.int64))
        assert np.array_equal(got, want), np.argwhere(got != want)[:4]
        # block by block it is predict_frame_w of the plane named, with that plane's weight; a block that names none keeps the sentinel
        for r in range(4):
            m = blocks_of(rf, per, lambda v: v == r)
            assert m.any() and np.array_equal(got[m], engine.predict_frame_w(planes[r], wps[r], field)[m])
        dead = blocks_of(rf, per, lambda v: v >= 4)
        assert dead.any() and (got[dead] == fill).all()
        # the identity's blocks are the unweighted call's, the others are not
        plain = engine.predict_refs_frame(planes, field, rf, out=np.full((H, W), fill, dt))
        ident = blocks_of(rf, per, lambda v: v == 1)
        assert np.array_equal(got[ident], plain[ident]) and not np.array_equal(got[~ident], plain[~ident])
        # fewer references: the index n_refs is now out of range and untouched
        got3 = engine.predict_refs_w_frame(planes[:3], wps[:3], field, rf, out=np.full((H, W), fill, dt))
        m3 = blocks_of(rf, per, lambda v: v >= 3)
        assert (got3[m3] == fill).all() and np.array_equal(got3[~m3], got[~m3])
        # a CTU sub-range and an image whose stride exceeds the width
        from hmme import api
        f, r8 = np.ascontiguousarray(field), np.ascontiguousarray(rf)
        ra = (C.c_void_p * 4)(*[p.h for p in planes])
        wa = (api.Weight * 4)(*[api.Weight(*w) for w in wps])
        check_strided_image(W, H, bd, lambda out, first, count: engine.predict_refs_w_frame(planes, wps, field, rf, out=out, ctu_first=first, ctu_count=count),
                            lambda fp, out, stride: engine.L.hmme_predict_refs_w_frame(engine.h, ra, 4, C.byref(fp), wa, f.ctypes.data, r8.ctypes.data, per, out, stride))
    finally:
        for p in planes:
            p.close()


@pytest.mark.parametrize("bd", [8, 12])
def test_all_identities_and_one_reference(engine, bd):
    refs = textures(bd, 2820 + bd, 3)
    planes = [mkplane(engine, r, W, H, bd) for r in refs]
    try:
        field, rf = inputs(64, 2821 + bd, n_refs=3)
        ids = [(1 << d, 0, d, rnd) for d, rnd in ((6, 32), (0, 0), (7, 3))]     # whatever the denominator and whatever round holds
        assert np.array_equal(engine.predict_refs_w_frame(planes, ids, field, rf), engine.predict_refs_frame(planes, field, rf))
        # one reference, every block naming it: predict_frame_w
        wp = (-37, 150 << (bd - 8), 5, 16)
        zeros = np.zeros((N, 64), np.uint8)
        assert np.array_equal(engine.predict_refs_w_frame(planes[:1], [wp], field, zeros), engine.predict_frame_w(planes[0], wp, field))
    finally:
        for p in planes:
            p.close()


def test_device_call_and_refusals(engine, hmo):
    import torch
    from hmme import api
    dev = torch.device("cuda", 0)
    refs = textures(8, 2830, 2)
    planes = [mkplane(engine, r, W, H, 8) for r in refs]
    L = api.load()
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        field, rf = inputs(64, 2831, n_refs=2)
        wps = weights(8)[:2]
        d_field, d_rf = torch.from_numpy(field).to(dev), torch.from_numpy(rf).to(dev)
        img = torch.full((H, W + 24), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        fp = api.FrameParams(1, 0, 8, 1, 4)
        # a refusal names the reference and writes nothing
        for bad, code, text in (([wps[0], (1 << 20, 0, 6, 32)], pm.ERR_UNSUPPORTED, "reference 1"), ([(1, 0, 16, 0), wps[1]], pm.ERR_ARG, "reference 0")):
            with pytest.raises(api.HmmeError, match=f"hmme error {code}: .*{text}"):
                engine.predict_refs_w_device(planes, fp, bad, d_field.data_ptr(), d_rf.data_ptr(), 64, img.data_ptr(), W + 24, 0)
            with pytest.raises(api.HmmeError, match=f"hmme error {code}: .*{text}"):
                engine.predict_refs_w_frame(planes, bad, field, rf)
        assert L.hmme_predict_refs_w_device(engine.h, (C.c_void_p * 2)(*[p.h for p in planes]), 2, C.byref(fp), None, d_field.data_ptr(), d_rf.data_ptr(), 64,
                                            img.data_ptr(), W + 24, None) == pm.ERR_ARG
        torch.cuda.synchronize()
        assert (img.cpu().numpy() == 0xA5).all()
        # the accepted neighbour: CTUs 1..4 into an image whose pitch exceeds the width
        engine.predict_refs_w_device(planes, fp, wps, d_field.data_ptr(), d_rf.data_ptr(), 64, img.data_ptr(), W + 24, 0)
        torch.cuda.synchronize()
        want = pm.refs_picture(hmo, refs, W, H, 8, field, rf, wps, np.full((H, W), 0xA5, np.int64), ctus=range(1, 5))
        got = img.cpu().numpy()
        assert np.array_equal(got[:, :W], want) and (got[:, W:] == 0xA5).all() and (want[:64, :64] == 0xA5).all() and (want != 0xA5).any()
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in planes:
            p.close()
