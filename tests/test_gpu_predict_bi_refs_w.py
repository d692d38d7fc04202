"""The prediction of a B picture with several references per list in a slice with explicit weighted prediction
(hmme_predict_bi_refs_w_device / _frame) and for the Cb / Cr of a 4:2:0 picture (hmme_predict_chroma_bi_refs_device / _frame) against
tests/predict_bi_refs_w_model.py and tests/predict_chroma_bi_refs_model.py, and bit for bit against the single-reference calls
Engine.predict_bi_w_frame / Engine.predict_chroma_bi_frame on the planes and weights a block's indices name.  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import predict_bi_refs_w_model as pbrw
import predict_chroma_bi_refs_model as pcbr
from frame_helpers import bind_hmo, check_strided_image, dims, mkplane
from test_gpu_predict_bi_refs import inputs, textures
from test_gpu_predict_chroma import make_field

pytestmark = pytest.mark.gpu

N0, N1 = 3, 2
PAIRS = ((0, 0), (2, 1), (1, 0))                     # the sampled (r0, r1) for the comparison with the single-reference calls
# (w0, offset in 8-bit units, shift) per reference: w0 on both sides of 1 << shift, offsets of both signs, one identity beside the others
LUMA = {"hm_like": (((70, -9, 6), (64, 0, 6), (55, 14, 6)), ((40, -5, 6), (90, 11, 6))),
        "negative": (((-37, 150, 5), (32, 0, 5), (61, -20, 5)), ((90, -3, 5), (-20, 170, 5)))}
# per component: the same shape; Cb and Cr differ in shift
CHROMA = {"hm_like": ((((70, 9, 6), (64, 0, 6), (55, -14, 6)), ((45, -6, 6), (80, 3, 6))),
                      (((40, -5, 5), (29, 11, 5), (32, 0, 5)), ((36, 7, 5), (25, -12, 5)))),
          "negative": ((((-37, 150, 5), (90, -3, 5), (32, 0, 5)), ((33, -8, 5), (-20, 170, 5))),
                       (((61, 4, 7), (128, 0, 7), (-20, 170, 7)), ((200, -30, 7), (100, 12, 7))))}
ERR_ARG, ERR_UNSUPPORTED = pbrw.ERR_ARG, pbrw.ERR_UNSUPPORTED


def scaled(lists, bd):
    """(wps0, wps1) at a bit depth: offsets scale with the depth, round is not used"""
    return tuple([(w, o * (1 << (bd - 8)), d, 1 << (d - 1)) for w, o, d in l] for l in lists)


def ident(shift, n):
    return [(1 << shift, 0, shift, 0)] * n


def sentinel(bd):
    return (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0x2A5)


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


def luma_mask(w, h, per, dirs, refs, n0, n1, pick, half=False):
    """boolean [h, w] ([h / 2, w / 2] with half): the samples of the LIVE blocks for which pick(direction, (r0, r1)) holds"""
    s = 2 if half else 1
    mask = np.zeros((dims(w, h)[1] * 64 // s, dims(w, h)[0] * 64 // s), bool)
    for _, _, cu_x, cu_y, bx, by, g, d, idx in pbrw.live_blocks(w, h, per, dirs, refs, n0, n1):
        if pick(d, idx):
            mask[(cu_y + by) // s:(cu_y + by + g) // s, (cu_x + bx) // s:(cu_x + bx + g) // s] = True
    return mask[:h // s, :w // s]


def names_pair(a, b):
    """the blocks whose prediction is the single-reference call's on (refs0[a], refs1[b])"""
    return lambda d, idx: (d == 3 and idx == (a, b)) or (d == 1 and idx[0] == a) or (d == 2 and idx[1] == b)


# ---- luma -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 64), (100, 70)])
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("wname", sorted(LUMA))
def test_luma_against_the_model_and_the_single_reference_call(engine, hmo, wname, bd, size):
    w, h = size
    pics = textures(w, h, bd, 3100 + bd + w, N0 + N1)
    planes = [mkplane(engine, r, w, h, bd) for r in pics]
    p0, p1 = planes[:N0], planes[N0:]
    try:
        dt, fill = sentinel(bd)
        wps0, wps1 = scaled(LUMA[wname], bd)
        field, dirs, refs = inputs(w, h, 64, 3110 + bd + w)
        got = engine.predict_bi_refs_w_frame(p0, p1, wps0, wps1, field, dirs, refs, out=np.full((h, w), fill, dt))
        want = pbrw.pred_picture(hmo, pics[:N0], pics[N0:], wps0, wps1, w, h, bd, field, dirs, refs, np.full((h, w), fill, np.int64))
        assert np.array_equal(got, want), np.argwhere(got != want)[:4]
        # about the recipe: all 16 phases in each list among the blocks that use it, mixed directions, all six pairs in bi blocks
        live = list(pbrw.live_blocks(w, h, 64, dirs, refs, N0, N1))
        for l in range(2):
            assert len({(int(field[l, c, b, 0]) & 3, int(field[l, c, b, 1]) & 3) for c, b, *_, d, _ in live if (d >> l) & 1}) == 16
        assert {d for *_, d, _ in live} == {1, 2, 3} and {idx for *_, d, idx in live if d == 3} == {(a, b) for a in range(N0) for b in range(N1)}
        # blocks that are not live keep the sentinel: 0xFF, other directions, indices >= n
        dead = ~luma_mask(w, h, 64, dirs, refs, N0, N1, lambda d, idx: True)
        assert dead.any() and (got[dead] == fill).all() and (got[~dead] != fill).any()
        # the weights matter, and so does the index that picks them
        plain = engine.predict_bi_refs_frame(p0, p1, field, dirs, refs, out=np.full((h, w), fill, dt))
        assert not np.array_equal(plain, got)
        moved = engine.predict_bi_refs_w_frame(p0, p1, wps0[1:] + wps0[:1], wps1, field, dirs, refs, out=np.full((h, w), fill, dt))
        assert not np.array_equal(moved, got)
        # one identity beside other weights: its uni-directional blocks are the unweighted samples
        m = luma_mask(w, h, 64, dirs, refs, N0, N1, lambda d, idx: d == 1 and idx[0] == 1)
        assert m.any() and np.array_equal(got[m], plain[m])
        # three sampled index pairs: every block that names them equals the single-reference call on those planes and weights
        for a, b in PAIRS:
            one = engine.predict_bi_w_frame(p0[a], p1[b], wps0[a], wps1[b], field, dirs, out=np.full((h, w), fill, dt))
            m = luma_mask(w, h, 64, dirs, refs, N0, N1, names_pair(a, b))
            assert m.any() and np.array_equal(got[m], one[m]), (a, b)
    finally:
        for p in planes:
            p.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_luma_identities_one_mv_per_ctu_sub_range_and_strided_image(engine, hmo, bd):
    w, h = 100, 70
    pics = textures(w, h, bd, 3200 + bd, N0 + N1)
    planes = [mkplane(engine, r, w, h, bd) for r in pics]
    p0, p1 = planes[:N0], planes[N0:]
    try:
        dt, fill = sentinel(bd)
        wps0, wps1 = scaled(LUMA["hm_like"], bd)
        f64, d64, r64 = inputs(w, h, 64, 3210 + bd)
        # all identities (whatever round holds): the unweighted call
        got = engine.predict_bi_refs_w_frame(p0, p1, [(8, 0, 3, 99)] * N0, ident(3, N1), f64, d64, r64, out=np.full((h, w), fill, dt))
        assert np.array_equal(got, engine.predict_bi_refs_frame(p0, p1, f64, d64, r64, out=np.full((h, w), fill, dt))) and (got != fill).any()
        # one MV per CTU
        field = np.zeros((2, 4, 1, 2), np.int16)
        field[0, :, 0] = [(-700, 650), (5, -3), (-18, 7), (33, 2)]
        field[1, :, 0] = [(700, -650), (6, 9), (3, 3), (-33, -2)]
        dirs = np.array([3, 1, 2, 3], np.uint8).reshape(4, 1)
        refs = np.array([[2, 0, 0xFF, N0], [1, 0xFF, 1, 0]], np.uint8).reshape(2, 4, 1)
        got = engine.predict_bi_refs_w_frame(p0, p1, wps0, wps1, field, dirs, refs, out=np.full((h, w), fill, dt))
        want = pbrw.pred_picture(hmo, pics[:N0], pics[N0:], wps0, wps1, w, h, bd, field, dirs, refs, np.full((h, w), fill, np.int64))
        assert np.array_equal(got, want) and (got[:64] != fill).any() and (got[64:, 64:] == fill).all()   # CTU 3: list 0's index beyond the list
        # a CTU sub-range: the rest of the caller's image keeps its samples
        whole = engine.predict_bi_refs_w_frame(p0, p1, wps0, wps1, f64, d64, r64, out=np.full((h, w), fill, dt))
        part = engine.predict_bi_refs_w_frame(p0, p1, wps0, wps1, f64, d64, r64, out=np.full((h, w), fill, dt), ctu_first=1, ctu_count=2)
        assert np.array_equal(part[:64, 64:], whole[:64, 64:]) and np.array_equal(part[64:, :64], whole[64:, :64]) and (whole[:64, 64:] != fill).any()
        assert (part[:64, :64] == fill).all() and (part[64:, 64:] == fill).all()
        # an image whose stride exceeds the width
        from hmme import api
        f = np.ascontiguousarray(f64)
        h0, h1, a0, a1 = api._handles(p0), api._handles(p1), engine._weights(wps0), engine._weights(wps1)
        check_strided_image(w, h, bd, lambda out, first, count: engine.predict_bi_refs_w_frame(p0, p1, wps0, wps1, f64, d64, r64, out=out, ctu_first=first, ctu_count=count),
                            lambda fp, out, stride: engine.L.hmme_predict_bi_refs_w_frame(engine.h, h0, N0, h1, N1, C.byref(fp), a0, a1, f.ctypes.data, d64.ctypes.data,
                                                                                          r64.ctypes.data, 64, out, stride))
        # a used context against a fresh one
        fresh = api.Engine(0, 64)
        q = [mkplane(fresh, r, w, h, bd) for r in pics]
        try:
            again = fresh.predict_bi_refs_w_frame(q[:N0], q[N0:], wps0, wps1, f64, d64, r64, out=np.full((h, w), fill, dt))
            assert np.array_equal(again, whole)
        finally:
            for p in q:
                p.close()
            fresh.close()
    finally:
        for p in planes:
            p.close()


def test_luma_device_call_with_sixteen_planes_per_list(engine, hmo):
    """hmme_predict_bi_refs_w_device on device buffers: 16 + 16 planes (the same few pictures under many handles, every handle its own weight)
    and a pitched image"""
    import torch
    from hmme import api
    w, h = 64, 64
    dev = torch.device("cuda", 0)
    pics = textures(w, h, 8, 3400, 4)
    planes = [mkplane(engine, r, w, h, 8) for r in pics]
    try:
        l0 = [planes[k % 4] for k in range(16)]
        l1 = [planes[(k + 1) % 4] for k in range(16)]
        wps0 = [(64 + 3 * k - 20, 2 * k - 15, 6, 32) for k in range(16)]
        wps1 = [(100 - 5 * k, 11 - k, 6, 32) for k in range(16)]
        field, dirs, refs = inputs(w, h, 64, 3410, 16, 16)
        d_field, d_dirs, d_refs = (torch.from_numpy(a).to(dev) for a in (field, dirs, refs))
        img = torch.full((h, w + 24), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        fp = api.FrameParams(1, 0, 8, 0, -1)
        engine.predict_bi_refs_w_device(l0, l1, fp, wps0, wps1, d_field.data_ptr(), d_dirs.data_ptr(), d_refs.data_ptr(), 64, img.data_ptr(), w + 24, 0)
        torch.cuda.synchronize()
        want = pbrw.pred_picture(hmo, [pics[k % 4] for k in range(16)], [pics[(k + 1) % 4] for k in range(16)], wps0, wps1, w, h, 8, field, dirs, refs,
                                 np.full((h, w), 0xA5, np.int64))
        got = img.cpu().numpy()
        assert np.array_equal(got[:, :w], want) and (got[:, w:] == 0xA5).all() and (want != 0xA5).any()
        assert refs.max() == 0xFF and (refs[(refs != 0xFF)] >= 8).any()             # about the recipe: high indices are named
    finally:
        for p in planes:
            p.close()


def test_luma_refusals(engine):
    from hmme import api
    w, h, n = 100, 70, 4
    field, dirs, refs = np.zeros((2, n, 64, 2), np.int16), np.full((n, 64), 3, np.uint8), np.zeros((2, n, 64), np.uint8)
    a, b, small, deep = engine.plane(w, h), engine.plane(w, h), engine.plane(64, 64), engine.plane(w, h, 10)
    L = api.load()
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        img = np.full((h, w), 0x5C, np.uint8)
        fp8 = api.FrameParams(1, 0, 8, 0, -1)
        ok, big = (70, -9, 6, 32), (60000, 0, 6, 32)                    # big: |w0| * 40 960 beyond int32 alone

        def frame(l0, l1, w0, w1, fp=fp8, n0=None, n1=None):
            p = lambda ws: None if ws is None else engine._weights(ws)
            return L.hmme_predict_bi_refs_w_frame(engine.h, api._handles(l0), len(l0) if n0 is None else n0, api._handles(l1), len(l1) if n1 is None else n1,
                                                  C.byref(fp), p(w0), p(w1), field.ctypes.data, dirs.ctypes.data, refs.ctypes.data, 64, img.ctypes.data, w)
        assert frame([a, b], [b], None, [ok]) == ERR_ARG and frame([a, b], [b], [ok, ok], None) == ERR_ARG
        assert frame([a, b], [b], [ok, (70, 0, 16, 0)], [ok]) == ERR_ARG                          # a shift outside 0..15
        assert frame([a, b], [b], [ok, ok], [(35, 0, 5, 16)]) == ERR_ARG                          # unequal shifts, between the lists only
        assert frame([a, b], [b], [big, ok], [(35, 0, 5, 16)]) == ERR_ARG                         # ... answers before list 0's range
        assert frame([a, b], [b], [ok, big], [ok]) == ERR_UNSUPPORTED and frame([a, b], [b], [ok, ok], [big]) == ERR_UNSUPPORTED
        half = (26300, 0, 6, 32)                                                                  # passes alone, not beside another of its size
        assert pbrw.check(8, [ok, half], [half]) == ERR_UNSUPPORTED and pbrw.check(8, [ok, half], [ok]) == 0
        assert frame([a, b], [b], [ok, half], [half]) == ERR_UNSUPPORTED
        assert frame([a, b], [b], [ok, ok], [ok], fp=api.FrameParams(1, 0, 13, 0, -1)) == ERR_ARG
        # the weights answer before the planes are looked at; with good weights the plane checks are the unweighted call's
        assert frame([a, small], [b], [ok, big], [ok]) == ERR_UNSUPPORTED
        assert frame([a, small], [b], [ok, ok], [ok]) == ERR_ARG and frame([a], [deep], [ok], [ok]) == ERR_ARG
        assert frame([a], [b], [ok], [ok], n0=0) == ERR_ARG and frame([a] * 16, [b], [ok] * 16, [ok], n0=17) == ERR_ARG
        assert (img == 0x5C).all()
        with pytest.raises(api.HmmeError, match="hmme_predict_bi_refs_w_frame.*list 0 reference 1 with list 1 reference 0"):
            engine.predict_bi_refs_w_frame([a, b], [b], [ok, half], [half], field, dirs, refs, out=img)
        assert (img == 0x5C).all()
        assert frame([a, b], [b], [ok, half], [ok]) == 0 and (img != 0x5C).any()                  # the accepted neighbour does run
        # the device entry refuses before anything is launched (addresses never dereferenced)
        one = C.c_void_p(256)
        call = lambda w0, w1: L.hmme_predict_bi_refs_w_device(engine.h, api._handles([a, b]), 2, api._handles([b]), 1, C.byref(fp8), engine._weights(w0), engine._weights(w1),
                                                             one, one, one, 64, one, w, None)
        assert call([ok, half], [half]) == ERR_UNSUPPORTED and call([ok, ok], [(35, 0, 5, 16)]) == ERR_ARG
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in (a, b, small, deep):
            p.close()


# ---- 4:2:0 ----------------------------------------------------------------------------------------------------------------------------------
class ChromaRefs:
    """n0 + n1 references' Cb and Cr of a w x h LUMA picture: unrelated textures, as padded arrays (model) and as planes (engine)"""

    def __init__(self, engine, w, h, bd, seed, n0, n1, distinct=None):
        from hmme import synth
        n = n0 + n1
        k_of = list(range(n)) if distinct is None else [k % distinct for k in range(n)]
        tex = {k: [synth.make_pair(w // 2, h // 2, seed=seed + 7 * k + 3 * c, bit_depth=bd, max_mv=2)[1] for c in range(2)] for k in set(k_of)}
        self.arrays = [tex[k] for k in k_of]                                   # [reference][component]
        self.planes = [[mkplane(engine, a, w // 2, h // 2, bd) for a in pic] for pic in self.arrays]
        self.n0, self.n1 = n0, n1

    def comps(self):
        """model order: [component][list][reference]"""
        return [[[self.arrays[k][c] for k in range(self.n0)], [self.arrays[self.n0 + k][c] for k in range(self.n1)]] for c in range(2)]

    def lists(self):
        """engine order: ([cb0, cr0, cb1, ...] of list 0, of list 1)"""
        flat = [p for pic in self.planes for p in pic]
        return flat[:2 * self.n0], flat[2 * self.n0:]

    def close(self):
        for pic in self.planes:
            for p in pic:
                p.close()


def chroma_weights(name, bd):
    """-> (model order wps[component][list][reference], engine order (weights0, weights1): (Cb, Cr) per reference)"""
    wps = [scaled(comp, bd) for comp in CHROMA[name]]
    flat = tuple([wps[c][l][r] for r in range(len(wps[0][l])) for c in range(2)] for l in range(2))
    return wps, flat


def chroma_inputs(w, h, per, seed, n0=N0, n1=N1):
    """the luma recipe's directions and indices with chroma MVs: all 64 eighth-pel phase pairs per list, MVs beyond the clip range"""
    _, dirs, refs = inputs(w, h, per, seed, n0, n1)
    field = np.stack([make_field(w, h, per, seed + 1 + 50 * l, rot=23 * l) for l in range(2)])
    return field, dirs, refs


def cfills(w, h, bd, dtype=None):
    dt, fill = sentinel(bd)
    return tuple(np.full((h // 2, w // 2), fill, dtype or dt) for _ in range(2))


@pytest.mark.parametrize("size", [(64, 64), (100, 70), (130, 66)])
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("wname", [None] + sorted(CHROMA))
def test_chroma_against_the_model_and_the_single_reference_call(engine, hmo, wname, bd, size):
    w, h = size
    ch = ChromaRefs(engine, w, h, bd, 3500 + bd + w, N0, N1)
    try:
        fill = sentinel(bd)[1]
        wps, (f0, f1) = (None, (None, None)) if wname is None else chroma_weights(wname, bd)
        l0, l1 = ch.lists()
        field, dirs, refs = chroma_inputs(w, h, 64, 3510 + bd + w)
        got = engine.predict_chroma_bi_refs_frame(l0, l1, w, h, field, dirs, refs, outs=cfills(w, h, bd), weights0=f0, weights1=f1)
        want = pcbr.bi_refs_picture(hmo, ch.comps(), w, h, bd, field, dirs, refs, cfills(w, h, bd, np.int64), wps)
        for c in range(2):
            assert np.array_equal(got[c], want[c]), ("Cb", "Cr")[c]
        assert not np.array_equal(got[0], got[1])
        # about the recipe: all 8 phases per axis and list among the blocks that use it, all six pairs in bi blocks
        live = list(pbrw.live_blocks(w, h, 64, dirs, refs, N0, N1))
        for l in range(2):
            for axis in range(2):
                assert {int(field[l, c, b, axis]) & 7 for c, b, *_, d, _ in live if (d >> l) & 1} == set(range(8))
        assert {d for *_, d, _ in live} == {1, 2, 3} and {idx for *_, d, idx in live if d == 3} == {(a, b) for a in range(N0) for b in range(N1)}
        dead = ~luma_mask(w, h, 64, dirs, refs, N0, N1, lambda d, idx: True, half=True)
        assert dead.any() and all((g[dead] == fill).all() and (g[~dead] != fill).any() for g in got)
        if wname is not None:
            plain = engine.predict_chroma_bi_refs_frame(l0, l1, w, h, field, dirs, refs, outs=cfills(w, h, bd))
            assert not np.array_equal(plain[0], got[0]) and not np.array_equal(plain[1], got[1])
        for a, b in PAIRS:
            one = engine.predict_chroma_bi_frame(ch.planes[a], ch.planes[N0 + b], w, h, field, dirs, outs=cfills(w, h, bd),
                                                 weights0=None if wname is None else f0[2 * a:2 * a + 2], weights1=None if wname is None else f1[2 * b:2 * b + 2])
            m = luma_mask(w, h, 64, dirs, refs, N0, N1, names_pair(a, b), half=True)
            assert m.any() and all(np.array_equal(got[c][m], one[c][m]) for c in range(2)), (a, b)
    finally:
        ch.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_chroma_equivalences_and_launch_forms(engine, hmo, bd):
    import torch
    from hmme import api
    w, h = 130, 66
    ch = ChromaRefs(engine, w, h, bd, 3600 + bd, N0, N1)
    try:
        dt, fill = sentinel(bd)
        wps, (f0, f1) = chroma_weights("hm_like", bd)
        l0, l1 = ch.lists()
        field, dirs, refs = chroma_inputs(w, h, 64, 3610 + bd)
        plain = engine.predict_chroma_bi_refs_frame(l0, l1, w, h, field, dirs, refs, outs=cfills(w, h, bd))
        # NULL weights and 1 + 1 references: predict_chroma_bi_frame
        zero = np.zeros_like(refs)
        one = engine.predict_chroma_bi_refs_frame(l0[:2], l1[:2], w, h, field, dirs, zero, outs=cfills(w, h, bd))
        sib = engine.predict_chroma_bi_frame(l0[:2], l1[:2], w, h, field, dirs, outs=cfills(w, h, bd))
        assert all(np.array_equal(one[c], sib[c]) and (one[c] != fill).any() for c in range(2))
        # identities throughout (Cb and Cr of different shifts, any round): the unweighted form
        ids0, ids1 = [(64, 0, 6, 7), (8, 0, 3, 0)] * N0, [(64, 0, 6, 0), (8, 0, 3, 4)] * N1
        same = engine.predict_chroma_bi_refs_frame(l0, l1, w, h, field, dirs, refs, outs=cfills(w, h, bd), weights0=ids0, weights1=ids1)
        assert all(np.array_equal(same[c], plain[c]) for c in range(2))
        # one MV per CTU
        f1c, d1c, r1c = chroma_inputs(w, h, 1, 3620 + bd)
        d1c[:, 0], r1c[0, :, 0], r1c[1, :, 0] = (3, 1, 2, 3, 3, 0xFF), (2, 0, 0xFF, 1, N0, 0), (1, 0xFF, 0, 0, 0, 0)
        got = engine.predict_chroma_bi_refs_frame(l0, l1, w, h, f1c, d1c, r1c, outs=cfills(w, h, bd), weights0=f0, weights1=f1)
        want = pcbr.bi_refs_picture(hmo, ch.comps(), w, h, bd, f1c, d1c, r1c, cfills(w, h, bd, np.int64), wps)
        assert all(np.array_equal(got[c], want[c]) for c in range(2)) and (got[0][:32, :64] != fill).any() and (got[0][32:, 32:] == fill).all()
        # the device entry: pitched images and a CTU sub-range; the rest keeps its samples
        whole = engine.predict_chroma_bi_refs_frame(l0, l1, w, h, field, dirs, refs, outs=cfills(w, h, bd), weights0=f0, weights1=f1)
        dev = torch.device("cuda", 0)
        d_field, d_dirs, d_refs = (torch.from_numpy(a).to(dev) for a in (field, dirs, refs))
        imgs = [torch.full((h // 2, w // 2 + 9), fill, dtype=torch.uint8 if bd == 8 else torch.int16, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        engine.predict_chroma_bi_refs_device(l0, l1, w, h, api.FrameParams(1, 0, bd, 1, 3), d_field.data_ptr(), d_dirs.data_ptr(), d_refs.data_ptr(), 64,
                                             imgs[0].data_ptr(), imgs[1].data_ptr(), (w // 2 + 9) * (1 if bd == 8 else 2), weights0=f0, weights1=f1)
        torch.cuda.synchronize()
        inside = np.zeros((h // 2, w // 2), bool)
        inside[:32, 32:] = True                                                   # CTUs 1, 2 of the first row ...
        inside[32:, :32] = True                                                   # ... and CTU 3
        for c in range(2):
            g = imgs[c].cpu().numpy().view(dt)
            assert np.array_equal(g[:, :w // 2][inside], whole[c][inside]) and (g[:, :w // 2][~inside] == fill).all() and (g[:, w // 2:] == fill).all()
        assert (whole[0][inside] != fill).any()
        # a used context against a fresh one
        fresh = api.Engine(0, 64)
        q = ChromaRefs(fresh, w, h, bd, 3600 + bd, N0, N1)
        try:
            again = fresh.predict_chroma_bi_refs_frame(*q.lists(), w, h, field, dirs, refs, outs=cfills(w, h, bd), weights0=f0, weights1=f1)
            assert all(np.array_equal(again[c], whole[c]) for c in range(2))
        finally:
            q.close()
            fresh.close()
    finally:
        ch.close()


def test_chroma_four_plus_four_is_served_and_five_plus_four_refused(engine, hmo):
    from hmme import api
    w, h, bd = 100, 70, 8
    ch = ChromaRefs(engine, w, h, bd, 3700, 5, 4, distinct=4)
    L = api.load()
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        fill = sentinel(bd)[1]
        flat = [p for pic in ch.planes for p in pic]
        l0, l1 = flat[:8], flat[10:]
        comps = [[[ch.arrays[k][c] for k in range(4)], [ch.arrays[5 + k][c] for k in range(4)]] for c in range(2)]
        wps = [[[(60 + 9 * r + 2 * c, 3 * r - 4, 6, 32) for r in range(4)], [(75 - 6 * r, 5 - 2 * r + c, 6, 32) for r in range(4)]] for c in range(2)]
        f0, f1 = ([wps[c][l][r] for r in range(4) for c in range(2)] for l in range(2))
        field, dirs, refs = chroma_inputs(w, h, 64, 3710, 4, 4)
        got = engine.predict_chroma_bi_refs_frame(l0, l1, w, h, field, dirs, refs, outs=cfills(w, h, bd), weights0=f0, weights1=f1)
        want = pcbr.bi_refs_picture(hmo, comps, w, h, bd, field, dirs, refs, cfills(w, h, bd, np.int64), wps)
        assert all(np.array_equal(got[c], want[c]) and (got[c] != fill).any() for c in range(2))
        assert {int(r) for r in refs[0][refs[0] != 0xFF]} >= set(range(4)) and {int(r) for r in refs[1][refs[1] != 0xFF]} >= set(range(4))
        # 5 + 4: 18 planes
        outs = cfills(w, h, bd)
        oa = (C.c_void_p * 2)(outs[0].ctypes.data, outs[1].ctypes.data)
        fp = api.FrameParams(1, 0, bd, 0, -1)
        frame = lambda a0, a1, w0=None, w1=None: L.hmme_predict_chroma_bi_refs_frame(
            engine.h, api._handles(a0), len(a0) // 2, api._handles(a1), len(a1) // 2, w, h, C.byref(fp), None if w0 is None else engine._weights(w0),
            None if w1 is None else engine._weights(w1), field.ctypes.data, dirs.ctypes.data, refs.ctypes.data, 64, oa, w // 2)
        assert frame(flat[:10], l1) == ERR_ARG and frame(l0, flat[8:]) == ERR_ARG
        # weights: one list without, a shift that differs inside a component, a range -- and Cb / Cr of different shifts are fine
        assert frame(l0, l1, f0, None) == ERR_ARG and frame(l0, l1, None, f1) == ERR_ARG
        bad = list(f1)
        bad[3] = (30, 0, 5, 16)                                                   # Cr of list 1's reference 1
        assert frame(l0, l1, f0, bad) == ERR_ARG
        bad[3] = (60000, 0, 6, 32)
        assert frame(l0, l1, f0, bad) == ERR_UNSUPPORTED
        assert all((o == fill).all() for o in outs)
        cr5 = lambda ws: [(v[0] // 2, v[1], 5, 16) if k % 2 else v for k, v in enumerate(ws)]
        assert frame(l0, l1, cr5(f0), cr5(f1)) == 0 and all((o != fill).any() for o in outs)
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        ch.close()


def test_chroma_refusals(engine):
    from hmme import api
    w, h, n = 100, 70, 4
    field, dirs, refs = np.zeros((2, n, 64, 2), np.int16), np.full((n, 64), 3, np.uint8), np.zeros((2, n, 64), np.uint8)
    other_engine = api.Engine(0, 64)
    cb, cr, luma, deep, foreign = engine.plane(50, 35), engine.plane(50, 35), engine.plane(w, h), engine.plane(50, 35, 10), other_engine.plane(50, 35)
    L = api.load()
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        outs = [np.full((35, 50), 0x5C, np.uint8) for _ in range(2)]
        oa = (C.c_void_p * 2)(outs[0].ctypes.data, outs[1].ctypes.data)
        fp8 = api.FrameParams(1, 0, 8, 0, -1)

        def frame(l0, l1, fp=fp8, ww=w, hh=h, f=field, d=dirs, r=refs, per=64, o=oa, stride=50, n0=None, n1=None):
            ptr = lambda x: None if x is None else x.ctypes.data
            return L.hmme_predict_chroma_bi_refs_frame(engine.h, api._handles(l0), len(l0) // 2 if n0 is None else n0, api._handles(l1), len(l1) // 2 if n1 is None else n1,
                                                       ww, hh, C.byref(fp), None, None, ptr(f), ptr(d), ptr(r), per, o, stride)
        good = [cb, cr]
        for l0, l1 in (([cb, luma], good), (good, [luma, cr]), ([cb, deep], good), (good, [deep, cr]), ([foreign, cr], good), (good, [cb, foreign])):
            assert frame(l0, l1) == ERR_ARG, (l0, l1)
        assert frame(good, good, ww=101) == ERR_ARG and frame(good, good, hh=8) == ERR_ARG and frame(good, good, n0=0) == ERR_ARG and frame(good, good, n1=0) == ERR_ARG
        assert frame(good, good, f=None) == ERR_ARG and frame(good, good, d=None) == ERR_ARG and frame(good, good, r=None) == ERR_ARG
        assert frame(good, good, per=2) == ERR_ARG and frame(good, good, o=None) == ERR_ARG and frame(good, good, stride=49) == ERR_ARG
        assert frame(good, good, fp=api.FrameParams(1, 0, 10, 0, -1)) == ERR_ARG and frame(good, good, fp=api.FrameParams(1, 0, 8, 4, 1)) == ERR_ARG
        assert all((o == 0x5C).all() for o in outs)
        assert frame(good, good) == 0 and all((o != 0x5C).any() for o in outs)           # the accepted neighbour does run
        one = C.c_void_p(256)
        call = lambda f=one, d=one, r=one, cbo=one, cro=one, pitch=50, l0=api._handles(good), n0=1: L.hmme_predict_chroma_bi_refs_device(
            engine.h, l0, n0, api._handles(good), 1, w, h, C.byref(fp8), None, None, f, d, r, 64, cbo, cro, pitch, None)
        assert call(f=None) == ERR_ARG and call(d=None) == ERR_ARG and call(r=None) == ERR_ARG and call(cbo=None) == ERR_ARG and call(cro=None) == ERR_ARG
        assert call(pitch=49) == ERR_ARG and call(l0=None) == ERR_ARG and call(n0=8) == ERR_ARG and call(l0=api._handles([cb, luma])) == ERR_ARG
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in (cb, cr, luma, deep, foreign):
            p.close()
        other_engine.close()
