"""The prediction of a B picture with several references per list (hmme_predict_bi_refs_device / _frame) against
tests/predict_bi_refs_model.py -- per block predict_bi_model on the two planes the block's indices name -- and bit for bit against its
single-reference siblings Engine.predict_bi_frame and Engine.predict_refs_frame where they define the same picture.  Every comparison is
bit-exact."""
import ctypes as C

import numpy as np
import pytest

import predict_bi_refs_model as pbrm
from frame_helpers import bind_hmo, check_strided_image, dims, mkplane

pytestmark = pytest.mark.gpu

SIZES = ((64, 64), (100, 70), (136, 72))                      # one CTU; partial CTUs on two edges and the corner; 3 x 2 CTUs
N0, N1 = 3, 2


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


def textures(w, h, bd, seed, n):
    """n unrelated padded pictures"""
    from hmme import synth
    return [synth.make_pair(w, h, seed=seed + 7 * k, bit_depth=bd, max_mv=2)[1] for k in range(n)]


def in_picture(w, h, per):
    cx_n, cy_n = dims(w, h)
    g = 64 if per == 1 else 8
    return [(c, b) for c in range(cx_n * cy_n) for b in range(per) if (c % cx_n) * 64 + (b % 8) * g < w and (c // cx_n) * 64 + (b // 8) * g < h]


def inputs(w, h, per, seed, n0=N0, n1=N1):
    """(field int16[2, n, per, 2], dirs uint8[n, per], refs uint8[2, n, per]).  The blocks inside the picture walk, list by list, through the
    16 quarter-pel phases; the first 48 of them are directions 3, 1, 2 in turn with indices inside their lists (every plane of both lists
    named), then come blocks that use an index of 0xFF or of the list's count, then draws from 1, 2, 3, 0xFF, 0 and 4.  MVs reach beyond
    TComDataCU::clipMv's range"""
    rng = np.random.default_rng(seed)
    n = dims(w, h)[0] * dims(w, h)[1]
    field = (4 * rng.integers(-200, 201, size=(2, n, per, 2))).astype(np.int16)
    dirs = rng.choice(np.array([1, 2, 3, 0xFF, 0, 4], np.uint8), size=(n, per))
    refs = np.stack([rng.integers(0, n0, size=(n, per)), rng.integers(0, n1, size=(n, per))]).astype(np.uint8)
    for j, (c, b) in enumerate(in_picture(w, h, per)):
        field[0, c, b] += (j & 3, (j >> 2) & 3)
        field[1, c, b] += ((j >> 2) & 3, j & 3)
        if j < 48:
            dirs[c, b] = (3, 1, 2)[j % 3]
            refs[0, c, b], refs[1, c, b] = (j // 3) % n0, (j // 3) % n1
        elif j < 54:                                           # a used list without a plane: 0xFF, or the first index beyond the list
            dirs[c, b] = (1, 2, 3, 3, 1, 2)[j - 48]
            refs[0, c, b] = (0xFF, 0, n0, 0, n0, 0)[j - 48]
            refs[1, c, b] = (0, 0xFF, 0, n1, 0, n1)[j - 48]
        elif j < 56:                                           # ... and an unused list's index is not looked at
            dirs[c, b] = (1, 2)[j - 54]
            refs[2 - dirs[c, b], c, b] = 0xFF
    return field, dirs, refs


def block_mask(w, h, per, pick):
    """boolean [h, w]: the samples of the blocks for which pick(ctu, block) holds"""
    cx_n, cy_n = dims(w, h)
    g = 64 if per == 1 else 8
    mask = np.zeros((h, w), bool)
    for c in range(cx_n * cy_n):
        for b in range(per):
            if pick(c, b):
                x0, y0 = (c % cx_n) * 64 + (b % 8) * g, (c // cx_n) * 64 + (b // 8) * g
                mask[y0:y0 + g, x0:x0 + g] = True
    return mask


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("bd", [8, 10])
def test_against_the_model(engine, hmo, bd, size):
    w, h = size
    pics = textures(w, h, bd, 1100 + bd + w, N0 + N1)
    planes = [mkplane(engine, r, w, h, bd) for r in pics]
    p0, p1 = planes[:N0], planes[N0:]
    try:
        dt, fill = (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0x2A5)
        field, dirs, refs = inputs(w, h, 64, 1110 + bd + w)
        got = engine.predict_bi_refs_frame(p0, p1, field, dirs, refs, out=np.full((h, w), fill, dt))
        want = pbrm.pred_picture(hmo, pics[:N0], pics[N0:], w, h, bd, field, dirs, refs, np.full((h, w), fill, np.int64))
        assert np.array_equal(got, want)
        # about the recipe: all 16 phases in each list among the blocks that use it, every plane named, every kind of dead block
        live = [(c, b) for c, b in in_picture(w, h, 64) if dirs[c, b] in (1, 2, 3)
                and all(not (dirs[c, b] >> l) & 1 or refs[l, c, b] < (N0, N1)[l] for l in range(2))]
        for l in range(2):
            used = [(c, b) for c, b in live if (dirs[c, b] >> l) & 1]
            assert len({(int(field[l, c, b, 0]) & 3, int(field[l, c, b, 1]) & 3) for c, b in used}) == 16
            assert {int(refs[l, c, b]) for c, b in used} == set(range((N0, N1)[l]))
        assert {int(dirs[c, b]) for c, b in live} == {1, 2, 3}
        no_plane = block_mask(w, h, 64, lambda c, b: dirs[c, b] in (1, 2, 3) and any((dirs[c, b] >> l) & 1 and refs[l, c, b] >= (N0, N1)[l] for l in range(2)))
        no_dir = block_mask(w, h, 64, lambda c, b: dirs[c, b] not in (1, 2, 3))
        assert no_plane.any() and no_dir.any() and (got[no_plane] == fill).all() and (got[no_dir] == fill).all()
        unused = block_mask(w, h, 64, lambda c, b: dirs[c, b] in (1, 2) and refs[2 - dirs[c, b], c, b] == 0xFF and refs[dirs[c, b] - 1, c, b] < (N0, N1)[dirs[c, b] - 1])
        assert unused.any() and (got[unused] != fill).any()
        # a block that names plane r differs from the same block read from another plane of its list
        swapped = refs.copy()
        swapped[0] = (swapped[0] + 1) % N0
        other = engine.predict_bi_refs_frame(p0, p1, field, dirs, swapped, out=np.full((h, w), fill, dt))
        alive = set(live)
        m = block_mask(w, h, 64, lambda c, b: (c, b) in alive and dirs[c, b] & 1)
        assert not np.array_equal(other[m], got[m])
    finally:
        for p in planes:
            p.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_one_mv_per_ctu_sub_range_and_strided_image(engine, hmo, bd):
    w, h = 136, 72
    pics = textures(w, h, bd, 1200 + bd, N0 + N1)
    planes = [mkplane(engine, r, w, h, bd) for r in pics]
    p0, p1 = planes[:N0], planes[N0:]
    try:
        dt, fill = (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0x2A5)
        field = np.zeros((2, 6, 1, 2), np.int16)
        field[0, :, 0] = [(-700, 650), (5, -3), (-18, 7), (33, 2), (-1, -1), (14, 12)]
        field[1, :, 0] = [(700, -650), (6, 9), (3, 3), (-33, -2), (-5, -7), (-14, 11)]
        dirs = np.array([3, 3, 1, 2, 0xFF, 3], np.uint8).reshape(6, 1)
        refs = np.array([[2, 0, 1, 0xFF, 0, N0], [1, 0, 0xFF, 1, 0, 0]], np.uint8).reshape(2, 6, 1)
        got = engine.predict_bi_refs_frame(p0, p1, field, dirs, refs, out=np.full((h, w), fill, dt))
        want = pbrm.pred_picture(hmo, pics[:N0], pics[N0:], w, h, bd, field, dirs, refs, np.full((h, w), fill, np.int64))
        assert np.array_equal(got, want)
        assert (got[:64, :128] != fill).any() and (got[64:, 64:] == fill).all()      # CTU 4: no direction; CTU 5: list 0's index beyond the list
        # a CTU sub-range of a field with one MV per block: the rest of the caller's image keeps its samples
        f64, d64, r64 = inputs(w, h, 64, 1210 + bd)
        whole = engine.predict_bi_refs_frame(p0, p1, f64, d64, r64, out=np.full((h, w), fill, dt))
        part = engine.predict_bi_refs_frame(p0, p1, f64, d64, r64, out=np.full((h, w), fill, dt), ctu_first=1, ctu_count=1)
        assert np.array_equal(part[:64, 64:128], whole[:64, 64:128]) and (whole[:64, 64:128] != fill).any()
        part[:64, 64:128] = fill
        assert (part == fill).all()
        # ... and into an image whose stride exceeds the width
        f = np.ascontiguousarray(f64)
        from hmme import api
        h0, h1 = api._handles(p0), api._handles(p1)
        check_strided_image(w, h, bd, lambda out, first, count: engine.predict_bi_refs_frame(p0, p1, f64, d64, r64, out=out, ctu_first=first, ctu_count=count),
                            lambda fp, out, stride: engine.L.hmme_predict_bi_refs_frame(engine.h, h0, N0, h1, N1, C.byref(fp), f.ctypes.data, d64.ctypes.data, r64.ctypes.data,
                                                                                        64, out, stride))
    finally:
        for p in planes:
            p.close()


@pytest.mark.parametrize("bd", [8, 10])
def test_siblings_bit_for_bit(engine, bd):
    """one plane per list: predict_bi_frame; direction 1 only: predict_refs_frame of list 0"""
    w, h = 100, 70
    pics = textures(w, h, bd, 1300 + bd, N0 + 1)
    planes = [mkplane(engine, r, w, h, bd) for r in pics]
    try:
        dt, fill = (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0x2A5)
        for per in (1, 64):
            field, dirs, _ = inputs(w, h, per, 1310 + bd + per)
            zero = np.zeros((2,) + dirs.shape, np.uint8)
            got = engine.predict_bi_refs_frame(planes[:1], planes[1:2], field, dirs, zero, out=np.full((h, w), fill, dt))
            assert np.array_equal(got, engine.predict_bi_frame(planes[0], planes[1], field, dirs, out=np.full((h, w), fill, dt))) and (got != fill).any()
            _, _, refs = inputs(w, h, per, 1320 + bd + per)
            ones = np.ones(dirs.shape, np.uint8)
            got = engine.predict_bi_refs_frame(planes[:N0], planes[N0:], field, ones, refs, out=np.full((h, w), fill, dt))
            want = engine.predict_refs_frame(planes[:N0], field[0], refs[0], out=np.full((h, w), fill, dt))
            assert np.array_equal(got, want) and (got != fill).any()
    finally:
        for p in planes:
            p.close()


def test_device_call_and_sixteen_planes_per_list(engine, hmo):
    """hmme_predict_bi_refs_device on device buffers, 16 + 16 planes (the same few pictures under many handles), a CTU sub-range and a pitched image"""
    import torch
    from hmme import api
    w, h, n = 136, 72, 6
    dev = torch.device("cuda", 0)
    pics = textures(w, h, 8, 1400, 4)
    planes = [mkplane(engine, r, w, h, 8) for r in pics]
    try:
        l0 = [planes[k % 4] for k in range(16)]
        l1 = [planes[(k + 1) % 4] for k in range(16)]
        field, dirs, refs = inputs(w, h, 64, 1410, 16, 16)
        d_field, d_dirs, d_refs = (torch.from_numpy(a).to(dev) for a in (field, dirs, refs))
        img = torch.full((h, w + 24), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        fp = api.FrameParams(1, 0, 8, 1, 4)                                     # CTUs 1..4
        engine.predict_bi_refs_device(l0, l1, fp, d_field.data_ptr(), d_dirs.data_ptr(), d_refs.data_ptr(), 64, img.data_ptr(), w + 24, 0)
        torch.cuda.synchronize()
        want = pbrm.pred_picture(hmo, [pics[k % 4] for k in range(16)], [pics[(k + 1) % 4] for k in range(16)], w, h, 8, field, dirs, refs,
                                 np.full((h, w), 0xA5, np.int64), ctus=range(1, 5))
        got = img.cpu().numpy()
        assert np.array_equal(got[:, :w], want) and (got[:, w:] == 0xA5).all()
        assert (want[:64, :64] == 0xA5).all() and (want[64:, 128:] == 0xA5).all() and (want != 0xA5).any()
        assert refs.max() == 0xFF and (refs[(refs != 0xFF)] >= 8).any()             # about the recipe: high indices are named
    finally:
        for p in planes:
            p.close()


def test_refusals(engine):
    from hmme import api
    w, h, n = 136, 72, 6
    field, dirs, refs = np.zeros((2, n, 64, 2), np.int16), np.full((n, 64), 3, np.uint8), np.zeros((2, n, 64), np.uint8)
    other_engine = api.Engine(0, 64)
    a, b, small, deep, foreign = engine.plane(w, h), engine.plane(w, h), engine.plane(64, 64), engine.plane(w, h, 10), other_engine.plane(w, h)
    L = api.load()
    prev = L.hmme_set_error_printing(engine.h, 0)
    try:
        img = np.full((h, w), 0x5C, np.uint8)
        fp8 = api.FrameParams(1, 0, 8, 0, -1)

        def frame(l0, l1, fp=fp8, f=field, d=dirs, r=refs, per=64, n0=None, n1=None, stride=w):
            ptr = lambda x: None if x is None else x.ctypes.data
            return L.hmme_predict_bi_refs_frame(engine.h, api._handles(l0), len(l0) if n0 is None else n0, api._handles(l1), len(l1) if n1 is None else n1, C.byref(fp),
                                                ptr(f), ptr(d), ptr(r), per, img.ctypes.data, stride)
        # every plane of both lists: one size, the call's bit depth, this context
        for l0, l1 in (([a, small], [b]), ([a], [b, small]), ([small], [a]), ([a, deep], [b]), ([a], [deep]), ([a, foreign], [b]), ([a], [b, foreign]), ([foreign], [a])):
            assert frame(l0, l1) == -1, (l0, l1)
        assert frame([a], [b], n0=0) == -1 and frame([a], [b], n1=0) == -1 and frame([a] * 16, [b], n0=17) == -1 and frame([a], [b] * 16, n1=17) == -1
        assert frame([a], [b], f=None) == -1 and frame([a], [b], d=None) == -1 and frame([a], [b], r=None) == -1 and frame([a], [b], per=256) == -1
        assert frame([a], [b], stride=w - 1) == -1
        for bad in (7, 13):
            assert frame([a], [b], fp=api.FrameParams(1, 0, bad, 0, -1)) == -1
        assert frame([a], [b], fp=api.FrameParams(1, 0, 10, 0, -1)) == -1             # 8-bit planes, a 10-bit call
        assert frame([a], [b], fp=api.FrameParams(1, 0, 8, 6, 1)) == -1               # a CTU range outside the picture
        assert (img == 0x5C).all()
        with pytest.raises(api.HmmeError):
            engine.predict_bi_refs_frame([a], [deep], field, dirs, refs, out=img)
        assert frame([a, b], [b]) == 0 and (img != 0x5C).any()                       # the accepted neighbour does run
        # the device entry refuses before anything is launched (addresses never dereferenced)
        one = C.c_void_p(256)
        ha, hb = api._handles([a]), api._handles([b])
        call = lambda fp=fp8, f=one, d=one, r=one, per=64, o=one, pitch=w, l0=ha, l1=hb, n0=1, n1=1: L.hmme_predict_bi_refs_device(
            engine.h, l0, n0, l1, n1, C.byref(fp), f, d, r, per, o, pitch, None)
        assert call(f=None) == -1 and call(d=None) == -1 and call(r=None) == -1 and call(o=None) == -1 and call(per=2) == -1 and call(pitch=w - 1) == -1
        assert call(l0=None) == -1 and call(l1=None) == -1 and call(n0=0) == -1 and call(n1=17) == -1
        assert call(l1=api._handles([small])) == -1 and call(l0=api._handles([foreign])) == -1
    finally:
        L.hmme_set_error_printing(engine.h, prev)
        for p in (a, b, small, deep, foreign):
            p.close()
        other_engine.close()
