"""4:2:0 chroma motion compensation without a GPU: the model of tests/predict_chroma_model.py against blocks recorded from the reference's
compiled TComInterpolationFilter (tests/golden/chroma_mc.npz) and against the live library where it was built, its fixed points, the exported
names, what is refused without a context, and yuv.read_chroma."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import oracle_py
import predict_bi_w_model as pbw
import predict_chroma_model as cm
import range_content as rc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "chroma_mc.npz")
NEW = ("hmme_predict_chroma_pairs_device", "hmme_predict_chroma_frame", "hmme_predict_chroma_refs_device", "hmme_predict_chroma_refs_frame",
       "hmme_predict_chroma_bi_device", "hmme_predict_chroma_bi_frame")
ERR_ARG = pbw.ERR_ARG


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def model_block(src, n, x_frac, y_frac, bd, bi):
    """the n x n block whose top-left sample is src[1, 1], by the model"""
    f = cm.inter_epel if bi else cm.pred_epel
    return f(src, 1, 1, n, n, x_frac, y_frac, bd)


def golden_blocks(g):
    """(source, block size, xFrac, yFrac, bit depth, bi, recorded block) of everything the file holds"""
    for i, bd in enumerate(g["bds"]):
        for c in range(3):
            for ph in range(64):
                for bi in range(2):
                    yield g["src4"][i, c], 4, ph & 7, ph >> 3, int(bd), bool(bi), g["out4"][i, c, ph, bi]
    for n in (2, 32):
        bd, fx, fy = (int(v) for v in g[f"at{n}"])
        for bi in range(2):
            yield g[f"src{n}"], n, fx, fy, bd, bool(bi), g[f"out{n}"][bi]


def test_golden_holds_what_it_should(golden):
    assert list(golden["bds"]) == [8, 9, 10, 12] and golden["src4"].shape == (4, 3, 7, 7) and golden["out4"].shape == (4, 3, 64, 2, 4, 4)
    for i, bd in enumerate(golden["bds"]):
        maxv = (1 << int(bd)) - 1
        assert set(np.unique(golden["src4"][i, 1])) == {0, maxv} and (golden["src4"][i, 2] == maxv).all()
    assert golden["out2"].shape == (2, 2, 2) and golden["out32"].shape == (2, 32, 32)
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "frac_wp.npz"))
    assert sum(1 for _ in golden_blocks(golden)) == 1536 + 4


def test_model_equals_the_recorded_reference(golden):
    for src, n, fx, fy, bd, bi, want in golden_blocks(golden):
        assert np.array_equal(model_block(src, n, fx, fy, bd, bi), want), (n, fx, fy, bd, bi)


@pytest.mark.skipif(not oracle_py.ref_available(), reason="oracle/_ref/libhmref.so is not built here")
def test_model_equals_the_live_reference(golden):
    spec = importlib.util.spec_from_file_location("gen_chroma_golden", os.path.join(HERE, "golden", "gen_chroma_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for src, n, fx, fy, bd, bi, want in golden_blocks(golden):                   # the recording is what the library answers now
        assert np.array_equal(gen.ref_block(src, n, fx, fy, bd, bi), want), (n, fx, fy, bd, bi)
    rng = np.random.default_rng(421)
    for k in range(200):                                                            # fresh blocks of other sizes, every depth 8..12
        bd, n = int(rng.integers(8, 13)), int(rng.choice([2, 4, 8, 16]))
        fx, fy, bi = int(rng.integers(0, 8)), int(rng.integers(0, 8)), bool(k & 1)
        src = gen.contents(rng, n, bd)[k % 3]
        assert np.array_equal(model_block(src, n, fx, fy, bd, bi), gen.ref_block(src, n, fx, fy, bd, bi)), (k, n, fx, fy, bd, bi)


@pytest.mark.parametrize("bd", [8, 9, 10, 11, 12])
def test_phase_zero_is_the_sample_itself(bd):
    rng = np.random.default_rng(430 + bd)
    plane = rng.integers(0, 1 << bd, size=(40, 40))
    for ex, ey in ((0, 0), (8, -16), (-24, 8)):
        want = plane[10 + (ey >> 3):18 + (ey >> 3), 12 + (ex >> 3):20 + (ex >> 3)]
        assert np.array_equal(cm.pred_epel(plane, 12, 10, 8, 8, ex, ey, bd), want)
        assert np.array_equal(cm.inter_epel(plane, 12, 10, 8, 8, ex, ey, bd), (want << max(2, 14 - bd)) - 8192)


def test_negative_mvs_floor():
    plane = np.arange(40 * 40).reshape(40, 40) % 251
    for e in (-1, -7, -8, -9, -17):
        a = cm.pred_epel(plane, 12, 10, 4, 4, e, e, 8)
        b = cm.pred_epel(plane, 12 + (e >> 3), 10 + (e >> 3), 4, 4, e & 7, e & 7, 8)
        assert (e >> 3) == -((-e + 7) // 8) and np.array_equal(a, b)


def test_taps_sum_to_64_and_mirror():
    assert (cm.CHROMA_TAPS.sum(axis=1) == 64).all()
    for p in range(1, 8):
        assert list(cm.CHROMA_TAPS[p]) == list(cm.CHROMA_TAPS[8 - p][::-1])


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_clip_behaviour_is_the_luma_models_at_both_ends(bd):
    """on binary content the unclipped sum over- and undershoots; the clip is range_content.pred_qpel's: [0, maxv], and nothing else changes"""
    maxv = (1 << bd) - 1
    rng = np.random.default_rng(440 + bd)
    plane = np.where(rng.integers(0, 2, size=(48, 48)) == 1, maxv, 0)
    lo = hi = False
    for ph in range(64):
        raw = cm.pred_epel(plane, 8, 8, 32, 32, ph & 7, ph >> 3, bd, clip=False)
        got = cm.pred_epel(plane, 8, 8, 32, 32, ph & 7, ph >> 3, bd)
        assert np.array_equal(got, np.clip(raw, 0, maxv))
        lo, hi = lo or bool((raw < 0).any()), hi or bool((raw > maxv).any())
    assert lo and hi
    # the luma model clips the same way: a flat picture at either end comes out as itself from both
    for v in (0, maxv):
        flat = np.full((48, 48), v)
        assert (rc.pred_qpel(flat, 16, 16, 8, 8, 5, 7, bd) == v).all() and (cm.pred_epel(flat, 16, 16, 8, 8, 5, 7, bd) == v).all()
    raw_l = rc.pred_qpel(plane, 16, 16, 8, 8, 2, 2, bd, clip=False)
    assert np.array_equal(rc.pred_qpel(plane, 16, 16, 8, 8, 2, 2, bd), np.clip(raw_l, 0, maxv))


def test_exported_names_and_null_contexts():
    from hmme import api
    L = api.load()
    for name in NEW:
        assert name in api.SYMBOLS and hasattr(L, name), name
    assert L.hmme_abi_version() == 6
    fp = api.FrameParams(1, 0, 8, 0, -1)
    a = C.c_void_p(256)   # never dereferenced
    pa = (C.c_void_p * 4)(256, 256, 256, 256)
    assert L.hmme_predict_chroma_pairs_device(None, pa, 1, 64, 64, C.byref(fp), None, a, 64, pa, 32, None) == ERR_ARG
    assert L.hmme_predict_chroma_frame(None, pa, 64, 64, C.byref(fp), None, a, 64, pa, 32) == ERR_ARG
    assert L.hmme_predict_chroma_refs_device(None, pa, 1, 64, 64, C.byref(fp), None, a, a, 64, a, a, 32, None) == ERR_ARG
    assert L.hmme_predict_chroma_refs_frame(None, pa, 1, 64, 64, C.byref(fp), None, a, a, 64, pa, 32) == ERR_ARG
    assert L.hmme_predict_chroma_bi_device(None, pa, pa, 1, 64, 64, C.byref(fp), None, None, a, a, 64, pa, 32, None) == ERR_ARG
    assert L.hmme_predict_chroma_bi_frame(None, pa, pa, 64, 64, C.byref(fp), None, None, a, a, 64, pa, 32) == ERR_ARG


def test_weight_refusals_are_the_luma_checks_per_component():
    """what the chroma calls run on every component's weights, asked without a context: the codes of the existing pure host checks.  (The
    refusals that need planes -- sizes, depths, contexts -- need a device to make the planes: tests/test_gpu_predict_chroma.py)"""
    from hmme import api
    good, other_shift, huge = (70, 9, 6, 32), (35, 9, 5, 16), (1 << 20, 0, 6, 32)
    assert api.predict_bi_weight_check(8, good, good) == 0
    assert api.predict_bi_weight_check(8, good, other_shift) == ERR_ARG             # the two lists of ONE component
    assert api.predict_bi_weight_check(8, other_shift, other_shift) == 0             # ... while Cb and Cr may differ from each other
    assert api.predict_bi_weight_check(8, huge, good) == pbw.ERR_UNSUPPORTED
    assert api.bipred_weight_check(8, pbw.ident(6), huge) == pbw.ERR_UNSUPPORTED and api.bipred_weight_check(8, pbw.ident(6), good) == 0


@pytest.mark.parametrize("bd", [8, 10])
def test_read_chroma_reads_back_a_written_file(tmp_path, bd):
    from hmme import yuv
    w, h = 36, 20
    rng = np.random.default_rng(450 + bd)
    dt = np.uint8 if bd == 8 else np.uint16
    frames = [(rng.integers(0, 1 << bd, size=(h, w)).astype(dt),) + tuple(rng.integers(0, 1 << bd, size=(h // 2, w // 2)).astype(dt) for _ in range(2))
              for _ in range(3)]
    path = str(tmp_path / "p.yuv")
    yuv.write_420(path, frames, bd)
    assert os.path.getsize(path) == 3 * yuv.frame_bytes(w, h, bd)
    f = yuv.LumaFile(path, w, h, bd)
    try:
        for t, (y, cb, cr) in enumerate(frames):
            got = yuv.read_chroma(path, w, h, t, bd)
            assert got[0].dtype == dt and np.array_equal(got[0], cb) and np.array_equal(got[1], cr)
            assert np.array_equal(yuv.read_luma(path, w, h, t, bd), y)
            again = f.chroma(t)
            assert np.array_equal(again[0], cb) and np.array_equal(again[1], cr)
        with pytest.raises(ValueError):
            yuv.read_chroma(path, w, h, 3, bd)
        with pytest.raises(ValueError):
            yuv.read_chroma(path, w + 1, h, 0, bd)
    finally:
        f.close()


def test_synthetic_chroma_follows_the_luma_motion():
    """make_chroma_pair: the chroma of a region is the reference's chroma displaced by the region's luma MV read in eighth chroma pels"""
    from hmme import synth
    w, h, m = 128, 64, synth.MARGIN
    cur, ref, mv = synth.make_pair(w, h, seed=31, max_mv=5, region=64)
    (ccb, ccr), (rcb, rcr) = synth.make_chroma_pair(w, h, mv, seed=31, region=64, noise_sigma=0.0)
    assert ccb.shape == (h // 2 + 2 * m, w // 2 + 2 * m) and not np.array_equal(rcb, rcr)
    for comp_cur, comp_ref in ((ccb, rcb), (ccr, rcr)):
        for i in range(2):
            dx, dy = int(mv[0, i, 0]), int(mv[0, i, 1])
            x0 = m + 32 * i + 8                                                      # an inner 16 x 16 window of the region's 32 x 32 chroma
            true = comp_cur[m + 8:m + 24, x0:x0 + 16].astype(np.int64)
            sad = lambda ex, ey: int(np.abs(cm.pred_epel(comp_ref, x0, m + 8, 16, 16, ex, ey, 8) - true).sum())
            assert sad(4 * dx, 4 * dy) < sad(0, 0) or (dx, dy) == (0, 0)
            assert sad(4 * dx, 4 * dy) <= min(sad(4 * dx + 4, 4 * dy), sad(4 * dx - 4, 4 * dy), sad(4 * dx, 4 * dy + 4), sad(4 * dx, 4 * dy - 4))
