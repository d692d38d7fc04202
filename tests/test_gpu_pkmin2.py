"""GPU check of the search kernel that holds the packed-minimum twin and its marker-free body (me_search_kernel<1, SPLIT, 2>: ME_PKMINE,
me_task_marker_free, me_pk_recover<true> in me_kernels.hpp; the tree of tools/gen_me_tree.py Tree(1, pk=2)), bit-exact against the oracle in
every launch form, at the smallest shapes that can still go wrong:
  * the per-CTU call (SPLIT 1) on one CTU with windows of 128 .. 132 x 8, 9 candidates: 32 or 33 quads per row, the last one whole or cut
    (the part that holds it runs the marker body, the 32-quad part the marker-free one), the folded last row at 9 rows, two window tiles
    beyond 129 columns;
  * a 192 x 128 picture at search range 64 (segments, SPLIT 2) with and without per-CTU predictors: windows clipped on every side;
  * a 128 x 128 picture at search range 8, which the planner runs as whole jobs (SPLIT 0): rows of 4 + 1 quads;
each with FEN on and off and at lambda 0, 57.9, at the largest value of the new gate, one above it (the PK = 1 kernel) and above the old
gate (the 32-bit kernel); flat pictures, where every candidate ties and raster order decides; and a pair whose 16x12 and 12x16 sums sit at
their maximum (current 0, reference 255) under the largest MV cost a launch can reach at the gate's lambda."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LQ = 3794534            # lambda 57.9
GATE2_LQ = 14680063     # the largest lambda_q16 of me_pk2_gate (tests/test_tree_pkmin2.py pins it)
GATE_LQ = 29132523      # the largest lambda_q16 of me_pk_gate (tests/test_tree_pkmin.py pins it)
LAMBDAS = [0, LQ, GATE2_LQ, GATE2_LQ + 1, GATE_LQ + 1]
WINDOWS = [(wx, wy) for wx in (128, 129, 130, 131, 132) for wy in (8, 9)]
M = 80                  # margin of the hand-made planes: a window of 132 candidates from -66 reads columns -66 .. 65 + 63


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 128)
    yield e
    e.close()


def body(lq, fen):
    from hmme import api
    L = api.load()
    L.hmme_test_pk_body.argtypes = [C.c_uint32, C.c_int]
    L.hmme_test_pk_body.restype = C.c_int
    return L.hmme_test_pk_body(lq, fen)


def tail_plan(w, h, sr):
    from hmme import api
    L = api.load()
    L.hmme_test_tail_plan.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)]
    out = (C.c_int * 4)()
    assert L.hmme_test_tail_plan(w, h, sr, 1, 512, out) == 0
    return tuple(out)


def ctu_planes(kind):
    """-> (cur, ref) int16 planes of one CTU at (M, M) with M samples around it"""
    n = 64 + 2 * M
    if kind == "flat":
        return np.full((n, n), 77, np.int16), np.full((n, n), 77, np.int16)
    if kind == "max":
        return np.zeros((n, n), np.int16), np.full((n, n), 255, np.int16)
    rng = np.random.default_rng(90210)
    ref = rng.integers(0, 256, size=(n, n))
    cur = np.clip(np.roll(ref, (2, -3), axis=(0, 1)) + rng.integers(-5, 6, size=(n, n)), 0, 255)
    return cur.astype(np.int16), ref.astype(np.int16)


def check_ctu(engine, oracle_lib, cur, ref, wx, wy, pred, lq, fen):
    from hmme import api
    lt = (-(wx // 2), -(wy // 2))
    rb = (lt[0] + wx - 1, lt[1] + wy - 1)
    engine.set_lambda_q16(lq)
    mv, sad = engine.search_ctu(cur, (M, M), ref, (M, M), api.SearchParams(lt[0], lt[1], rb[0], rb[1], pred[0], pred[1], fen, 8))
    ox, oy, osad = oracle_lib.search_ctu(cur, (M, M), ref, (M, M), oracle_lib.make_params(lt, rb, pred, lq, fen, 8))
    bad = np.argwhere((mv[:, 0] != ox) | (mv[:, 1] != oy) | (sad != osad)).ravel()
    assert len(bad) == 0, (wx, wy, lq, fen, len(bad), bad[:8].tolist())
    return mv, sad


def test_the_cases_are_what_they_claim():
    assert [body(lq, 1) for lq in LAMBDAS] == [2, 2, 2, 1, 0] and [body(lq, 0) for lq in LAMBDAS] == [1, 1, 1, 1, 0]
    assert tail_plan(128, 128, 8) == (4, 4, 0, 0), "four whole jobs"
    jobs, head, segments, one = tail_plan(192, 128, 64)
    assert (jobs, head, one) == (6, 0, 1) and segments > 6, "six jobs, all dealt as segments"


@pytest.mark.parametrize("lq", LAMBDAS)
@pytest.mark.parametrize("fen", [1, 0])
def test_per_ctu_call_at_windows_around_32_and_33_quads(engine, oracle_lib, fen, lq):
    cur, ref = ctu_planes("noise")
    for wx, wy in WINDOWS:
        check_ctu(engine, oracle_lib, cur, ref, wx, wy, (9, -14), lq, fen)


@pytest.mark.parametrize("wx,wy", [(128, 8), (129, 9), (131, 9), (132, 8)])
def test_per_ctu_call_on_flat_pictures(engine, oracle_lib, wx, wy):
    cur, ref = ctu_planes("flat")
    mv, sad = check_ctu(engine, oracle_lib, cur, ref, wx, wy, (0, 0), 0, 1)
    assert (mv[:, 0] == -(wx // 2)).all() and (mv[:, 1] == -(wy // 2)).all() and (sad == 0).all(), "the first candidate in raster order"


@pytest.mark.parametrize("wx,wy", [(128, 8), (129, 9), (130, 8)])
def test_per_ctu_call_with_sums_at_their_maximum(engine, oracle_lib, wx, wy):
    """current 0, reference 255, the gate's largest lambda and a predictor at the end of int16: an MV costs 66 bits (14 783), the
    16x12 and 12x16 slots 48 960 + that in every candidate"""
    cur, ref = ctu_planes("max")
    mv, sad = check_ctu(engine, oracle_lib, cur, ref, wx, wy, (-32768, -32768), GATE2_LQ, 1)
    assert sad[288] == sad[352] == 48960 and sad[448] == sad[480] == 32640 and sad[256] == sad[320] == 16320


FRAMES = {
    # name -> (width, height, search range, content)
    "segments":       (192, 128, 64, "noise"),
    "segments_pred":  (192, 128, 64, "noise_out"),      # predictors that push the windows over the picture's sides
    "whole":          (128, 128, 8, "noise"),
    "whole_flat":     (128, 128, 8, "flat"),
    "segments_flat":  (192, 128, 64, "flat"),
    "segments_max":   (192, 128, 64, "max"),
}
_FRAME = {}


def frame(name):
    from hmme import synth
    if name not in _FRAME:
        w, h, sr, kind = FRAMES[name]
        pred = None
        if kind == "flat":
            cur, ref = np.full((h, w), 77, np.uint8), np.full((h, w), 77, np.uint8)
        elif kind == "max":
            cur, ref = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
        else:
            rng = np.random.default_rng(1234 + w + sr)
            ref = rng.integers(0, 256, size=(h, w))
            cur = np.clip(np.roll(ref, (3, -5), axis=(0, 1)) + rng.integers(-5, 6, size=(h, w)), 0, 255)
            if kind == "noise_out":
                pred = np.array([[-70 * 4, -69 * 4], [3 * 4, -70 * 4], [69 * 4, -70 * 4], [-69 * 4, 70 * 4], [-2 * 4, 69 * 4], [70 * 4, 69 * 4]], np.int16)
        _FRAME[name] = (synth.pad_plane(cur), synth.pad_plane(ref), pred)
    return _FRAME[name]


def check_frame(engine, oracle_lib, name, lq, fen):
    from hmme import synth
    w, h, sr, kind = FRAMES[name]
    cur, ref, pred = frame(name)
    m = synth.MARGIN
    engine.set_lambda_q16(lq)
    with engine.plane(w, h) as pc, engine.plane(w, h) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        mv, sad = engine.search_frame(pc, pr, sr, pred, fen=fen)
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pred, lq, fen, 8, n_threads=8)
    bad = np.argwhere((mv[:, :, 0] != ox) | (mv[:, :, 1] != oy) | (sad != osad))
    assert len(bad) == 0, (name, lq, fen, len(bad), bad[:8].tolist())
    return mv, sad


@pytest.mark.parametrize("lq", LAMBDAS)
@pytest.mark.parametrize("fen", [1, 0])
@pytest.mark.parametrize("name", ["segments", "segments_pred", "whole"])
def test_picture_search_as_segments_and_as_whole_jobs(engine, oracle_lib, name, fen, lq):
    if name == "segments_pred":
        from refine_tables import oracle_windows
        win = oracle_windows(192, 128, 64, frame(name)[2])
        plain = oracle_windows(192, 128, 64)
        assert all(tuple(a) != tuple(b) for a, b in zip(win, plain)), "every CTU's window is moved by its predictor"
        assert all(w[2] - w[0] < 128 or w[3] - w[1] < 128 for w in win), "and clipped by the picture"
    check_frame(engine, oracle_lib, name, lq, fen)


@pytest.mark.parametrize("name", ["whole_flat", "segments_flat"])
def test_picture_search_on_flat_pictures(engine, oracle_lib, name):
    mv, sad = check_frame(engine, oracle_lib, name, 0, 1)
    assert (sad == 0).all()


def test_picture_search_with_sums_at_their_maximum(engine, oracle_lib):
    mv, sad = check_frame(engine, oracle_lib, "segments_max", GATE2_LQ, 1)
    assert (sad[:, 288] == 48960).all() and (sad[:, 352] == 48960).all()
