"""GPU check of the full-task twin of the search kernel (me_search_kernel<1, SPLIT, 2>: me_task_full, ME_PKMIN16_*, me_pmerge2 / 3,
ME_KEY16_*, the group scan of me_pk_recover<true> in me_kernels.hpp; the tree of tools/gen_me_tree.py Tree(1, pk=3)), bit-exact against
the oracle in every launch form, at the smallest shapes that can still go wrong:
  * the per-CTU call (SPLIT 1) on one CTU with windows that make full tasks of every part size (16, 32, 64, 128 candidates per row:
    k = 2 .. 5), a full part beside a narrower one (20, 48), windows with no full task at all (12: no part of four quads; 15: the cut
    quad lies in the four-quad part), a partial last lane-iteration (16 x 17), and the fold and the cut quad beside full tasks (129, 131);
  * a 128 x 64 picture at search range 8, which the planner runs as whole jobs (SPLIT 0): rows of 4 + 1 quads, the 4 full;
  * a 192 x 128 picture at search range 64 (segments, SPLIT 2): windows clipped on every side;
each at lambda 0, 57.9, 224 (the largest value of the gate) and 225 (the packed-minimum twin alone); ties -- flat pictures, references
periodic in x with period 4 (equal costs in neighbouring quads of one 16-candidate group), 16 (in neighbouring groups) and 64 (in lanes
that differ in lane bit 4 of the twin's layout), and rows shifted against each other so that the equal candidate of the next row lies at
a smaller x; and sums at their maximum (current 0 against reference 255 and the reverse: 16x12 and 12x16 reach 48 960) at lambda 224.
A half of a packed register that the hardware did not keep, a swap that moved the wrong rows, a key formed from the wrong half or a
group recovered from the wrong quad would each show as wrong tables here."""
import numpy as np
import pytest

import test_gpu_pkmin2 as B

pytestmark = pytest.mark.gpu

LQ, GATE2_LQ, M = B.LQ, B.GATE2_LQ, B.M
LQ225 = 225 << 16
LAMBDAS = [0, LQ, GATE2_LQ, LQ225]
WINDOWS = [(16, 16), (16, 17), (20, 16), (12, 16), (15, 16), (32, 9), (64, 8), (128, 8), (48, 16), (129, 9), (131, 9)]


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 128)
    yield e
    e.close()


def tie_planes(kind):
    """-> (cur, ref) int16 planes; cur == ref: MV (0, 0) costs no SAD, and so does every candidate the content repeats at"""
    n = 64 + 2 * M
    rng = np.random.default_rng(4711)
    if kind == "flat":
        ref = np.full((n, n), 77)
    elif kind == "rows":      # every row the row above shifted left by three: (x - 3, y + 1) sees what (x, y) sees
        line = rng.integers(0, 256, size=n + 3 * n)
        ref = np.stack([line[3 * r:3 * r + n] for r in range(n)])
    else:                     # periodic in x
        ref = np.tile(rng.integers(0, 256, size=(n, kind)), (1, n // kind + 1))[:, :n]
    return ref.astype(np.int16), ref.astype(np.int16)


def test_the_cases_are_what_they_claim():
    from hmme import api
    import ctypes as C
    assert [B.body(lq, 1) for lq in LAMBDAS] == [2, 2, 2, 1]
    assert B.tail_plan(128, 64, 8) == (2, 2, 0, 0), "two whole jobs"
    jobs, head, segments, one = B.tail_plan(192, 128, 64)
    assert (jobs, head, one) == (6, 0, 1) and segments > 6, "six jobs, all dealt as segments"
    L = api.load()
    L.hmme_test_pk_task_full.argtypes = [C.c_int] * 5
    L.hmme_test_pk_task_full.restype = C.c_int
    full = lambda wx, wy, k, it: L.hmme_test_pk_task_full(wx, wy, k, it, 1)      # the per-CTU call deals single lane-iterations
    assert full(16, 16, 2, 0) and full(16, 17, 2, 0) and not full(16, 17, 2, 1)
    assert full(20, 16, 2, 0) and not full(20, 16, 0, 0) and not full(12, 16, 1, 0) and not full(15, 16, 2, 0)
    assert full(32, 9, 3, 0) and not full(32, 9, 3, 1) and full(64, 8, 4, 1) and full(128, 8, 5, 3)
    assert full(48, 16, 3, 1) and full(48, 16, 2, 0)
    assert full(129, 9, 5, 3) and not full(129, 9, 5, 4) and not full(129, 9, 0, 0) and full(131, 9, 5, 0)


@pytest.mark.parametrize("lq", LAMBDAS)
def test_per_ctu_call_at_windows_of_every_part_size(engine, oracle_lib, lq):
    cur, ref = B.ctu_planes("noise")
    for wx, wy in WINDOWS:
        B.check_ctu(engine, oracle_lib, cur, ref, wx, wy, (9, -14), lq, 1)


@pytest.mark.parametrize("lq", [0, LQ])
@pytest.mark.parametrize("kind", ["flat", 4, 16, 64, "rows"])
def test_per_ctu_call_on_ties(engine, oracle_lib, kind, lq):
    cur, ref = tie_planes(kind)
    for wx, wy in [(128, 8), (129, 9), (64, 8), (48, 16), (16, 17)]:
        mv, sad = B.check_ctu(engine, oracle_lib, cur, ref, wx, wy, (5, -3), lq, 1)
        if lq == 0 and kind != "rows":      # the first candidate in raster order that the content repeats at
            period = 1 if kind == "flat" else kind
            first = -(wx // 2) + (wx // 2) % period
            assert (sad == 0).all() and (mv[:, 0] == first).all() and (mv[:, 1] == (-(wy // 2) if kind == "flat" else 0)).all()
        if lq == 0 and kind == "rows":      # zero SAD along x + 3 y = 0: the topmost row that holds one wins, whatever its x
            y = min(yy for yy in range(-(wy // 2), wy - wy // 2) if -(wx // 2) <= -3 * yy < wx - wx // 2)
            assert (sad == 0).all() and (mv[:, 1] == y).all() and (mv[:, 0] == -3 * y).all()


@pytest.mark.parametrize("cur_value", [0, 255])
def test_per_ctu_call_with_sums_at_their_maximum(engine, oracle_lib, cur_value):
    """every sample difference 255, the gate's largest lambda and a predictor at the end of int16: the 16x12 and 12x16 slots hold
    48 960 + the MV cost in every candidate"""
    n = 64 + 2 * M
    cur, ref = np.full((n, n), cur_value, np.int16), np.full((n, n), 255 - cur_value, np.int16)
    for wx, wy in [(16, 16), (64, 8), (128, 8), (129, 9)]:
        mv, sad = B.check_ctu(engine, oracle_lib, cur, ref, wx, wy, (-32768, -32768), GATE2_LQ, 1)
        assert sad[288] == sad[352] == 48960 and sad[448] == sad[480] == 32640 and sad[256] == sad[320] == 16320


FRAMES = {
    # name -> (width, height, search range, content)
    "whole":         (128, 64, 8, "noise"),
    "whole_flat":    (128, 64, 8, "flat"),
    "whole_max":     (128, 64, 8, "max"),
    "whole_p4":      (128, 64, 8, 4),
    "whole_p16":     (128, 64, 8, 16),
    "segments":      (192, 128, 64, "noise"),
    "segments_flat": (192, 128, 64, "flat"),
    "segments_max":  (192, 128, 64, "max"),
    "segments_p16":  (192, 128, 64, 16),
    "segments_p64":  (192, 128, 64, 64),
}
_FRAME = {}


def frame(name):
    from hmme import synth
    if name not in _FRAME:
        w, h, sr, kind = FRAMES[name]
        if kind == "noise":
            rng = np.random.default_rng(99 + w + sr)
            ref = rng.integers(0, 256, size=(h, w))
            cur = np.clip(np.roll(ref, (3, -5), axis=(0, 1)) + rng.integers(-5, 6, size=(h, w)), 0, 255)
        elif kind == "flat":
            cur = ref = np.full((h, w), 77)
        elif kind == "max":
            cur, ref = np.full((h, w), 255), np.zeros((h, w))
        else:
            cur = ref = np.tile(np.random.default_rng(kind).integers(0, 256, size=(h, kind)), (1, w // kind))
        _FRAME[name] = (synth.pad_plane(cur.astype(np.uint8)), synth.pad_plane(ref.astype(np.uint8)))
    return _FRAME[name]


def check_frame(engine, oracle_lib, name, lq):
    from hmme import synth
    w, h, sr, kind = FRAMES[name]
    cur, ref = frame(name)
    m = synth.MARGIN
    engine.set_lambda_q16(lq)
    with engine.plane(w, h) as pc, engine.plane(w, h) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        mv, sad = engine.search_frame(pc, pr, sr, None, fen=1)
    ox, oy, osad = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, None, lq, 1, 8, n_threads=8)
    bad = np.argwhere((mv[:, :, 0] != ox) | (mv[:, :, 1] != oy) | (sad != osad))
    assert len(bad) == 0, (name, lq, len(bad), bad[:8].tolist())
    return mv, sad


@pytest.mark.parametrize("lq", LAMBDAS)
@pytest.mark.parametrize("name", ["whole", "segments"])
def test_picture_search_as_whole_jobs_and_as_segments(engine, oracle_lib, name, lq):
    check_frame(engine, oracle_lib, name, lq)


@pytest.mark.parametrize("lq", [0, LQ])
@pytest.mark.parametrize("name", ["whole_flat", "whole_p4", "whole_p16", "segments_flat", "segments_p16", "segments_p64"])
def test_picture_search_on_ties(engine, oracle_lib, name, lq):
    mv, sad = check_frame(engine, oracle_lib, name, lq)
    if lq == 0:
        assert (sad == 0).all()


@pytest.mark.parametrize("name", ["whole_max", "segments_max"])
def test_picture_search_with_sums_at_their_maximum(engine, oracle_lib, name):
    mv, sad = check_frame(engine, oracle_lib, name, GATE2_LQ)
    assert (sad[:, 288] == 48960).all() and (sad[:, 352] == 48960).all()
