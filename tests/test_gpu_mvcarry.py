"""GPU check of the full-task body that carries the MV costs in its sums (me_search_kernel<1, SPLIT, 2> with me_tree_pk4_fen1.inc, the
tree of tools/gen_me_tree.py Tree(1, pk=4); me_pksub as two asm subtracts in every 8-bit tree), bit-exact against the oracle's exhaustive
search for all 593 slots:
  * a 64 x 64 picture (one CTU) at search range 64: the full 129 x 129 window, 64 full lane-iterations and the 3 of the twin;
  * a 128 x 80 picture at search range 64: a partial bottom CTU row whose windows are clipped below (129 x 88), both bodies in every job;
each on noise, on a saturated pair (current 0, reference 255: every candidate's SAD ties, the sums sit at their maxima) and on an
exact-match pair (the winner's sums are 0: a carried cost is all a field holds), at lambda 57.9 and at the largest lambda of me_pk2_gate;
  * the per-CTU call with a predictor at the end of int16, far from the window, on the saturated pair at the gate's lambda: 16x12 and
    12x16 hold 48 960 + the MV cost, the carried 16x8 sums 32 640 + the MV cost, in every candidate.
A cost carried twice or not at all, a strip that kept its cost on the way to the 32x32 level, or a 16x12 slot summed from the wrong
rows would each show as wrong tables here."""
import numpy as np
import pytest

import test_gpu_pkmin2 as B

pytestmark = pytest.mark.gpu

LQ, GATE2_LQ, M = B.LQ, B.GATE2_LQ, B.M
PICTURES = {"one_ctu": (64, 64), "partial_row": (128, 80)}
SR = 64
_PAIR = {}


@pytest.fixture(scope="module")
def engine():
    from hmme import api
    e = api.Engine(0, 128)
    yield e
    e.close()


def pair(w, h, kind):
    from hmme import synth
    if (w, h, kind) not in _PAIR:
        rng = np.random.default_rng(7 + w + h)
        if kind == "saturated":
            cur, ref = np.zeros((h, w)), np.full((h, w), 255)
        elif kind == "exact":
            cur = ref = rng.integers(0, 256, size=(h, w))
        else:
            ref = rng.integers(0, 256, size=(h, w))
            cur = np.clip(np.roll(ref, (3, -5), axis=(0, 1)) + rng.integers(-5, 6, size=(h, w)), 0, 255)
        _PAIR[(w, h, kind)] = (synth.pad_plane(cur.astype(np.uint8)), synth.pad_plane(ref.astype(np.uint8)))
    return _PAIR[(w, h, kind)]


_ORACLE = {}


def oracle(oracle_lib, name, kind, lq):
    """the exhaustive search of one case, computed once"""
    from hmme import synth
    if (name, kind, lq) not in _ORACLE:
        w, h = PICTURES[name]
        cur, ref = pair(w, h, kind)
        _ORACLE[(name, kind, lq)] = oracle_lib.search_frame(cur, ref, (synth.MARGIN, synth.MARGIN), w, h, SR, None, lq, 1, 8, n_threads=8)
    return _ORACLE[(name, kind, lq)]


def test_the_cases_are_what_they_claim():
    from hmme import api
    import ctypes as C
    assert B.body(LQ, 1) == 2 and B.body(GATE2_LQ, 1) == 2 and B.body(GATE2_LQ + 1, 1) == 1
    L = api.load()
    L.hmme_test_pk_task_full.argtypes = [C.c_int] * 5
    L.hmme_test_pk_task_full.restype = C.c_int
    # the unclipped window: lane-iterations 0..63 of the 32-quad part are full in tasks of any size, the folded 65th and the 33rd quad are not
    assert all(L.hmme_test_pk_task_full(129, 129, 5, it, n) for it, n in ((0, 4), (60, 4), (63, 1)))
    assert not L.hmme_test_pk_task_full(129, 129, 5, 64, 1) and not L.hmme_test_pk_task_full(129, 129, 0, 0, 1)
    # the bottom CTU row of the 128 x 80 picture starts at 64: its windows are cut below (clipMv: 80 + 8 - 64 - 1 = 23 rows down), 88 rows,
    # no fold: all 44 lane-iterations of the 32-quad part are full, the 33rd quad's 88 run the twin
    assert L.hmme_test_pk_task_full(129, 88, 5, 40, 4) and not L.hmme_test_pk_task_full(129, 88, 0, 84, 4)


@pytest.mark.parametrize("lq", [LQ, GATE2_LQ])
@pytest.mark.parametrize("kind", ["noise", "saturated", "exact"])
@pytest.mark.parametrize("name", list(PICTURES))
def test_picture_search_equals_the_exhaustive_search(engine, oracle_lib, name, kind, lq):
    from hmme import synth
    w, h = PICTURES[name]
    cur, ref = pair(w, h, kind)
    m = synth.MARGIN
    engine.set_lambda_q16(lq)
    with engine.plane(w, h) as pc, engine.plane(w, h) as pr:
        pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
        mv, sad = engine.search_frame(pc, pr, SR, None, fen=1)
    ox, oy, osad = oracle(oracle_lib, name, kind, lq)
    bad = np.argwhere((mv[:, :, 0] != ox) | (mv[:, :, 1] != oy) | (sad != osad))
    assert len(bad) == 0, (name, kind, lq, len(bad), bad[:8].tolist())
    if kind == "saturated":
        assert (sad[:, 288] == 48960).all() and (sad[:, 448] == 32640).all() and (sad[:, 256] == 16320).all()
    if kind == "exact":
        assert (sad == 0).all() and (mv == 0).all()


@pytest.mark.parametrize("wx,wy", [(128, 8), (129, 9), (16, 17)])
def test_per_ctu_call_with_a_predictor_far_from_the_window(engine, oracle_lib, wx, wy):
    """the MV cost of every candidate is the largest the gate admits within a bit: the packed costs approach 65 535"""
    cur, ref = B.ctu_planes("max")
    mv, sad = B.check_ctu(engine, oracle_lib, cur, ref, wx, wy, (-32768, -32768), GATE2_LQ, 1)
    assert sad[288] == sad[352] == 48960 and sad[448] == sad[480] == 32640 and sad[256] == sad[320] == 16320
