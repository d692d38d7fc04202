"""TComYuv::addAvg as tests/predict_bi_model.py restates it, without a GPU: against the oracle's uni-directional prediction where both
lists are the same, on flat planes, and on binary pictures where the clip acts at both ends."""
import ctypes as C

import numpy as np
import pytest

import bipred_wp_model as bwm
import predict_bi_model as pbm
import range_content as rc
from frame_helpers import bind_hmo


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return bind_hmo(oracle_lib)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_both_lists_equal_is_the_uni_directional_prediction(hmo, bd):
    """(2P + 2^(s-1) + 2 * 8192) >> s = (P + 2^(s-2) + 8192) >> (s-1): addAvg of P with itself is the rounding of bi = false"""
    from hmme import synth
    m, n = synth.MARGIN, 16
    _, ref, _ = synth.make_pair(96, 80, seed=40 + bd, bit_depth=bd, max_mv=2)
    p16 = C.POINTER(C.c_int16)
    rs = ref.shape[1]
    for qy in range(-5, -1):
        for qx in range(9, 13):                                                # all 16 phases, integer parts of both signs
            got = pbm.pred_bi(ref, ref, m + 24, m + 16, n, n, (qx, qy), (qx, qy), bd)
            want = np.zeros((n, n), np.int16)
            hmo.hmo_pred_block_qpel(C.cast(ref.ctypes.data + 2 * ((m + 16) * rs + m + 24), p16), rs, n, n, qx, qy, bd, want.ctypes.data_as(p16), n)
            assert np.array_equal(got, want), (bd, qx, qy)
    assert len({(qx & 3, qy & 3) for qy in range(-5, -1) for qx in range(9, 13)}) == 16


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_flat_planes_average_with_rounding(bd):
    maxv = (1 << bd) - 1
    for a, b in ((0, 0), (0, 1), (1, 2), (maxv, maxv), (maxv, 0), (maxv - 1, maxv), (37, 200)):
        p0, p1 = np.full((40, 40), a, np.int16), np.full((40, 40), b, np.int16)
        for mv0, mv1 in (((0, 0), (0, 0)), ((1, 2), (3, 3)), ((-6, 5), (2, -7))):
            assert (pbm.pred_bi(p0, p1, 12, 12, 8, 8, mv0, mv1, bd) == (a + b + 1) >> 1).all(), (bd, a, b, mv0, mv1)


@pytest.mark.parametrize("bd", [8, 10])
def test_the_clip_acts_at_both_ends_on_binary_pictures(bd):
    from hmme import synth
    w, h, m = 192, 72, synth.MARGIN
    maxv = (1 << bd) - 1
    _, ref0, ref1 = rc.extreme_triple(w, h, bd, seed=50 + bd)
    shift = max(2, 14 - bd) + 1
    lo = hi = inside = 0
    for k, (mv0, mv1) in enumerate((((2, 2), (2, 2)), ((1, 3), (3, 1)), ((-6, 5), (6, -5)), ((2, 0), (0, 2)))):
        x, y = m + 8 + 16 * k, m + 8
        raw = (bwm.inter_qpel(ref0, x, y, 32, 32, *mv0, bd) + bwm.inter_qpel(ref1, x, y, 32, 32, *mv1, bd) + (1 << (shift - 1)) + 2 * 8192) >> shift
        got = pbm.pred_bi(ref0, ref1, x, y, 32, 32, mv0, mv1, bd)
        assert np.array_equal(got, np.clip(raw, 0, maxv)) and got.min() >= 0 and got.max() <= maxv
        lo, hi, inside = lo + int((raw < 0).sum()), hi + int((raw > maxv).sum()), inside + int(((raw > 0) & (raw < maxv)).sum())
    assert lo > 0 and hi > 0 and inside > 0                                     # undershoot, overshoot and samples the clip leaves alone
