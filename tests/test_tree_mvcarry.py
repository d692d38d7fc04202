"""CPU check of the full-task twin that carries the MV costs in its sums (tools/gen_me_tree.py, Tree(1, pk=4) -> me_tree_pk4_fen1.inc:
the left 8x8 CUs of every 16x16 region add the packed MV costs to one leaf sum, every all-rows sum that contains it once is a packed
cost as it stands (PKMIN16M), the 16x8 strip a region hands to its 32x32 gives the costs back, and 16x12 is an 8-row half plus the four
rows next to it).  The generator's numpy interpreter runs that op list inside the task-loop model of tests/test_tree_pkswap.py, in the
place of Tree(1, pk=3), and must give the 32-bit tree's table for all 593 slots -- on noise, on a saturated pair (current 0, reference
255: every candidate's SAD ties) and on an exact-match pair, at lambda 57.9 and at the largest lambda of me_pk2_gate with a predictor at
the end of int16 (the MV cost then reaches PK2_COST_MAX and a packed cost 65 535).  The interpreter itself holds every packed field to
its 16 bits and counts how often a value contains the MV costs; the strips are held against sums taken straight from the window."""
import numpy as np
import pytest

import test_tree_pkswap as S

G, P2, T = S.G, S.P2, S.T
LQ, GATE2_LQ = S.LQ, P2.GATE2_LQ
LT, PRED = (32750, 32757), (-32768, -32768)      # test_tree_pkswap's geometry of the largest MV cost
WX, WY = 16, 17                                   # one four-quad part: lane-iteration 0 is a full task, the one-row rest runs the twin


def pair(kind):
    if kind == "saturated":
        return np.zeros((64, 64), np.uint8), np.full((160, 200), 255, np.uint8)
    ref = P2.noise(17, (160, 200))
    if kind == "exact":                               # the block at window (5, 3): its candidate costs its MV alone
        return ref[3:67, 5:69].copy(), ref
    cur = np.clip(ref[2:66, 7:71].astype(np.int64) + np.random.default_rng(5).integers(-6, 7, size=(64, 64)), 0, 255).astype(np.uint8)
    return cur, ref


@pytest.fixture
def carry_model(monkeypatch):
    """the model of test_tree_pkswap with Tree(1, 4) where it runs Tree(1, 3); every run of the carry tree is probed -> list of checks done"""
    seen = []
    real = G.simulate

    def simulate(tree, window, cur, lane_off, c, best, pk=None):
        if tree.pk != 4:
            return real(tree, window, cur, lane_off, c, best, pk=pk)
        probe = {}
        out = real(tree, window, cur, lane_off, c, best, pk=pk, probe=probe)
        flat = np.concatenate([window.reshape(-1), np.zeros(8, np.uint8)]).astype(np.int64)
        pitch = window.shape[1]
        assert len(tree.strips) == 16
        for name, x, y, w, h in tree.strips:
            assert probe["mvc"][name] == 0, "the strip handed to the 32x32 level carries an MV cost"
            idx = (lane_off[:, None, None, None] + np.arange(4)[None, :, None, None]
                   + (y + np.arange(h))[None, None, :, None] * pitch + (x + np.arange(w))[None, None, None, :])
            want = np.abs(flat[idx] - cur[y:y + h, x:x + w].astype(np.int64)[None, None]).sum(axis=(2, 3))
            assert np.array_equal(probe["val"][name].astype(np.int64), want), (name, x, y)
        packed = [v for n, v in probe["val"].items() if n[0] in "pq"]
        assert max(int(v.max()) for v in packed) <= 0xFFFF
        seen.append(max(int(probe["val"][o[2]].max()) for o in tree.ops if o[0] == "PKMIN16M"))
        return out

    monkeypatch.setattr(G, "simulate", simulate)
    monkeypatch.setattr(S, "tree", lambda pk: P2.tree(4 if pk == 3 else pk))
    return seen


@pytest.mark.parametrize("lq", [LQ, GATE2_LQ])
@pytest.mark.parametrize("kind", ["noise", "saturated", "exact"])
def test_carry_tree_gives_the_32_bit_tree_s_table(carry_model, kind, lq):
    cur, ref = pair(kind)
    rb = (LT[0] + WX - 1, LT[1] + WY - 1)
    out, ran = S.both(cur, ref, (-LT[0], -LT[1]), LT, rb, PRED, lq, (True, True), lambda iters: [(i, 1) for i in range(iters)])
    assert ran[True] == 1 and len(carry_model) == 1
    if kind == "saturated":
        assert (out[256, 2], out[448, 2], out[480, 2], out[288, 2], out[352, 2], out[320, 2]) == (16320, 32640, 32640, 48960, 48960, 16320)
        if lq == GATE2_LQ:      # 16x8 with the cost carried: 32 640 + the largest MV cost
            assert S.mv_cost(lq, LT[0], LT[1], PRED) == G.PK2_COST_MAX and carry_model[0] == 32640 + G.PK2_COST_MAX
    if kind == "exact":
        assert (out[:, 0] == LT[0] + 5).all() and (out[:, 1] == LT[1] + 3).all() and (out[:, 2] == 0).all()


def test_carry_tree_in_a_wide_part_with_an_ordinary_predictor(carry_model):
    """the 32-quad part (the benchmark's): two full lane-iterations in one task, the MV costs differ from quad to quad"""
    ref = P2.noise(3, (100, 264))
    cur = np.clip(ref[10:74, 40:104].astype(np.int64) + np.random.default_rng(3).integers(-6, 7, size=(64, 64)), 0, 255).astype(np.uint8)
    out, ran = S.both(cur, ref, (30, 8), (-6, -2), (-6 + 127, 1), (11, -3), LQ, (True, False))
    assert ran[True] == 2 and len(carry_model) == 2


def test_operation_count_and_slot_map():
    pk3, pk4 = P2.tree(3), P2.tree(4)
    n3, n4 = G.valu_count(pk3), G.valu_count(pk4)
    assert n3[0] - n4[0] >= 120 and (n3[0], n4[0]) == (3996, 3868)
    assert np.array_equal(pk3.slot_of_lane(), pk4.slot_of_lane()) and pk3.emitted == pk4.emitted
    # per 16x16 region: 2 MV-cost adds and one give-back where 10 sums paid an add each; 2 subtract pairs fewer
    c3, c4 = n3[1], n4[1]
    assert (c4["PKADDM"], c4["PKSUBM"], c4["PKMIN16M"], c4["PKMIN16"]) == (32, 16, 160, 512 - 160)
    assert (c3["PKSUB"], c4["PKSUB"]) == (64, 32) and c4["PKADD"] == c3["PKADD"] + 48
    # the same slots are packed, and only all-rows slots (never the doubled even-row sums) take a ready cost
    slots = lambda t, kinds: sorted(o[5] for o in t.ops if o[0] in kinds)
    assert slots(pk4, ("PKMIN16", "PKMIN16M")) == slots(pk3, ("PKMIN16",))
    assert all(o[4] == 0 and P2.slot_rect2(o[5])[4] == 1 for o in pk4.ops if o[0] == "PKMIN16M")
    # everything but the packed sums and their minima is the yardstick's, op for op
    rest = lambda t: [o[0] for o in t.ops if o[0] in ("KEYS", "LIN", "SUB", "MIN4", "MERGE", "PMERGE", "KEY16", "ACC", "QSAD")]
    assert rest(pk3) == rest(pk4)
