"""CPU checks of the 8-bit reduction tree's use of key linearity (tools/gen_me_tree.py, class Tree): a slot is formed with one key
operation (K(a) - K(b) + C) wherever the keys of its parts exist -- the right 4x8 half of an 8x8 CU, the 12x16 slots of a 16x16
region --, and the two tall-family 32x8 strips of a 32x32 stay packed u16 sums until ONE key is made of each.  The op counts are
those of that scheme, the emission order (and with it the slot map) is what it was, and the numpy interpreter of the op list
reproduces the oracle bit for bit on contents that put every packed sum at its maximum, make every subtraction see equal keys,
spread a subtraction's two keys as far apart as they go, and on random pictures."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_me_tree as G  # noqa: E402
from test_tree_sim import model_search  # noqa: E402

# PKADD + 2 * PKSUB + 4 * (KEYS + LIN + SUB) of the generator before this scheme, without FEN: 448 + 2 * 64 + 4 * (416 + 181 + 20)
FEN0_WEIGHTED_BEFORE = 3044


def _counts(fen):
    c = {}
    for op in G.Tree(fen).build().ops:
        c[op[0]] = c.get(op[0], 0) + 1
    return c


def _weighted(c):
    return c["PKADD"] + 2 * c["PKSUB"] + 4 * (c["KEYS"] + c["LIN"] + c["SUB"])


def test_op_counts_with_fen():
    c = _counts(1)
    assert {k: c[k] for k in ("PKADD", "PKSUB", "KEYS", "LIN", "SUB")} == {"PKADD": 584, "PKSUB": 32, "KEYS": 312, "LIN": 173, "SUB": 116}
    assert _weighted(c) == 3052


def test_op_counts_without_fen_fall_too():
    assert _weighted(_counts(0)) < FEN0_WEIGHTED_BEFORE


@pytest.mark.parametrize("fen", [0, 1])
def test_every_difference_is_emitted_in_one_block_with_its_minimum(fen):
    """the emitter fuses SUB + MIN4 (ME_SUBMIN4); the op list that `simulate` interprets keeps both, and the generated source is current"""
    tree = G.Tree(fen).build()
    n_sub = sum(1 for op in tree.ops if op[0] == "SUB")
    fused = G.fuse_sub_min(tree.ops)
    assert sum(1 for op in fused if op[0] == "SUBMIN4") == n_sub and not any(op[0] == "SUB" for op in fused)
    assert len(fused) == len(tree.ops) - n_sub and sum(1 for op in fused if op[0] == "MIN4") == 593 - n_sub
    spaced = [op for op, _ in G.space_merges(fused, enable=True)]
    assert sorted(map(repr, spaced)) == sorted(map(repr, fused))          # spacing reorders, it neither drops nor invents an op
    text = open(os.path.join(G.OUT_DIR, "me_tree_fen%d.inc" % fen)).read()
    assert text.count("ME_SUBMIN4(") == n_sub and "ME_SUB(" not in text and text.count("ME_MIN4(") == 593 - n_sub


def _emission_order(fen):
    """slot ids in emission order, 8x8 CUs first, exactly as the tree's levels ask for them (written out here, not taken from the tree)"""
    order = []
    for qy in range(2):
        for qx in range(2):
            for ry in range(2):
                for rx in range(2):
                    for cy in range(2):
                        for cx in range(2):
                            x, y = qx * 4 + rx * 2 + cx, qy * 4 + ry * 2 + cy
                            order += [G.slot_2NxN(8, x, y, 0), G.slot_2NxN(8, x, y, 1), G.slot_Nx2N(8, x, y, 0), G.slot_Nx2N(8, x, y, 1),
                                      G.slot_2Nx2N(8, x, y)]
                    x, y = qx * 2 + rx, qy * 2 + ry
                    order += [G.slot_2NxN(16, x, y, 0), G.slot_2NxN(16, x, y, 1), G.slot_AMP(16, x, y, 0), G.slot_AMP(16, x, y, 1),
                              G.slot_Nx2N(16, x, y, 0), G.slot_Nx2N(16, x, y, 1), G.slot_2Nx2N(16, x, y)]
                    order += [G.slot_AMP(16, x, y, k) for k in range(2, 8)]
            order += [G.slot_2NxN(32, qx, qy, 0), G.slot_2NxN(32, qx, qy, 1), G.slot_Nx2N(32, qx, qy, 0), G.slot_Nx2N(32, qx, qy, 1),
                      G.slot_2Nx2N(32, qx, qy)]
            order += [G.slot_AMP(32, qx, qy, k) for k in range(8)]
    order += [G.slot_2NxN(64, 0, 0, 0), G.slot_2NxN(64, 0, 0, 1), G.slot_Nx2N(64, 0, 0, 0), G.slot_Nx2N(64, 0, 0, 1), G.slot_2Nx2N(64, 0, 0)]
    order += [G.slot_AMP(64, 0, 0, k) for k in range(8)]
    return order


@pytest.mark.parametrize("fen", [0, 1])
def test_emission_order_and_slot_map_are_unchanged(fen):
    tree = G.Tree(fen).build()
    want = _emission_order(fen)
    assert len(want) == 593
    assert tree.emitted == want + [None] * (G.N_GROUPS * 64 - 593)
    # the committed slot map is this order seen from the lanes: lane l of group g holds emission index (role bits of l)
    text = open(os.path.join(G.OUT_DIR, "me_slotmap.inc")).read()
    rows = [[int(v) for v in m.group(1).split(",")] for m in re.finditer(r"^\s*\{([-\d, ]+)\},\s*$", text, re.M)]
    committed = np.array(rows, np.int32)
    assert committed.shape == (G.N_GROUPS, 64)
    assert np.array_equal(committed, tree.slot_of_lane())
    emitted = {}
    for g in range(G.N_GROUPS):
        for lane in range(64):
            e = sum(((lane >> G.LEVEL_ROLE_BIT[lv]) & 1) << lv for lv in range(6))
            emitted[g * 64 + e] = None if committed[g, lane] < 0 else int(committed[g, lane])
    assert [emitted[i] for i in range(G.N_GROUPS * 64)] == tree.emitted


def test_the_16_bit_tree_has_the_op_list_it_had():
    """its sums are exact 32-bit values, not keys: none of the three rewrites applies, and its generated sources do not change"""
    for fen, adds in ((0, 256), (1, 448)):
        c = {}
        for op in G.Tree16(fen).build().ops:
            c[op[0]] = c.get(op[0], 0) + 1
        assert (c["ADDSHLN"], c["ADDN"], c["SUBN"], c["KEYMINN"]) == (adds, 373, 84, 593)


# ---- the interpreter against the oracle -------------------------------------------------------------------------------------------
LT, RB = (-6, -4), (5, 3)                      # a 12 x 8-candidate window: three quads per row -> a 2-quad and a 1-quad part
PRED = (7, -9)
PAD = 4
LAMBDAS = (0.0, 57.9, 4000.0)                  # 4000.0: the largest value tests/test_gpu_parity.py uses


def _contents():
    """name -> (cur uint8[64, 64], ref uint8[rows, cols]); the CTU's origin in ref is (PAD - LT[0], PAD - LT[1])"""
    wx, wy = RB[0] - LT[0] + 1, RB[1] - LT[1] + 1
    shape = (wy + 63 + 2 * PAD, wx + 63 + 2 * PAD)
    ox, oy = PAD - LT[0], PAD - LT[1]
    out = {}
    # every packed sum at its maximum: 16x16 = 65 280 (all rows), 32x8 = 65 280 without FEN / 32 640 (even rows, 32x4) with it
    out["max"] = (np.zeros((64, 64), np.uint8), np.full(shape, 255, np.uint8))
    # every SAD is 0 at every candidate: each subtraction sees two equal keys, every slot is an all-candidate tie
    out["equal"] = (np.full((64, 64), 77, np.uint8), np.full(shape, 77, np.uint8))
    # the pictures differ only inside ONE 4x8 block, the right half of an 8x8 CU (and of its 16x16 region's right 4x16 column):
    # K(8x8) - K(left half) and K(16x16) - K(4x16) have the largest whole over the smallest part
    cur = np.zeros((64, 64), np.uint8)
    cur[40:48, 44:48] = 255
    out["one_4x8"] = (cur, np.zeros(shape, np.uint8))
    rng = np.random.default_rng(20240607)
    ref = rng.integers(0, 256, size=shape).astype(np.uint8)
    cur = ref[oy + 2:oy + 66, ox - 3:ox + 61].astype(np.int16) + rng.integers(-6, 7, size=(64, 64))
    out["random"] = (np.clip(cur, 0, 255).astype(np.uint8), ref)
    return out


CONTENTS = _contents()
_oracle_cache = {}


def _oracle(oracle_lib, name, lam, fen):
    key = (name, lam, fen)
    if key not in _oracle_cache:
        cur, ref = CONTENTS[name]
        lq = oracle_lib.oracle().hmo_lambda_q16(lam)
        p = oracle_lib.make_params(LT, RB, PRED, lq, fen, 8)
        ox, oy, osad = oracle_lib.search_ctu(np.ascontiguousarray(cur, dtype=np.int16), (0, 0), np.ascontiguousarray(ref, dtype=np.int16),
                                             (PAD - LT[0], PAD - LT[1]), p)
        _oracle_cache[key] = (lq, np.stack([ox, oy, osad], axis=1).astype(np.int64))
    return _oracle_cache[key]


_trees = {}


def _tree(fen):
    if fen not in _trees:
        _trees[fen] = G.Tree(fen).build()
    return _trees[fen]


@pytest.mark.parametrize("fen", [0, 1])
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", sorted(CONTENTS))
def test_interpreted_tree_equals_the_oracle(oracle_lib, name, lam, fen):
    cur, ref = CONTENTS[name]
    lq, want = _oracle(oracle_lib, name, lam, fen)
    got = model_search(_tree(fen), cur, ref, (PAD - LT[0], PAD - LT[1]), LT, RB, PRED, lq)
    assert got.shape == (593, 3)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:16]


def test_the_contents_reach_the_extremes_they_are_meant_for(oracle_lib):
    """the 'max' content really puts 65 280 into the 16x16 and (without FEN) the 32x8 sums, and ties resolve in raster order"""
    table = oracle_lib.slot_table()
    _, want = _oracle(oracle_lib, "max", 0.0, 0)
    for s in (G.slot_2Nx2N(16, 1, 2), G.slot_AMP(32, 1, 0, 0)):
        assert int(table[s][2]) * int(table[s][3]) == 256 and want[s, 2] == 65280
    _, want = _oracle(oracle_lib, "max", 0.0, 1)
    assert want[G.slot_AMP(32, 0, 1, 1), 2] == 65280 and want[G.slot_AMP(32, 0, 1, 2), 2] == 2 * 32 * 12 * 255   # 32x8 all rows; 32x24 every 2nd row << 1
    for name in ("max", "equal"):
        for fen in (0, 1):
            _, want = _oracle(oracle_lib, name, 0.0, fen)
            assert (want[:, 0] == LT[0]).all() and (want[:, 1] == LT[1]).all()
