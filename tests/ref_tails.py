"""The reference's recorded answers for prediction blocks, prediction tails, the weighted-prediction estimator and the block distortions
(tests/golden/ref_blocks.npz, ref_tails.npz, ref_wp_estimate.npz, ref_dist.npz, written by tests/golden/gen_ref_tails_golden.py, whose
docstring describes the arrays), and what tests/test_ref_tails_cpu.py and tests/test_gpu_ref_tails.py share to read them.  Plain numpy; nothing
here computes a prediction, a weight or a distortion."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_WEIGHTS = 60
SPACING, FIRST = 16, 8        # golden blocks sit at luma (8 + 16 i, 8 + 16 j) of a 64x64 picture: 3 x 3 of them, sources apart
PER_PICTURE = 9


@functools.lru_cache(maxsize=None)
def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as g:
        return {k: g[k] for k in g.files}


def hmme_weight(triple, bd):
    """HM's syntax triple (iWeight, iOffset, log2WeightDenom) -> hmme_weight (w0, offset, shift, round) by the mapping include/hmme.h documents
    for hmme_wp_estimate, step 4: w0 = weight, offset = offset << (bd - 8), shift = d, round = d ? 1 << (d - 1) : 0"""
    w, o, d = (int(v) for v in triple)
    return (w, o * (1 << (bd - 8)), d, (1 << (d - 1)) if d else 0)


def bi_weights(entry, bd):
    """an entry of ref_tails.npz's bi_weights -> the two lists' hmme_weight, sharing the denominator"""
    w0, o0, w1, o1, d = (int(v) for v in entry)
    return hmme_weight((w0, o0, d), bd), hmme_weight((w1, o1, d), bd)


def cr_index(k):
    return (k + int(load("ref_tails")["cr_shift"])) % N_WEIGHTS


def geometry(kind):
    """-> (block size, rows / columns of source before the block, phases per axis) of a luma / chroma golden block"""
    return (8, 3, 4) if kind == "luma" else (4, 1, 8)


def source(kind, i, content):
    return load("ref_blocks")[kind + "_src"][i, content]


def block(kind, i, content, phase, bi):
    """the reference's block of source `content` of bit depth index i at `phase`: bi = 0 the clipped sample, 1 the Pel intermediate"""
    B = load("ref_blocks")
    if content < 3:
        return B[kind + "_out"][i, content, phase, bi]
    assert (content - 3) // 2 == phase          # a tap-sign picture is recorded at its own phase
    return B[kind + "_sign_out"][i, phase, (content - 3) & 1, bi]


def operand(kind, i, op):
    """operand `op` (0 largest, 1 smallest, 2, 3 random) of bit depth index i -> (content, phase, the Pel intermediate)"""
    content, phase = (int(v) for v in load("ref_tails")["ops_" + kind][i, op])
    return content, phase, block(kind, i, content, phase, 1)


def all_block_cases(kind):
    """every (content, phase) the blocks file records for a bit depth"""
    nph = geometry(kind)[2] ** 2
    return [(c, ph) for c in range(3) for ph in range(nph)] + [(3 + 2 * ph + k, ph) for ph in range(nph) for k in range(2)]


# ---- golden blocks inside a 64x64 luma (32x32 chroma) picture ------------------------------------------------------------------------------
def slot_xy(n):
    """luma position of golden block n (0..8) of a picture"""
    return FIRST + SPACING * (n % 3), FIRST + SPACING * (n // 3)


def picture(kind, sources, fill):
    """sources: up to 9 golden sources -> the [64, 64] luma or [32, 32] chroma picture that holds source n around block n, `fill` elsewhere"""
    size, before, _ = geometry(kind)
    side = 64 if kind == "luma" else 32
    pic = np.full((side, side), fill, np.int64)
    for n, s in enumerate(sources):
        x, y = (v * size // 8 for v in slot_xy(n))
        pic[y - before:y - before + s.shape[0], x - before:x - before + s.shape[1]] = s
    return pic


def cut(kind, image, n):
    """golden block n of a predicted picture"""
    size = geometry(kind)[0]
    x, y = (v * size // 8 for v in slot_xy(n))
    return np.asarray(image)[y:y + size, x:x + size].astype(np.int64)


def phase_mv(kind, phase):
    """the quarter-pel luma MV whose fraction is `phase` of the block kind (chroma: eighth chroma pels = quarter luma pels, 0..7)"""
    n = geometry(kind)[2]
    return phase % n, phase // n


def field(kind, phases):
    """int16 [1, 64, 2]: the motion field of the one-CTU picture with golden block n at phases[n]"""
    f = np.zeros((1, 64, 2), np.int16)
    for n, ph in enumerate(phases):
        x, y = slot_xy(n)
        f[0, (y // 8) * 8 + x // 8] = phase_mv(kind, ph)
    return f


def block_index(n):
    x, y = slot_xy(n)
    return (y // 8) * 8 + x // 8


# ---- the estimator's cases ---------------------------------------------------------------------------------------------------------------------
def wp_cases():
    """-> list of dicts(name, fmt, bd, n_l0, n_l1, start, pics, table, final, flags): pics = the current picture, then the references; a picture
    is a luma array (4:0:0) or a (y, cb, cr) triple (4:2:0)"""
    g = load("ref_wp_estimate")
    out = []
    for i in range(int(g["n"])):
        fmt, bd, n_l0, n_l1, start = (int(v) for v in g[f"c{i}_meta"])
        y = g[f"c{i}_y"].astype(np.int64)
        if fmt == 420:
            cb, cr = g[f"c{i}_cb"].astype(np.int64), g[f"c{i}_cr"].astype(np.int64)
            pics = [(y[p], cb[p], cr[p]) for p in range(len(y))]
        else:
            pics = [y[p] for p in range(len(y))]
        out.append(dict(name=str(g["names"][i]), fmt=fmt, bd=bd, n_l0=n_l0, n_l1=n_l1, start=start, pics=pics, table=g[f"c{i}_table"],
                        final=g[f"c{i}_final"], flags=g[f"c{i}_flags"]))
    return out


# ---- the distortion cases ----------------------------------------------------------------------------------------------------------------------
SSE, HADS, SAD = 0, 1, 2
DIST_CONTENTS = ("random", "binary", "spectral", "small")


def dist_cases():
    """-> list of (w, h, bd, content, org int16 [h, w], pred, (sse, hads, sad))"""
    g = load("ref_dist")
    out = []
    for s, (w, h) in enumerate(g["sizes"]):
        for i, bd in enumerate(g["bds"]):
            for c in range(4):
                out.append((int(w), int(h), int(bd), c, g[f"org_{w}x{h}"][i, c], g[f"pred_{w}x{h}"][i, c], tuple(int(v) for v in g["dist"][s, i, c])))
    return out
