"""What a context keeps between launches must not show in any result (hm-opencl_amd/csrc/hmme.hip): the job-table tags (jobs_tag,
frac_jobs_tag) that let a launch without predictors keep the table of the launch before, best_clean of the merge table, every scratch
buffer that grows through ensure(), the event ring that orders streams, the once-per-context kernel opt-ins and the per-CTU call block.

One long-lived Engine(0, 128) runs a sequence of calls.  After every call its complete output is compared, np.array_equal, with what a
FRESH context -- freshly created planes with the same contents -- returns for that call alone; the fresh result is computed once per
distinct call (the label of a step names everything the call depends on).  So that both contexts cannot be wrong alike, every call family
is checked once on the USED context's output against the oracle or model its own test file uses, on the first CTU, the last CTU and up to
eight seeded ones.  No tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import frame_helpers as fh
import predict_bi_model as pbm
import predict_bi_w_model as pbw
import predict_chroma_model as pcm
import select_dirs_model as sdm
import select_model as sm
import select_refs_model as srm
import wp_estimate_model as wem

pytestmark = pytest.mark.gpu

LAMBDA = 57.9
GEOM = {"S": (320, 192), "T": (256, 128), "M": (640, 384), "L": (1216, 384), "P": (1088, 384)}   # all multiples of 64: 15, 8, 60, 114, 102 CTUs
SEED = {"S": 4100, "T": 4200, "M": 4300, "L": 4400, "P": 4500}
FADE, FADE2 = (40, 12, 6, 32), (-30, 180, 5, 16)          # (w0, offset at 8 bit, shift, round): a fade, and a negative weight
BI_W, BI_OW = (40, -12, 5, 16), (-20, 200, 5, 16)         # the searched list's and the other list's weight of the weighted bi calls
BAD_WEIGHT = (64, 0, 16, 0)                               # shift 16: outside 0..15, refused before anything is staged
# (current, reference) contents of pair i of a multi-pair launch: three pictures give eight different pairs
COMBOS = ((0, 1), (2, 1), (0, 2), (1, 2), (1, 0), (2, 0), (0, 0), (1, 1))


def at(wp, bd):
    return (wp[0], wp[1] << (bd - 8), wp[2], wp[3])


def n_ctu(g):
    return (GEOM[g][0] // 64) * (GEOM[g][1] // 64)


@functools.lru_cache(maxsize=None)
def pictures(w, h, bd, seed):
    """three padded int16 planes of one scene (frame_helpers.three_planes), drawn once and never modified"""
    t = fh.three_planes(w, h, bd, seed)
    for a in t:
        a.setflags(write=False)
    return t


def cid(g, bd, k, half=False):
    """the id of a plane's contents: picture k (0: current, 1: reference, 2: other) of geometry g; half: a 4:2:0 chroma plane of it"""
    w, h = GEOM[g]
    return (w // 2, h // 2, bd, SEED[g] + bd + 50 + 7 * k, 1) if half else (w, h, bd, SEED[g] + bd, k)


def content(c):
    return pictures(*c[:4])[c[4]]


def pl(g, bd, name, k, half=False):
    """(plane slot of a context, contents it must hold for the step): a slot whose contents change is re-uploaded, not re-created"""
    return (f"{g}{bd}.{name}", cid(g, bd, k, half))


def preds(g, seed, lead=()):
    from hmme import synth
    if seed is None:
        return None
    n = n_ctu(g)
    if not lead:
        return synth.random_predictors(n, seed=seed, max_pel=6)
    return np.ascontiguousarray(np.stack([synth.random_predictors(n, seed=seed + i, max_pel=6) for i in range(lead[0])]))


class Ctx:
    """a context and the planes it holds, by slot"""

    def __init__(self):
        from hmme import api
        self.eng = api.Engine(0, 128)
        self.eng.L.hmme_set_error_printing(self.eng.h, 0)   # the refused calls of the sequences would print
        self.held = {}

    def plane(self, slot, c):
        from hmme import synth
        w, h, bd = c[:3]
        if slot not in self.held:
            self.held[slot] = [self.eng.plane(w, h, bd), None]
        p, have = self.held[slot]
        assert (p.width, p.height, p.bit_depth) == (w, h, bd), slot
        if have != c:
            a, m = content(c), synth.MARGIN
            if bd == 8:
                p.upload_u8(a[m:m + h, m:m + w].astype(np.uint8))
            else:
                p.upload_pel(a, (m, m))
            self.held[slot][1] = c
        return p

    def close(self):
        for p, _ in self.held.values():
            p.close()
        self.eng.close()


class Step:
    """one call: label = everything it depends on (the key of the fresh results), planes = [(slot, contents)], run(engine, planes) ->
    tuple of arrays, info = what the spot checks need to restate it"""

    def __init__(self, label, planes, run, lam=LAMBDA, **info):
        self.label, self.planes, self.run, self.lam, self.info = label, planes, run, lam, info

    def execute(self, ctx):
        ctx.eng.set_lambda(self.lam)
        return tuple(self.run(ctx.eng, [ctx.plane(s, c) for s, c in self.planes]))


FRESH = {}   # label -> the fresh context's outputs (read-only), shared by the tests of this file


def fresh_result(step):
    if step.label not in FRESH:
        ctx = Ctx()
        try:
            out = step.execute(ctx)
        finally:
            ctx.close()
        for a in out:
            a.setflags(write=False)
        FRESH[step.label] = out
    return FRESH[step.label]


def run_sequence(used, steps, tag=""):
    """every step on the used context, its complete output against the fresh context's -> the used context's outputs, by step"""
    outs = []
    for i, st in enumerate(steps):
        got = st.execute(used)
        want = fresh_result(st)
        assert len(got) == len(want), (tag, i, st.label)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and a.dtype == b.dtype, (tag, i, st.label, k)
            assert np.array_equal(a, b), f"{tag} step {i} [{st.label}] output {k}: {int((a != b).sum())} of {a.size} entries differ from the fresh context's" \
                                         f" (the step before: [{steps[i - 1].label if i else '-'}])"
        outs.append(got)
    return outs


# ---- the calls -----------------------------------------------------------------------------------------------------------------------------
def plain(g, bd, sr, pred=None, first=0, count=-1, fen=1, lam=LAMBDA, refk=1):
    """search_frame; refk: which picture the REFERENCE plane holds (another one = the plane is re-uploaded)"""
    def run(eng, P):
        return eng.search_frame(P[0], P[1], sr, preds(g, pred), fen=fen, ctu_first=first, ctu_count=count)
    return Step(f"plain {g} {bd}b sr{sr} pred{pred} ctus{first}+{count} fen{fen} lam{lam} ref{refk}", [pl(g, bd, "cur", 0), pl(g, bd, "ref", refk)], run, lam,
                kind="plain", g=g, bd=bd, sr=sr, pred=pred, first=first, fen=fen, refk=refk)


def weighted(g, bd, sr, wp=FADE, pred=None, first=0, count=-1):
    def run(eng, P):
        return eng.search_frame_w(P[0], P[1], sr, at(wp, bd), preds(g, pred), ctu_first=first, ctu_count=count)
    return Step(f"weighted {g} {bd}b sr{sr} wp{wp} pred{pred} ctus{first}+{count}", [pl(g, bd, "cur", 0), pl(g, bd, "ref", 1)], run,
                kind="weighted", g=g, bd=bd, sr=sr, pred=pred, first=first, wp=at(wp, bd))


def field_of(g, per, seed=11):
    return fh.random_field(n_ctu(g), per, SEED[g] + seed)


def bi(g, bd, sr, center=None, pred=None, per=1, fen=1, wps=None):
    """search_frame_bi, or search_frame_bi_w with wps = (searched list's weight, other list's)"""
    def run(eng, P):
        if wps is None:
            return eng.search_frame_bi(P[0], P[1], P[2], sr, field_of(g, per), center_q=preds(g, center), pred_q=preds(g, pred), fen=fen)
        return eng.search_frame_bi_w(P[0], P[1], P[2], sr, at(wps[0], bd), at(wps[1], bd), field_of(g, per), center_q=preds(g, center), pred_q=preds(g, pred))
    return Step(f"bi {g} {bd}b sr{sr} centre{center} pred{pred} per{per} fen{fen} wps{wps}", [pl(g, bd, "cur", 0), pl(g, bd, "ref", 1), pl(g, bd, "other", 2)], run,
                kind="bi" if wps is None else "bi_w", g=g, bd=bd, sr=sr, center=center, pred=pred, per=per, fen=fen,
                wps=None if wps is None else (at(wps[0], bd), at(wps[1], bd)))


def pairs(g, bd, sr, n_pairs, pred=None, fen=1, form="pairs"):
    """search_pairs_device with n_pairs pairs of different pictures on the null stream; form "multi_device": search_frame_multi_device with
    n_pairs references (the same `pairs` count in the table's tag, the same stream); form "multi": the synchronous search_frame_multi"""
    planes = [pl(g, bd, f"p{k}", k) for k in range(3)]

    def run(eng, P):
        import torch
        from hmme import api
        n = n_ctu(g)
        pq = preds(g, pred, (n_pairs,))
        multi_refs = [P[1 + i % 2] for i in range(n_pairs)]       # one current picture against pictures 1 and 2
        if form == "multi":
            return eng.search_frame_multi(P[0], multi_refs, sr, pq, fen=fen)
        dev = torch.device("cuda", 0)
        d_pred = torch.from_numpy(pq).to(dev) if pq is not None else None
        d_mv, d_sad = fh.device_tables(n_pairs, n, dev)
        fp = api.FrameParams(sr, fen, bd, 0, n)
        refs = [P[COMBOS[i][1]] for i in range(n_pairs)]
        torch.cuda.synchronize()
        if form == "pairs":
            eng.search_pairs_device([P[COMBOS[i][0]] for i in range(n_pairs)], refs, fp, d_pred.data_ptr() if pq is not None else None, d_mv.data_ptr(), d_sad.data_ptr(), 0)
        else:
            eng.search_frame_multi_device(P[0], multi_refs, fp, d_pred.data_ptr() if pq is not None else None, d_mv.data_ptr(), d_sad.data_ptr(), 0)
        torch.cuda.synchronize()
        return d_mv.cpu().numpy(), d_sad.cpu().numpy().view(np.uint32)
    return Step(f"{form} {g} {bd}b sr{sr} x{n_pairs} pred{pred} fen{fen}", planes, run, kind="pairs", g=g, bd=bd, sr=sr, n_pairs=n_pairs, pred=pred, fen=fen, form=form)


def ctu_call(g, bd, sr, ctu, wp=None):
    """search_ctu on one CTU of the geometry's pictures, or search_refine_ctu_w with the weight wp: the per-CTU call block"""
    def run(eng, P):
        from hmme import api, synth
        m = synth.MARGIN
        w, h = GEOM[g]
        x, y = fh.ctu_origin(ctu, w)
        p = api.SearchParams(*api.set_search_range(0, 0, sr, x, y, w, h), 0, 0, 1, bd)
        cur, ref = content(cid(g, bd, 0)), content(cid(g, bd, 1))
        if wp is None:
            return eng.search_ctu(cur, (m + x, m + y), ref, (m + x, m + y), p)
        return eng.search_refine_ctu_w(cur, (m + x, m + y), ref, (m + x, m + y), p, at(wp, bd))
    return Step(f"ctu {g} {bd}b sr{sr} ctu{ctu} wp{wp}", [], run, kind="ctu")


def refused(g, bd, what):
    """a call the library refuses: a weight outside the accepted range, or a search range above the context's sr_max = 128"""
    def run(eng, P):
        from hmme import api
        with pytest.raises(api.HmmeError):
            if what == "weight":
                eng.search_frame_w(P[0], P[1], 16, BAD_WEIGHT)
            elif what == "refine_weight":
                eng.refine_frame_w(P[0], P[1], 16, BAD_WEIGHT, np.zeros((n_ctu(g), 593, 2), np.int16))
            else:
                eng.search_frame(P[0], P[1], 129)
        return ()
    return Step(f"refused {g} {bd}b {what}", [pl(g, bd, "cur", 0), pl(g, bd, "ref", 1)], run, kind="refused")


def refine(g, bd, sr, form, had=True, pred=None, center=None, per=1):
    """a search and the refinement of its winners with the same arguments -> (mv, sad, qmv, cost).  form: "plain", "w2" (two pairs with
    different weights in one refine_pairs_w_device call: two runs), "w" (search_frame_w and refine_frame_w with the weight FADE), "bi", "bi_w" """
    names = [pl(g, bd, "cur", 0), pl(g, bd, "ref", 1), pl(g, bd, "other", 2)]

    def run(eng, P):
        import torch
        from hmme import api
        n = n_ctu(g)
        pq, cq = preds(g, pred), preds(g, center)
        if form == "plain":
            mv, sad = eng.search_frame(P[0], P[1], sr, pq)
            return (mv, sad) + eng.refine_frame(P[0], P[1], sr, mv, pq, use_hadamard=had)
        if form == "w":
            mv, sad = eng.search_frame_w(P[0], P[1], sr, at(FADE, bd), pq)
            return (mv, sad) + eng.refine_frame_w(P[0], P[1], sr, at(FADE, bd), mv, pq, use_hadamard=had)
        if form == "bi":
            f = field_of(g, per)
            mv, sad = eng.search_frame_bi(P[0], P[1], P[2], sr, f, center_q=cq, pred_q=pq)
            return (mv, sad) + eng.refine_frame_bi(P[0], P[1], P[2], sr, f, mv, center_q=cq, pred_q=pq, use_hadamard=had)
        if form == "bi_w":
            f, w0, w1 = field_of(g, per), at(BI_W, bd), at(BI_OW, bd)
            mv, sad = eng.search_frame_bi_w(P[0], P[1], P[2], sr, w0, w1, f, center_q=cq, pred_q=pq)
            return (mv, sad) + eng.refine_frame_bi_w(P[0], P[1], P[2], sr, w0, w1, f, mv, center_q=cq, pred_q=pq, use_hadamard=had)
        assert form == "w2"
        dev = torch.device("cuda", 0)
        wps = [at(FADE, bd), at(FADE2, bd)]
        pq2 = preds(g, pred, (2,))
        d_pred = torch.from_numpy(pq2).to(dev) if pq2 is not None else None
        ptr = d_pred.data_ptr() if pq2 is not None else None
        fp = api.FrameParams(sr, 0, bd, 0, n)
        curs, refs = [P[0], P[2]], [P[1], P[1]]
        d_mv, d_sad = fh.device_tables(2, n, dev)
        d_q, d_c = fh.device_tables(2, n, dev)
        torch.cuda.synchronize()
        eng.search_pairs_w_device(curs, refs, fp, wps, ptr, d_mv.data_ptr(), d_sad.data_ptr(), 0)
        eng.refine_pairs_w_device(curs, refs, fp, wps, ptr, d_mv.data_ptr(), int(had), d_q.data_ptr(), d_c.data_ptr(), 0)
        torch.cuda.synchronize()
        return d_mv.cpu().numpy(), d_sad.cpu().numpy().view(np.uint32), d_q.cpu().numpy(), d_c.cpu().numpy().view(np.uint32)
    return Step(f"refine {form} {g} {bd}b sr{sr} had{had} pred{pred} centre{center} per{per}", names, run,
                kind="refine_" + form, g=g, bd=bd, sr=sr, had=int(had), pred=pred, center=center, per=per)


# ---- spot checks of the used context's output against the families' own references ---------------------------------------------------------
def spot_ctus(n, seed, first=0, count=-1):
    """first and last CTU of the range and up to eight seeded ones between -> picture CTU numbers"""
    count = n - first if count < 0 else count
    inner = np.arange(first + 1, first + count - 1)
    rng = np.random.default_rng(seed)
    pick = rng.choice(inner, size=min(8, len(inner)), replace=False) if len(inner) else []
    return sorted({first, first + count - 1, *[int(v) for v in pick]})


def lambda_q16(lam=LAMBDA):
    """what hmme_set_lambda stores for lam (asked of a context once)"""
    if lam not in lambda_q16.seen:
        ctx = Ctx()
        ctx.eng.set_lambda(lam)
        lambda_q16.seen[lam] = ctx.eng.lambda_q16
        ctx.close()
    return lambda_q16.seen[lam]


lambda_q16.seen = {}


def origin_of(hmo, i):
    """the bi-prediction origin 2 * cur - P of a bi step, P from the oracle (unweighted) or from bipred_wp_model (weighted)"""
    import bipred_wp_model as bwm
    g, bd = i["g"], i["bd"]
    w, h = GEOM[g]
    cur, other = content(cid(g, bd, 0)), content(cid(g, bd, 2))
    f = field_of(g, i["per"])
    if i.get("wps") is None:
        return fh.origin_picture(cur, fh.oracle_prediction(hmo, other, w, h, bd, f), w, h)
    return bwm.origin(cur, bwm.pred_picture(hmo, other, w, h, bd, f, i["wps"][1]), w, h)


def spot_search(oracle_lib, hmo, step, got, seed=1, stride=1):
    """(mv, sad) of a search step of the used context against the oracle leg of the family's own test file (stride: every stride-th of the
    spot CTUs and the last, where an oracle CTU is dear)"""
    from hmme import synth
    i, m = step.info, synth.MARGIN
    g, bd, sr = i["g"], i["bd"], i["sr"]
    w, h = GEOM[g]
    first = i.get("first", 0)
    ctus = spot_ctus(n_ctu(g), seed, first, got[0].shape[-3])
    ctus = sorted({*ctus[::stride], ctus[-1]})
    rows = [c - first for c in ctus]
    lq = lambda_q16(step.lam)
    pq = preds(g, i["pred"])
    cur, ref = content(cid(g, bd, 0)), content(cid(g, bd, i.get("refk", 1)))
    if i["kind"] == "plain":
        omv = np.zeros((len(ctus), 593, 2), np.int16)
        osad = np.zeros((len(ctus), 593), np.uint32)
        for k, c in enumerate(ctus):
            ox, oy, os_ = oracle_lib.search_frame(cur, ref, (m, m), w, h, sr, pq, lq, i["fen"], bd, ctu_first=c, ctu_count=1)
            omv[k, :, 0], omv[k, :, 1], osad[k] = ox[0], oy[0], os_[0]
    elif i["kind"] == "weighted":
        omv, osad = fh.oracle_search_w(oracle_lib, cur, ref, w, h, sr, pq, lq, bd, i["wp"], ctus)
    elif i["kind"] == "bi":
        omv, osad = fh.oracle_bi_search(oracle_lib, origin_of(hmo, i), ref, w, h, sr, preds(g, i["center"]), pq, lq, i["fen"], bd, ctus)
    else:
        assert i["kind"] == "bi_w"
        omv, osad = fh.oracle_origin_search_w(oracle_lib, origin_of(hmo, i), ref, w, h, sr, preds(g, i["center"]), pq, lq, bd, i["wps"][0], ctus)
    assert np.array_equal(got[0][rows], omv) and np.array_equal(got[1][rows], osad), f"[{step.label}] on the used context differs from the oracle"


def spot_refine(oracle_lib, hmo, step, got, seed=2):
    """(qmv, cost) of a refinement step against hmo_refine_frame (plain, bi) or hmo_frac_refine_w per slot (weighted forms)"""
    from hmme import synth
    i, m = step.info, synth.MARGIN
    g, bd, had = i["g"], i["bd"], i["had"]
    w, h = GEOM[g]
    ctus = spot_ctus(n_ctu(g), seed)
    lq = lambda_q16(step.lam)
    pq = preds(g, i["pred"])
    cur, ref, other = (content(cid(g, bd, k)) for k in range(3))
    mv, _, qmv, cost = got
    if i["kind"] in ("refine_plain", "refine_bi"):
        org = cur if i["kind"] == "refine_plain" else np.ascontiguousarray(np.pad(origin_of(hmo, i), m))
        for c in ctus:
            oq, oc = oracle_lib.refine_frame(org, ref, (m, m), w, h, mv[c:c + 1], pq, lq, had, bd, ctu_first=c, ctu_count=1)
            assert np.array_equal(qmv[c], oq[0]) and np.array_equal(cost[c], oc[0]), f"[{step.label}] CTU {c} on the used context differs from the oracle"
    elif i["kind"] == "refine_w":
        blocks = np.ascontiguousarray(cur[m:m + h, m:m + w])   # (the picture's CTU blocks at origin (0, 0): GEOM sizes are whole CTUs)
        oq, oc = fh.oracle_origin_refine_w(oracle_lib, blocks, ref, w, h, mv[ctus], pq, lq, had, bd, at(FADE, bd), ctus)
        assert np.array_equal(qmv[ctus], oq) and np.array_equal(cost[ctus], oc), f"[{step.label}] on the used context differs from the oracle"
    elif i["kind"] == "refine_bi_w":
        i = dict(i, wps=(at(BI_W, bd), at(BI_OW, bd)))
        oq, oc = fh.oracle_origin_refine_w(oracle_lib, origin_of(hmo, i), ref, w, h, mv[ctus], pq, lq, had, bd, i["wps"][0], ctus)
        assert np.array_equal(qmv[ctus], oq) and np.array_equal(cost[ctus], oc), f"[{step.label}] on the used context differs from the oracle"
    else:
        assert i["kind"] == "refine_w2"
        pq2 = preds(g, i["pred"], (2,))
        for pair, (org, wp) in enumerate(((cur, FADE), (other, FADE2))):
            blocks = np.ascontiguousarray(org[m:m + h, m:m + w])   # the picture's CTU blocks at origin (0, 0), as oracle_origin_refine_w takes an origin
            oq, oc = fh.oracle_origin_refine_w(oracle_lib, blocks, ref, w, h, mv[pair][ctus], None if pq2 is None else pq2[pair], lq, had, bd, at(wp, bd), ctus)
            assert np.array_equal(qmv[pair][ctus], oq) and np.array_equal(cost[pair][ctus], oc), f"[{step.label}] pair {pair} on the used context differs from the oracle"


@pytest.fixture(scope="module")
def hmo(oracle_lib):
    return fh.bind_hmo(oracle_lib)


@pytest.fixture()
def used():
    ctx = Ctx()
    yield ctx
    ctx.close()


def last_of(steps, outs, kind, **want):
    """the LAST step of a kind (and info) in a sequence with its output on the used context: the one with the most history behind it"""
    for st, got in reversed(list(zip(steps, outs))):
        if st.info.get("kind") == kind and all(st.info.get(k) == v for k, v in want.items()):
            return st, got
    raise AssertionError(f"the sequence holds no {kind} step {want}")


# ---- a: search tables ----------------------------------------------------------------------------------------------------------------------
def test_search_tables_after_any_other_search(used, oracle_lib, hmo):
    """jobs_tag and the buffers it names (prep_jobs).  Each transition below is framed by the unchanged call before and after it, so the
    keep-the-table path runs on both sides."""
    S = [
        # 1. plain 8 bit, then weighted 8 bit of the same size, range, CTU range and pair count: only the tag's 0x100 differs
        plain("S", 8, 16), plain("S", 8, 16), weighted("S", 8, 16), weighted("S", 8, 16), plain("S", 8, 16), weighted("S", 8, 16),
        # 2. weighted, then bi without centres or predictors: the same tag, the table is shared
        bi("S", 8, 16), bi("S", 8, 16), weighted("S", 8, 16), bi("S", 8, 16, wps=(BI_W, BI_OW)), weighted("S", 8, 16),
        # 3. the same bi call WITH window centres (must leave no reusable tag), then the calls without again, then the plain call
        bi("S", 8, 16), bi("S", 8, 16, center=31), bi("S", 8, 16), bi("S", 8, 16, center=31, pred=32, per=64), weighted("S", 8, 16), plain("S", 8, 16),
        # 4. 8 bit, then 10 bit at the same size and range (and the 10-bit weighted call, whose table IS the plain 10-bit one)
        plain("S", 10, 16), plain("S", 10, 16), weighted("S", 10, 16), plain("S", 10, 16), plain("S", 8, 16), weighted("S", 8, 16), plain("S", 10, 16),
        # 5. range 64 (15 jobs: all tail, segments), then 96 (tiles), on the same picture
        plain("S", 8, 64), plain("S", 8, 64), plain("S", 8, 96), plain("S", 8, 96), plain("S", 8, 64), weighted("S", 8, 96), plain("S", 8, 96),
        # 6. one pair, two pairs of the same picture size, search_frame_multi with two references (the same pairs count)
        pairs("S", 8, 16, 1), pairs("S", 8, 16, 1), pairs("S", 8, 16, 2), pairs("S", 8, 16, 2), pairs("S", 8, 16, 2, form="multi_device"),
        pairs("S", 8, 16, 2), pairs("S", 8, 16, 2, form="multi"), pairs("S", 8, 16, 2, form="multi"), pairs("S", 8, 16, 1), plain("S", 8, 16),
        # 7. whole picture, CTU sub-range, whole picture
        plain("S", 8, 16), plain("S", 8, 16, first=2, count=5), plain("S", 8, 16, first=2, count=5), plain("S", 8, 16),
        weighted("S", 8, 16), weighted("S", 8, 16, first=7, count=8), weighted("S", 8, 16),
        # 8. a launch with predictors between two without, in every table layout: whole jobs, 16-bit strips (weighted, 10 bit, bi), segments,
        #    tiles, two pairs
        plain("S", 8, 16), plain("S", 8, 16, pred=41), plain("S", 8, 16),
        weighted("S", 8, 16), weighted("S", 8, 16, pred=42), weighted("S", 8, 16),
        plain("S", 10, 16), plain("S", 10, 16, pred=43), plain("S", 10, 16),
        bi("S", 8, 16), bi("S", 8, 16, pred=44), bi("S", 8, 16),
        plain("S", 8, 64), plain("S", 8, 64, pred=45), plain("S", 8, 64),
        plain("S", 8, 96), plain("S", 8, 96, pred=46), plain("S", 8, 96),
        pairs("S", 8, 16, 2), pairs("S", 8, 16, 2, pred=47), pairs("S", 8, 16, 2),
        # 10. set_lambda changed between two otherwise equal launches (9, the four job counts, is the test below)
        plain("S", 8, 16), plain("S", 8, 16, lam=20.25), plain("S", 8, 16), weighted("S", 8, 64), weighted("S", 8, 64), plain("S", 8, 64, lam=20.25), plain("S", 8, 64),
        # 11. the reference plane re-uploaded with another picture between equal launches: the table stays, the results follow the picture
        plain("S", 8, 16), plain("S", 8, 16, refk=2), plain("S", 8, 16, refk=2), plain("S", 8, 16),
        # 12. a refused call between two equal launches: a weight outside the accepted range, a search range above sr_max
        weighted("S", 8, 16), refused("S", 8, "weight"), weighted("S", 8, 16), plain("S", 8, 16), refused("S", 8, "sr"), plain("S", 8, 16),
        plain("S", 8, 64), refused("S", 8, "sr"), plain("S", 8, 64),
        # 13. per-CTU calls (their own call block, merge-table preset and call_seq) between two equal picture launches
        plain("S", 8, 16), ctu_call("S", 8, 16, 7), plain("S", 8, 16), weighted("S", 8, 16), ctu_call("S", 8, 16, 8, wp=FADE), weighted("S", 8, 16),
        plain("S", 8, 64), ctu_call("S", 8, 64, 7), plain("S", 8, 64), ctu_call("S", 10, 16, 3), plain("S", 10, 16),
        # the other small picture and the other ranges, 8 and 10 bit: every call finds tables of the same and of another geometry behind it
        plain("T", 8, 8), weighted("T", 8, 8), plain("T", 10, 8), plain("T", 10, 8), weighted("T", 10, 8, pred=51), plain("T", 10, 8), plain("T", 10, 24), bi("T", 10, 24, pred=48), plain("T", 10, 24), plain("T", 8, 24), plain("T", 8, 8),
        plain("S", 8, 8), plain("T", 8, 8), bi("T", 8, 8, center=49), weighted("T", 8, 8), plain("S", 10, 24), weighted("S", 10, 24, pred=50), plain("S", 10, 24),
    ]
    outs = run_sequence(used, S, "a")
    # the results do follow lambda and the re-uploaded picture (the transitions are real ones)
    by = {st.label: o for st, o in zip(S, outs)}
    assert not np.array_equal(by[plain("S", 8, 16).label][1], by[plain("S", 8, 16, lam=20.25).label][1])
    assert not np.array_equal(by[plain("S", 8, 16).label][1], by[plain("S", 8, 16, refk=2).label][1])
    assert not np.array_equal(by[plain("S", 8, 16).label][0], by[plain("S", 8, 16, pred=41).label][0])
    for kind, want in (("plain", dict(sr=16, bd=8, pred=None, first=0)), ("plain", dict(sr=64, bd=8)), ("plain", dict(sr=96, pred=None)), ("plain", dict(bd=10, sr=16, pred=None)),
                       ("plain", dict(first=2)), ("weighted", dict(sr=16, bd=8, pred=None, first=0)), ("weighted", dict(bd=10)), ("bi", dict(center=None, pred=None)),
                       ("bi", dict(center=31, pred=32)), ("bi_w", {})):
        st, got = last_of(S, outs, kind, **want)
        spot_search(oracle_lib, hmo, st, got)


def tail_plan(g, n_pairs, sr=64):
    from hmme import api
    L = api.load()
    L.hmme_test_tail_plan.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)]
    out = (C.c_int * 4)()
    assert L.hmme_test_tail_plan(GEOM[g][0], GEOM[g][1], sr, n_pairs, 512, out) == 0
    return tuple(out)


def test_search_tables_at_the_four_launch_shapes(used, oracle_lib, hmo):
    """transition 9 of the list above: the 8-bit launch shapes at search range 64 on a 256-CU part (512 workgroup slots), from pairs of small
    pictures -- 342 jobs all tail, then 456, 570 (head, then the tail in a launch of its own: its table at tail_jobs_off), 912 (head and tail
    in one launch), 510 (whole), 570 again -- so kJobs, kFirstStrip and the merge table grow between uses and every layout follows every
    other.  (The cost model of plan_tail8 runs 456 jobs whole, like 510: 456 x 17 units on 512 segments are 16 lane-iterations against 17
    of whole jobs, not the 8 % it asks for.  The count stays in the sequence as a second whole-jobs table of another size; the all-tail shape
    comes from 342.)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"the launch shapes of this test are those of a 256-CU part (512 workgroup slots); this device has {cus} CUs")
    assert tail_plan("L", 3) == (342, 0, 512, 1)            # all tail: one segment table, no head
    assert tail_plan("L", 4) == (456, 456, 0, 0)            # whole (see above)
    assert tail_plan("L", 5) == (570, 512, 512, 0)          # head, then the tail: two launches
    assert tail_plan("L", 8)[:2] == (912, 512) and tail_plan("L", 8)[2] > 0 and tail_plan("L", 8)[3] == 1   # head and tail in one launch
    assert tail_plan("P", 5) == (510, 510, 0, 0)            # whole
    S = [pairs("L", 8, 64, 3), pairs("L", 8, 64, 3), pairs("L", 8, 64, 3, pred=60), pairs("L", 8, 64, 3),
         pairs("L", 8, 64, 4), pairs("L", 8, 64, 4), pairs("L", 8, 64, 4, pred=61), pairs("L", 8, 64, 4),
         pairs("L", 8, 64, 5), pairs("L", 8, 64, 5), pairs("L", 8, 64, 5, pred=62), pairs("L", 8, 64, 5),
         pairs("L", 8, 64, 8), pairs("L", 8, 64, 8), pairs("L", 8, 64, 8, pred=63), pairs("L", 8, 64, 8),
         pairs("P", 8, 64, 5), pairs("P", 8, 64, 5), pairs("P", 8, 64, 5, pred=64), pairs("P", 8, 64, 5),
         pairs("L", 8, 64, 5), pairs("L", 8, 64, 5, pred=62), pairs("L", 8, 64, 5), pairs("L", 8, 64, 3), pairs("L", 8, 64, 4), pairs("P", 8, 64, 5), pairs("L", 8, 64, 8),
         pairs("L", 8, 64, 3)]
    outs = run_sequence(used, S, "a9")
    # the first and the last pair of the last launch of each shape against the oracle.  An oracle CTU at range 64 costs 0.13 s of CPU, so
    # this spot check takes the first CTU, the last and every third of the eight seeded ones (4 or 5 CTUs per pair, 10 pairs), not all ten
    from hmme import synth
    m = synth.MARGIN
    for n_pairs, g in ((3, "L"), (4, "L"), (5, "L"), (8, "L"), (5, "P")):
        st, got = last_of(S, outs, "pairs", n_pairs=n_pairs, g=g, pred=None)
        w, h = GEOM[g]
        n = n_ctu(g)
        for pair in (0, n_pairs - 1):
            cur, ref = content(cid(g, 8, COMBOS[pair][0])), content(cid(g, 8, COMBOS[pair][1]))
            for c in spot_ctus(n, 3 + pair)[::3] + [n - 1]:
                ox, oy, os_ = oracle_lib.search_frame(cur, ref, (m, m), w, h, 64, None, lambda_q16(), 1, 8, ctu_first=c, ctu_count=1)
                assert np.array_equal(got[0][pair, c, :, 0], ox[0]) and np.array_equal(got[0][pair, c, :, 1], oy[0]) and np.array_equal(got[1][pair, c], os_[0]), \
                    f"[{st.label}] pair {pair} CTU {c} on the used context differs from the oracle"


# ---- b: merge table ------------------------------------------------------------------------------------------------------------------------
def test_merge_table_grows_between_two_launches_that_merge_through_it(used, oracle_lib, hmo):
    """kBest and best_clean (merge_table, finalize_best).  Each sequence makes the table grow between two launches that merge through it
    and ends with a launch smaller than the one before: stale keys of the larger launch would lie beyond what the last finalize reset."""
    S = [
        # all-tail 8 bit (15 jobs), 10-bit strips of a larger picture (60), all-tail 8 bit again
        plain("S", 8, 64), plain("M", 10, 16), plain("M", 10, 16), plain("S", 8, 64), plain("S", 8, 64),
        # tiles (8 jobs, four tiles each), then segments of more jobs than the table held when it was made ... and tiles again
        plain("T", 8, 96), plain("S", 8, 64), plain("T", 8, 96), plain("M", 8, 64), plain("T", 8, 96), plain("S", 8, 64),
        # beyond 64 jobs the table grows to twice what the launch needs: 60 -> 114 jobs of 10-bit strips (weighted: the u16 copies), then fewer
        weighted("M", 8, 16), weighted("L", 8, 16), weighted("M", 8, 16), plain("M", 10, 16), plain("T", 8, 96), plain("S", 10, 16),
    ]
    outs = run_sequence(used, S, "b")
    for kind, want in (("plain", dict(g="S", sr=64)), ("plain", dict(g="T", sr=96)), ("plain", dict(g="M", bd=10)), ("weighted", dict(g="M"))):
        st, got = last_of(S, outs, kind, **want)
        spot_search(oracle_lib, hmo, st, got, seed=5)


def test_merge_table_in_a_context_of_its_own_first_small_then_large():
    """the same growth seen from a context that has done nothing else: a table made for 8 jobs, grown for 15, 60 and 114, each followed
    by the small launch again (every context of this test is fresh: the used one per sequence, the reference per call)"""
    for seq in ((plain("T", 8, 96), plain("S", 8, 64), plain("T", 8, 96)),
                (plain("T", 8, 64), plain("M", 10, 16), plain("T", 8, 64)),
                (plain("S", 10, 16), weighted("L", 8, 16), plain("S", 10, 16), plain("S", 8, 64)),
                (plain("S", 8, 64), plain("M", 8, 64), plain("S", 8, 64), plain("S", 8, 96))):
        ctx = Ctx()
        try:
            run_sequence(ctx, list(seq), "b'")
        finally:
            ctx.close()


# ---- c: refinement -------------------------------------------------------------------------------------------------------------------------
def test_refinement_forms_in_alternation(used, oracle_lib, hmo):
    """frac_jobs_tag, the kWp0..kWp3 copies, the staging arena, the LDS opt-in and occupancy query of each me_frac_kernel build (launch_refine): plain, weighted
    (two pairs with different weights: two runs in one call), bi and bi-weighted refinement in alternation on one size, Hadamard and SAD,
    8 and 10 bit, with and without predictors and centres.  The six builds are (Hadamard | SAD) x (8-bit planes, 16-bit planes, weighted):
    each is first used after another one has taken its opt-in."""
    from hmme import api
    for bd in (8, 10):
        assert api.bipred_weight_check(bd, at(BI_W, bd), at(BI_OW, bd), 1) == 0 and api.weight_check(bd, at(FADE2, bd), 1) == 0
    S = [
        refine("S", 8, 16, "plain"), refine("S", 8, 16, "w2"), refine("S", 8, 16, "plain"),              # Hadamard: 8-bit, weighted, 8-bit
        refine("S", 8, 16, "bi"), refine("S", 8, 16, "plain", had=False), refine("S", 8, 16, "bi_w"),    # SAD 8-bit after Hadamard weighted
        refine("S", 10, 16, "plain"), refine("S", 8, 16, "w2", had=False), refine("S", 10, 16, "plain", had=False),   # 16-bit planes, SAD weighted, SAD 16-bit
        # without predictors: plain keeps its table's tag (kReuse), the weighted and bi forms write theirs; then the same with predictors between
        refine("S", 8, 16, "plain"), refine("S", 8, 16, "plain", pred=71), refine("S", 8, 16, "plain"),
        refine("S", 8, 16, "w2"), refine("S", 8, 16, "w2", pred=72), refine("S", 8, 16, "w2"),
        refine("S", 8, 16, "bi"), refine("S", 8, 16, "bi", pred=73), refine("S", 8, 16, "bi", center=74), refine("S", 8, 16, "bi", center=74, pred=73, per=64),
        refine("S", 8, 16, "bi"), refine("S", 8, 16, "plain"),
        refine("S", 8, 16, "bi_w", center=75, pred=76, had=False), refine("S", 8, 16, "bi_w"), refine("S", 8, 16, "w2"), refused("S", 8, "refine_weight"), refine("S", 8, 16, "w2"),
        # 10 bit: the planes serve as they are (no widened copies), the same alternation
        refine("S", 10, 16, "plain"), refine("S", 10, 16, "w2"), refine("S", 10, 16, "bi", center=77, pred=78), refine("S", 10, 16, "plain", pred=79),
        refine("S", 10, 16, "bi_w", had=False), refine("S", 10, 16, "w2", had=False, pred=80), refine("S", 10, 16, "bi", had=False), refine("S", 10, 16, "plain"),
        # 8 bit once more behind the 10-bit launches, and the other size and ranges
        refine("S", 8, 16, "plain"), refine("S", 8, 16, "bi"), refine("T", 8, 8, "w2"), refine("T", 10, 24, "bi_w", center=81), refine("T", 8, 8, "plain"), refine("S", 8, 16, "w2"),
    ]
    outs = run_sequence(used, S, "c")
    for kind, want in (("refine_plain", dict(bd=8, had=1, pred=None, g="S")), ("refine_plain", dict(bd=10, pred=79)), ("refine_plain", dict(had=0, bd=8)),
                       ("refine_w2", dict(bd=8, had=1, pred=None, g="S")), ("refine_w2", dict(bd=10, had=0)), ("refine_bi", dict(bd=8, center=74, pred=73)),
                       ("refine_bi", dict(bd=10, had=0)), ("refine_bi_w", dict(bd=8, had=0)), ("refine_bi_w", dict(bd=10, g="S"))):
        st, got = last_of(S, outs, kind, **want)
        spot_refine(oracle_lib, hmo, st, got)


# ---- d: host-facing staging ----------------------------------------------------------------------------------------------------------------
CHROMA_W = (((70, 9, 6, 32), (55, -14, 6, 32)), ((40, -5, 5, 16), (29, 11, 5, 16)))   # [component][list]: the lists of a component share the shift


@functools.lru_cache(maxsize=None)
def staging_inputs(g):
    """the tables and fields the staging calls of one picture size are fed (drawn once, read-only)"""
    n = n_ctu(g)
    rng = np.random.default_rng(SEED[g] + 9)
    d = dict(field1=fh.random_field(n, 1, SEED[g] + 21), field64=fh.random_field(n, 64, SEED[g] + 22),
             field2=np.ascontiguousarray(np.stack([fh.random_field(n, 64, SEED[g] + 23), fh.random_field(n, 64, SEED[g] + 24)])),
             refs64=rng.integers(0, 3, size=(n, 64)).astype(np.uint8),          # index 2 of two references: blocks that are not written
             dirs64=rng.choice(np.array([1, 2, 3, 3, 0xFF], np.uint8), size=(n, 64)),
             tables=sm.random_tables(n, seed=SEED[g] + 25), ref_tables=srm.random_ref_tables(2, n, seed=SEED[g] + 26), ref_pred=srm.ref_predictors(2, n, SEED[g] + 27),
             dir_pred=sdm.predictors(n, SEED[g] + 28))
    d["dir_tables"] = sdm.random_dir_tables(n, n, SEED[g] + 29, d["dir_pred"], 0, lambda_q16())
    for v in d.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return d


def staging_calls(g, bd=8):
    """the fourteen host-facing calls on one picture size, by name"""
    from hmme import api
    w, h = GEOM[g]
    luma = [pl(g, bd, "cur", 0), pl(g, bd, "ref", 1), pl(g, bd, "other", 2)]
    chroma = [pl(g, bd, f"c{k}{c}", 2 * k + c, half=True) for k in range(2) for c in range(2)]    # cb0, cr0, cb1, cr1
    d = lambda: staging_inputs(g)
    w0, w1 = at(FADE, bd), at(FADE2, bd)
    cw = [[at(wp, bd) for wp in comp] for comp in CHROMA_W]
    flat_w = lambda: [cw[c][k] for k in range(2) for c in range(2)]                              # engine order: cb0, cr0, cb1, cr1
    sel = lambda **kw: api.SelectParams(64, **kw)
    calls = {
        "predict_frame": (luma, lambda e, P: (e.predict_frame(P[1], d()["field64"]),)),
        "predict_frame_w": (luma, lambda e, P: (e.predict_frame_w(P[1], w0, d()["field1"]),)),
        "predict_refs_frame": (luma, lambda e, P: (e.predict_refs_frame([P[1], P[2]], d()["field64"], d()["refs64"]),)),
        "predict_refs_w_frame": (luma, lambda e, P: (e.predict_refs_w_frame([P[1], P[2]], [w0, w1], d()["field64"], d()["refs64"]),)),
        "predict_bi_frame": (luma, lambda e, P: (e.predict_bi_frame(P[1], P[2], d()["field2"], d()["dirs64"]),)),
        "predict_bi_w_frame": (luma, lambda e, P: (e.predict_bi_w_frame(P[1], P[2], at(BI_W, bd), at(BI_OW, bd), d()["field2"], d()["dirs64"]),)),
        "predict_chroma_frame": (chroma, lambda e, P: e.predict_chroma_frame(P[:2], w, h, d()["field64"])),
        "predict_chroma_refs_frame": (chroma, lambda e, P: e.predict_chroma_refs_frame(P, w, h, d()["field64"], d()["refs64"], weights=flat_w())),
        "predict_chroma_bi_frame": (chroma, lambda e, P: e.predict_chroma_bi_frame(P[:2], P[2:], w, h, d()["field2"], d()["dirs64"])),
        "select_frame": ([], lambda e, P: e.select_frame(w, h, sel(price_mv=1), *d()["tables"], pred_q=d()["ref_pred"][0])),
        "select_refs_frame": ([], lambda e, P: e.select_refs_frame(w, h, sel(), *d()["ref_tables"], ref_cost=[3, 11], pred_q=d()["ref_pred"])),
        "select_dirs_frame": ([], lambda e, P: e.select_dirs_frame(w, h, sel(), api.DirParams(*sdm.HM_BITS), *d()["dir_tables"], pred_q=d()["dir_pred"])),
        "wp_estimate": (luma, lambda e, P: _wp_estimate(e, P)),
        "plane_stats": (luma, lambda e, P: (np.array(e.plane_stats(P[2]), np.int64),)),
    }
    return {name: Step(f"{name} {g} {bd}b", planes, run, kind=name, g=g, bd=bd) for name, (planes, run) in calls.items()}


def _wp_estimate(e, P):
    weights, infos = e.wp_estimate(P[0], [P[1], P[2]])
    return np.array(weights, np.int64), np.array([[i.as_dict()[k] for k in wem.INFO_FIELDS] for i in infos], np.int64)


def spot_staging(oracle_lib, hmo, step, got):
    """one staging call's output on the used context against the model of its family, on the spot CTUs"""
    from hmme import api, synth
    name, g, bd = step.info["kind"], step.info["g"], step.info["bd"]
    w, h = GEOM[g]
    m, n, d = synth.MARGIN, n_ctu(g), staging_inputs(g)
    ctus = spot_ctus(n, 7)
    lq = lambda_q16()
    luma = [content(cid(g, bd, k)) for k in range(3)]
    chroma = [[content(cid(g, bd, 2 * k + c, half=True)) for c in range(2)] for k in range(2)]   # [picture][component]
    comps = [[chroma[k][c] for k in range(2)] for c in range(2)]                                 # model order: [component][picture]
    w0, w1 = at(FADE, bd), at(FADE2, bd)
    cw = [[at(wp, bd) for wp in comp] for comp in CHROMA_W]
    mv_cost = lambda q, x, y, px, py, scale: oracle_lib.oracle().hmo_mv_cost(q, x, y, px, py, scale)

    def area(img, half=False):
        """the samples of the spot CTUs"""
        s = 32 if half else 64
        return np.concatenate([img[(c // (w // 64)) * s:(c // (w // 64) + 1) * s, (c % (w // 64)) * s:(c % (w // 64) + 1) * s].ravel() for c in ctus]).astype(np.int64)

    def same_images(gots, wants, half=False):
        for a, b in zip(gots, wants):
            assert np.array_equal(area(a, half), area(b, half)), f"[{step.label}] on the used context differs from its model"

    fill = lambda half=False: np.zeros((h // 2, w // 2) if half else (h, w), np.int64)   # the wrappers hand the engine zeros: unwritten blocks stay 0
    if name == "predict_frame":
        same_images(got, [fh.oracle_prediction(hmo, luma[1], w, h, bd, d["field64"])])
    elif name == "predict_frame_w":
        same_images(got, [pbw.refs_picture(hmo, [luma[1]], w, h, bd, d["field1"], np.zeros((n, 1), np.uint8), [w0], fill(), ctus)])
    elif name == "predict_refs_frame":
        per_ref = [fh.oracle_prediction(hmo, a, w, h, bd, d["field64"]).astype(np.int64) for a in luma[1:]]
        idx = d["refs64"].reshape(h // 64, w // 64, 8, 8).transpose(0, 2, 1, 3).reshape(h // 8, w // 8).repeat(8, axis=0).repeat(8, axis=1)   # per sample
        same_images(got, [np.where(idx == 0, per_ref[0], np.where(idx == 1, per_ref[1], 0))])
    elif name == "predict_refs_w_frame":
        same_images(got, [pbw.refs_picture(hmo, luma[1:], w, h, bd, d["field64"], d["refs64"], [w0, w1], fill(), ctus)])
    elif name == "predict_bi_frame":
        same_images(got, [pbm.pred_picture(hmo, luma[1:], w, h, bd, d["field2"], d["dirs64"], fill(), ctus)])
    elif name == "predict_bi_w_frame":
        same_images(got, [pbw.pred_picture(hmo, luma[1:], w, h, bd, d["field2"], d["dirs64"], (at(BI_W, bd), at(BI_OW, bd)), fill(), ctus)])
    elif name == "predict_chroma_frame":
        same_images(got, pcm.pairs_picture(hmo, chroma[0], w, h, bd, d["field64"], (fill(True), fill(True)), None, ctus), True)
    elif name == "predict_chroma_refs_frame":
        same_images(got, pcm.refs_picture(hmo, comps, w, h, bd, d["field64"], d["refs64"], (fill(True), fill(True)), cw, ctus), True)
    elif name == "predict_chroma_bi_frame":
        same_images(got, pcm.bi_picture(hmo, comps, w, h, bd, d["field2"], d["dirs64"], (fill(True), fill(True)), None, ctus), True)
    elif name == "select_frame":
        mv, cost = d["tables"]
        for c in ctus:
            f, s, cc, _ = sm.select_picture(mv[c:c + 1], cost[c:c + 1], api.SelectParams(64, price_mv=1), w, h, c, d["ref_pred"][0], lq, mv_cost)
            assert np.array_equal(got[0][c], f[0]) and np.array_equal(got[1][c], s[0]) and got[2][c] == cc[0], f"[{step.label}] CTU {c} differs from select_model"
    elif name == "select_refs_frame":
        mv, cost = d["ref_tables"]
        for c in ctus:
            f, r, s, cc, _ = srm.select_refs_picture(mv[:, c:c + 1], cost[:, c:c + 1], api.SelectParams(64), w, h, [3, 11], c, d["ref_pred"], lq, mv_cost)
            assert np.array_equal(got[0][c], f[0]) and np.array_equal(got[1][c], r[0]) and np.array_equal(got[2][c], s[0]) and got[3][c] == cc[0], \
                f"[{step.label}] CTU {c} differs from select_refs_model"
    elif name == "select_dirs_frame":
        t = d["dir_tables"]
        for c in ctus:
            f, dr, s, cc = sdm.select_dirs_picture(*[a[:, c:c + 1] for a in t[:4]], t[4], api.SelectParams(64), w, h, sdm.HM_BITS, c, d["dir_pred"], lq)
            assert np.array_equal(got[0][:, c], f[:, 0]) and np.array_equal(got[1][c], dr[0]) and np.array_equal(got[2][c], s[0]) and got[3][c] == cc[0], \
                f"[{step.label}] CTU {c} differs from select_dirs_model"
    elif name == "wp_estimate":
        pics = [a[m:m + h, m:m + w].astype(np.int64) for a in luma]
        want = wem.estimate(pics[0], pics[1:], bd)
        assert [tuple(int(v) for v in r) for r in got[0]] == [tuple(x["wp"]) for x in want], f"[{step.label}] weights differ from wp_estimate_model"
        assert [[int(v) for v in r] for r in got[1]] == [[int(x[k]) for k in wem.INFO_FIELDS] for x in want], f"[{step.label}] statistics differ from wp_estimate_model"
    else:
        assert name == "plane_stats"
        assert tuple(int(v) for v in got[0]) == tuple(int(v) for v in wem.plane_stats(luma[2][m:m + h, m:m + w].astype(np.int64))), f"[{step.label}] differs from the model"


def search_calls(g, bd=8, sr=8):
    """the synchronous search and refinement forms on one picture size (the steps of sections a and c): search_frame, search_frame_multi with
    two references, refine_frame, search_frame_w / refine_frame_w, search_frame_bi / refine_frame_bi and their _w forms, with and without
    predictors and centres, one and 64 MVs per CTU in the other list's field -- items of the arena that are there in one call and not in the next"""
    return [plain(g, bd, sr, pred=91), pairs(g, bd, sr, 2, pred=92, form="multi"), refine(g, bd, sr, "plain", pred=93), weighted(g, bd, sr),
            refine(g, bd, sr, "w", pred=94), bi(g, bd, sr, center=95, pred=96, per=64), bi(g, bd, sr, wps=(BI_W, BI_OW)),
            refine(g, bd, sr, "bi", center=97), refine(g, bd, sr, "bi_w", pred=98, per=64)]


def spot_multi(oracle_lib, step, got):
    """search_frame_multi of the used context (one current picture against pictures 1 and 2) against the oracle, per reference"""
    from hmme import synth
    i, m = step.info, synth.MARGIN
    g, bd = i["g"], i["bd"]
    w, h = GEOM[g]
    pq = preds(g, i["pred"], (i["n_pairs"],))
    for r in range(i["n_pairs"]):
        cur, ref = content(cid(g, bd, 0)), content(cid(g, bd, 1 + r % 2))
        for c in spot_ctus(n_ctu(g), 11 + r):
            ox, oy, os_ = oracle_lib.search_frame(cur, ref, (m, m), w, h, i["sr"], None if pq is None else pq[r], lambda_q16(step.lam), i["fen"], bd, ctu_first=c, ctu_count=1)
            assert np.array_equal(got[0][r, c, :, 0], ox[0]) and np.array_equal(got[0][r, c, :, 1], oy[0]) and np.array_equal(got[1][r, c], os_[0]), \
                f"[{step.label}] reference {r} CTU {c} on the used context differs from the oracle"


@pytest.mark.parametrize("seed", [20261, 77003])
def test_host_staging_calls_in_shuffled_order(used, oracle_lib, hmo, seed):
    """The staging arena (kStage) behind every synchronous, host-array form, and kWpEst: the fourteen prediction, selection and estimation
    calls and the nine search and refinement forms, all of them on a small picture, then on a larger one (the arena grows in the middle of
    the sequence), then on the small one again, each pass in a seeded order.  One arena serves them all, so a search's tables land where a
    selection's outputs were and a short field where a long one was."""
    rng = np.random.default_rng(seed)
    S = []
    for g in ("T", "S", "T"):
        calls = list(staging_calls(g).values()) + search_calls(g)
        S += [calls[k] for k in rng.permutation(len(calls))]
    outs = run_sequence(used, S, f"d (shuffle seed {seed})")
    seen = set()
    for st, got in reversed(list(zip(S, outs))):   # each family once, where it has the most history behind it: the last pass
        kind = st.info["kind"]
        if kind in seen:
            continue
        seen.add(kind)
        if kind in ("plain", "weighted", "bi", "bi_w"):
            spot_search(oracle_lib, hmo, st, got)
        elif kind == "pairs":
            spot_multi(oracle_lib, st, got)
        elif kind.startswith("refine_"):
            spot_refine(oracle_lib, hmo, st, got)
        else:
            spot_staging(oracle_lib, hmo, st, got)
    assert len(seen) == 14 + 9


ODD_W, ODD_H, ODD_FIRST, ODD_COUNT, ODD_SPARE = 200, 72, 1, 3, 3      # 4 x 2 CTUs, partial on both edges; 100 x 36 chroma


@pytest.mark.parametrize("bd", [8, 10])
def test_host_staging_at_a_size_where_no_item_is_a_multiple_of_the_alignment(bd):
    """The arena's items at sizes that are no multiple of its alignment: a 200 x 72 picture (8 CTUs, 100 x 36 chroma), the CTU range
    [1, 4), images whose stride is the width + 3 samples.  predict_frame, predict_chroma_frame, predict_bi_frame, select_frame and
    select_dirs_frame run through the C entries on one context, in an order in which every call follows one of another family, the
    selections with all optional outputs and with each one left out; every output array and image is pre-filled with a sentinel.  Each
    call's outputs equal a fresh context's, every sentinel outside the CTU range and in the stride padding is untouched, and something
    inside the range is written."""
    from hmme import api
    w, h, first, cnt, spare = ODD_W, ODD_H, ODD_FIRST, ODD_COUNT, ODD_SPARE
    n, ctus_x = sdm.n_ctus(w, h), (w + 63) // 64
    assert n == 8
    rng = np.random.default_rng(9100 + bd)
    dt, sentinel = (np.uint8, 0xA5) if bd == 8 else (np.uint16, 0xA5A5)
    pics = [rng.integers(0, 1 << bd, size=(h, w)).astype(np.int16) for _ in range(2)] + [rng.integers(0, 1 << bd, size=(h // 2, w // 2)).astype(np.int16) for _ in range(2)]
    field64, field1 = fh.random_field(n, 64, 9101), fh.random_field(n, 1, 9102)
    field2 = np.ascontiguousarray(np.stack([fh.random_field(n, 64, 9103), fh.random_field(n, 64, 9104)]))
    dirs64 = rng.choice(np.array([1, 2, 3, 3, 0xFF], np.uint8), size=(n, 64))
    t_mv, t_cost = (np.ascontiguousarray(a) for a in sm.random_tables(cnt, seed=9105))
    pred = np.ascontiguousarray(sdm.predictors(n, 9106))
    dir_tabs = [np.ascontiguousarray(a) for a in sdm.random_dir_tables(n, cnt, 9107, pred, first, lambda_q16())]
    fp, sel, dp = api.FrameParams(1, 0, bd, first, cnt), api.SelectParams(64), api.DirParams(*sdm.HM_BITS)
    fp_sel = api.FrameParams(1, 0, 8, first, cnt)
    ptr = lambda a: None if a is None else a.ctypes.data

    def inside(half):
        """the samples of the CTU range in an image of the picture (half: of a chroma plane)"""
        s = 32 if half else 64
        m = np.zeros((h // 2, w // 2) if half else (h, w), bool)
        for c in range(first, first + cnt):
            m[(c // ctus_x) * s:(c // ctus_x + 1) * s, (c % ctus_x) * s:(c % ctus_x + 1) * s] = True
        return m

    def image(half=False):
        return np.full((h // 2, w // 2 + spare) if half else (h, w + spare), sentinel, dt)

    def check_image(img, half=False):
        wi, m = img.shape[1] - spare, inside(half)
        assert (img[:, wi:] == sentinel).all() and (img[:, :wi][~m] == sentinel).all() and (img[:, :wi][m] != sentinel).any()

    def check_rows(a, fill, axis=0):
        """a select output: the entries of the CTUs outside the range keep the sentinel, those inside do not all"""
        a = np.moveaxis(a, axis, 0)
        out = np.ones(n, bool)
        out[first:first + cnt] = False
        assert (a[out] == fill).all() and (a[~out] != fill).any()

    def predict(e, P):
        img = image()
        assert e.L.hmme_predict_frame(e.h, P[0].h, C.byref(fp), ptr(field64), 64, ptr(img), w + spare) == 0
        check_image(img)
        return (img,)

    def predict1(e, P):
        img = image()
        assert e.L.hmme_predict_frame(e.h, P[1].h, C.byref(fp), ptr(field1), 1, ptr(img), w + spare) == 0
        check_image(img)
        return (img,)

    def predict_chroma(e, P):
        cb, cr = image(True), image(True)
        planes, outs = (C.c_void_p * 2)(P[2].h, P[3].h), (C.c_void_p * 2)(ptr(cb), ptr(cr))
        assert e.L.hmme_predict_chroma_frame(e.h, planes, w, h, C.byref(fp), None, ptr(field64), 64, outs, w // 2 + spare) == 0
        check_image(cb, True)
        check_image(cr, True)
        return cb, cr

    def predict_bi(e, P):
        img = image()
        assert e.L.hmme_predict_bi_frame(e.h, P[0].h, P[1].h, C.byref(fp), ptr(field2), ptr(dirs64), 64, ptr(img), w + spare) == 0
        check_image(img)
        return (img,)

    def select(slot, cost, with_pred):
        def run(e, P):
            f = np.full((n, 64, 2), 0x1111, np.int16)
            s = np.full((n, 64), 0x3333, np.uint16) if slot else None
            c = np.full(n, 0x44444444, np.uint32) if cost else None
            assert e.L.hmme_select_frame(e.h, w, h, C.byref(fp_sel), C.byref(sel), ptr(t_mv), ptr(t_cost), ptr(pred[0]) if with_pred else None, ptr(f), ptr(s), ptr(c)) == 0
            for a, fill in ((f, 0x1111), (s, 0x3333), (c, 0x44444444)):
                if a is not None:
                    check_rows(a, fill)
            return tuple(a for a in (f, s, c) if a is not None)
        return run

    def select_dirs(slot, cost, with_pred):
        def run(e, P):
            f, d = np.full((2, n, 64, 2), 0x1111, np.int16), np.full((n, 64), 0x22, np.uint8)
            s = np.full((n, 64), 0x3333, np.uint16) if slot else None
            c = np.full(n, 0x44444444, np.uint32) if cost else None
            assert e.L.hmme_select_dirs_frame(e.h, w, h, C.byref(fp_sel), C.byref(sel), C.byref(dp), *[ptr(a) for a in dir_tabs], ptr(pred) if with_pred else None,
                                              ptr(f), ptr(d), ptr(s), ptr(c)) == 0
            check_rows(f, 0x1111, axis=1)
            for a, fill in ((d, 0x22), (s, 0x3333), (c, 0x44444444)):
                if a is not None:
                    check_rows(a, fill)
            return tuple(a for a in (f, d, s, c) if a is not None)
        return run

    calls = [("predict_frame", predict), ("select all", select(True, True, True)), ("predict_chroma_frame", predict_chroma), ("select no slot", select(False, True, True)),
             ("predict_bi_frame", predict_bi), ("select_dirs all", select_dirs(True, True, True)), ("select no cost", select(True, False, False)),
             ("predict_frame per 1", predict1), ("select_dirs no slot", select_dirs(False, True, False)), ("predict_chroma_frame", predict_chroma),
             ("select_dirs no cost", select_dirs(True, False, True)), ("select fields only", select(False, False, True)), ("predict_bi_frame", predict_bi),
             ("select_dirs fields only", select_dirs(False, False, True)), ("predict_frame", predict), ("select all", select(True, True, True))]

    def context():
        ctx = Ctx()
        ctx.eng.set_lambda(LAMBDA)
        planes = []
        for a in pics:
            p = ctx.eng.plane(a.shape[1], a.shape[0], bd)
            p.upload_u8(a.astype(np.uint8)) if bd == 8 else p.upload_pel(a, (0, 0))
            planes.append(p)
        return ctx, planes

    def close(ctx, planes):
        for p in planes:
            p.close()
        ctx.close()

    fresh = {}
    for name, run in calls:
        if name not in fresh:
            ctx, planes = context()
            try:
                fresh[name] = run(ctx.eng, planes)
            finally:
                close(ctx, planes)
    ctx, planes = context()
    try:
        for k, (name, run) in enumerate(calls):
            got = run(ctx.eng, planes)
            assert len(got) == len(fresh[name])
            for j, (a, b) in enumerate(zip(got, fresh[name])):
                assert np.array_equal(a, b), f"call {k} [{name}] output {j} differs from the fresh context's (the call before: [{calls[k - 1][0] if k else '-'}])"
    finally:
        close(ctx, planes)


# ---- d': B pictures with several references per list, and the 4:2:0 estimate --------------------------------------------------------------
def more(g, bd, name, k):
    """a plane slot with a picture of a second scene of the geometry: the other list of the bi-refs calls"""
    w, h = GEOM[g]
    return (f"{g}{bd}.{name}", (w, h, bd, SEED[g] + bd + 500, k))


def ref_field_of(g, per):
    """reference indices 0 / 1 that change from block to block (one MV per CTU: from CTU to CTU)"""
    b, c = np.arange(per), np.arange(n_ctu(g))[:, None]
    return (((b % 8) + (b // 8) + c) % 2).astype(np.uint8)


def bi_refs(g, bd, sr, had=True, center=None, pred=None, per=64, refk=1, swap=False):
    """search_frame_bi_refs and refine_frame_bi_refs of its winners: the references are the slots "ref" and "other" of the older calls (refk:
    the picture the first one holds), the other list two slots of its own (swap: their pictures exchanged) -> (mv, sad, qmv, cost)"""
    names = [pl(g, bd, "cur", 0), pl(g, bd, "ref", refk), pl(g, bd, "other", 2), more(g, bd, "o0", int(swap)), more(g, bd, "o1", 1 - int(swap))]

    def run(eng, P):
        f, rf = field_of(g, per, 13), ref_field_of(g, per)
        pq, cq = preds(g, pred, (2,)), preds(g, center, (2,))
        mv, sad = eng.search_frame_bi_refs(P[0], P[1:3], P[3:], sr, f, rf, center_q=cq, pred_q=pq, fen=1)
        return (mv, sad) + eng.refine_frame_bi_refs(P[0], P[1:3], P[3:], sr, f, rf, mv, center_q=cq, pred_q=pq, use_hadamard=had)
    return Step(f"bi_refs {g} {bd}b sr{sr} had{had} centre{center} pred{pred} per{per} ref{refk} swap{swap}", names, run,
                kind="bi_refs", g=g, bd=bd, sr=sr, had=int(had), center=center, pred=pred, per=per, refk=refk, swap=swap)


def spot_bi_refs(oracle_lib, hmo, step, got, seed=3):
    """the four tables of a bi_refs step against the oracle on the origin built here (tests/bipred_refs_bands.refs_prediction)"""
    from bipred_refs_bands import refs_prediction
    from hmme import synth
    i, m = step.info, synth.MARGIN
    g, bd, sr = i["g"], i["bd"], i["sr"]
    w, h = GEOM[g]
    ctus = spot_ctus(n_ctu(g), seed)
    lq = lambda_q16(step.lam)
    cur, refs = content(cid(g, bd, 0)), [content(cid(g, bd, i["refk"])), content(cid(g, bd, 2))]
    others = [content(more(g, bd, "o", k)[1]) for k in ((1, 0) if i["swap"] else (0, 1))]
    org = fh.origin_picture(cur, refs_prediction(hmo, others, w, h, bd, field_of(g, i["per"], 13), ref_field_of(g, i["per"])), w, h)
    pq, cq = preds(g, i["pred"], (2,)), preds(g, i["center"], (2,))
    mv, sad, qmv, cost = got
    for r in range(2):
        omv, osad = fh.oracle_bi_search(oracle_lib, org, refs[r], w, h, sr, None if cq is None else cq[r], None if pq is None else pq[r], lq, 1, bd, ctus)
        assert np.array_equal(mv[r][ctus], omv) and np.array_equal(sad[r][ctus], osad), f"[{step.label}] reference {r} on the used context differs from the oracle"
        for c in ctus:
            oq, oc = oracle_lib.refine_frame(np.ascontiguousarray(np.pad(org, m)), refs[r], (m, m), w, h, mv[r][c:c + 1], None if pq is None else pq[r], lq, i["had"], bd,
                                             ctu_first=c, ctu_count=1)
            assert np.array_equal(qmv[r][c], oq[0]) and np.array_equal(cost[r][c], oc[0]), f"[{step.label}] reference {r} CTU {c} on the used context differs from the oracle"


def planes_420(g, bd, cb=2):
    """the nine planes of a 4:2:0 estimate with two references: the luma slots of the older calls and chroma slots c<picture><component>;
    cb: the picture reference 0's Cb slot holds (another one = the plane is re-uploaded)"""
    chroma = lambda k, c, j: pl(g, bd, f"c{k}{c}", j, half=True)
    return [pl(g, bd, "cur", 0), chroma(0, 0, 0), chroma(0, 1, 1), pl(g, bd, "ref", 1), chroma(1, 0, cb), chroma(1, 1, 3), pl(g, bd, "other", 2), chroma(2, 0, 4), chroma(2, 1, 5)]


def wp420(g, bd, cb=2):
    def run(eng, P):
        wl, wc, infos = eng.wp_estimate_420(P[:3], [P[3:6], P[6:9]])
        return np.array(wl, np.int64), np.array(wc, np.int64), np.array([[i.as_dict()[k] for k in wem.INFO_FIELDS] for i in infos], np.int64)
    return Step(f"wp_estimate_420 {g} {bd}b cb{cb}", planes_420(g, bd, cb), run, kind="wp420", g=g, bd=bd, cb=cb)


def spot_wp420(step, got):
    import wp_estimate_420_model as model
    from hmme import synth
    m = synth.MARGIN
    area = lambda c: content(c)[m:m + c[1], m:m + c[0]].astype(np.int64)
    pics = [area(c) for _, c in step.planes]
    want = model.estimate(tuple(pics[:3]), [tuple(pics[3:6]), tuple(pics[6:9])], step.info["bd"])
    flat = [e for r in want for e in r]
    assert [tuple(int(v) for v in r) for r in got[0]] == [tuple(r[0]["wp"]) for r in want], f"[{step.label}] luma weights differ from wp_estimate_420_model"
    assert [tuple(int(v) for v in r) for r in got[1]] == [tuple(e["wp"]) for r in want for e in r[1:]], f"[{step.label}] chroma weights differ from wp_estimate_420_model"
    assert [[int(v) for v in r] for r in got[2]] == [[int(e[k]) for k in wem.INFO_FIELDS] for e in flat], f"[{step.label}] statistics differ from wp_estimate_420_model"


@functools.lru_cache(maxsize=None)
def refs_inputs(g, count=-1):
    """what select_dirs_refs and predict_bi_refs of one picture size are fed (drawn once, read-only): two references per list; count: the
    tables of the first `count` CTUs only"""
    import select_dirs_refs_model as drm
    n = n_ctu(g)
    rng = np.random.default_rng(SEED[g] + 30)
    pred = drm.predictors(2, n, SEED[g] + 31)
    d = dict(pred=pred, tables=drm.random_tables(2, n, n if count < 0 else count, SEED[g] + 32, pred, 0, lambda_q16()),
             field2=np.ascontiguousarray(np.stack([fh.random_field(n, 64, SEED[g] + 33), fh.random_field(n, 64, SEED[g] + 34)])),
             dirs64=rng.choice(np.array([1, 2, 3, 3, 0xFF], np.uint8), size=(n, 64)),
             refs64=rng.integers(0, 3, size=(2, n, 64)).astype(np.uint8))       # index 2 of two references: blocks that are not written
    for v in d.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
    return d


def dirs_refs(g):
    import select_dirs_refs_model as drm

    def run(eng, P):
        from hmme import api
        d, b = refs_inputs(g), drm.hm_bits(2, 2, 0b10)
        return eng.select_dirs_refs_frame(*GEOM[g], api.SelectParams(64), api.DirRefsParams(b.dir_bits, b.n_refs, b.ref_bits, b.l1_valid_mask), *d["tables"], d["pred"])
    return Step(f"select_dirs_refs_frame {g}", [], run, kind="dirs_refs", g=g)


def spot_dirs_refs(step, got):
    import select_dirs_refs_model as drm
    from hmme import api
    g = step.info["g"]
    d, t = refs_inputs(g), refs_inputs(g)["tables"]
    for c in spot_ctus(n_ctu(g), 7)[:4]:                                       # (the model takes 593 slots x references per CTU in Python)
        f, r, dr, s, cc = drm.select_dirs_refs_picture(*[a[:, :, c:c + 1] for a in t[:4]], t[4], t[5], api.SelectParams(64), *GEOM[g], drm.hm_bits(2, 2, 0b10), c, d["pred"],
                                                       lambda_q16())
        assert np.array_equal(got[0][:, c], f[:, 0]) and np.array_equal(got[1][:, c], r[:, 0]) and np.array_equal(got[2][c], dr[0]) and np.array_equal(got[3][c], s[0]) \
            and got[4][c] == cc[0], f"[{step.label}] CTU {c} on the used context differs from select_dirs_refs_model"


def predict_bi_refs(g, bd, refk=1):
    names = [pl(g, bd, "ref", refk), pl(g, bd, "other", 2), more(g, bd, "o0", 0), more(g, bd, "o1", 1)]

    def run(eng, P):
        d = refs_inputs(g)
        return (eng.predict_bi_refs_frame(P[:2], P[2:], d["field2"], d["dirs64"], d["refs64"]),)
    return Step(f"predict_bi_refs_frame {g} {bd}b ref{refk}", names, run, kind="predict_bi_refs", g=g, bd=bd, refk=refk)


def spot_predict_bi_refs(hmo, step, got):
    import predict_bi_refs_model as pbrm
    g, bd = step.info["g"], step.info["bd"]
    w, h = GEOM[g]
    d, ctus = refs_inputs(g), spot_ctus(n_ctu(g), 7)
    pics = [content(c) for _, c in step.planes]
    want = pbrm.pred_picture(hmo, pics[:2], pics[2:], w, h, bd, d["field2"], d["dirs64"], d["refs64"], np.zeros((h, w), np.int64), ctus)   # the wrapper hands the engine zeros
    for c in ctus:
        x, y = fh.ctu_origin(c, w)
        assert np.array_equal(got[0][y:y + 64, x:x + 64], want[y:y + 64, x:x + 64]), f"[{step.label}] CTU {c} on the used context differs from predict_bi_refs_model"


def test_b_pictures_with_several_references_between_the_older_calls(used, oracle_lib, hmo):
    """hmme_search / refine_frame_bi_refs share the scratch kWp0..kWp3 (through ensure), the CopyCache entries keyed by plane and bias and the
    job tables (FracTable::kAlways) with the weighted and bi calls; hmme_wp_estimate_420 shares kWpEst and the per-plane sums with
    hmme_wp_estimate and hmme_plane_stats; hmme_select_dirs_refs_frame and hmme_predict_bi_refs_frame the staging arena with every host form"""
    st = staging_calls("S")
    S = [
        # 1. two references after a weighted search of a larger geometry, then after one of a smaller: scratch sized by another call
        weighted("M", 8, 16), bi_refs("S", 8, 8), bi_refs("S", 8, 8), weighted("T", 8, 8), bi_refs("S", 8, 8), refine("M", 8, 16, "w2"), bi_refs("S", 8, 8, pred=101),
        # 2. the same call with one reference plane re-uploaded in between, then one plane of the other list: the copies keyed by plane and bias
        bi_refs("S", 8, 8), bi_refs("S", 8, 8, refk=2), bi_refs("S", 8, 8, refk=2), bi_refs("S", 8, 8), bi_refs("S", 8, 8, swap=True), bi_refs("S", 8, 8),
        refine("S", 8, 8, "bi"), bi_refs("S", 8, 8), refine("S", 8, 8, "bi_w"), bi_refs("S", 8, 8, center=102, pred=103, per=1),
        # 3. after a plain refinement without predictors, and before one: the job-table tags
        refine("S", 8, 8, "plain"), bi_refs("S", 8, 8), refine("S", 8, 8, "plain"), bi_refs("S", 8, 8, had=False), refine("S", 8, 8, "plain", had=False),
        # 4. 8 bit, then 10 bit of the same size (kWp2 serves 8 bit only), and back
        bi_refs("S", 8, 8), bi_refs("S", 10, 8), bi_refs("S", 10, 8), bi_refs("S", 8, 8), bi_refs("S", 10, 8, center=104, pred=105),
        # 5. the 4:2:0 estimate after the luma estimate, the plane statistics and a weighted search, and again after a chroma plane was re-uploaded
        st["wp_estimate"], st["plane_stats"], weighted("S", 8, 16), wp420("S", 8), wp420("S", 8), wp420("S", 8, cb=6), wp420("S", 8), st["wp_estimate"], st["plane_stats"],
        wp420("S", 10), bi_refs("S", 8, 8), wp420("S", 8, cb=6),
        # 6. the decision and the prediction between launches of other families
        dirs_refs("S"), st["select_dirs_frame"], dirs_refs("S"), bi_refs("S", 8, 8), predict_bi_refs("S", 8), st["predict_bi_frame"], predict_bi_refs("S", 8),
        predict_bi_refs("S", 8, refk=2), predict_bi_refs("S", 10), dirs_refs("T"), predict_bi_refs("T", 8), weighted("S", 8, 16), dirs_refs("S"), predict_bi_refs("S", 8),
    ]
    outs = run_sequence(used, S, "d'")
    by = {s.label: o for s, o in zip(S, outs)}
    # the results do follow the re-uploaded planes (the transitions are real ones)
    assert not np.array_equal(by[bi_refs("S", 8, 8).label][1][0], by[bi_refs("S", 8, 8, refk=2).label][1][0])
    assert not np.array_equal(by[bi_refs("S", 8, 8).label][1], by[bi_refs("S", 8, 8, swap=True).label][1])
    assert not np.array_equal(by[wp420("S", 8).label][2], by[wp420("S", 8, cb=6).label][2])
    assert not np.array_equal(by[predict_bi_refs("S", 8).label][0], by[predict_bi_refs("S", 8, refk=2).label][0])
    for want in (dict(bd=8, had=1, pred=None, center=None, refk=1, swap=False), dict(bd=10, center=104)):
        spot_bi_refs(oracle_lib, hmo, *last_of(S, outs, "bi_refs", **want))
    spot_wp420(*last_of(S, outs, "wp420", cb=6))
    spot_dirs_refs(*last_of(S, outs, "dirs_refs", g="S"))
    spot_predict_bi_refs(hmo, *last_of(S, outs, "predict_bi_refs", g="S", bd=8, refk=1))


# ---- e: streams ----------------------------------------------------------------------------------------------------------------------------
def test_streams_share_tables_scratch_and_the_event_ring(used, oracle_lib, hmo):
    """scratch_acquire / launch_end, the table tags that carry the stream, and the planes' fill and read events (plane_wait,
    plane_write_wait, read_done: an entry of the 64-event ring).  80 launches without predictors on one geometry alternate between two
    streams, every launch into tensors of its own, no host synchronisation until the end: plain and weighted searches and refinements,
    each form on both streams.  Three refills from registered host buffers run on a THIRD stream, which neither the last reader of the plane
    nor the next launch uses, so the refill's wait for the last read and the next launch's wait for the fill are both real waits:
      - launch 37: the reference plane gets another picture.  The launch before it is a weighted search at range 64 (the 16-bit kernel over
        60 CTUs: long enough that the refill is enqueued while it still runs); it and every launch before it must show the old picture,
        every launch after it the new one;
      - launch 70: a second reference plane, read by launch 0 alone and left alone since, is refilled and read again by launch 71.  By then
        the ring has wrapped: the plane's read_done is an entry that launch 64 recorded again;
      - launch 75: the first reference plane gets its old picture back, behind another long reader, with every event it holds recorded in
        the ring's second turn."""
    import torch
    from hmme import api, synth
    g, bd, sr, sr_long = "M", 8, 16, 64
    w, h = GEOM[g]
    n, m = n_ctu(g), synth.MARGIN
    dev = torch.device("cuda", 0)
    wp = at(FADE, bd)

    def both(eng, P, wk):
        if wk:
            mv, sad = eng.search_frame_w(P[0], P[1], sr, wp)
            return (mv, sad) + eng.refine_frame_w(P[0], P[1], sr, wp, mv)
        mv, sad = eng.search_frame(P[0], P[1], sr, fen=0)
        return (mv, sad) + eng.refine_frame(P[0], P[1], sr, mv)

    # the fresh contexts' results per reference picture (1 and 2): the four alternating calls and the long reader, each pinned to the oracle
    want = {}
    for refk in (1, 2):
        planes = [pl(g, bd, "cur", 0), pl(g, bd, "ref", refk)]
        for wk in (0, 1):
            st = Step(f"streams {g} {bd}b sr{sr} ref{refk} weighted{wk}", planes, lambda e, P, wk=wk: both(e, P, wk), kind="weighted" if wk else "plain",
                      g=g, bd=bd, sr=sr, pred=None, first=0, fen=0, refk=refk, wp=wp)
            want[refk, wk] = fresh_result(st)
            spot_search(oracle_lib, hmo, st, want[refk, wk][:2], seed=9)
        st = Step(f"streams {g} {bd}b sr{sr_long} ref{refk} long", planes, lambda e, P: e.search_frame_w(P[0], P[1], sr_long, wp), kind="weighted",
                  g=g, bd=bd, sr=sr_long, pred=None, first=0, refk=refk, wp=wp)
        want[refk, "long"] = fresh_result(st)
        spot_search(oracle_lib, hmo, st, want[refk, "long"], seed=9, stride=4)   # (an oracle CTU at range 64 costs 0.13 s: three or four of them)
    assert not np.array_equal(want[1, 0][1], want[2, 0][1]) and not np.array_equal(want[1, "long"][1], want[2, "long"][1])   # the refills do change the results
    # beside four of the launches, on the stream the launch does NOT use: the decision of a B picture with two references per list over the
    # first six CTUs and its prediction from the current and the reference plane (hmme_select_dirs_refs_device, hmme_predict_bi_refs_device);
    # they are no launches of the count above and take entries of the event ring of their own
    import select_dirs_refs_model as drm
    bd_in, bits = refs_inputs(g, 6), drm.hm_bits(2, 2, 0b10)
    b_fp, b_sel, b_dirs = api.FrameParams(1, 0, 8, 0, 6), api.SelectParams(64), [api.DirRefsParams(bits.dir_bits, bits.n_refs, bits.ref_bits, bits.l1_valid_mask)]
    to_dev = lambda a: torch.from_numpy(np.array(a).view(np.int32) if a.dtype == np.uint32 else np.array(a)).to(dev)   # (copies: the inputs are read-only)

    def b_inputs():
        return [to_dev(a) for a in bd_in["tables"]] + [to_dev(bd_in[k]) for k in ("pred", "field2", "dirs64", "refs64")]

    def b_outputs():
        return [torch.zeros((2, n, 64, 2), dtype=torch.int16, device=dev), torch.zeros((2, n, 64), dtype=torch.uint8, device=dev), torch.zeros((n, 64), dtype=torch.uint8, device=dev),
                torch.zeros((n, 64), dtype=torch.int16, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros((h, w), dtype=torch.uint8, device=dev)]

    def b_launch(e, cur, ref, d_in, d_out, s):
        t, (d_pred, d_f2, d_dirs, d_refs) = d_in[:6], d_in[6:]
        e.select_dirs_refs_device(w, h, 1, 2, b_fp, b_sel, b_dirs, *[x.data_ptr() for x in t], d_pred.data_ptr(), *[x.data_ptr() for x in d_out[:5]], s)
        e.predict_bi_refs_device([cur, ref], [ref, cur], api.FrameParams(1, 0, bd, 0, n), d_f2.data_ptr(), d_dirs.data_ptr(), d_refs.data_ptr(), 64, d_out[5].data_ptr(), w, s)

    def b_fresh(e, P):
        d_in, d_out = b_inputs(), b_outputs()
        torch.cuda.synchronize()
        b_launch(e, P[0], P[1], d_in, d_out, 0)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in d_out]
    b_want = {refk: fresh_result(Step(f"streams {g} {bd}b b-picture ref{refk}", [pl(g, bd, "cur", 0), pl(g, bd, "ref", refk)], b_fresh, kind="b_picture")) for refk in (1, 2)}
    assert b_want[1][2][:6].any() and not b_want[1][2][6:].any() and b_want[1][5].any() and not np.array_equal(b_want[1][5], b_want[2][5])
    b_at = {10: None, 40: None, 72: None, 78: None}                            # launch -> (the picture the reference plane held, the outputs)
    eng = used.eng
    eng.set_lambda(LAMBDA)
    pc, pr, pi = used.plane(*pl(g, bd, "cur", 0)), used.plane(*pl(g, bd, "ref", 1)), used.plane(*pl(g, bd, "idle", 1))
    host = {k: np.ascontiguousarray(content(cid(g, bd, k))[m:m + h, m:m + w].astype(np.uint8)) for k in (1, 2)}
    for a in host.values():
        eng.host_register(a)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    third = torch.cuda.Stream(dev)
    d_imv = {(refk, wk): torch.from_numpy(np.array(want[refk, wk][0])).to(dev) for refk in (1, 2) for wk in (0, 1)}
    fp, fp_long = api.FrameParams(sr, 0, bd, 0, n), api.FrameParams(sr_long, 0, bd, 0, n)
    n_launches = 80
    refills = {37: ("ref", 2), 70: ("idle", 2), 75: ("ref", 1)}      # before launch k: plane, the picture it gets
    long_readers, idle_reads = (36, 74), (0, 71)
    holds, plane_of = {"ref": 1, "idle": 1}, {"ref": pr, "idle": pi}
    outs = [fh.device_tables(1, n, dev) for _ in range(n_launches)]
    b_in = b_inputs()
    for k in b_at:
        b_at[k] = [None, b_outputs()]
    torch.cuda.synchronize()
    launched, j = [], 0
    try:
        for k in range(n_launches):
            s = streams[k % 2].cuda_stream
            if k in refills:
                name, newk = refills[k]
                plane_of[name].upload_async(host[newk].ctypes.data, w, 1, third.cuda_stream)
                holds[name] = newk
            a, b = outs[k]
            if k in idle_reads:
                form, wk, refk = "search", 0, holds["idle"]
                eng.search_frame_device(pc, pi, fp, None, a.data_ptr(), b.data_ptr(), s)
            elif k in long_readers:
                form, wk, refk = "long", "long", holds["ref"]
                eng.search_pairs_w_device([pc], [pr], fp_long, [wp], None, a.data_ptr(), b.data_ptr(), s)
            else:
                form, wk, refk = ("search", "refine")[(j // 2) % 2], (j // 4) % 2, holds["ref"]   # s s r r S S R R ...: each form on both streams
                j += 1
                if form == "search" and wk:
                    eng.search_pairs_w_device([pc], [pr], fp, [wp], None, a.data_ptr(), b.data_ptr(), s)
                elif form == "search":
                    eng.search_frame_device(pc, pr, fp, None, a.data_ptr(), b.data_ptr(), s)
                elif wk:
                    eng.refine_pairs_w_device([pc], [pr], fp, [wp], None, d_imv[refk, wk].data_ptr(), 1, a.data_ptr(), b.data_ptr(), s)
                else:
                    eng.refine_pairs_device([pc], [pr], fp, None, d_imv[refk, wk].data_ptr(), 1, a.data_ptr(), b.data_ptr(), s)
            launched.append((form, wk, refk, k % 2))
            if k in b_at:
                b_at[k][0] = holds["ref"]
                b_launch(eng, pc, pr, b_in, b_at[k][1], streams[(k + 1) % 2].cuda_stream)
        torch.cuda.synchronize()
        eng.upload_status(third.cuda_stream)
    finally:
        torch.cuda.synchronize()
        for a in host.values():
            eng.host_unregister(a)
    used.held[pl(g, bd, "idle", 1)[0]][1] = cid(g, bd, 2)   # what the planes hold now (the reference plane has picture 1 again)
    every = {(f, wk, st_) for f in ("search", "refine") for wk in (0, 1) for st_ in (0, 1)}
    assert every <= {(f, wk, st_) for f, wk, _, st_ in launched[:37]} and every <= {(f, wk, st_) for f, wk, _, st_ in launched[37:75]}
    assert [refk for _, _, refk, _ in launched[:37]] == [1] * 37 and launched[71][2] == 2 and launched[0][2] == 1
    for k, (form, wk, refk, st_) in enumerate(launched):
        mv, cost = outs[k][0].cpu().numpy()[0], outs[k][1].cpu().numpy().view(np.uint32)[0]
        ref_out = want[refk, wk][2:] if form == "refine" else want[refk, wk][:2]
        assert np.array_equal(mv, ref_out[0]) and np.array_equal(cost, ref_out[1]), \
            f"launch {k} ({form}, weighted {wk}, stream {st_}, reference picture {refk}) differs from the fresh context's"
    assert [b_at[k][0] for k in sorted(b_at)] == [1, 2, 2, 1]
    for k, (refk, d_out) in b_at.items():
        for j, (a, b) in enumerate(zip(d_out, b_want[refk])):
            assert np.array_equal(a.cpu().numpy(), b), f"the B picture beside launch {k} (reference picture {refk}): output {j} differs from the fresh context's"
