#!/usr/bin/env python3
"""The weighted and the bi-prediction refinement of three picture pairs in one launch each, on a picture of 3 x 3 CTUs (168x136: partial at
the right and at the bottom, the smallest grid at which me_frac_deal leaves the plain order) -> one JSON line with the CRC32s of their
tables.  The launch modes (HMME_FRAC_GRID, HMME_FRAC_JOB_TABLE) are read once per process, so tests/test_gpu_parity.py runs this once
per mode and compares; it also calls weighted() / bi() itself for the tables that go to the oracle.
usage: refine_modes.py <bit depth> ..."""
import json, os, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hm-opencl_amd"))
import numpy as np
import torch   # before the engine: torch brings a HIP runtime of its own, and the one loaded first in a process is the one that sees the GPU
from hmme import api, synth

W, H, SR, N_CTU = 168, 136, 12, 9
WP_A, WP_B = (50, -90, 6, 32), (3, -5, 0, 0)   # w0, offset (at 8 bits), shift, round: both reach below zero (a biased current copy)


def _plane(eng, padded, bd):
    p = eng.plane(W, H, bd)
    p.upload_pel(padded, (synth.MARGIN, synth.MARGIN))
    return p


def _tables(n, dev):
    return torch.zeros((n, N_CTU, 593, 2), dtype=torch.int16, device=dev), torch.zeros((n, N_CTU, 593), dtype=torch.int32, device=dev)


def weighted(eng, bd):
    """weights [A, A, B]: a run of two pairs (they share the current picture) and a run of one, each with its own job table and counter"""
    dev = torch.device("cuda", 0)
    wps = [(w0, off << (bd - 8), sh, rnd) for w0, off, sh, rnd in (WP_A, WP_A, WP_B)]
    assert all(api.weight_check(bd, wp, 1) == 0 for wp in wps)
    maxv = (1 << bd) - 1
    fade = lambda a, wp: np.ascontiguousarray(np.clip(((wp[0] * a.astype(np.int64) + wp[3]) >> wp[2]) + wp[1], 0, maxv).astype(np.int16))
    c0, r0, _ = synth.make_pair(W, H, seed=2100 + bd, bit_depth=bd, max_mv=9, region=64)
    _, r1, _ = synth.make_pair(W, H, seed=2110 + bd, bit_depth=bd, max_mv=9, region=64)
    c2, r2, _ = synth.make_pair(W, H, seed=2120 + bd, bit_depth=bd, max_mv=9, region=64)
    curs, refs = [fade(c0, wps[0]), fade(c0, wps[0]), fade(c2, wps[2])], [r0, r1, r2]
    pred = np.stack([synth.random_predictors(N_CTU, seed=2130 + i, max_pel=10) for i in range(3)])
    assert np.any(pred != 0)
    pc, pc2 = _plane(eng, curs[0], bd), _plane(eng, curs[2], bd)
    pr = [_plane(eng, r, bd) for r in refs]
    try:
        fp = api.FrameParams(SR, 1, bd, 0, N_CTU)
        d_pred = torch.from_numpy(pred).to(dev)
        (d_mv, d_sad), (d_q, d_c) = _tables(3, dev), _tables(3, dev)
        eng.search_pairs_w_device([pc, pc, pc2], pr, fp, wps, d_pred.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), 0)
        eng.refine_pairs_w_device([pc, pc, pc2], pr, fp, wps, d_pred.data_ptr(), d_mv.data_ptr(), 1, d_q.data_ptr(), d_c.data_ptr(), 0)
        torch.cuda.synchronize()
        return dict(curs=curs, refs=refs, wps=wps, pred=pred, mv=d_mv.cpu().numpy(), qmv=d_q.cpu().numpy(), cost=d_c.cpu().numpy().astype(np.uint32))
    finally:
        for p in [pc, pc2] + pr:
            p.close()


def bi(eng, bd):
    """pairs 0 and 1: the two directions of one B picture; pair 2: other pictures.  A motion field per 8x8 block, window centres given"""
    dev = torch.device("cuda", 0)
    pic = lambda seed: synth.make_pair(W, H, seed=seed, bit_depth=bd, max_mv=5, region=64)
    cur, r0, _ = pic(2200 + bd)
    _, r1, _ = pic(2210 + bd)
    cur2, r2, _ = pic(2220 + bd)
    _, o2, _ = pic(2230 + bd)
    field = np.random.default_rng(2240 + bd).integers(-24, 25, size=(3, N_CTU, 64, 2)).astype(np.int16)
    pred = np.stack([synth.random_predictors(N_CTU, seed=2250 + i, max_pel=6) for i in range(3)])
    center = np.stack([synth.random_predictors(N_CTU, seed=2260 + i, max_pel=6) for i in range(3)])
    assert np.any(center != pred)
    pc, p0, p1, pc2, p2, po2 = planes = [_plane(eng, a, bd) for a in (cur, r0, r1, cur2, r2, o2)]
    try:
        curs, refs, others = [pc, pc, pc2], [p0, p1, p2], [p1, p0, po2]
        fp = api.FrameParams(SR, 1, bd, 0, N_CTU)
        d_f, d_pred, d_center = (torch.from_numpy(a).to(dev) for a in (field, pred, center))
        (d_mv, d_sad), (d_q, d_c) = _tables(3, dev), _tables(3, dev)
        eng.search_pairs_bi_device(curs, refs, others, fp, d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(), d_mv.data_ptr(), d_sad.data_ptr(), 0)
        eng.refine_pairs_bi_device(curs, refs, others, fp, d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(), d_mv.data_ptr(), 1,
                                   d_q.data_ptr(), d_c.data_ptr(), 0)
        torch.cuda.synchronize()
        return dict(curs=[cur, cur, cur2], refs=[r0, r1, r2], others=[r1, r0, o2], field=field, pred=pred, center=center, mv=d_mv.cpu().numpy(),
                    qmv=d_q.cpu().numpy(), cost=d_c.cpu().numpy().astype(np.uint32))
    finally:
        for p in planes:
            p.close()


def crc(r):
    return zlib.crc32(r["cost"].tobytes(), zlib.crc32(r["qmv"].tobytes()))


def engine():
    eng = api.Engine(0, 64)
    eng.set_lambda(57.9)
    return eng


if __name__ == "__main__":
    eng = engine()
    out = {bd: {"weighted_crc32": crc(weighted(eng, int(bd))), "bi_crc32": crc(bi(eng, int(bd)))} for bd in sys.argv[1:]}
    eng.close()
    print(json.dumps(out))
