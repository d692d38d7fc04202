#!/usr/bin/env python3
"""cost of the bi-prediction pass at picture size (device-resident, torch events): one 2160p pair at 8 and at 10 bits, SR 4 (HM's
BipredSearchRange), the other list's field one MV per 8x8 block

  origin_ms        the origin pass alone: me_predict_kernel<.., 1> over the whole picture (hmme_test_time_bipred_origin)
  weight_pass_ms   the yardstick: me_weight_plane_kernel over the padded reference, the existing pass with comparable traffic
                   (hmme_test_time_weight_passes); origin_over_weight_pass = the ratio of the medians
  search_bi_ms     hmme_search_pairs_bi_device (reference copy + origin pass + job table + search)
  refine_bi_ms_*   hmme_refine_pairs_bi_device on the search's integer MVs, Hadamard and SAD
  per_ctu_ms       the job this replaces: one hmme_search_refine_ctu call per CTU on origins of the same content built on the host
                   (the host's share -- downloading tables, compensating, building the origins -- is not even counted), wall clock

REPS (default 7) repeats of each from a warm clock; median, min and max.  usage: tools/bipred_rate.py [out.json]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hm-opencl_amd"))
import numpy as np
import torch
from hmme import api, synth

REPS = int(os.environ.get("REPS", "7"))
w, h = (int(v) for v in os.environ.get("SIZE", "3840x2160").split("x"))
SR = int(os.environ.get("SR", "4"))
m = synth.MARGIN
dev = torch.device("cuda", 0)
eng = api.Engine(0, 128); eng.set_lambda(57.9)
n = api.load().hmme_num_ctus(w, h)
ctus_x = (w + 63) // 64
st = torch.cuda.current_stream().cuda_stream


def stats(t, nd=3):
    return {"median": round(statistics.median(t), nd), "min": round(min(t), nd), "max": round(max(t), nd)}


def timed(fn):
    """REPS single launches, each between its own pair of events -> (median, min, max) ms"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) for a, b in ev])


out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "search_range": SR, "reps": REPS, "cases": []}
for bd in (8, 10):
    cur, ref, _ = synth.make_pair(w, h, seed=1234, bit_depth=bd, max_mv=6)
    _, other, _ = synth.make_pair(w, h, seed=2234, bit_depth=bd, max_mv=6)
    pc, pr, po = (eng.plane(w, h, bd) for _ in range(3))
    for p, a in ((pc, cur), (pr, ref), (po, other)):
        p.upload_pel(a, (m, m))
    rng = np.random.default_rng(99)
    field = rng.integers(-24, 25, size=(1, n, 64, 2)).astype(np.int16)
    pred = synth.random_predictors(n, seed=5, max_pel=6)[None]
    center = synth.random_predictors(n, seed=6, max_pel=6)[None]
    d_f, d_pred, d_center = (torch.from_numpy(a).to(dev) for a in (field, pred, center))
    d_mv = torch.zeros((n, 593, 2), dtype=torch.int16, device=dev); d_sad = torch.zeros((n, 593), dtype=torch.int32, device=dev)
    d_q = torch.zeros_like(d_mv); d_c = torch.zeros_like(d_sad)
    fp = api.FrameParams(SR, 1, bd, 0, n)
    search = lambda: eng.search_pairs_bi_device([pc], [pr], [po], fp, d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(),
                                                d_mv.data_ptr(), d_sad.data_ptr(), st)
    for _ in range(3):     # warm clock, scratch grown
        search()
    torch.cuda.synchronize()
    case = {"bit_depth": bd, "mv_per_ctu": 64}
    case["origin_ms"] = stats([eng.time_bipred_origin(pc, po, d_f.data_ptr(), 64, st, reps=5) for _ in range(REPS)], 4)
    case["weight_pass_ms"] = stats([eng.time_weight_passes(pc, pr, (1, 0, 0, 0), st, reps=5)[0] for _ in range(REPS)], 4)
    case["origin_over_weight_pass"] = round(case["origin_ms"]["median"] / case["weight_pass_ms"]["median"], 2)
    case["search_bi_ms"] = timed(search)
    case["origin_over_search_bi"] = round(case["origin_ms"]["median"] / case["search_bi_ms"]["median"], 3)
    for had in (1, 0):
        refine = lambda: eng.refine_pairs_bi_device([pc], [pr], [po], fp, d_f.data_ptr(), 64, d_center.data_ptr(), d_pred.data_ptr(),
                                                    d_mv.data_ptr(), had, d_q.data_ptr(), d_c.data_ptr(), st)
        for _ in range(2):
            refine()
        torch.cuda.synchronize()
        case["refine_bi_ms_" + ("hadamard" if had else "sad")] = timed(refine)
    # the replaced job: per-CTU calls on host-built origins of the same content (the engine's own prediction stands in for the host's)
    pred_img = eng.predict_frame(po, field[0]).astype(np.int32)
    org = np.ascontiguousarray((2 * cur[m:m + h, m:m + w].astype(np.int32) - pred_img).astype(np.int16))
    ctus = [c for c in range(n) if (c % ctus_x) * 64 + 64 <= w and (c // ctus_x) * 64 + 64 <= h]   # whole CTUs; scaled to all n below
    params = []
    for c in ctus:
        x, y = (c % ctus_x) * 64, (c // ctus_x) * 64
        lt_x, lt_y, rb_x, rb_y = api.set_search_range(int(center[0, c, 0]), int(center[0, c, 1]), SR, x, y, w, h)
        params.append((x, y, api.SearchParams(lt_x, lt_y, rb_x, rb_y, int(pred[0, c, 0]), int(pred[0, c, 1]), 1, bd)))
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for x, y, p in params:
            eng.search_refine_ctu(org, (x, y), ref, (m + x, m + y), p, True)
        t.append((time.perf_counter() - t0) * 1e3 * n / len(ctus))
    case["per_ctu_ms"] = stats(t, 1)
    case["per_ctu_calls"] = n
    out["cases"].append(case)
    for p in (pc, pr, po):
        p.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
