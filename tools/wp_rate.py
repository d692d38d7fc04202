#!/usr/bin/env python3
"""cost of explicit weighted prediction at picture size (device-resident, torch events): for 2160p 8-bit SR 64 and 2160p 10-bit SR 128

  search_w_ms      hmme_search_pairs_w_device, one pair, a fade
  search_ref_ms    the reference leg: the SAME library's unweighted search of u16 planes of that geometry with fen = 0 -- the same
                   kernel (me_search16_kernel<0, PDW>) over the same candidates (8-bit content: in 9-bit planes)
  pass_ref_ms / pass_cur_ms   the two plane passes on their own (weighting the padded reference; the u16 CTU-blocked current picture)
  refine_w_ms / refine_ms     weighted against unweighted refinement on the same integer MVs (Hadamard and SAD)

REPS (default 7) repeats of each from a warm clock; median, min and max.  Expectation: search_w = search_ref + the passes, within
search_ref's own spread.  usage: tools/wp_rate.py [out.json]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hm-opencl_amd"))
import numpy as np
import torch
from hmme import api, synth

REPS = int(os.environ.get("REPS", "7"))
w, h = (int(v) for v in os.environ.get("SIZE", "3840x2160").split("x"))
m = synth.MARGIN
dev = torch.device("cuda", 0)
eng = api.Engine(0, 128); eng.set_lambda(57.9)
n = api.load().hmme_num_ctus(w, h)
st = torch.cuda.current_stream().cuda_stream


def timed(fn):
    """REPS single launches, each between its own pair of events -> (median, min, max) ms"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) for a, b in ev]
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "reps": REPS, "cases": []}
for bd, sr in ((8, 64), (10, 128)):
    wp = (40, 12 << (bd - 8), 6, 32)
    cur, ref, _ = synth.make_pair(w, h, seed=1234, bit_depth=bd)
    maxv = (1 << bd) - 1
    cur = np.ascontiguousarray(np.clip(((wp[0] * cur.astype(np.int64) + wp[3]) >> wp[2]) + wp[1], 0, maxv).astype(np.int16))   # the fade
    pc, pr = eng.plane(w, h, bd), eng.plane(w, h, bd)
    pc.upload_pel(cur, (m, m)); pr.upload_pel(ref, (m, m))
    bd16 = max(bd, 9)      # the reference leg's u16 planes
    qc, qr = eng.plane(w, h, bd16), eng.plane(w, h, bd16)
    qc.upload_pel(cur, (m, m)); qr.upload_pel(ref, (m, m))
    d_mv = torch.zeros((n, 593, 2), dtype=torch.int16, device=dev); d_sad = torch.zeros((n, 593), dtype=torch.int32, device=dev)
    d_mv0 = torch.zeros_like(d_mv); d_sad0 = torch.zeros_like(d_sad)
    d_q = torch.zeros_like(d_mv); d_c = torch.zeros_like(d_sad)
    fp, fp16 = api.FrameParams(sr, 0, bd, 0, n), api.FrameParams(sr, 0, bd16, 0, n)
    search_w = lambda: eng.search_pairs_w_device([pc], [pr], fp, [wp], None, d_mv.data_ptr(), d_sad.data_ptr(), st)
    search_ref = lambda: eng.search_pairs_device([qc], [qr], fp16, None, d_mv0.data_ptr(), d_sad0.data_ptr(), st)
    for _ in range(3):     # warm clock, scratch grown, job tables in place
        search_ref(); search_w()
    torch.cuda.synchronize()
    case = {"bit_depth": bd, "search_range": sr, "weight": wp}
    case["search_ref_ms"] = timed(search_ref)
    case["search_w_ms"] = timed(search_w)
    case["search_ref_ms_again"] = timed(search_ref)     # the reference leg's own run-to-run spread, around the weighted leg
    passes = [eng.time_weight_passes(pc, pr, wp, st, reps=5) for _ in range(REPS)]
    for k, name in enumerate(("pass_ref_ms", "pass_cur_ms")):
        t = [p[k] for p in passes]
        case[name] = {"median": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    case["expected_search_w_ms"] = round(case["search_ref_ms"]["median"] + case["pass_ref_ms"]["median"] + case["pass_cur_ms"]["median"], 3)
    search_w(); torch.cuda.synchronize()
    for had in (1, 0):
        rw = lambda: eng.refine_pairs_w_device([pc], [pr], fp, [wp], None, d_mv.data_ptr(), had, d_q.data_ptr(), d_c.data_ptr(), st)
        ru = lambda: eng.refine_pairs_device([pc], [pr], fp, None, d_mv.data_ptr(), had, d_q.data_ptr(), d_c.data_ptr(), st)
        for _ in range(2):
            ru(); rw()
        torch.cuda.synchronize()
        key = "hadamard" if had else "sad"
        case["refine_ms_" + key] = timed(ru)
        case["refine_w_ms_" + key] = timed(rw)
    out["cases"].append(case)
    for p in (pc, pr, qc, qr):
        p.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
