#!/usr/bin/env python3
"""cost of the final prediction in a slice with explicit weighted prediction, beside the unweighted kernels of the same run (device-resident
fields, torch events): one 2160p picture, one MV per 8x8 block

  predict_bi_ms        hmme_predict_bi_device (me_predict_bi_kernel<T, 0>) on a field whose blocks are L0, L1 and bi in equal parts
  predict_bi_w_ms      hmme_predict_bi_w_device (me_predict_bi_kernel<T, 1>) on the same planes, field and directions with two HM-like weights
  predict_bi_w_ident_ms  ... with two identity weights: the host picks the unweighted kernel, so this is predict_bi_ms plus the check
  predict_refs_ms      hmme_predict_refs_device (me_predict_kernel<T, 0, 0, 1>), four references drawn per block
  predict_refs_w_ms    hmme_predict_refs_w_device (me_predict_kernel<T, 0, 2, 1>) on the same field and indices with four weights
  *_ratio              weighted median over unweighted median

Both bit depths 8 and 10.  REPS (default 7) repeats of each from a warm clock; median, min and max.  usage: tools/predict_w_rate.py [out.json]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hm-opencl_amd"))
import numpy as np
import torch
from hmme import api

REPS = int(os.environ.get("REPS", "7"))
w, h = (int(v) for v in os.environ.get("SIZE", "3840x2160").split("x"))
dev = torch.device("cuda", 0)
eng = api.Engine(0, 64)
n = api.load().hmme_num_ctus(w, h)
st = torch.cuda.current_stream().cuda_stream


def stats(t, nd=4):
    return {"median": round(statistics.median(t), nd), "min": round(min(t), nd), "max": round(max(t), nd)}


def timed(fn):
    """REPS single launches, each between its own pair of events -> ms"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) for a, b in ev])


out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "n_ctu": n, "mv_per_ctu": 64, "reps": REPS}
g = torch.Generator(device=dev); g.manual_seed(1)
rng = np.random.default_rng(3)
for bd in (8, 10):
    fp = api.FrameParams(1, 0, bd, 0, n)
    o = 1 << (bd - 8)
    wps = [(70, 9 * o, 6, 32), (55, -14 * o, 6, 32), (60, 3 * o, 6, 32), (75, -5 * o, 6, 32)]
    ident = (64, 0, 6, 32)
    planes = []
    for r in range(4):
        p = eng.plane(w, h, bd)
        img = rng.integers(0, 1 << bd, size=(h, w))
        if bd == 8:
            p.upload_u8(img.astype(np.uint8))
        else:
            p.upload_pel(np.ascontiguousarray(img.astype(np.int16)), (0, 0))
        planes.append(p)
    tdt = torch.uint8 if bd == 8 else torch.int16
    d_field = torch.randint(-40, 41, (1, 2, n, 64, 2), generator=g, device=dev, dtype=torch.int16)   # quarter-pel MVs of a plausible size, all phases
    d_dir = torch.randint(1, 4, (1, n, 64), generator=g, device=dev, dtype=torch.uint8)
    d_ref = torch.randint(0, 4, (n, 64), generator=g, device=dev, dtype=torch.uint8)
    d_img = torch.zeros((h, w), dtype=tdt, device=dev)
    pitch = w * (1 if bd == 8 else 2)
    runs = {
        "predict_bi_ms": lambda: eng.predict_bi_device([planes[0]], [planes[1]], fp, d_field.data_ptr(), d_dir.data_ptr(), 64, [d_img.data_ptr()], pitch, st),
        "predict_bi_w_ms": lambda: eng.predict_bi_w_device([planes[0]], [planes[1]], fp, [wps[0]], [wps[1]], d_field.data_ptr(), d_dir.data_ptr(), 64, [d_img.data_ptr()],
                                                          pitch, st),
        "predict_bi_w_ident_ms": lambda: eng.predict_bi_w_device([planes[0]], [planes[1]], fp, [ident], [ident], d_field.data_ptr(), d_dir.data_ptr(), 64,
                                                                [d_img.data_ptr()], pitch, st),
        "predict_refs_ms": lambda: eng.predict_refs_device(planes, fp, d_field.data_ptr(), d_ref.data_ptr(), 64, d_img.data_ptr(), pitch, st),
        "predict_refs_w_ms": lambda: eng.predict_refs_w_device(planes, fp, wps, d_field.data_ptr(), d_ref.data_ptr(), 64, d_img.data_ptr(), pitch, st),
    }
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    case = {k: timed(fn) for k, fn in runs.items()}
    case["predict_bi_w_ratio"] = round(case["predict_bi_w_ms"]["median"] / case["predict_bi_ms"]["median"], 3)
    case["predict_refs_w_ratio"] = round(case["predict_refs_w_ms"]["median"] / case["predict_refs_ms"]["median"], 3)
    case["blocks_per_direction"] = np.bincount(d_dir.cpu().numpy().reshape(-1), minlength=4)[1:4].tolist()
    out[f"{bd}bit"] = case
    for p in planes:
        p.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
