#!/usr/bin/env python3
"""cost of the prediction from one MV per 4x4 block, beside the 64 form of the same run (device-resident fields, torch events): one 2160p
picture, four references, luma and Cb + Cr

  predict_refs_ms            hmme_predict_refs_device (me_predict_kernel<T, 0, 0, 1>) on a field of one MV per 8x8 block: the yardstick
  predict_refs4_same_ms      hmme_predict_refs4_device (me_predict4_kernel<T, 0>) on (a): that field replicated to the 256 layout
  predict_refs4_mixed_ms     ... on (b): a field in which the four 4x4 blocks of every 8x8 block hold four different MVs and references
  predict_chroma_refs_ms, predict_chroma_refs4_same_ms, predict_chroma_refs4_mixed_ms: the same three for Cb + Cr
                             (me_predict_chroma_kernel<T, 1, 0, 64> / me_predict_chroma4_kernel<T, 0>)
  *_ratio                    median over the median of the 64 form; the min .. max of the 64 form is the noise of the run

Both bit depths 8 and 10.  REPS (default 7) repeats of each from a warm clock; median, min and max.  usage: tools/predict4_rate.py [out.json]"""
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


def replicate(t):
    """[n, 64, ...] -> [n, 256, ...]: every 4x4 block carries its 8x8 block's entry"""
    g = t.reshape((n, 8, 8) + tuple(t.shape[2:]))
    return g.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).reshape((n, 256) + tuple(t.shape[2:])).contiguous()


out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "n_ctu": n, "n_refs": 4, "reps": REPS}
g = torch.Generator(device=dev); g.manual_seed(1)
rng = np.random.default_rng(3)
for bd in (8, 10):
    fp = api.FrameParams(1, 0, bd, 0, n)

    def plane(pw, ph):
        p = eng.plane(pw, ph, bd)
        img = rng.integers(0, 1 << bd, size=(ph, pw))
        if bd == 8:
            p.upload_u8(img.astype(np.uint8))
        else:
            p.upload_pel(np.ascontiguousarray(img.astype(np.int16)), (0, 0))
        return p

    luma = [plane(w, h) for _ in range(4)]
    chroma = [plane(w // 2, h // 2) for _ in range(8)]
    tdt = torch.uint8 if bd == 8 else torch.int16
    d_f64 = torch.randint(-40, 41, (n, 64, 2), generator=g, device=dev, dtype=torch.int16)   # quarter-pel MVs of a plausible size, all phases
    d_r64 = torch.randint(0, 4, (n, 64), generator=g, device=dev, dtype=torch.uint8)
    d_f_same, d_r_same = replicate(d_f64), replicate(d_r64)
    # (b): the four entries of an 8x8 block differ in MV and in reference: quadrant q reads reference (r + q) % 4 at the block's MV + 5 q
    quad = torch.tensor([[0, 1], [2, 3]], device=dev).repeat(8, 8).reshape(1, 256)         # the quadrant of entry b
    d_f_mixed = (d_f_same + (5 * quad).to(torch.int16).unsqueeze(-1)).contiguous()
    d_r_mixed = ((d_r_same.to(torch.int32) + quad) % 4).to(torch.uint8).contiguous()
    d_img = torch.zeros((h, w), dtype=tdt, device=dev)
    d_cb, d_cr = (torch.zeros((h // 2, w // 2), dtype=tdt, device=dev) for _ in range(2))
    bps = 1 if bd == 8 else 2
    runs = {
        "predict_refs_ms": lambda: eng.predict_refs_device(luma, fp, d_f64.data_ptr(), d_r64.data_ptr(), 64, d_img.data_ptr(), w * bps, st),
        "predict_refs4_same_ms": lambda: eng.predict_refs4_device(luma, fp, d_f_same.data_ptr(), d_r_same.data_ptr(), d_img.data_ptr(), w * bps, stream=st),
        "predict_refs4_mixed_ms": lambda: eng.predict_refs4_device(luma, fp, d_f_mixed.data_ptr(), d_r_mixed.data_ptr(), d_img.data_ptr(), w * bps, stream=st),
        "predict_chroma_refs_ms": lambda: eng.predict_chroma_refs_device(chroma, w, h, fp, d_f64.data_ptr(), d_r64.data_ptr(), 64, d_cb.data_ptr(), d_cr.data_ptr(),
                                                                         w // 2 * bps, stream=st),
        "predict_chroma_refs4_same_ms": lambda: eng.predict_chroma_refs4_device(chroma, w, h, fp, d_f_same.data_ptr(), d_r_same.data_ptr(), d_cb.data_ptr(), d_cr.data_ptr(),
                                                                                w // 2 * bps, stream=st),
        "predict_chroma_refs4_mixed_ms": lambda: eng.predict_chroma_refs4_device(chroma, w, h, fp, d_f_mixed.data_ptr(), d_r_mixed.data_ptr(), d_cb.data_ptr(), d_cr.data_ptr(),
                                                                                 w // 2 * bps, stream=st),
    }
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    case = {k: timed(fn) for k, fn in runs.items()}
    for form, base in (("predict_refs4", "predict_refs_ms"), ("predict_chroma_refs4", "predict_chroma_refs_ms")):
        for field in ("same", "mixed"):
            case[f"{form}_{field}_ratio"] = round(case[f"{form}_{field}_ms"]["median"] / case[base]["median"], 3)
    out[f"{bd}bit"] = case
    for p in luma + chroma:
        p.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
