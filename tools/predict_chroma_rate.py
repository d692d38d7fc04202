#!/usr/bin/env python3
"""cost of the 4:2:0 chroma prediction (both components, one launch) beside the luma call of the same form on the same field in the same run
(device-resident fields, torch events): one 2160p picture, one random quarter-pel MV per 8x8 block

  pairs_luma_ms / pairs_chroma_ms        hmme_predict_pairs_device / hmme_predict_chroma_pairs_device
  pairs_w_luma_ms / pairs_w_chroma_ms    ... with HM-like weights (hmme_predict_pairs_w_device / weights per component)
  refs_*                                 hmme_predict_refs(_w)_device / hmme_predict_chroma_refs_device, four references drawn per block
  bi_*                                   hmme_predict_bi(_w)_device / hmme_predict_chroma_bi_device, blocks L0, L1 and bi in equal parts
  *_ratio                                chroma median over luma median
  crc32 (per form)                       CRC-32 of the image(s) the form wrote, downloaded after its timed repeats: two libraries that
                                         report the same value computed the same samples at the size timed

Both bit depths 8 and 10.  REPS (default 7) repeats of each from a warm clock; median, min and max.  usage: tools/predict_chroma_rate.py [out.json]"""
import json, os, statistics, sys, zlib
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


def timed(fn, images):
    """REPS single launches, each between its own pair of events -> ms, and the CRC-32 of what the last one left in `images`"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    res = stats([a.elapsed_time(b) for a, b in ev])
    crc = 0
    for t in images:
        crc = zlib.crc32(t.cpu().numpy().tobytes(), crc)
    res["crc32"] = f"{crc:08x}"
    return res


def plane(pw, ph, bd, rng):
    p = eng.plane(pw, ph, bd)
    img = rng.integers(0, 1 << bd, size=(ph, pw))
    if bd == 8:
        p.upload_u8(img.astype(np.uint8))
    else:
        p.upload_pel(np.ascontiguousarray(img.astype(np.int16)), (0, 0))
    return p


out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "n_ctu": n, "mv_per_ctu": 64, "reps": REPS}
g = torch.Generator(device=dev); g.manual_seed(1)
rng = np.random.default_rng(3)
for bd in (8, 10):
    fp = api.FrameParams(1, 0, bd, 0, n)
    o = 1 << (bd - 8)
    wps = [(70, 9 * o, 6, 32), (55, -14 * o, 6, 32), (60, 3 * o, 6, 32), (75, -5 * o, 6, 32)]                  # luma, per reference
    cwps = [(66, 4 * o, 6, 32), (58, -6 * o, 6, 32), (35, 2 * o, 5, 16), (30, -3 * o, 5, 16)] * 2              # chroma: (Cb, Cr) per reference
    luma = [plane(w, h, bd, rng) for _ in range(4)]
    chroma = [plane(w // 2, h // 2, bd, rng) for _ in range(8)]                                                # cb0, cr0, cb1, cr1, ...
    tdt = torch.uint8 if bd == 8 else torch.int16
    d_field = torch.randint(-40, 41, (1, 2, n, 64, 2), generator=g, device=dev, dtype=torch.int16)   # quarter-pel MVs of a plausible size, all phases
    d_dir = torch.randint(1, 4, (1, n, 64), generator=g, device=dev, dtype=torch.uint8)
    d_ref = torch.randint(0, 4, (n, 64), generator=g, device=dev, dtype=torch.uint8)
    d_img = torch.zeros((h, w), dtype=tdt, device=dev)
    d_c = [torch.zeros((h // 2, w // 2), dtype=tdt, device=dev) for _ in range(2)]
    bps = 1 if bd == 8 else 2
    pitch, cpitch = w * bps, (w // 2) * bps
    f, d, r, img, cimg = d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), d_img.data_ptr(), [t.data_ptr() for t in d_c]
    runs = {
        "pairs_luma_ms": lambda: eng.predict_pairs_device(luma[:1], fp, f, 64, [img], pitch, st),
        "pairs_chroma_ms": lambda: eng.predict_chroma_pairs_device(chroma[:2], w, h, fp, f, 64, cimg, cpitch, None, st),
        "pairs_w_luma_ms": lambda: eng.predict_pairs_w_device(luma[:1], fp, wps[:1], f, 64, [img], pitch, st),
        "pairs_w_chroma_ms": lambda: eng.predict_chroma_pairs_device(chroma[:2], w, h, fp, f, 64, cimg, cpitch, [cwps[0], cwps[2]], st),
        "refs_luma_ms": lambda: eng.predict_refs_device(luma, fp, f, r, 64, img, pitch, st),
        "refs_chroma_ms": lambda: eng.predict_chroma_refs_device(chroma, w, h, fp, f, r, 64, cimg[0], cimg[1], cpitch, None, st),
        "refs_w_luma_ms": lambda: eng.predict_refs_w_device(luma, fp, wps, f, r, 64, img, pitch, st),
        "refs_w_chroma_ms": lambda: eng.predict_chroma_refs_device(chroma, w, h, fp, f, r, 64, cimg[0], cimg[1], cpitch, cwps, st),
        "bi_luma_ms": lambda: eng.predict_bi_device([luma[0]], [luma[1]], fp, f, d, 64, [img], pitch, st),
        "bi_chroma_ms": lambda: eng.predict_chroma_bi_device(chroma[0:2], chroma[2:4], w, h, fp, f, d, 64, cimg, cpitch, None, None, st),
        "bi_w_luma_ms": lambda: eng.predict_bi_w_device([luma[0]], [luma[1]], fp, [wps[0]], [wps[1]], f, d, 64, [img], pitch, st),
        "bi_w_chroma_ms": lambda: eng.predict_chroma_bi_device(chroma[0:2], chroma[2:4], w, h, fp, f, d, 64, cimg, cpitch, [cwps[0], cwps[2]], [cwps[1], cwps[3]], st),
    }
    for _ in range(3):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    case = {k: timed(fn, d_c if "chroma" in k else [d_img]) for k, fn in runs.items()}
    for form in ("pairs", "pairs_w", "refs", "refs_w", "bi", "bi_w"):
        case[f"{form}_ratio"] = round(case[f"{form}_chroma_ms"]["median"] / case[f"{form}_luma_ms"]["median"], 3)
    case["blocks_per_direction"] = np.bincount(d_dir.cpu().numpy().reshape(-1), minlength=4)[1:4].tolist()
    out[f"{bd}bit"] = case
    for p in luma + chroma:
        p.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
