#!/usr/bin/env python3
"""cost of the B-picture calls from one MV per 4x4 block, each beside its 64-form sibling of the same run (device-resident fields and tables,
torch events): one 2160p B picture, one reference per list, luma and Cb + Cr

  predict_bi_ms / predict_bi4_{same,mixed}_ms                 hmme_predict_bi_device (me_predict_bi_kernel<T, 0>) / hmme_predict_bi4_device (me_predict_bi4_kernel<T>)
  predict_chroma_bi_ms / predict_chroma_bi4_{same,mixed}_ms   me_predict_chroma_kernel<T, 2, 0, 64> / me_predict_chroma_bi4_kernel<T>
  select_dirs_ms / select_dirs4_{same,mixed}_ms               me_select_dirs_kernel<false> at 64 / <true> at 256, on the same four random table sets
  search_bi_ms / search_bi4_{same,mixed}_ms                   hmme_search_pairs_bi_device / _bi4_device, one pair, range 4: origin + copies + search
  refine_bi_ms / refine_bi4_{same,mixed}_ms                   hmme_refine_pairs_bi_device / _bi4_device, one pair, Hadamard
    same   (a): the 64 form's field (and directions) replicated to the 256 layout
    mixed  (b): a field in which the four 4x4 blocks of every 8x8 block differ in direction and MV
  *_ratio   median over the median of the 64 form; the min .. max of the 64 form is the noise of the run

Both bit depths 8 and 10.  REPS (default 7) repeats of each from a warm clock; median, min and max.  usage: tools/bi4_rate.py [out.json]"""
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
eng.set_lambda_q16(500000)
n = api.load().hmme_num_ctus(w, h)
st = torch.cuda.current_stream().cuda_stream


def stats(t, nd=4):
    return {"median": round(statistics.median(t), nd), "min": round(min(t), nd), "max": round(max(t), nd)}


def timed(fn):
    """REPS single calls, each between its own pair of events -> ms"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) for a, b in ev])


def replicate(t, lead=0):
    """[..., n, 64, ...] -> [..., n, 256, ...] (lead dimensions in front of n): every 4x4 block carries its 8x8 block's entry"""
    front, rest = tuple(t.shape[:lead]), tuple(t.shape[lead + 2:])
    g = t.reshape(front + (n, 8, 8) + rest)
    return g.repeat_interleave(2, dim=lead + 1).repeat_interleave(2, dim=lead + 2).reshape(front + (n, 256) + rest).contiguous()


out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "n_ctu": n, "reps": REPS}
g = torch.Generator(device=dev); g.manual_seed(1)
rng = np.random.default_rng(3)
quad = torch.tensor([[0, 1], [2, 3]], device=dev).repeat(8, 8).reshape(256)             # the quadrant of entry b
# the four table sets of the decision: random costs and MVs (the decision reads tables, not pictures)
d_mvt = [torch.randint(-60, 61, (1, 2, n, 593, 2), generator=g, device=dev, dtype=torch.int16) for _ in range(2)]
d_ct = [torch.randint(2000, 60000, (1, 2, n, 593), generator=g, device=dev, dtype=torch.int32) for _ in range(2)]
dirp = [api.DirParams((3, 3, 5), (2, 1))]
for bd in (8, 10):
    fp = api.FrameParams(4, 1, bd, 0, n)

    def plane(pw, ph):
        p = eng.plane(pw, ph, bd)
        img = rng.integers(0, 1 << bd, size=(ph, pw))
        if bd == 8:
            p.upload_u8(img.astype(np.uint8))
        else:
            p.upload_pel(np.ascontiguousarray(img.astype(np.int16)), (0, 0))
        return p

    cur, l0, l1 = (plane(w, h) for _ in range(3))
    c0 = [plane(w // 2, h // 2) for _ in range(2)]
    c1 = [plane(w // 2, h // 2) for _ in range(2)]
    tdt = torch.uint8 if bd == 8 else torch.int16
    bps = 1 if bd == 8 else 2
    d_f64 = torch.randint(-40, 41, (1, 2, n, 64, 2), generator=g, device=dev, dtype=torch.int16)   # quarter-pel MVs of a plausible size, all phases
    d_d64 = torch.randint(1, 4, (1, n, 64), generator=g, device=dev, dtype=torch.uint8)
    d_f_same, d_d_same = replicate(d_f64, 2), replicate(d_d64, 1)
    # (b): quadrant q of an 8x8 block takes direction 1 + (d + q) % 3 and the block's MVs + 5 q
    d_f_mixed = (d_f_same + (5 * quad).to(torch.int16).reshape(1, 1, 1, 256, 1)).contiguous()
    d_d_mixed = (1 + (d_d_same.to(torch.int32) + quad.reshape(1, 1, 256)) % 3).to(torch.uint8).contiguous()
    d_img = torch.zeros((h, w), dtype=tdt, device=dev)
    d_cb, d_cr = (torch.zeros((h // 2, w // 2), dtype=tdt, device=dev) for _ in range(2))
    # the decision's outputs, at the larger layout
    o_f, o_d = torch.zeros((1, 2, n, 256, 2), dtype=torch.int16, device=dev), torch.zeros((1, n, 256), dtype=torch.uint8, device=dev)
    o_s, o_c = torch.zeros((1, n, 256), dtype=torch.int16, device=dev), torch.zeros((1, n), dtype=torch.int32, device=dev)
    sel64, sel256 = api.SelectParams(64), api.SelectParams(256)
    # the bi pass: one pair, its tables
    t_mv, t_c = torch.zeros((1, n, 593, 2), dtype=torch.int16, device=dev), torch.zeros((1, n, 593), dtype=torch.int32, device=dev)
    t_q, t_qc = torch.zeros((1, n, 593, 2), dtype=torch.int16, device=dev), torch.zeros((1, n, 593), dtype=torch.int32, device=dev)
    d_imv = torch.zeros((1, n, 593, 2), dtype=torch.int16, device=dev)
    o64, o_same, o_mixed = d_f64[0, 1].contiguous(), d_f_same[0, 1].contiguous(), d_f_mixed[0, 1].contiguous()   # the other list's field

    def select(entry, sel, uni):
        return lambda: entry(w, h, 1, fp, sel, dirp, d_mvt[0].data_ptr(), d_ct[0].data_ptr(), d_mvt[1].data_ptr(), d_ct[1].data_ptr(), uni.data_ptr(), None, o_f.data_ptr(),
                             o_d.data_ptr(), o_s.data_ptr(), o_c.data_ptr(), st)

    runs = {
        "predict_bi_ms": lambda: eng.predict_bi_device([l0], [l1], fp, d_f64.data_ptr(), d_d64.data_ptr(), 64, [d_img.data_ptr()], w * bps, st),
        "predict_bi4_same_ms": lambda: eng.predict_bi4_device([l0], [l1], fp, d_f_same.data_ptr(), d_d_same.data_ptr(), [d_img.data_ptr()], w * bps, st),
        "predict_bi4_mixed_ms": lambda: eng.predict_bi4_device([l0], [l1], fp, d_f_mixed.data_ptr(), d_d_mixed.data_ptr(), [d_img.data_ptr()], w * bps, st),
        "predict_chroma_bi_ms": lambda: eng.predict_chroma_bi_device(c0, c1, w, h, fp, d_f64.data_ptr(), d_d64.data_ptr(), 64, [d_cb.data_ptr(), d_cr.data_ptr()], w // 2 * bps,
                                                                     stream=st),
        "predict_chroma_bi4_same_ms": lambda: eng.predict_chroma_bi4_device(c0, c1, w, h, fp, d_f_same.data_ptr(), d_d_same.data_ptr(), [d_cb.data_ptr(), d_cr.data_ptr()],
                                                                            w // 2 * bps, st),
        "predict_chroma_bi4_mixed_ms": lambda: eng.predict_chroma_bi4_device(c0, c1, w, h, fp, d_f_mixed.data_ptr(), d_d_mixed.data_ptr(), [d_cb.data_ptr(), d_cr.data_ptr()],
                                                                             w // 2 * bps, st),
        "select_dirs_ms": select(eng.select_dirs_device, sel64, d_f64),
        "select_dirs4_same_ms": select(eng.select_dirs4_device, sel256, d_f_same),
        "select_dirs4_mixed_ms": select(eng.select_dirs4_device, sel256, d_f_mixed),
        "search_bi_ms": lambda: eng.search_pairs_bi_device([cur], [l0], [l1], fp, o64.data_ptr(), 64, None, None, t_mv.data_ptr(), t_c.data_ptr(), st),
        "search_bi4_same_ms": lambda: eng.search_pairs_bi4_device([cur], [l0], [l1], fp, o_same.data_ptr(), None, None, t_mv.data_ptr(), t_c.data_ptr(), st),
        "search_bi4_mixed_ms": lambda: eng.search_pairs_bi4_device([cur], [l0], [l1], fp, o_mixed.data_ptr(), None, None, t_mv.data_ptr(), t_c.data_ptr(), st),
        "refine_bi_ms": lambda: eng.refine_pairs_bi_device([cur], [l0], [l1], fp, o64.data_ptr(), 64, None, None, d_imv.data_ptr(), 1, t_q.data_ptr(), t_qc.data_ptr(), st),
        "refine_bi4_same_ms": lambda: eng.refine_pairs_bi4_device([cur], [l0], [l1], fp, o_same.data_ptr(), None, None, d_imv.data_ptr(), 1, t_q.data_ptr(), t_qc.data_ptr(), st),
        "refine_bi4_mixed_ms": lambda: eng.refine_pairs_bi4_device([cur], [l0], [l1], fp, o_mixed.data_ptr(), None, None, d_imv.data_ptr(), 1, t_q.data_ptr(), t_qc.data_ptr(), st),
    }
    for _ in range(2):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    case = {k: timed(fn) for k, fn in runs.items()}
    for form, base in (("predict_bi4", "predict_bi_ms"), ("predict_chroma_bi4", "predict_chroma_bi_ms"), ("select_dirs4", "select_dirs_ms"), ("search_bi4", "search_bi_ms"),
                       ("refine_bi4", "refine_bi_ms")):
        for field in ("same", "mixed"):
            case[f"{form}_{field}_ratio"] = round(case[f"{form}_{field}_ms"]["median"] / case[base]["median"], 3)
    out[f"{bd}bit"] = case
    for p in [cur, l0, l1] + c0 + c1:
        p.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
