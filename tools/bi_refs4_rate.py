#!/usr/bin/env python3
"""cost of the multi-reference B-picture calls from one MV per 4x4 block (the "bi_refs4" family) at picture size (device-resident buffers,
torch events): one 2160p 8-bit B picture with 2 and with 4 references per list, random fields that name every reference.  Per reference count
each new call is timed beside its 64-form sibling (the bi_refs family) AND beside its bi4 sibling (one reference per list), in the same run:

  predict          hmme_predict_bi_refs4_device (me_predict_bi4_kernel<T, 1>) / hmme_predict_bi_refs_device at 64 / hmme_predict_bi4_device
  predict_chroma   hmme_predict_chroma_bi_refs4_device (me_predict_chroma_bi4_kernel<T, 1>) / hmme_predict_chroma_bi_refs_device / _bi4_device
  select           hmme_select_dirs_refs4_device (me_select_dirs_refs_kernel<true>) / hmme_select_dirs_refs_device on the same random table sets /
                   hmme_select_dirs4_device on the first set of each list
  search, refine   hmme_search / refine_frame_bi_refs4_device of list 0 over its references, bi range 4, Hadamard / the _bi_refs_device calls /
                   hmme_search / refine_pairs_bi4_device of one pair
    same   the 64 form's fields replicated to the 256 layout: where the 4 form and the 64 form compute the same thing (checked for the images)
    mixed  the four 4x4 blocks of every 8x8 block differ in direction, MV and reference index
  ratio_to_64 / ratio_to_bi4   median over the sibling's median

REPS (default 7) repeats of each from a warm clock; median, min and max.  usage: tools/bi_refs4_rate.py [out.json]"""
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
fp = api.FrameParams(4, 1, 8, 0, n)


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


def legs(runs, form):
    """{same, mixed, at_64, bi4} -> the timings and the two ratios per field"""
    for _ in range(2):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    r = {f"{form}_{k}_ms": timed(fn) for k, fn in runs.items()}
    for field in ("same", "mixed"):
        r[f"{field}_ratio_to_64"] = round(r[f"{form}_{field}_ms"]["median"] / r[f"{form}_at_64_ms"]["median"], 3)
        r[f"{field}_ratio_to_bi4"] = round(r[f"{form}_{field}_ms"]["median"] / r[f"{form}_bi4_ms"]["median"], 3)
    return r


rng = np.random.default_rng(3)
planes, cplanes = [], []
for r in range(9):                                                                                   # the current picture, 4 + 4 references
    p = eng.plane(w, h)
    p.upload_u8(rng.integers(0, 256, size=(h, w), dtype=np.uint8))
    planes.append(p)
for r in range(16):                                                                                  # (Cb, Cr) of the 4 + 4 references
    p = eng.plane(w // 2, h // 2)
    p.upload_u8(rng.integers(0, 256, size=(h // 2, w // 2), dtype=np.uint8))
    cplanes.append(p)
cur, lists = planes[0], (planes[1:5], planes[5:9])
clists = (cplanes[:8], cplanes[8:])
quad = torch.tensor([[0, 1], [2, 3]], device=dev).repeat(8, 8).reshape(256)                          # the quadrant of entry b
out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "n_ctu": n, "reps": REPS, "cases": {}}
for R in (2, 4):
    g = torch.Generator(device=dev); g.manual_seed(R)
    d_f64 = torch.randint(-40, 41, (2, n, 64, 2), generator=g, device=dev, dtype=torch.int16)
    d_d64 = torch.randint(1, 4, (n, 64), generator=g, device=dev, dtype=torch.uint8)
    d_r64 = torch.randint(0, R, (2, n, 64), generator=g, device=dev, dtype=torch.uint8)
    d_f_same, d_d_same, d_r_same = replicate(d_f64, 1), replicate(d_d64, 0), replicate(d_r64, 1)
    # mixed: quadrant q of an 8x8 block takes direction 1 + (d + q) % 3, the block's MVs + 5 q and index (r + q) % R
    d_f_mixed = (d_f_same + (5 * quad).to(torch.int16).reshape(1, 1, 256, 1)).contiguous()
    d_d_mixed = (1 + (d_d_same.to(torch.int32) + quad.reshape(1, 256)) % 3).to(torch.uint8).contiguous()
    d_r_mixed = ((d_r_same.to(torch.int32) + quad.reshape(1, 1, 256)) % R).to(torch.uint8).contiguous()
    d_img, d_img2 = (torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(2))
    d_c = [torch.zeros((h // 2, w // 2), dtype=torch.uint8, device=dev) for _ in range(4)]
    l0, l1 = lists[0][:R], lists[1][:R]
    c0, c1 = clists[0][:2 * R], clists[1][:2 * R]
    case = {}
    P = lambda t: t.data_ptr()

    case["predict"] = legs({
        "same": lambda: eng.predict_bi_refs4_device(l0, l1, fp, P(d_f_same), P(d_d_same), P(d_r_same), P(d_img), w, st),
        "mixed": lambda: eng.predict_bi_refs4_device(l0, l1, fp, P(d_f_mixed), P(d_d_mixed), P(d_r_mixed), P(d_img2), w, st),
        "at_64": lambda: eng.predict_bi_refs_device(l0, l1, fp, P(d_f64), P(d_d64), P(d_r64), 64, P(d_img2), w, st),
        "bi4": lambda: eng.predict_bi4_device(l0[:1], l1[:1], fp, P(d_f_mixed), P(d_d_mixed), [P(d_img2)], w, st)}, "predict")
    eng.predict_bi_refs4_device(l0, l1, fp, P(d_f_same), P(d_d_same), P(d_r_same), P(d_img), w, st)
    eng.predict_bi_refs_device(l0, l1, fp, P(d_f64), P(d_d64), P(d_r64), 64, P(d_img2), w, st)
    torch.cuda.synchronize()
    case["predict"]["same_equals_the_64_form"] = bool(torch.equal(d_img, d_img2))

    case["predict_chroma"] = legs({
        "same": lambda: eng.predict_chroma_bi_refs4_device(c0, c1, w, h, fp, P(d_f_same), P(d_d_same), P(d_r_same), P(d_c[0]), P(d_c[1]), w // 2, st),
        "mixed": lambda: eng.predict_chroma_bi_refs4_device(c0, c1, w, h, fp, P(d_f_mixed), P(d_d_mixed), P(d_r_mixed), P(d_c[2]), P(d_c[3]), w // 2, st),
        "at_64": lambda: eng.predict_chroma_bi_refs_device(c0, c1, w, h, fp, P(d_f64), P(d_d64), P(d_r64), 64, P(d_c[2]), P(d_c[3]), w // 2, stream=st),
        "bi4": lambda: eng.predict_chroma_bi4_device(c0[:2], c1[:2], w, h, fp, P(d_f_mixed), P(d_d_mixed), [P(d_c[2]), P(d_c[3])], w // 2, st)}, "predict_chroma")
    eng.predict_chroma_bi_refs4_device(c0, c1, w, h, fp, P(d_f_same), P(d_d_same), P(d_r_same), P(d_c[0]), P(d_c[1]), w // 2, st)
    eng.predict_chroma_bi_refs_device(c0, c1, w, h, fp, P(d_f64), P(d_d64), P(d_r64), 64, P(d_c[2]), P(d_c[3]), w // 2, stream=st)
    torch.cuda.synchronize()
    case["predict_chroma"]["same_equals_the_64_form"] = bool(torch.equal(d_c[0], d_c[2])) and bool(torch.equal(d_c[1], d_c[3]))

    # the decision: random costs and MVs (it reads tables, not pictures); the bi4 sibling takes the first set of each list
    d_mvt = [torch.randint(-60, 61, (1, 2, R, n, 593, 2), generator=g, device=dev, dtype=torch.int16) for _ in range(2)]
    d_ct = [torch.randint(2000, 60000, (1, 2, R, n, 593), generator=g, device=dev, dtype=torch.int32) for _ in range(2)]
    d_mv1 = [t[:, :, 0].contiguous() for t in d_mvt]
    d_c1 = [t[:, :, 0].contiguous() for t in d_ct]
    o_f, o_r = torch.zeros((1, 2, n, 256, 2), dtype=torch.int16, device=dev), torch.zeros((1, 2, n, 256), dtype=torch.uint8, device=dev)
    o_d, o_s, o_c = torch.zeros((1, n, 256), dtype=torch.uint8, device=dev), torch.zeros((1, n, 256), dtype=torch.int16, device=dev), torch.zeros((1, n), dtype=torch.int32, device=dev)
    sel64, sel256 = api.SelectParams(64), api.SelectParams(256)
    dirp = [api.DirRefsParams((3, 3, 5), (R, R), (list(range(1, R + 1)), list(range(1, R + 1))))]
    dirp1 = [api.DirParams((3, 3, 5), (2, 1))]

    def select(entry, sel, uni, uref):
        return lambda: entry(w, h, 1, R, fp, sel, dirp, P(d_mvt[0]), P(d_ct[0]), P(d_mvt[1]), P(d_ct[1]), P(uni), P(uref), None, P(o_f), P(o_r), P(o_d), P(o_s), P(o_c), st)

    case["select"] = legs({
        "same": select(eng.select_dirs_refs4_device, sel256, d_f_same, d_r_same),
        "mixed": select(eng.select_dirs_refs4_device, sel256, d_f_mixed, d_r_mixed),
        "at_64": select(eng.select_dirs_refs_device, sel64, d_f64, d_r64),
        "bi4": lambda: eng.select_dirs4_device(w, h, 1, fp, sel256, dirp1, P(d_mv1[0]), P(d_c1[0]), P(d_mv1[1]), P(d_c1[1]), P(d_f_mixed), None, P(o_f), P(o_d), P(o_s), P(o_c), st)},
        "select")

    # the bi pass of list 0 over its R references against list 1's field and indices; the bi4 sibling: one pair
    t_mv, t_c = torch.zeros((R, n, 593, 2), dtype=torch.int16, device=dev), torch.zeros((R, n, 593), dtype=torch.int32, device=dev)
    t_q, t_qc = torch.zeros((R, n, 593, 2), dtype=torch.int16, device=dev), torch.zeros((R, n, 593), dtype=torch.int32, device=dev)
    d_imv = torch.zeros((R, n, 593, 2), dtype=torch.int16, device=dev)
    o64, r64 = d_f64[1].contiguous(), d_r64[1].contiguous()
    o_same, r_same, o_mixed, r_mixed = d_f_same[1].contiguous(), d_r_same[1].contiguous(), d_f_mixed[1].contiguous(), d_r_mixed[1].contiguous()
    case["search"] = legs({
        "same": lambda: eng.search_frame_bi_refs4_device(cur, l0, l1, fp, P(o_same), P(r_same), None, None, P(t_mv), P(t_c), st),
        "mixed": lambda: eng.search_frame_bi_refs4_device(cur, l0, l1, fp, P(o_mixed), P(r_mixed), None, None, P(t_mv), P(t_c), st),
        "at_64": lambda: eng.search_frame_bi_refs_device(cur, l0, l1, fp, P(o64), P(r64), 64, None, None, P(t_mv), P(t_c), st),
        "bi4": lambda: eng.search_pairs_bi4_device([cur], l0[:1], l1[:1], fp, P(o_mixed), None, None, P(t_mv), P(t_c), st)}, "search")
    case["refine"] = legs({
        "same": lambda: eng.refine_frame_bi_refs4_device(cur, l0, l1, fp, P(o_same), P(r_same), None, None, P(d_imv), 1, P(t_q), P(t_qc), st),
        "mixed": lambda: eng.refine_frame_bi_refs4_device(cur, l0, l1, fp, P(o_mixed), P(r_mixed), None, None, P(d_imv), 1, P(t_q), P(t_qc), st),
        "at_64": lambda: eng.refine_frame_bi_refs_device(cur, l0, l1, fp, P(o64), P(r64), 64, None, None, P(d_imv), 1, P(t_q), P(t_qc), st),
        "bi4": lambda: eng.refine_pairs_bi4_device([cur], l0[:1], l1[:1], fp, P(o_mixed), None, None, P(d_imv), 1, P(t_q), P(t_qc), st)}, "refine")
    out["cases"][f"{R}_refs_per_list"] = case
for p in planes + cplanes:
    p.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
