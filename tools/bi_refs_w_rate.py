#!/usr/bin/env python3
"""cost of the explicit-weight and 4:2:0 forms of a multi-reference B picture at picture size (device-resident buffers, torch events): one
2160p B picture with 2 and with 4 references per list, one MV per 8x8 block, random fields that name every reference.  Four legs per
reference count, each beside its unweighted / single-reference sibling in the same run:

  luma       hmme_predict_bi_refs_w_device beside hmme_predict_bi_refs_device (the same fields; me_predict_bi_kernel<T, 2, 1> beside <T, 0, 1>)
  chroma     hmme_predict_chroma_bi_refs_device, with and without weights, beside hmme_predict_chroma_bi_device on index-0 fields -- where the
             two write the same images, which is checked
  bi_search  hmme_search_frame_bi_refs_w_device beside hmme_search_frame_bi_refs_device at fen = 0; bi range 4
  bi_refine  hmme_refine_frame_bi_refs_w_device beside hmme_refine_frame_bi_refs_device: every reference its own weight, so one refinement
             launch per reference beside one launch in all

REPS (default 7) repeats of each from a warm clock; median, min and max.  usage: tools/bi_refs_w_rate.py [out.json]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hm-opencl_amd"))
import numpy as np
import torch
from hmme import api

REPS = int(os.environ.get("REPS", "7"))
w, h = (int(v) for v in os.environ.get("SIZE", "3840x2160").split("x"))
dev = torch.device("cuda", 0)
eng = api.Engine(0, 64); eng.set_lambda(57.9)
n = api.load().hmme_num_ctus(w, h)
st = torch.cuda.current_stream().cuda_stream
fp = api.FrameParams(1, 0, 8, 0, n)
fp_bi = api.FrameParams(4, 0, 8, 0, n)
# (w0, offset, shift, round): HM-like fades, no two equal; Cr of another denominator than Cb
LUMA = [(70, -9, 6, 32), (55, 14, 6, 32), (61, 3, 6, 32), (80, -20, 6, 32), (40, -5, 6, 32), (90, 11, 6, 32), (66, 1, 6, 32), (50, 25, 6, 32)]
CB = [(60 + 3 * k, 2 * k - 7, 6, 32) for k in range(8)]
CR = [(30 + 2 * k, 5 - k, 5, 16) for k in range(8)]


def stats(t, nd=4):
    return {"median": round(statistics.median(t), nd), "min": round(min(t), nd), "max": round(max(t), nd)}


def timed(fn):
    """REPS single calls, each between its own pair of events -> ms"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) for a, b in ev])


def beside(new, old, names):
    """both warmed, then new, old, new again"""
    for _ in range(3):
        new(); old()
    torch.cuda.synchronize()
    r = {names[0] + "_ms": timed(new), names[1] + "_ms": timed(old), names[0] + "_ms_again": timed(new)}
    r["ratio_of_medians"] = round(min(r[names[0] + "_ms"]["median"], r[names[0] + "_ms_again"]["median"]) / r[names[1] + "_ms"]["median"], 3)
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
out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "n_ctu": n, "reps": REPS, "cases": {}}
for R in (2, 4):
    g = torch.Generator(device=dev); g.manual_seed(R)
    d_field = torch.randint(-40, 41, (2, n, 64, 2), generator=g, device=dev, dtype=torch.int16)
    d_dir = torch.randint(1, 4, (n, 64), generator=g, device=dev, dtype=torch.uint8)
    d_ref = torch.randint(0, R, (2, n, 64), generator=g, device=dev, dtype=torch.uint8)
    d_zero = torch.zeros((2, n, 64), dtype=torch.uint8, device=dev)
    d_img, d_img2 = (torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(2))
    d_c = [torch.zeros((h // 2, w // 2), dtype=torch.uint8, device=dev) for _ in range(4)]
    w0, w1 = LUMA[:R], LUMA[4:4 + R]
    case = {"blocks_per_direction": np.bincount(d_dir.cpu().numpy().reshape(-1), minlength=4)[1:4].tolist()}

    # luma: the same fields with and without weights
    weighted = lambda: eng.predict_bi_refs_w_device(lists[0][:R], lists[1][:R], fp, w0, w1, d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), 64, d_img.data_ptr(), w, st)
    plain = lambda: eng.predict_bi_refs_device(lists[0][:R], lists[1][:R], fp, d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), 64, d_img2.data_ptr(), w, st)
    case["luma"] = beside(weighted, plain, ("predict_bi_refs_w", "predict_bi_refs"))
    # ... and identities through the _w call are the unweighted picture
    eng.predict_bi_refs_w_device(lists[0][:R], lists[1][:R], fp, [(64, 0, 6, 32)] * R, [(64, 0, 6, 0)] * R, d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), 64,
                                 d_img.data_ptr(), w, st)
    torch.cuda.synchronize()
    case["luma"]["identities_equal_the_unweighted_picture"] = bool(torch.equal(d_img, d_img2))

    # chroma: per-block references, with and without weights, beside the single-reference call on index-0 fields
    c0, c1 = clists[0][:2 * R], clists[1][:2 * R]
    cw0 = [x for k in range(R) for x in (CB[k], CR[k])]
    cw1 = [x for k in range(R) for x in (CB[4 + k], CR[4 + k])]
    refs_w = lambda: eng.predict_chroma_bi_refs_device(c0, c1, w, h, fp, d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), 64, d_c[0].data_ptr(), d_c[1].data_ptr(),
                                                       w // 2, weights0=cw0, weights1=cw1, stream=st)
    refs_plain = lambda: eng.predict_chroma_bi_refs_device(c0, c1, w, h, fp, d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), 64, d_c[0].data_ptr(),
                                                           d_c[1].data_ptr(), w // 2, stream=st)
    refs_zero = lambda: eng.predict_chroma_bi_refs_device(c0, c1, w, h, fp, d_field.data_ptr(), d_dir.data_ptr(), d_zero.data_ptr(), 64, d_c[0].data_ptr(),
                                                          d_c[1].data_ptr(), w // 2, stream=st)
    single = lambda: eng.predict_chroma_bi_device(c0[:2], c1[:2], w, h, fp, d_field.data_ptr(), d_dir.data_ptr(), 64, [d_c[2].data_ptr(), d_c[3].data_ptr()], w // 2,
                                                  stream=st)
    case["chroma"] = beside(refs_zero, single, ("predict_chroma_bi_refs_index_0", "predict_chroma_bi"))
    case["chroma"]["equal_images_at_index_0"] = bool(torch.equal(d_c[0], d_c[2])) and bool(torch.equal(d_c[1], d_c[3]))
    case["chroma"].update({"predict_chroma_bi_refs_ms": timed(refs_plain), "predict_chroma_bi_refs_weighted_ms": timed(refs_w), "predict_chroma_bi_ms_again": timed(single)})

    # the bi pass of list 0 over its R references against list 1's field and indices
    tabs = [(torch.zeros((R, n, 593, 2), dtype=torch.int16, device=dev), torch.zeros((R, n, 593), dtype=torch.int32, device=dev)) for _ in range(4)]
    (mv_w, sad_w), (mv_u, sad_u), (q_w, c_w), (q_u, c_u) = tabs
    s_w = lambda: eng.search_frame_bi_refs_w_device(cur, lists[0][:R], lists[1][:R], fp_bi, w0, w1, d_field[1].data_ptr(), d_ref[1].data_ptr(), 64, None, None,
                                                    mv_w.data_ptr(), sad_w.data_ptr(), st)
    s_u = lambda: eng.search_frame_bi_refs_device(cur, lists[0][:R], lists[1][:R], fp_bi, d_field[1].data_ptr(), d_ref[1].data_ptr(), 64, None, None, mv_u.data_ptr(),
                                                  sad_u.data_ptr(), st)
    case["bi_search"] = beside(s_w, s_u, ("search_frame_bi_refs_w", "search_frame_bi_refs"))
    r_w = lambda: eng.refine_frame_bi_refs_w_device(cur, lists[0][:R], lists[1][:R], fp_bi, w0, w1, d_field[1].data_ptr(), d_ref[1].data_ptr(), 64, None, None,
                                                    mv_w.data_ptr(), 1, q_w.data_ptr(), c_w.data_ptr(), st)
    r_u = lambda: eng.refine_frame_bi_refs_device(cur, lists[0][:R], lists[1][:R], fp_bi, d_field[1].data_ptr(), d_ref[1].data_ptr(), 64, None, None, mv_u.data_ptr(), 1,
                                                  q_u.data_ptr(), c_u.data_ptr(), st)
    case["bi_refine"] = beside(r_w, r_u, ("refine_frame_bi_refs_w", "refine_frame_bi_refs"))
    # identities through the _w calls are the unweighted tables at fen = 0
    ids = [(64, 0, 6, 32)] * R
    eng.search_frame_bi_refs_w_device(cur, lists[0][:R], lists[1][:R], fp_bi, ids, ids, d_field[1].data_ptr(), d_ref[1].data_ptr(), 64, None, None, mv_w.data_ptr(),
                                      sad_w.data_ptr(), st)
    torch.cuda.synchronize()
    case["bi_search"]["identities_equal_the_unweighted_tables"] = bool(torch.equal(mv_w, mv_u)) and bool(torch.equal(sad_w, sad_u))
    out["cases"][f"{R}_refs_per_list"] = case
for p in planes + cplanes:
    p.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
