#!/usr/bin/env python3
"""cost of a B picture with several references per list at picture size (device-resident buffers, torch events): one 2160p B picture with
2 and with 4 references per list, one MV per 8x8 block.  Three legs per reference count:

  select     hmme_select_dirs_refs_device alone (me_select_dirs_refs_kernel: reads 4 n table sets, the lists' fields and reference indices,
             writes the two-list field, the two reference fields, directions, slots and CTU costs), the bytes it has to move over its time
             beside the chip's HBM rate -- and replaced_*: what a caller did before the call existed, in the same run: all table sets device ->
             page-locked host memory, the rule's per-reference recombination and minima and the three-way comparison per slot in numpy, the
             merged tables host -> device.  The partition on the merged tables and the cut of the fields are not timed: the route's floor
  predict    hmme_predict_bi_refs_device with the fields just decided, beside hmme_predict_bi_device's time for the same picture (the same
             field and directions, one plane per list)
  bi_pass    hmme_search_frame_bi_refs_device over the n references of a list (ONE origin) beside n single-pair hmme_search_pairs_bi_device
             calls that each rebuild the origin; bi range 4, FEN on

REPS (default 7) repeats of each from a warm clock; median, min and max.  usage: tools/select_dirs_refs_rate.py [out.json]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hm-opencl_amd"))
import numpy as np
import torch
from hmme import api

REPS = int(os.environ.get("REPS", "7"))
w, h = (int(v) for v in os.environ.get("SIZE", "3840x2160").split("x"))
HBM_TBS = {"spec": 8.0, "measured_copy": 6.29}   # MI355X: HBM3E peak and what a float4 copy reaches
DIR_BITS = (3, 3, 5)
dev = torch.device("cuda", 0)
eng = api.Engine(0, 64); eng.set_lambda(57.9)
lq = eng.lambda_q16
n = api.load().hmme_num_ctus(w, h)
st = torch.cuda.current_stream().cuda_stream
fp = api.FrameParams(1, 0, 8, 0, n)
fp_bi = api.FrameParams(4, 1, 8, 0, n)
sel = api.SelectParams(64)


def stats(t, nd=4):
    return {"median": round(statistics.median(t), nd), "min": round(min(t), nd), "max": round(max(t), nd)}


def timed(fn):
    """REPS single calls, each between its own pair of events -> ms"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) for a, b in ev])


def wall(fn):
    t = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return stats(t, 3)


def bits(v):   # the exp-Golomb length of an MV difference, predictor (0,0)
    t = np.where(v <= 0, 1 - 2 * v, 2 * v).astype(np.float64)
    return 2 * (np.frexp(t)[1] - 1) + 1


def gc(nbits):
    return ((lq * nbits.astype(np.uint64)) & 0xFFFFFFFF) >> 16


rng = np.random.default_rng(3)
planes = []
for r in range(9):                                                                                   # the current picture, 4 + 4 references
    p = eng.plane(w, h)
    p.upload_u8(rng.integers(0, 256, size=(h, w), dtype=np.uint8))
    planes.append(p)
cur, lists = planes[0], (planes[1:5], planes[5:9])
out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "n_ctu": n, "dir_bits": DIR_BITS, "reps": REPS, "hbm_tb_per_s": HBM_TBS,
       "cases": {}}
for R in (2, 4):
    ref_bits = [api.ref_idx_bits(R, r) + 1 for r in range(R)]
    dirs = [api.DirRefsParams(DIR_BITS, (R, R), (ref_bits, ref_bits))]
    g = torch.Generator(device=dev); g.manual_seed(R)
    d_mv = torch.randint(-40, 41, (2, 2, R, n, 593, 2), generator=g, device=dev, dtype=torch.int16)   # [uni | bi][list][reference]
    d_cost = torch.randint(1 << 12, 1 << 20, (2, 2, R, n, 593), generator=g, device=dev, dtype=torch.int32)
    d_cost[1] *= 2                                                                                   # the bi pass's distortion is halved by the rule
    d_uni = torch.randint(-40, 41, (2, n, 64, 2), generator=g, device=dev, dtype=torch.int16)
    d_uref = torch.randint(0, R, (2, n, 64), generator=g, device=dev, dtype=torch.uint8)
    d_field = torch.zeros((1, 2, n, 64, 2), dtype=torch.int16, device=dev)
    d_ref = torch.zeros((1, 2, n, 64), dtype=torch.uint8, device=dev)
    d_dir = torch.zeros((1, n, 64), dtype=torch.uint8, device=dev)
    d_slot = torch.zeros((1, n, 64), dtype=torch.int16, device=dev)
    d_cc = torch.zeros((1, n), dtype=torch.int32, device=dev)
    run = lambda: eng.select_dirs_refs_device(w, h, 1, R, fp, sel, dirs, d_mv[0].data_ptr(), d_cost[0].data_ptr(), d_mv[1].data_ptr(), d_cost[1].data_ptr(),
                                              d_uni.data_ptr(), d_uref.data_ptr(), None, d_field.data_ptr(), d_ref.data_ptr(), d_dir.data_ptr(), d_slot.data_ptr(),
                                              d_cc.data_ptr(), st)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    case = {"select_dirs_refs_ms": timed(run)}
    moved = n * (4 * R * 593 * 8 + 2 * 64 * 5 + 2 * 64 * 5 + 64 * 3 + 4)
    case["bytes_moved"] = moved
    case["gb_per_s"] = round(moved / case["select_dirs_refs_ms"]["median"] * 1e-6, 1)
    case["of_hbm_measured_copy"] = round(case["gb_per_s"] / (HBM_TBS["measured_copy"] * 1e3), 3)

    # the replaced route
    h_mv = torch.empty(d_mv.shape, dtype=d_mv.dtype, pin_memory=True)
    h_cost = torch.empty(d_cost.shape, dtype=d_cost.dtype, pin_memory=True)
    h_mmv = torch.empty((n, 593, 2), dtype=torch.int16, pin_memory=True)
    h_mcost = torch.empty((n, 593), dtype=torch.int32, pin_memory=True)
    h_mdir, h_mref = np.zeros((n, 593), np.uint8), np.zeros((2, n, 593), np.uint8)
    d_mmv, d_mcost = torch.zeros((n, 593, 2), dtype=torch.int16, device=dev), torch.zeros((n, 593), dtype=torch.int32, device=dev)
    rb = np.array(ref_bits, np.int64)[None, :, None, None]

    def down():
        h_mv.copy_(d_mv, non_blocking=True); h_cost.copy_(d_cost, non_blocking=True)

    def recombine():
        mv, cost = h_mv.numpy().astype(np.int64), h_cost.numpy().view(np.uint32).astype(np.int64)
        b = bits(mv[..., 0]) + bits(mv[..., 1])                                                      # [2, 2, R, n, 593]
        dist = np.maximum(cost - gc(b).astype(np.int64), 0)
        dbits = np.array(DIR_BITS[:2], np.int64)[:, None, None, None]
        c = dist[0] + gc(dbits + rb + b[0]).astype(np.int64)                                         # [2, R, n, 593]
        ru = c.argmin(axis=1)                                                                        # the first minimum: the lowest index wins ties
        cu = np.take_along_axis(c, ru[:, None], 1)[:, 0]
        mot = np.take_along_axis(rb + b[0], ru[:, None], 1)[:, 0]                                    # [2, n, 593]
        cb = (dist[1] >> 1) + gc(DIR_BITS[2] + rb + b[1] + mot[::-1][:, None]).astype(np.int64)
        rbi = cb.argmin(axis=1)
        cbl = np.take_along_axis(cb, rbi[:, None], 1)[:, 0]
        bl = cbl[1] < cbl[0]
        cbi = np.where(bl, cbl[1], cbl[0])
        is_bi = (cbi <= cu[0]) & (cbi <= cu[1])                                                      # (the whole mask: every reference of list 1 may win)
        is_l0 = ~is_bi & (cu[0] <= cu[1])
        h_mdir[...] = np.where(is_bi, 3, np.where(is_l0, 1, 2))
        h_mref[0] = np.where(is_bi, rbi[0], ru[0]); h_mref[1] = np.where(is_bi, rbi[1], ru[1])
        h_mcost.numpy()[...] = np.minimum(np.where(is_bi, cbi, np.where(is_l0, cu[0], cu[1])), 0x7FFFFFFF)
        m = h_mv.numpy().view(np.int32)[..., 0]                                                      # [2, 2, R, n, 593]
        pick = lambda t, l, idx: np.take_along_axis(m[t, l], idx[None], 0)[0]
        h_mmv.numpy().view(np.int32)[..., 0] = np.where(is_bi, np.where(bl, pick(1, 1, rbi[1]), pick(1, 0, rbi[0])), np.where(is_l0, pick(0, 0, ru[0]), pick(0, 1, ru[1])))

    def up():
        d_mmv.copy_(h_mmv, non_blocking=True); d_mcost.copy_(h_mcost, non_blocking=True)

    down(); torch.cuda.synchronize(); recombine(); up()
    case["replaced_download_ms"] = wall(down)
    case["replaced_numpy_recombine_ms"] = wall(recombine)
    case["replaced_upload_ms"] = wall(up)
    case["replaced_total_ms"] = round(sum(case[k]["median"] for k in case if k.startswith("replaced_")), 3)
    # the decision itself agrees with the route it replaces on every slot a CU of the field was cut from
    run(); torch.cuda.synchronize()
    slot = d_slot.cpu().numpy().view(np.uint16)[0]
    live = slot != 0xFFFF
    ctu_of = np.broadcast_to(np.arange(n)[:, None], slot.shape)
    case["directions_agree_with_the_numpy_route"] = bool((h_mdir[ctu_of[live], slot[live]] == d_dir.cpu().numpy()[0][live]).all())

    # prediction: the fields just decided
    d_img = torch.zeros((h, w), dtype=torch.uint8, device=dev)
    refs_call = lambda: eng.predict_bi_refs_device(lists[0][:R], lists[1][:R], fp, d_field.data_ptr(), d_dir.data_ptr(), d_ref.data_ptr(), 64, d_img.data_ptr(), w, st)
    one_call = lambda: eng.predict_bi_device(lists[0][:1], lists[1][:1], fp, d_field.data_ptr(), d_dir.data_ptr(), 64, [d_img.data_ptr()], w, st)
    for _ in range(3):
        refs_call(); one_call()
    torch.cuda.synchronize()
    pred = {"predict_bi_refs_ms": timed(refs_call), "predict_bi_ms": timed(one_call), "predict_bi_refs_ms_again": timed(refs_call),
            "blocks_per_direction": np.bincount(d_dir.cpu().numpy().reshape(-1), minlength=256)[[1, 2, 3, 255]].tolist()}

    # the bi pass of list 0 over its R references against list 1's field and indices
    d_bmv = torch.zeros((R, n, 593, 2), dtype=torch.int16, device=dev)
    d_bsad = torch.zeros((R, n, 593), dtype=torch.int32, device=dev)
    d_bmv1 = torch.zeros((R, n, 593, 2), dtype=torch.int16, device=dev)
    d_bsad1 = torch.zeros((R, n, 593), dtype=torch.int32, device=dev)
    d_zero = torch.zeros((n, 64), dtype=torch.uint8, device=dev)
    joint = lambda: eng.search_frame_bi_refs_device(cur, lists[0][:R], lists[1][:R], fp_bi, d_uni[1].data_ptr(), d_uref[1].data_ptr(), 64, None, None, d_bmv.data_ptr(),
                                                    d_bsad.data_ptr(), st)

    def singles():
        for r in range(R):
            eng.search_pairs_bi_device([cur], [lists[0][r]], [lists[1][0]], fp_bi, d_uni[1].data_ptr(), 64, None, None, d_bmv1[r].data_ptr(), d_bsad1[r].data_ptr(), st)

    for _ in range(3):
        joint(); singles()
    torch.cuda.synchronize()
    bi = {"search_frame_bi_refs_ms": timed(joint), "single_pair_calls_ms": timed(singles), "search_frame_bi_refs_ms_again": timed(joint)}
    # with index 0 everywhere the joint call IS the single-pair calls: the same tables
    eng.search_frame_bi_refs_device(cur, lists[0][:R], lists[1][:R], fp_bi, d_uni[1].data_ptr(), d_zero.data_ptr(), 64, None, None, d_bmv.data_ptr(), d_bsad.data_ptr(), st)
    torch.cuda.synchronize()
    bi["equal_tables_at_index_0"] = bool(torch.equal(d_bmv, d_bmv1)) and bool(torch.equal(d_bsad, d_bsad1))
    out["cases"][f"{R}_refs_per_list"] = {"select": case, "predict": pred, "bi_pass": bi}
for p in planes:
    p.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
