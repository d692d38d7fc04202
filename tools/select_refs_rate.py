#!/usr/bin/env python3
"""cost of choosing the reference picture per PU at picture size (device-resident tables, torch events): one 2160p picture with four
references, one MV per 8x8 and per 4x4 block

  select_refs_ms   hmme_select_refs_device alone (me_select_refs_kernel: reads the four references' 593-slot tables, writes field,
                   reference indices, slots and CTU costs)
  gb_per_s         the bytes the kernel has to move over select_refs_ms, beside the chip's HBM rate
  replaced_*       what a caller did before the call existed, measured in the same run on the entry points that were there: the four
                   table sets device -> page-locked host memory, the per-slot minimum in numpy (strict compares reference by reference:
                   the lowest index wins ties), the merged tables host -> device, hmme_select_pairs_device on them, the slots device -> host and the numpy gather of
                   the reference index of every block.  No MV cost and no reference price on the host: the route's floor
  predict_refs_ms  hmme_predict_refs_device with the field and reference indices just decided, beside predict_pairs_x4_ms:
                   hmme_predict_pairs_device for four whole pictures, what a caller had to run before cutting the prediction together on
                   the host (that cut is not timed)

REPS (default 7) repeats of each from a warm clock; median, min and max.  usage: tools/select_refs_rate.py [out.json]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hm-opencl_amd"))
import numpy as np
import torch
from hmme import api

REPS = int(os.environ.get("REPS", "7"))
N_REFS = int(os.environ.get("N_REFS", "4"))
w, h = (int(v) for v in os.environ.get("SIZE", "3840x2160").split("x"))
HBM_TBS = {"spec": 8.0, "measured_copy": 6.29}   # MI355X: HBM3E peak and what a float4 copy reaches
dev = torch.device("cuda", 0)
eng = api.Engine(0, 64); eng.set_lambda(57.9)
n = api.load().hmme_num_ctus(w, h)
st = torch.cuda.current_stream().cuda_stream
fp = api.FrameParams(1, 0, 8, 0, n)
ref_cost = [(eng.lambda_q16 * api.ref_idx_bits(N_REFS, r)) >> 16 for r in range(N_REFS)]


def stats(t, nd=4):
    return {"median": round(statistics.median(t), nd), "min": round(min(t), nd), "max": round(max(t), nd)}


def timed(fn):
    """REPS single launches, each between its own pair of events -> ms"""
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


out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "n_ctu": n, "n_refs": N_REFS, "ref_cost": ref_cost, "reps": REPS,
       "hbm_tb_per_s": HBM_TBS, "cases": []}
g = torch.Generator(device=dev); g.manual_seed(1)
d_mv = torch.randint(-800, 801, (N_REFS, n, 593, 2), generator=g, device=dev, dtype=torch.int16)
d_cost = torch.randint(0, 1 << 20, (N_REFS, n, 593), generator=g, device=dev, dtype=torch.int32)
h_mv = torch.empty(d_mv.shape, dtype=d_mv.dtype, pin_memory=True)
h_cost = torch.empty(d_cost.shape, dtype=d_cost.dtype, pin_memory=True)
h_mmv = torch.empty(d_mv.shape[1:], dtype=d_mv.dtype, pin_memory=True)       # the merged tables of the replaced route
h_mcost = torch.empty(d_cost.shape[1:], dtype=d_cost.dtype, pin_memory=True)
d_mmv, d_mcost = torch.zeros_like(d_mv[0]), torch.zeros_like(d_cost[0])
best = np.zeros((n, 593), np.int64)
for per in (64, 256):
    sel = api.SelectParams(per)
    d_field = torch.zeros((1, n, per, 2), dtype=torch.int16, device=dev)
    d_ref = torch.zeros((1, n, per), dtype=torch.uint8, device=dev)
    d_slot = torch.zeros((1, n, per), dtype=torch.int16, device=dev)
    d_cc = torch.zeros((1, n), dtype=torch.int32, device=dev)
    run = lambda: eng.select_refs_device(w, h, 1, N_REFS, fp, sel, ref_cost, d_mv.data_ptr(), d_cost.data_ptr(), None, d_field.data_ptr(), d_ref.data_ptr(),
                                         d_slot.data_ptr(), d_cc.data_ptr(), st)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    case = {"mv_per_ctu": per}
    case["select_refs_ms"] = timed(run)
    moved = n * (N_REFS * 593 * 8 + per * 7 + 4)
    case["bytes_moved"] = moved
    case["gb_per_s"] = round(moved / case["select_refs_ms"]["median"] * 1e-6, 1)
    case["of_hbm_measured_copy"] = round(case["gb_per_s"] / (HBM_TBS["measured_copy"] * 1e3), 3)

    # the replaced route, on the entry points that existed before
    d_field2, d_slot2, d_cc2 = torch.zeros_like(d_field), torch.zeros_like(d_slot), torch.zeros_like(d_cc)
    h_slot = torch.empty(d_slot2.shape, dtype=torch.int16, pin_memory=True)
    h_ref = np.zeros((n, per), np.uint8)

    def down():
        h_mv.copy_(d_mv, non_blocking=True); h_cost.copy_(d_cost, non_blocking=True)

    def merge():   # reference by reference, masked copies of costs, MV dwords and indices: several times faster than argmin + take_along_axis
        c, m = h_cost.numpy(), h_mv.numpy().view(np.int32)[..., 0]
        bc, bm = h_mcost.numpy(), h_mmv.numpy().view(np.int32)[..., 0]
        bc[...] = c[0]; bm[...] = m[0]; best[...] = 0
        for r in range(1, N_REFS):
            lt = c[r] < bc                                  # strict: the lowest index wins ties
            np.copyto(bc, c[r], where=lt); np.copyto(bm, m[r], where=lt); np.copyto(best, r, where=lt)

    def up():
        d_mmv.copy_(h_mmv, non_blocking=True); d_mcost.copy_(h_mcost, non_blocking=True)

    sel_run = lambda: eng.select_pairs_device(w, h, 1, fp, sel, d_mmv.data_ptr(), d_mcost.data_ptr(), None, d_field2.data_ptr(), d_slot2.data_ptr(), d_cc2.data_ptr(), st)

    def gather():
        h_slot.copy_(d_slot2[0:1], non_blocking=True)
        torch.cuda.synchronize()
        s = h_slot.numpy()[0].view(np.uint16).astype(np.int64)
        none = s == 0xFFFF
        h_ref[...] = np.where(none, 0xFF, np.take_along_axis(best, np.where(none, 0, s), axis=1))

    down(); torch.cuda.synchronize(); merge(); up(); sel_run(); gather()
    case["replaced_download_ms"] = wall(down)
    case["replaced_numpy_min_ms"] = wall(merge)
    case["replaced_upload_ms"] = wall(up)
    case["replaced_select_pairs_ms"] = timed(sel_run)
    case["replaced_ref_gather_ms"] = wall(gather)
    case["replaced_total_ms"] = round(sum(case[k]["median"] for k in case if k.startswith("replaced_")), 3)
    out["cases"].append(case)

# prediction: the field and reference indices of a decision with one MV per 8x8 block
sel = api.SelectParams(64)
d_field = torch.zeros((1, n, 64, 2), dtype=torch.int16, device=dev)
d_ref = torch.zeros((1, n, 64), dtype=torch.uint8, device=dev)
d_mv.clamp_(-40, 40)   # quarter-pel MVs of a plausible size (all 16 phases)
eng.select_refs_device(w, h, 1, N_REFS, fp, sel, ref_cost, d_mv.data_ptr(), d_cost.data_ptr(), None, d_field.data_ptr(), d_ref.data_ptr(), None, None, st)
torch.cuda.synchronize()
rng = np.random.default_rng(3)
planes = []
for r in range(N_REFS):
    p = eng.plane(w, h)
    p.upload_u8(rng.integers(0, 256, size=(h, w), dtype=np.uint8))
    planes.append(p)
d_img = torch.zeros((h, w), dtype=torch.uint8, device=dev)
d_imgs = [torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(N_REFS)]
d_fields = d_field.expand(N_REFS, n, 64, 2).contiguous()
pfp = api.FrameParams(1, 0, 8, 0, n)
one = lambda: eng.predict_refs_device(planes, pfp, d_field.data_ptr(), d_ref.data_ptr(), 64, d_img.data_ptr(), w, st)
four = lambda: eng.predict_pairs_device(planes, pfp, d_fields.data_ptr(), 64, [t.data_ptr() for t in d_imgs], w, st)
for _ in range(3):
    one(); four()
torch.cuda.synchronize()
out["predict"] = {"predict_refs_ms": timed(one), f"predict_pairs_x{N_REFS}_ms": timed(four),
                  "blocks_per_reference": np.bincount(d_ref.cpu().numpy().reshape(-1), minlength=256)[:N_REFS].tolist()}
for p in planes:
    p.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
