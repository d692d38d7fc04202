#!/usr/bin/env python3
"""cost of choosing L0, L1 or bi per PU at picture size (device-resident tables, torch events): one 2160p B picture, four 593-slot table
sets, one MV per 8x8 block

  select_dirs_ms   hmme_select_dirs_device alone (me_select_dirs_kernel: reads the four table sets and the lists' fields, writes the
                   two-list field, directions, slots and CTU costs)
  gb_per_s         the bytes the kernel has to move over select_dirs_ms, beside the chip's HBM rate
  replaced_*       what a caller did before the call existed, measured in the same run: the four table sets device -> page-locked host
                   memory, HM's recombination floor(0.5 * (cost - mvcost)) + getCost(bits) and the three-way comparison per slot in numpy,
                   the merged tables (winner's MV and cost) host -> device.  The partition on the merged tables and the cut of the field
                   are not timed: the route's floor
  predict_bi_ms    hmme_predict_bi_device with the field and directions just decided, beside replaced_predict_*: hmme_predict_pairs_device
                   for the two lists' whole pictures, both device -> host, and the rounded average in numpy (which is not even addAvg: the
                   host has no 14-bit intermediates)

REPS (default 7) repeats of each from a warm clock; median, min and max.  usage: tools/select_dirs_rate.py [out.json]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hm-opencl_amd"))
import numpy as np
import torch
from hmme import api

REPS = int(os.environ.get("REPS", "7"))
w, h = (int(v) for v in os.environ.get("SIZE", "3840x2160").split("x"))
HBM_TBS = {"spec": 8.0, "measured_copy": 6.29}   # MI355X: HBM3E peak and what a float4 copy reaches
DIR_BITS, LIST_BITS = (3, 3, 5), (2, 1)
dev = torch.device("cuda", 0)
eng = api.Engine(0, 64); eng.set_lambda(57.9)
lq = eng.lambda_q16
n = api.load().hmme_num_ctus(w, h)
st = torch.cuda.current_stream().cuda_stream
fp = api.FrameParams(1, 0, 8, 0, n)
sel = api.SelectParams(64)
dirs = [api.DirParams(DIR_BITS, LIST_BITS)]


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


out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "n_ctu": n, "dir_bits": DIR_BITS, "list_bits": LIST_BITS, "reps": REPS,
       "hbm_tb_per_s": HBM_TBS}
g = torch.Generator(device=dev); g.manual_seed(1)
d_mv = torch.randint(-40, 41, (2, 2, n, 593, 2), generator=g, device=dev, dtype=torch.int16)        # [uni | bi][list]: quarter-pel MVs of a plausible size
d_cost = torch.randint(1 << 12, 1 << 20, (2, 2, n, 593), generator=g, device=dev, dtype=torch.int32)
d_cost[1] *= 2                                                                                      # the bi pass's distortion is halved by the rule
d_uni = torch.randint(-40, 41, (2, n, 64, 2), generator=g, device=dev, dtype=torch.int16)
d_field = torch.zeros((1, 2, n, 64, 2), dtype=torch.int16, device=dev)
d_dir = torch.zeros((1, n, 64), dtype=torch.uint8, device=dev)
d_slot = torch.zeros((1, n, 64), dtype=torch.int16, device=dev)
d_cc = torch.zeros((1, n), dtype=torch.int32, device=dev)
run = lambda: eng.select_dirs_device(w, h, 1, fp, sel, dirs, d_mv[0].data_ptr(), d_cost[0].data_ptr(), d_mv[1].data_ptr(), d_cost[1].data_ptr(), d_uni.data_ptr(), None,
                                     d_field.data_ptr(), d_dir.data_ptr(), d_slot.data_ptr(), d_cc.data_ptr(), st)
for _ in range(3):
    run()
torch.cuda.synchronize()
case = {"select_dirs_ms": timed(run)}
moved = n * (4 * 593 * 8 + 2 * 64 * 4 + 2 * 64 * 4 + 64 * 3 + 4)
case["bytes_moved"] = moved
case["gb_per_s"] = round(moved / case["select_dirs_ms"]["median"] * 1e-6, 1)
case["of_hbm_measured_copy"] = round(case["gb_per_s"] / (HBM_TBS["measured_copy"] * 1e3), 3)

# the replaced route
h_mv = torch.empty(d_mv.shape, dtype=d_mv.dtype, pin_memory=True)
h_cost = torch.empty(d_cost.shape, dtype=d_cost.dtype, pin_memory=True)
h_mmv = torch.empty((n, 593, 2), dtype=torch.int16, pin_memory=True)
h_mcost = torch.empty((n, 593), dtype=torch.int32, pin_memory=True)
h_mdir = np.zeros((n, 593), np.uint8)
d_mmv, d_mcost = torch.zeros((n, 593, 2), dtype=torch.int16, device=dev), torch.zeros((n, 593), dtype=torch.int32, device=dev)


def down():
    h_mv.copy_(d_mv, non_blocking=True); h_cost.copy_(d_cost, non_blocking=True)


def bits(v):   # the exp-Golomb length of an MV difference, predictor (0,0)
    t = np.where(v <= 0, 1 - 2 * v, 2 * v).astype(np.float64)
    return 2 * (np.frexp(t)[1] - 1) + 1


def gc(nbits):
    return ((lq * nbits.astype(np.uint64)) & 0xFFFFFFFF) >> 16


def recombine():
    mv, cost = h_mv.numpy().astype(np.int64), h_cost.numpy().view(np.uint32).astype(np.int64)
    b = bits(mv[..., 0]) + bits(mv[..., 1])                                                         # [2, 2, n, 593]
    dist = np.maximum(cost - gc(b).astype(np.int64), 0)
    c = [dist[0, l] + gc(DIR_BITS[l] + LIST_BITS[l] + b[0, l]).astype(np.int64) for l in range(2)]
    cb = [(dist[1, l] >> 1) + gc(DIR_BITS[2] + sum(LIST_BITS) + b[1, l] + b[0, 1 - l]).astype(np.int64) for l in range(2)]
    bl = cb[1] < cb[0]
    cbi = np.where(bl, cb[1], cb[0])
    is_bi = (cbi <= c[0]) & (cbi <= c[1])
    is_l0 = ~is_bi & (c[0] <= c[1])
    h_mdir[...] = np.where(is_bi, 3, np.where(is_l0, 1, 2))
    h_mcost.numpy()[...] = np.minimum(np.where(is_bi, cbi, np.where(is_l0, c[0], c[1])), 0x7FFFFFFF)
    m = h_mv.numpy().view(np.int32)[..., 0]
    h_mmv.numpy().view(np.int32)[..., 0] = np.where(is_bi, np.where(bl, m[1, 1], m[1, 0]), np.where(is_l0, m[0, 0], m[0, 1]))


def up():
    d_mmv.copy_(h_mmv, non_blocking=True); d_mcost.copy_(h_mcost, non_blocking=True)


down(); torch.cuda.synchronize(); recombine(); up()
case["replaced_download_ms"] = wall(down)
case["replaced_numpy_recombine_ms"] = wall(recombine)
case["replaced_upload_ms"] = wall(up)
case["replaced_total_ms"] = round(sum(case[k]["median"] for k in case if k.startswith("replaced_")), 3)
out["select"] = case

# prediction: the field and directions just decided
run(); torch.cuda.synchronize()
rng = np.random.default_rng(3)
planes = []
for r in range(2):
    p = eng.plane(w, h)
    p.upload_u8(rng.integers(0, 256, size=(h, w), dtype=np.uint8))
    planes.append(p)
d_img = torch.zeros((h, w), dtype=torch.uint8, device=dev)
d_imgs = [torch.zeros((h, w), dtype=torch.uint8, device=dev) for _ in range(2)]
h_imgs = [torch.empty((h, w), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
h_avg = np.zeros((h, w), np.uint8)
bi = lambda: eng.predict_bi_device([planes[0]], [planes[1]], fp, d_field.data_ptr(), d_dir.data_ptr(), 64, [d_img.data_ptr()], w, st)
two = lambda: eng.predict_pairs_device(planes, fp, d_field.data_ptr(), 64, [t.data_ptr() for t in d_imgs], w, st)


def down_imgs():
    for a, b in zip(h_imgs, d_imgs):
        a.copy_(b, non_blocking=True)


def average():
    h_avg[...] = (h_imgs[0].numpy().astype(np.uint16) + h_imgs[1].numpy() + 1) >> 1


for _ in range(3):
    bi(); two()
down_imgs(); torch.cuda.synchronize(); average()
pred = {"predict_bi_ms": timed(bi), "replaced_predict_pairs_x2_ms": timed(two), "replaced_download_ms": wall(down_imgs), "replaced_numpy_average_ms": wall(average),
        "blocks_per_direction": np.bincount(d_dir.cpu().numpy().reshape(-1), minlength=256)[[1, 2, 3, 255]].tolist()}
pred["replaced_total_ms"] = round(sum(pred[k]["median"] for k in pred if k.startswith("replaced_")), 3)
out["predict"] = pred
for p in planes:
    p.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
