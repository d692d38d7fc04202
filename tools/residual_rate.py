#!/usr/bin/env python3
"""cost of the residual / distortion pass at picture size (device-resident planes, images and slot maps, torch events): 2160p, 8- and 10-bit,
64 and 256 blocks per CTU, Hadamard and SAD, with and without the residual image

  residual_ms   hmme_residual_pairs_device alone (me_residual_kernel: reads the current picture's CTU blocks, the predicted image and the slot
                map, writes PU errors, CU SSEs, CTU sums and -- with_residual -- the int16 image)
  residual_ms_back_to_back   the same per launch of 50 enqueued back to back between one pair of events
  gb_per_s      the bytes the kernel has to move over residual_ms, beside the chip's HBM rate
  host_route_*  the route it replaces, timed in the same run: the predicted image and the slot map device -> page-locked host memory, then
                numpy: the subtraction, an 8x8 (or 4x4) Hadamard of EVERY block and the per-block SSE.  No sum per PU or CU is formed from the
                slot map at all: a host that forms them pays that on top, so this is the route's floor

The slot map is a real partition: me_select_kernel's decision over random tables.  REPS (default 7) repeats of each from a warm clock;
median, min and max.  usage: tools/residual_rate.py [out.json]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hm-opencl_amd"))
import numpy as np
import torch
from hmme import api, synth

REPS = int(os.environ.get("REPS", "7"))
w, h = (int(v) for v in os.environ.get("SIZE", "3840x2160").split("x"))
HBM_TBS = {"spec": 8.0, "measured_copy": 6.29}   # MI355X: HBM3E peak and what a float4 copy reaches
dev = torch.device("cuda", 0)
eng = api.Engine(0, 64); eng.set_lambda(57.9)
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


BATCH = 50


def timed_batch(fn):
    """REPS windows of BATCH back-to-back launches each -> ms per launch (a single launch of tens of microseconds is near what an event pair
    resolves; back to back the launches overlap their ramps, so this is the sustained figure)"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record()
        for _ in range(BATCH):
            fn()
        b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) / BATCH for a, b in ev])


def wall(fn):
    t = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return stats(t, 3)


def hadamard(k):
    m = np.array([[1]], np.int32)
    while m.shape[0] < k:
        m = np.kron(np.array([[1, 1], [1, -1]], np.int32), m)
    return m


def host_model(cur, pred, k, bd):
    """subtraction, k x k Hadamard of every block with xCalcHADs' rounding, per-block SSE with xGetSSE's per-sample shift"""
    d = cur.astype(np.int32) - pred.astype(np.int32)
    hh, ww = d.shape[0] // k * k, d.shape[1] // k * k
    blocks = d[:hh, :ww].reshape(hh // k, k, ww // k, k).transpose(0, 2, 1, 3)
    hm = hadamard(k)
    coef = hm @ blocks @ hm.T
    had = (np.abs(coef).sum(axis=(2, 3)) + (2 if k == 8 else 1)) >> (2 if k == 8 else 1)
    sse = ((blocks * blocks) >> ((bd - 8) << 1)).sum(axis=(2, 3))
    return d.astype(np.int16), had, sse


out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "n_ctu": n, "reps": REPS, "hbm_tb_per_s": HBM_TBS, "cases": []}
g = torch.Generator(device=dev); g.manual_seed(1)
rng = np.random.default_rng(1)
d_mv = torch.randint(-800, 801, (1, n, 593, 2), generator=g, device=dev, dtype=torch.int16)
d_cost = torch.randint(0, 1 << 20, (1, n, 593), generator=g, device=dev, dtype=torch.int32)
for bd in (8, 10):
    bps, dt = (1, np.uint8) if bd == 8 else (2, np.uint16)
    maxv = (1 << bd) - 1
    cur = rng.integers(0, maxv + 1, size=(h, w)).astype(np.int16)
    pred = np.clip(cur + rng.integers(-6 << (bd - 8), (6 << (bd - 8)) + 1, size=(h, w)), 0, maxv).astype(dt)
    plane = eng.plane(w, h, bd)
    if bd == 8:
        plane.upload_u8(cur.astype(np.uint8))
    else:
        plane.upload_pel(synth.pad_plane(cur), (synth.MARGIN, synth.MARGIN))
    d_pred = torch.from_numpy(pred if bd == 8 else pred.view(np.int16)).to(dev)
    h_pred = torch.empty(d_pred.shape, dtype=d_pred.dtype, pin_memory=True)
    d_res = torch.zeros((h, w), dtype=torch.int16, device=dev)
    fp = api.FrameParams(1, 0, bd, 0, n)
    for per in (64, 256):
        d_field = torch.zeros((1, n, per, 2), dtype=torch.int16, device=dev)
        d_slot = torch.zeros((1, n, per), dtype=torch.int16, device=dev)
        eng.select_pairs_device(w, h, 1, api.FrameParams(1, 0, 8, 0, n), api.SelectParams(per), d_mv.data_ptr(), d_cost.data_ptr(), None, d_field.data_ptr(),
                                d_slot.data_ptr(), None, st)
        h_slot = torch.empty(d_slot.shape, dtype=d_slot.dtype, pin_memory=True)
        d_pu = torch.zeros((1, n, per), dtype=torch.int32, device=dev); d_cu = torch.zeros_like(d_pu)
        d_ctu = torch.zeros((1, n, 2), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        distinct = int(np.unique(d_slot.cpu().numpy()).size)

        def down():
            h_pred.copy_(d_pred, non_blocking=True); h_slot.copy_(d_slot, non_blocking=True)

        def model():
            host_model(cur, h_pred.numpy().view(dt), 8 if per == 64 else 4, bd)

        down(); model()
        route = {"host_route_download_ms": wall(down), "host_route_numpy_ms": wall(model)}
        route["host_route_total_ms"] = round(sum(v["median"] for v in route.values()), 3)
        for had in (1, 0):
            for with_res in (False, True):
                run = lambda: eng.residual_pairs_device([plane], [d_pred.data_ptr()], w * bps, fp, d_slot.data_ptr(), per, had,
                                                        [d_res.data_ptr()] if with_res else None, w * 2, d_pu.data_ptr(), d_cu.data_ptr(), d_ctu.data_ptr(), st)
                for _ in range(3):
                    run()
                torch.cuda.synchronize()
                case = {"bit_depth": bd, "blocks_per_ctu": per, "use_hadamard": had, "with_residual": with_res, "distinct_slots_in_map": distinct}
                case["residual_ms"] = timed(run)
                case["residual_ms_back_to_back"] = timed_batch(run)
                moved =n * 4096 * bps + w * h * bps + n * (per * 2 + per * 8 + 8) + (w * h * 2 if with_res else 0)
                case["bytes_moved"] = moved
                case["gb_per_s"] = round(moved / case["residual_ms"]["median"] * 1e-6, 1)
                case["of_hbm_measured_copy"] = round(case["gb_per_s"] / (HBM_TBS["measured_copy"] * 1e3), 3)
                if had and with_res:   # the replaced route computes Hadamards and the residual
                    case.update(route)
                out["cases"].append(case)
    plane.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
