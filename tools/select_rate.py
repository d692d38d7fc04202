#!/usr/bin/env python3
"""cost of the partition decision at picture size (device-resident tables, torch events): 2160p, one and four pairs per launch, one MV per
8x8 and per 4x4 block

  select_ms     hmme_select_pairs_device alone (me_select_kernel: reads both 593-slot tables, writes field, slots and CTU costs)
  gb_per_s      the bytes the kernel has to move (tables in, three results out) over select_ms, beside the chip's HBM rate
  host_route_*  the route it replaces, for comparison: the two tables device -> page-locked host memory, a numpy gather of a field from them,
                the field host -> device.  The gather here takes a FIXED partition (the 64 8x8 2Nx2N slots of every CTU, no comparison of
                costs at all): a host that DECIDES per CTU pays that on top, so this is the route's floor

REPS (default 7) repeats of each from a warm clock; median, min and max.  usage: tools/select_rate.py [out.json]"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hm-opencl_amd"))
import numpy as np
import torch
from hmme import api

REPS = int(os.environ.get("REPS", "7"))
w, h = (int(v) for v in os.environ.get("SIZE", "3840x2160").split("x"))
HBM_TBS = {"spec": 8.0, "measured_copy": 6.29}   # MI355X: HBM3E peak and what a float4 copy reaches
dev = torch.device("cuda", 0)
eng = api.Engine(0, 64); eng.set_lambda(57.9)
n = api.load().hmme_num_ctus(w, h)
st = torch.cuda.current_stream().cuda_stream
fp = api.FrameParams(1, 0, 8, 0, n)


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


# the 64 8x8 2Nx2N slots in raster order of the blocks: what a host that takes a fixed partition gathers
slots8 = np.array([api.slot_index(0, 3, 0, sum(((bx * 2 >> b) & 1) << (2 * b) | ((by * 2 >> b) & 1) << (2 * b + 1) for b in range(4)))
                   for by in range(8) for bx in range(8)])
out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "n_ctu": n, "reps": REPS, "hbm_tb_per_s": HBM_TBS, "cases": []}
g = torch.Generator(device=dev); g.manual_seed(1)
for n_pairs in (1, 4):
    d_mv = torch.randint(-800, 801, (n_pairs, n, 593, 2), generator=g, device=dev, dtype=torch.int16)
    d_cost = torch.randint(0, 1 << 20, (n_pairs, n, 593), generator=g, device=dev, dtype=torch.int32)
    h_mv = torch.empty(d_mv.shape, dtype=d_mv.dtype, pin_memory=True)
    h_cost = torch.empty(d_cost.shape, dtype=d_cost.dtype, pin_memory=True)
    for per in (64, 256):
        sel = api.SelectParams(per)
        d_field = torch.zeros((n_pairs, n, per, 2), dtype=torch.int16, device=dev)
        d_slot = torch.zeros((n_pairs, n, per), dtype=torch.int16, device=dev)
        d_cc = torch.zeros((n_pairs, n), dtype=torch.int32, device=dev)
        run = lambda: eng.select_pairs_device(w, h, n_pairs, fp, sel, d_mv.data_ptr(), d_cost.data_ptr(), None, d_field.data_ptr(), d_slot.data_ptr(),
                                              d_cc.data_ptr(), st)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        case = {"pairs_per_launch": n_pairs, "mv_per_ctu": per}
        case["select_ms"] = timed(run)
        moved = n_pairs * n * (593 * 8 + per * 6 + 4)
        case["bytes_moved"] = moved
        case["gb_per_s"] = round(moved / case["select_ms"]["median"] * 1e-6, 1)
        case["of_hbm_measured_copy"] = round(case["gb_per_s"] / (HBM_TBS["measured_copy"] * 1e3), 3)
        if per == 64:   # the replaced route moves the same tables whatever the field's layout
            h_field = torch.empty(d_field.shape, dtype=torch.int16, pin_memory=True)

            def down():
                h_mv.copy_(d_mv, non_blocking=True); h_cost.copy_(d_cost, non_blocking=True)

            def gather():
                h_field.numpy()[...] = h_mv.numpy()[:, :, slots8]

            def up():
                d_field.copy_(h_field, non_blocking=True)

            down(); gather(); up()
            case["host_route_download_ms"] = wall(down)
            case["host_route_numpy_gather_ms"] = wall(gather)
            case["host_route_upload_ms"] = wall(up)
            case["host_route_total_ms"] = round(sum(case[k]["median"] for k in ("host_route_download_ms", "host_route_numpy_gather_ms", "host_route_upload_ms")), 3)
        out["cases"].append(case)
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
