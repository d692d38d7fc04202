#!/usr/bin/env python3
"""cost of estimating explicit weighted-prediction parameters at picture size (device-resident planes), for a 2160p 8-bit and a 2160p 10-bit fade:

  stats_ms            the two statistics launches over a set of one plane, me_plane_stats_kernel (device events around `PASS_REPS` back-to-back repeats)
  sad_ms[n]           me_wp_sad_set_kernel, one current picture against n = 1, 4, 16 references: n pairs in one launch (the same)
  estimate_ms[n]      hmme_wp_estimate end to end on the host clock, statistics cached (1 launch: the SAD pass) / not cached (3: two statistics
                      launches for all 1 + n planes together, then the SAD pass; fresh uploads are outside the clock); the counts are written
                      beside the times ("launches")
  host_route_ms       the route it replaces: the picture areas of both planes brought to the host (torch, page-locked target) and the numpy
                      model of tests/wp_estimate_model.py on them; nothing uploaded
  copy_ms             a float4 device copy of the bytes ONE pass over one plane reads (torch copy_ of a 16-byte-element tensor): the bandwidth yardstick

REPS (default 7) repeats of each from a warm clock; median, min and max.  usage: tools/wp_estimate_rate.py [out.json]

tools/wp_estimate_rate.py --420 [out.json] measures the estimator of a 4:2:0 slice instead (Y, Cb, Cr planes, 1, 4 and 16 references, 8 and 10
bit), each on the host clock around a call that ends in the call's own wait, with the per-plane sums cached ("cached") and dropped by fresh
uploads outside the clock ("cold"):

  plane_set_ms[n]     hmme_wp_estimate_420: the same two kernels -- cold 2 statistics launches for all 3 (n + 1) planes + 1 SAD launch, cached 1
  composition_ms[n]   what the library offered for the same bytes before that call: hmme_plane_stats on every plane, then one hmme_wp_estimate
                      per component -- cold 2 launches per plane (each plane a set of one) + 3 SAD launches, cached 3.  (It reads what the 4:2:0 call reads and gives its
                      sums, not its decision: the three calls share neither the denominator nor the ratio.)

The two are timed alternately, repeat by repeat; the launch counts are written beside the times.  Before the clock starts the per-plane sums
and the per-component SADs of the two routes are compared wherever the routes arrive at the same parameters."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hm-opencl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from hmme import api, synth
import wp_estimate_model as model

REPS = int(os.environ.get("REPS", "7"))
PASS_REPS = int(os.environ.get("PASS_REPS", "20"))
w, h = (int(v) for v in os.environ.get("SIZE", "3840x2160").split("x"))
dev = torch.device("cuda", 0)
eng = api.Engine(0, 64)
st = torch.cuda.current_stream().cuda_stream


def summary(t, digits=4):
    return {"median": round(statistics.median(t), digits), "min": round(min(t), digits), "max": round(max(t), digits)}


def host_ms(fn):
    t = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return summary(t, 3)


def leg_420(path):
    out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h} luma, 4:2:0", "reps": REPS, "cases": []}
    for bd in (8, 10):
        maxv = (1 << bd) - 1
        dt = np.uint8 if bd == 8 else np.uint16
        sizes = ((w, h), (w // 2, h // 2), (w // 2, h // 2))
        base = [synth.Sequence(ww, hh, 2, seed=99 + c, bit_depth=bd).luma(0).astype(np.int64) for c, (ww, hh) in enumerate(sizes)]
        cur_img = [np.clip((48 * b + 32 >> 6) + 10 * (1 << (bd - 8)), 0, maxv).astype(dt) for b in base]       # the fade (48, 10, 6, 32) on all components
        ref_imgs = [[base[c].astype(dt) if i % 2 == 0 else np.clip(base[c] + i, 0, maxv).astype(dt) for i in range(16)] for c in range(3)]
        ref_img = lambda c, i: ref_imgs[c][i]

        def up(plane, img):
            if bd == 8:
                plane.upload_u8(img)
            else:
                eng._check(eng.L.hmme_plane_upload_pel(plane.h, img.ctypes.data, img.shape[1]))
        cur = [eng.plane(ww, hh, bd) for ww, hh in sizes]
        refs = [[eng.plane(ww, hh, bd) for ww, hh in sizes] for _ in range(16)]

        def fill(n):
            for c in range(3):
                up(cur[c], cur_img[c])
                for i in range(n):
                    up(refs[i][c], ref_img(c, i))

        def plane_set(n):
            return eng.wp_estimate_420(cur, refs[:n], 7 if n > 3 else 6)

        def composition(n):
            for p in cur + [p for r in refs[:n] for p in r]:
                eng.plane_stats(p)
            return [eng.wp_estimate(cur[c], [r[c] for r in refs[:n]], 7 if n > 3 else 6) for c in range(3)]
        case = {"bit_depth": bd, "bytes_read_per_pass": {}, "launches": {}, "plane_set_ms": {"cold": {}, "cached": {}}, "composition_ms": {"cold": {}, "cached": {}}}
        fill(16)
        for n in (1, 4, 16):          # warm every shape; the two routes agree on what both compute
            (wl, wc, infos), comp = plane_set(n), composition(n)
            for c in range(3):
                for r in range(n):
                    a, b = infos[3 * r + c].as_dict(), comp[c][1][r].as_dict()
                    assert all(a[k] == b[k] for k in ("cur_dc_sum", "cur_ac", "ref_dc_sum", "ref_ac")), (bd, n, r, c)
                    if (a["log2_denom"], a["present"]) == (b["log2_denom"], b["present"]) and c == 0:
                        assert (a["sad_wp"], a["sad_nowp"], a["weight"], a["offset"]) == (b["sad_wp"], b["sad_nowp"], b["weight"], b["offset"]), (bd, n, r)
            if n == 1:
                case["estimate"] = {"luma": list(wl[0]), "cb": list(wc[0]), "cr": list(wc[1]), "present": infos[0].present}
        for n in (1, 4, 16):
            planes = 3 * (n + 1)
            plane_bytes = sum(ww * hh for ww, hh in sizes) * np.dtype(dt).itemsize
            case["bytes_read_per_pass"][str(n)] = {"statistics (each of two passes)": int(plane_bytes * (n + 1)), "SAD": int(2 * plane_bytes * n)}
            case["launches"][str(n)] = {"plane_set": {"cold": 3, "cached": 1}, "composition": {"cold": 2 * planes + 3, "cached": 3}}
            t = {"plane_set": {"cold": [], "cached": []}, "composition": {"cold": [], "cached": []}}
            for _ in range(REPS):
                for name, fn in (("plane_set", plane_set), ("composition", composition)):
                    fill(n)                         # outside the clock: a fill drops the plane's sums
                    for state in ("cold", "cached"):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn(n)
                        t[name][state].append((time.perf_counter() - t0) * 1e3)
            for name in t:
                for state in t[name]:
                    case[name + "_ms"][state][str(n)] = summary(t[name][state], 3)
        out["cases"].append(case)
        for p in cur + [p for r in refs for p in r]:
            p.close()
    eng.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if path:
        open(path, "w").write(txt + "\n")


if "--420" in sys.argv[1:]:
    rest = [a for a in sys.argv[1:] if a != "--420"]
    leg_420(rest[0] if rest else None)
    sys.exit(0)

out = {"hmme_build_id": api.build_id(), "device": eng.device_info, "size": f"{w}x{h}", "reps": REPS, "pass_reps": PASS_REPS, "cases": []}
for bd in (8, 10):
    maxv = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    base = synth.Sequence(w, h, 2, seed=99, bit_depth=bd).luma(0).astype(np.int64)
    ref_img = base.astype(dt)
    cur_img = np.clip((48 * base + 32 >> 6) + 10 * (1 << (bd - 8)), 0, maxv).astype(dt)       # the fade (48, 10, 6, 32)

    def up(plane, img):
        if bd == 8:
            plane.upload_u8(img)
        else:
            eng._check(eng.L.hmme_plane_upload_pel(plane.h, img.ctypes.data, w))
    pc = eng.plane(w, h, bd); up(pc, cur_img)
    refs = [eng.plane(w, h, bd) for _ in range(16)]
    for i, r in enumerate(refs):
        up(r, ref_img if i % 2 == 0 else np.clip(ref_img.astype(np.int64) + i, 0, maxv).astype(dt))
    wp = (48, 10, 6, 32)
    case = {"bit_depth": bd, "plane_bytes": int(w * h * np.dtype(dt).itemsize), "sad_ms": {}, "estimate_cached_ms": {}, "estimate_uncached_ms": {},
            "launches": {"stats": 2, "sad": 1, "estimate_cached": 1, "estimate_uncached": 3}}
    weights, infos = eng.wp_estimate(pc, refs[:1])
    case["estimate"] = {"weight": list(weights[0]), "present": infos[0].present}
    for _ in range(3):          # warm clock
        eng.time_wp_estimate_passes(pc, refs, wp, st, reps=PASS_REPS)
    for n in (1, 4, 16):
        p = [eng.time_wp_estimate_passes(pc, refs[:n], wp, st, reps=PASS_REPS) for _ in range(REPS)]
        if n == 1:
            case["stats_ms"] = summary([a for a, _ in p])
        case["sad_ms"][str(n)] = summary([b for _, b in p])
        case["estimate_cached_ms"][str(n)] = host_ms(lambda: eng.wp_estimate(pc, refs[:n], 7 if n > 3 else 6))

        # not cached: an upload drops a plane's sums, so the planes are uploaded again (outside the clock) before every repeat
        t = []
        for _ in range(REPS):
            up(pc, cur_img)
            for r, img_i in zip(refs[:n], range(n)):
                up(r, ref_img if img_i % 2 == 0 else np.clip(ref_img.astype(np.int64) + img_i, 0, maxv).astype(dt))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.wp_estimate(pc, refs[:n], 7 if n > 3 else 6)
            t.append((time.perf_counter() - t0) * 1e3)
        case["estimate_uncached_ms"][str(n)] = summary(t, 3)
    # the route this replaces: both picture areas to the host, the numpy model there
    t_dt = torch.uint8 if bd == 8 else torch.int16
    d_cur, d_ref = torch.from_numpy(cur_img.view(np.uint8 if bd == 8 else np.int16)).to(dev), torch.from_numpy(ref_img.view(np.uint8 if bd == 8 else np.int16)).to(dev)
    h_cur, h_ref = torch.empty((h, w), dtype=t_dt, pin_memory=True), torch.empty((h, w), dtype=t_dt, pin_memory=True)

    def host_route():
        h_cur.copy_(d_cur, non_blocking=True); h_ref.copy_(d_ref, non_blocking=True)
        torch.cuda.synchronize()
        model.estimate(h_cur.numpy().view(dt), [h_ref.numpy().view(dt)], bd, 6)
    host_route()
    case["host_route_ms"] = host_ms(host_route)
    # the yardstick: a device copy of one plane's bytes in 16-byte elements
    n16 = case["plane_bytes"] // 16
    src = torch.zeros((n16, 4), dtype=torch.float32, device=dev); dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    t = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(PASS_REPS):
            dst.copy_(src)
        b.record(); torch.cuda.synchronize()
        t.append(a.elapsed_time(b) / PASS_REPS)
    case["copy_ms"] = summary(t)
    mb = case["plane_bytes"] / 1e6
    case["gb_per_s"] = {"copy (read + write)": round(2 * mb / case["copy_ms"]["median"], 1),
                        "stats (two reads of the plane)": round(2 * mb / case["stats_ms"]["median"], 1),
                        **{f"sad, {n} refs (2 planes read per reference)": round(2 * int(n) * mb / case["sad_ms"][n]["median"], 1) for n in case["sad_ms"]}}
    out["cases"].append(case)
    pc.close()
    for r in refs:
        r.close()
eng.close()
txt = json.dumps(out, indent=1)
print(txt)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(txt + "\n")
