"""tools/window_bench.py -- what a render window buys (profiles/window_render.json): kernel ms of the centre quarter of the headline frame against the whole frame; wall time per frame and retained
device memory of a bucketed frame against an unbucketed one, with and without firefly_clamp_passes (4 passes).  One JSON line."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from scene_util import Cornell, hjr

W, H, SPP = 1920, 1080, 256
c = Cornell()
res = {}

def kernel_ms(dev, p, shape, reps=3):
    buf = [torch.empty(shape + (4,), dtype=torch.float32, device="cuda") for _ in range(3)]
    ms = []
    for _ in range(reps + 1):
        dev.render_device(p, buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr())
        dev.synchronize()
        ms.append(dev.stats()["last_kernel_ms"])
    return ms[1:]

dev = c.device()
res["whole_frame_kernel_ms"] = kernel_ms(dev, c.hjr_params(W, H, SPP), (H, W))
win = (480, 272, 1440, 808)
res["centre_quarter_window"] = list(win)
res["centre_quarter_kernel_ms"] = kernel_ms(dev, c.hjr_params(W, H, SPP, window=win), (win[3] - win[1], win[2] - win[0]))
dev.close()

def frame(bucket, ff):
    """one frame in 4 passes (ff: firefly_clamp 4 + firefly_clamp_passes) or one shot, whole or in buckets; (wall ms, retained MiB, image)"""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    dev = c.device({"firefly_clamp": 4, "firefly_clamp_passes": 1} if ff else None)
    bounds = hjr.pass_bounds(SPP, 4) if ff else [(0, 0)]
    d_frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    wins = hjr.bucket_windows(W, H, *bucket) if bucket else [None]
    d_b = torch.empty((bucket[1], bucket[0], 4), dtype=torch.float32, device="cuda") if bucket else None
    walls = []
    for rep in range(2):
        t0 = time.perf_counter()
        for w in wins:
            for b, e in bounds:
                p = c.hjr_params(W, H, SPP, window=w, sample_begin=b, sample_end=e)
                dev.render_device(p, (d_b if w else d_frame).data_ptr())
            if w:
                dev.blit_window_device(d_b.data_ptr(), w, d_frame.data_ptr(), W, H)
        dev.synchronize()
        img = d_frame.cpu().numpy()
        walls.append((time.perf_counter() - t0) * 1e3)
    free1 = torch.cuda.mem_get_info()[0]
    dev.close()
    return walls[1], (free0 - free1) / 2**20, img

for ff in (False, True):
    a = frame(None, ff)
    b = frame((480, 272), ff)
    res["firefly_clamp_passes" if ff else "plain"] = {"unbucketed": {"wall_ms": a[0], "retained_device_MiB": a[1]}, "bucket_480x272": {"wall_ms": b[0], "retained_device_MiB": b[1]},
                                                       "identical_bits": bool((a[2].view(np.uint32) == b[2].view(np.uint32)).all())}
print("WINDOW_MEASURE " + json.dumps(res))
