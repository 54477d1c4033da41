#!/usr/bin/env python3
"""A batch of RandomResizedCrop boxes out of device-resident frames, each to 224 x 224: the one-launch
RoiResizer against the only path the library had before it -- one packed resizer per distinct box shape
(built and prepared outside the timed windows) and resize_device (or iqo_hip_resize_device_norm) per box
through an offset pointer.  Not the headline metric (bench.py).

  python benchmark/roi_crops.py [--boxes 256] [--frames 64] [--steps 3] [--reps 5] [--only lanczos3-u8]

256 seeded boxes (area 8-100 % of the frame, aspect 3/4-4/3 log-uniform, half of them flipped) over 64 RGB
1920 x 1080 frames; two frame sets are rotated, so no step reads frames the previous step left in the caches
(one set is 398 MB, the last-level cache 256 MiB).  Windows of `steps` batches are timed between device
events, the two paths alternated.  The per-box path cannot mirror, so its flipped boxes are stored unflipped
(no extra work for it) and mirrored back on the host for the bit comparison only.

One JSON line per configuration: ms per batch of both paths for every window and their medians, the ratio,
whether every window of the new call beat every window of the loop, host milliseconds per call with the
table cache cold and warm (host clock, no device wait), arena bytes, and the achieved bytes/s over the
algorithmic bytes (box source bytes plus output bytes) beside the HBM peak.
"""
import argparse
import ctypes
import json
import math
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FW, FH, C = 1920, 1080, 3
DW, DH = 224, 224
METHODS = {"lanczos3": ("lanczos", 3), "area": ("area", 0)}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E peak, as bench.py


def random_resized_crops(n, frames, seed):
    """torchvision's RandomResizedCrop.get_params (scale 0.08-1, ratio 3/4-4/3), seeded, plus a frame and a flip."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        for _ in range(10):
            area = FW * FH * rng.uniform(0.08, 1.0)
            ar = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
            w, h = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
            if 0 < w <= FW and 0 < h <= FH:
                break
        else:
            w, h = FH, FH  # the fallback: the central square
        out.append((rng.randrange(frames), rng.randint(0, FW - w), rng.randint(0, FH - h), w, h, i % 2))
    return out


def window(step, stream, dev, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        step()
    e1.record(stream)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / steps


def main():
    import torch

    import libiqo_amd

    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="", help="<method>-<u8|fp16>, e.g. lanczos3-u8")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    L = libiqo_amd.lib()
    N, F = args.boxes, args.frames
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    srcs = [torch.randint(0, 256, (F, FH, FW, C), dtype=torch.uint8, device=dev, generator=g) for _ in range(2)]
    boxes = random_resized_crops(N, F, 2024)
    other = random_resized_crops(N, F, 7)  # sizes the arenas before the cold-cache call
    flipped = torch.tensor([bool(b[5]) for b in boxes], device=dev)
    src_bytes = sum(b[3] * b[4] * C for b in boxes)
    scale = tuple(1.0 / (255.0 * s) for s in STD)
    bias = tuple(-m / s for m, s in zip(MEAN, STD))
    norm = libiqo_amd.Norm(libiqo_amd.OUT_F16, 3)
    for i in range(3):
        norm.order[i], norm.scale[i], norm.bias[i] = i, scale[i], bias[i]
    st, fst = srcs[0].stride(1), srcs[0].stride(0)

    for mname, (m, d) in METHODS.items():
        # the per-box path's plans: one per distinct shape, tables uploaded now
        plans = {}
        for b in boxes:
            if (b[3], b[4]) not in plans:
                p = libiqo_amd.make_resizer(m, d, b[3], b[4], DW, DH, 1, channels=C)
                p.prepare()
                plans[(b[3], b[4])] = p
        for oname in ("u8", "fp16"):
            if args.only and args.only != "%s-%s" % (mname, oname):
                continue
            is_u8 = oname == "u8"
            shape = (N, DH, DW, C) if is_u8 else (N, 3, DH, DW)
            dtype = torch.uint8 if is_u8 else torch.float16
            out_new, out_old = torch.empty(shape, dtype=dtype, device=dev), torch.empty(shape, dtype=dtype, device=dev)
            one = out_old.stride(0) * out_old.element_size()
            r = libiqo_amd.RoiResizer(m, d, DW, DH, channels=C)

            def new(k, bx=boxes):
                if is_u8:
                    return r.resize_rois(srcs[k % 2], bx, out=out_new, stream=stream)
                return r.resize_rois_normalized(srcs[k % 2], bx, scale, bias, dtype=dtype, out=out_new, stream=stream)

            def old(k):
                base, o = srcs[k % 2].data_ptr(), out_old.data_ptr()
                for i, (f, x, y, w, h, _) in enumerate(boxes):
                    plan, ptr = plans[(w, h)]._plan, base + f * fst + y * st + x * C
                    if is_u8:
                        rc = L.iqo_hip_resize_device(plan, 1, st, fst, ptr, DW * C, one, o + i * one, sp)
                    else:
                        rc = L.iqo_hip_resize_device_norm(plan, 1, st, fst, ptr, ctypes.byref(norm), DW * 2, DW * DH * 2,
                                                          one, o + i * one, sp)
                    assert rc == 0, (rc, i)
                return out_old

            # host cost of a call: arenas sized by another batch, then this batch cold and warm
            new(0, other)
            new(1, other)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            new(0)
            t1 = time.perf_counter()
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
            new(1)
            t3 = time.perf_counter()
            torch.cuda.synchronize(dev)
            host_cold, host_warm = (t1 - t0) * 1e3, (t3 - t2) * 1e3
            t4 = time.perf_counter()
            old(1)
            host_loop = (time.perf_counter() - t4) * 1e3
            torch.cuda.synchronize(dev)

            a, b = new(0), old(0)
            a = torch.where(flipped.view(N, 1, 1, 1), a.flip(2 if is_u8 else 3), a)
            bits = torch.uint8 if is_u8 else torch.int16
            same = bool(torch.equal(a.contiguous().view(bits), b.contiguous().view(bits)))
            del a, b

            k = [0, 0]

            def step(i):
                def s():
                    k[i] += 1
                    (new, old)[i](k[i])
                return s

            steps = [step(0), step(1)]
            for _ in range(args.warmup):
                for s in steps:
                    s()
            torch.cuda.synchronize(dev)
            t_new, t_old = [], []
            for _ in range(args.reps):  # alternated windows
                t_new.append(window(steps[0], stream, dev, args.steps))
                t_old.append(window(steps[1], stream, dev, args.steps))
            ms_new, ms_old = statistics.median(t_new), statistics.median(t_old)
            stats = libiqo_amd.host_roi_arena_stats(m, d, DW, DH, C, boxes, F, FW, FH)
            algo = src_bytes + N * DW * DH * 3 * out_new.element_size()
            gbps = algo / (ms_new / 1e3) / 1e9
            print(json.dumps({
                "workload": "%d RandomResizedCrop boxes of %d RGB 1080p frames -> %dx%d %s %s" % (N, F, DW, DH, mname, oname),
                "bit_identical": same, "roi_call_ms": round(ms_new, 4), "per_box_loop_ms": round(ms_old, 4),
                "speedup": round(ms_old / ms_new, 2), "every_roi_window_faster": max(t_new) < min(t_old),
                "roi_windows_ms": [round(t, 4) for t in t_new], "loop_windows_ms": [round(t, 4) for t in t_old],
                "host_ms_per_call": {"tables_cold": round(host_cold, 3), "tables_warm": round(host_warm, 3),
                                     "per_box_loop": round(host_loop, 3)},
                "distinct_shapes": len(plans), "arena": stats,
                "algorithmic_bytes": algo, "achieved_gb_s": round(gbps, 1), "hbm_peak_gb_s": HBM_PEAK_GBPS,
                "frac_of_peak": round(gbps / HBM_PEAK_GBPS, 4)}), flush=True)
            del r, out_new, out_old
        del plans
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
