#!/usr/bin/env python3
"""Boxes into destination rectangles (letterbox) in one launch, against what a caller did before: fill the batch
with the pad colour, then one prepared resizer per distinct shape writing through destination strides.  Not the
headline metric (bench.py).

  python benchmark/roi_fit.py [--steps 3] [--reps 5] [--only rgb-lanczos3] [--append profiles/roi_fit.jsonl]

Two workloads, each bit-compared against the path it is timed against before anything is timed:
  rgb   256 seeded boxes (area 2-60 % of the frame, aspect 1:3 .. 3:1 log-uniform) of 64 RGB 1080p frames,
        letterboxed to 224 x 224 U8.  Baseline: out.fill(pad) and, per box, a prepared packed resizer
        (w, h) -> (iw, ih) through an offset source pointer, writing at (ox, oy) with the canvas' strides.
  nv12  64 whole NV12 1080p frames letterboxed to 640 x 640 fp16 planes.  Baseline: a fill and ONE batched
        Nv12Resizer(1080p -> 640 x 360, chroma="full").resize_normalized into a strided view of the batch -- a launch
        of the streaming kernels over the whole batch, which may well win.
Two frame sets are rotated, so no step reads frames the previous step left in the caches; windows of `steps`
batches are timed between device events, the two paths alternated.  One JSON line per configuration: both paths'
windows and medians and their ratio, as measured.  No ratio is required of either workload.
"""
import argparse
import json
import math
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FW, FH = 1920, 1080
METHODS = {"lanczos3": ("lanczos", 3), "area": ("area", 0)}
PAD = (114, 114, 114)


def aspect_boxes(n, frames, seed):
    """n seeded boxes: area 2-60 % of the frame, aspect (w : h) log-uniform in 1:3 .. 3:1, a frame each."""
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        area = FW * FH * rng.uniform(0.02, 0.6)
        ar = math.exp(rng.uniform(math.log(1 / 3), math.log(3)))
        w, h = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
        if 0 < w <= FW and 0 < h <= FH:
            out.append((rng.randrange(frames), rng.randint(0, FW - w), rng.randint(0, FH - h), w, h))
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


def measure(name, new, old, same, args, stream, dev, extra):
    import torch
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
    row = dict({"workload": name, "bit_identical": same, "fit_call_ms": round(ms_new, 4), "baseline_ms": round(ms_old, 4),
                "baseline_over_fit": round(ms_old / ms_new, 3), "fit_windows_ms": [round(t, 4) for t in t_new],
                "baseline_windows_ms": [round(t, 4) for t in t_old]}, **extra)
    line = json.dumps(row)
    print(line, flush=True)
    if args.append:
        with open(args.append, "a") as f:
            f.write(line + "\n")


def main():
    import torch

    import libiqo_amd

    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="", help="<rgb|nv12>-<method>, e.g. rgb-lanczos3")
    ap.add_argument("--append", default="", help="also append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    L = libiqo_amd.lib()
    N, F = args.boxes, args.frames
    g = torch.Generator(device=dev)
    g.manual_seed(11)

    # ---- workload 1: boxes of RGB frames, letterboxed to 224 x 224 U8
    C, DW, DH = 3, 224, 224
    wanted = [m for m in METHODS if not args.only or args.only == "rgb-" + m]
    if wanted:
        srcs = [torch.randint(0, 256, (F, FH, FW, C), dtype=torch.uint8, device=dev, generator=g) for _ in range(2)]
        boxes = aspect_boxes(N, F, 2025)
        rects = libiqo_amd.fit_rects(boxes, DW, DH, "letterbox")
        st, fst = srcs[0].stride(1), srcs[0].stride(0)
        pad_px = torch.tensor(PAD, dtype=torch.uint8, device=dev)
        for mname in wanted:
            m, d = METHODS[mname]
            plans = {}
            for b, rc in zip(boxes, rects):
                key = (b[3], b[4], rc[2], rc[3])
                if key not in plans:
                    plans[key] = libiqo_amd.make_resizer(m, d, b[3], b[4], rc[2], rc[3], 1, channels=C)
                    plans[key].prepare()
            out_new = torch.empty((N, DH, DW, C), dtype=torch.uint8, device=dev)
            out_old = torch.empty_like(out_new)
            one = out_old.stride(0)
            r = libiqo_amd.RoiResizer(m, d, DW, DH, channels=C)

            def new(k):
                return r.resize_rois(srcs[k % 2], boxes, out=out_new, stream=stream, rects=rects, pad=PAD)

            def old(k):
                out_old[...] = pad_px
                base, o = srcs[k % 2].data_ptr(), out_old.data_ptr()
                for i, ((f, x, y, w, h), (ox, oy, iw, ih)) in enumerate(zip(boxes, rects)):
                    rc = L.iqo_hip_resize_device(plans[(w, h, iw, ih)]._plan, 1, st, fst, base + f * fst + y * st + x * C,
                                                 DW * C, one, o + i * one + (oy * DW + ox) * C, sp)
                    assert rc == 0, (rc, i)
                return out_old

            same = bool(torch.equal(new(0), old(0)))
            stats = libiqo_amd.host_roi_arena_stats(m, d, DW, DH, C, boxes, F, FW, FH, rects=rects)
            measure("%d boxes (aspect 1:3 .. 3:1) of %d RGB 1080p frames letterboxed to %dx%d U8, %s; baseline: fill + a "
                    "prepared resizer per shape through destination strides" % (N, F, DW, DH, mname), new, old, same, args,
                    stream, dev, {"distinct_shapes": len(plans), "arena": stats})
            del plans, r, out_new, out_old
        del srcs
        torch.cuda.empty_cache()

    # ---- workload 2: whole NV12 frames letterboxed to 640 x 640 fp16 planes
    DW, DH = 640, 640
    wanted = [m for m in METHODS if not args.only or args.only == "nv12-" + m]
    if wanted:
        n = FW * FH * 3 // 2
        srcs = [torch.randint(0, 256, (F, n), dtype=torch.uint8, device=dev, generator=g) for _ in range(2)]
        boxes = [(f, 0, 0, FW, FH) for f in range(F)]
        rects = libiqo_amd.fit_rects(boxes, DW, DH, "letterbox")
        ox, oy, iw, ih = rects[0]
        scale, bias = (1.0 / 255.0,) * 3, (0.0, 0.0, 0.0)
        for mname in wanted:
            m, d = METHODS[mname]
            out_new = torch.empty((F, 3, DH, DW), dtype=torch.float16, device=dev)
            out_old = torch.empty_like(out_new)
            r = libiqo_amd.YuvRoiResizer(m, d, DW, DH, layout="nv12")
            p = libiqo_amd.Nv12Resizer(m, d, FW, FH, iw, ih, chroma="full")
            # the pad as the kernel normalises it: float32(114) * scale + bias, rounded to fp16
            pad_f = (torch.tensor(float(PAD[0]), dtype=torch.float32) * torch.tensor(scale[0], dtype=torch.float32)).to(torch.float16)
            inner = out_old[:, :, oy:oy + ih, ox:ox + iw]

            def new(k):
                return r.resize_rois_normalized(srcs[k % 2], boxes, FW, FH, scale, bias, dtype=torch.float16, out=out_new,
                                                stream=stream, rects=rects, pad=PAD)

            def old(k):
                out_old.fill_(pad_f.item())
                p.resize_normalized(srcs[k % 2], scale, bias, dtype=torch.float16, out=inner, stream=stream)
                return out_old

            same = bool(torch.equal(new(0).view(torch.int16), old(0).view(torch.int16)))
            lay = libiqo_amd.host_roi_yuv_fit_box_layout(m, d, "nv12", DW, DH, FW, FH, rects[0])
            measure("%d NV12 1080p frames letterboxed to %dx%d fp16 planes, %s; baseline: fill + one batched "
                    "Nv12Resizer(chroma=full).resize_normalized into a strided view" % (F, DW, DH, mname), new, old, same,
                    args, stream, dev, {"rect": list(rects[0]), "box_layout": lay})
            del r, p, out_new, out_old, inner
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
