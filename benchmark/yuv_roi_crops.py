#!/usr/bin/env python3
"""A batch of RandomResizedCrop boxes out of device-resident NV12 1080p frames, each to 224 x 224 RGB: the
one-launch YuvRoiResizer (leg A) against the only bit-identical path the library had before it (leg B) -- per box a
prepared planar resizer on Y and a prepared 2-channel packed resizer on UV (w/2 x h/2 -> 224 x 224) through offset
pointers, then the same integer matrix (and the normalisation) in torch, once over the batch -- and, for
information, against converting whole frames first (leg C).  Not the headline metric (bench.py).

  python benchmark/yuv_roi_crops.py [--boxes 256] [--frames 64] [--steps 3] [--reps 5] [--only lanczos3-u8] [--out F]

256 seeded boxes (area 8-100 % of the frame, aspect 3/4-4/3 log-uniform, rounded outward to even coordinates and
clipped to the frame, half of them flipped) over 64 NV12 1920 x 1080 frames; two frame sets are rotated.  Windows of
`steps` batches are timed between device events, legs A and B alternated, leg C after them.  Leg B cannot mirror, so
its flipped boxes are stored unflipped (no extra work for it) and mirrored for the bit comparison only, which is
made before anything is timed.

Leg C is Nv12Resizer(1080p -> 1080p, chroma="full").resize_rgb over all frames, then RoiResizer on the RGB frames.
It is NOT the same definition -- chroma is filtered over the whole frame before the crop, and the box's RGB is
resized instead of its Y, U and V -- so it is timed only.

One JSON line per configuration (also appended to --out): ms per batch of every window of the three legs and their
medians, the A/B ratio, whether every window of leg A beat every window of leg B, the arena statistics, and the
achieved bytes/s of leg A over the algorithmic bytes (box luma + box chroma + output bytes) beside the HBM peak.
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
DW, DH = 224, 224
METHODS = {"lanczos3": ("lanczos", 3), "area": ("area", 0)}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
STANDARD = "bt709"
BT709_LIMITED = (16, 19077, 29372, 3494, 8731, 34610)  # include/iqo_hip.h IQO_CS_BT709_LIMITED
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E peak, as bench.py


def random_resized_crops(n, frames, seed):
    """torchvision's RandomResizedCrop.get_params (scale 0.08-1, ratio 3/4-4/3), seeded, rounded outward to even
    coordinates and clipped to the frame, plus a frame and a flip."""
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
        x, y = rng.randint(0, FW - w), rng.randint(0, FH - h)
        x0, y0 = x & ~1, y & ~1
        x1, y1 = min(FW, (x + w + 1) & ~1), min(FH, (y + h + 1) & ~1)
        out.append((rng.randrange(frames), x0, y0, x1 - x0, y1 - y0, i % 2))
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
    ap.add_argument("--out", default="", help="append the JSON lines to this file too")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = stream.cuda_stream
    L = libiqo_amd.lib()
    N, F = args.boxes, args.frames
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    nbytes = FW * FH * 3 // 2
    srcs = [torch.randint(0, 256, (F, nbytes), dtype=torch.uint8, device=dev, generator=g) for _ in range(2)]
    boxes = random_resized_crops(N, F, 2024)
    assert all(not (b[1] | b[2] | b[3] | b[4]) & 1 and b[1] + b[3] <= FW and b[2] + b[4] <= FH for b in boxes)
    flipped = torch.tensor([bool(b[5]) for b in boxes], device=dev)
    src_bytes = sum(b[3] * b[4] * 3 // 2 for b in boxes)
    scale = tuple(1.0 / (255.0 * s) for s in STD)
    bias = tuple(-m / s for m, s in zip(MEAN, STD))
    t_scale = torch.tensor(scale, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    t_bias = torch.tensor(bias, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    fst = srcs[0].stride(0)
    yoff, cy, crv, cgu, cgv, cbu = BT709_LIMITED

    def matrix(y, uv):
        """colorspace.hpp's yuv_to_rgb in int32 on y [N, H, W] and uv [N, H, W, 2]: uint8 [N, H, W, 3]."""
        l = cy * (y.to(torch.int32) - yoff) + 8192
        u, v = uv[..., 0].to(torch.int32) - 128, uv[..., 1].to(torch.int32) - 128
        rgb = torch.stack([l + crv * v, l - cgu * u - cgv * v, l + cbu * u], dim=3) >> 14
        return rgb.clamp_(0, 255).to(torch.uint8)

    for mname, (m, d) in METHODS.items():
        # leg B's plans: one planar and one 2-channel packed plan per distinct shape, tables uploaded now
        plans = {}
        for b in boxes:
            if (b[3], b[4]) not in plans:
                py = libiqo_amd.make_resizer(m, d, b[3], b[4], DW, DH, 1, channels=1)
                pc = libiqo_amd.make_resizer(m, d, b[3] // 2, b[4] // 2, DW, DH, 1, channels=2)
                py.prepare()
                pc.prepare()
                plans[(b[3], b[4])] = (py, pc)
        ws_y = torch.empty((N, DH, DW), dtype=torch.uint8, device=dev)
        ws_uv = torch.empty((N, DH, DW, 2), dtype=torch.uint8, device=dev)
        full = libiqo_amd.Nv12Resizer(m, d, FW, FH, FW, FH, chroma="full")
        rgb_frames = torch.empty((F, FH, FW, 3), dtype=torch.uint8, device=dev)
        for oname in ("u8", "fp16"):
            if args.only and args.only != "%s-%s" % (mname, oname):
                continue
            is_u8 = oname == "u8"
            shape = (N, DH, DW, 3) if is_u8 else (N, 3, DH, DW)
            dtype = torch.uint8 if is_u8 else torch.float16
            out_a = torch.empty(shape, dtype=dtype, device=dev)
            out_c = torch.empty(shape, dtype=dtype, device=dev)
            r = libiqo_amd.YuvRoiResizer(m, d, DW, DH, layout="nv12")
            rc = libiqo_amd.RoiResizer(m, d, DW, DH, channels=3)

            def leg_a(k):
                if is_u8:
                    return r.resize_rois_rgb(srcs[k % 2], boxes, FW, FH, standard=STANDARD, out=out_a, stream=stream)
                return r.resize_rois_normalized(srcs[k % 2], boxes, FW, FH, scale, bias, standard=STANDARD, dtype=dtype,
                                                out=out_a, stream=stream)

            def leg_b(k):
                base, oy, ouv = srcs[k % 2].data_ptr(), ws_y.data_ptr(), ws_uv.data_ptr()
                for i, (f, x, y, w, h, _) in enumerate(boxes):
                    py, pc = plans[(w, h)]
                    rc1 = L.iqo_hip_resize_device(py._plan, 1, FW, fst, base + f * fst + y * FW + x, DW, DW * DH,
                                                  oy + i * DW * DH, sp)
                    rc2 = L.iqo_hip_resize_device(pc._plan, 1, FW, fst, base + f * fst + FW * FH + (y // 2) * FW + x,
                                                  DW * 2, DW * DH * 2, ouv + i * DW * DH * 2, sp)
                    assert rc1 == 0 and rc2 == 0, (rc1, rc2, i)
                rgb = matrix(ws_y, ws_uv)
                if is_u8:
                    return rgb
                return ((rgb.permute(0, 3, 1, 2).to(torch.float32) * t_scale) + t_bias).to(dtype)

            def leg_c(k):
                full.resize_rgb(srcs[k % 2], standard=STANDARD, out=rgb_frames, stream=stream)
                if is_u8:
                    return rc.resize_rois(rgb_frames, boxes, out=out_c, stream=stream)
                return rc.resize_rois_normalized(rgb_frames, boxes, scale, bias, dtype=dtype, out=out_c, stream=stream)

            # the bit comparison, before anything is timed
            a, b = leg_a(0), leg_b(0)
            a = torch.where(flipped.view(N, 1, 1, 1), a.flip(2 if is_u8 else 3), a)
            bits = torch.uint8 if is_u8 else torch.int16
            same = bool(torch.equal(a.contiguous().view(bits), b.contiguous().view(bits)))
            del a, b
            leg_c(0)
            torch.cuda.synchronize(dev)

            k = [0, 0, 0]
            legs = (leg_a, leg_b, leg_c)

            def step(i):
                def s():
                    k[i] += 1
                    legs[i](k[i])
                return s

            steps = [step(i) for i in range(3)]
            for _ in range(args.warmup):
                for s in steps:
                    s()
            torch.cuda.synchronize(dev)
            t_a, t_b, t_c = [], [], []
            for _ in range(args.reps):  # alternated windows
                t_a.append(window(steps[0], stream, dev, args.steps))
                t_b.append(window(steps[1], stream, dev, args.steps))
            for _ in range(args.reps):
                t_c.append(window(steps[2], stream, dev, args.steps))
            ms_a, ms_b, ms_c = (statistics.median(t) for t in (t_a, t_b, t_c))
            stats = libiqo_amd.host_roi_yuv_arena_stats(m, d, DW, DH, "nv12", boxes, F, FW, FH)
            algo = src_bytes + N * DW * DH * 3 * out_a.element_size()
            gbps = algo / (ms_a / 1e3) / 1e9
            line = json.dumps({
                "workload": "%d RandomResizedCrop boxes of %d NV12 1080p frames -> %dx%d RGB %s %s" % (N, F, DW, DH, mname, oname),
                "a_b_bit_identical": same, "a_one_launch_ms": round(ms_a, 4), "b_per_box_loop_ms": round(ms_b, 4),
                "c_convert_frames_then_roi_ms": round(ms_c, 4),
                "c_note": "another definition (chroma filtered over the whole frame, RGB resized): timed only",
                "a_over_b_speedup": round(ms_b / ms_a, 2), "every_a_window_faster_than_every_b": max(t_a) < min(t_b),
                "a_windows_ms": [round(t, 4) for t in t_a], "b_windows_ms": [round(t, 4) for t in t_b],
                "c_windows_ms": [round(t, 4) for t in t_c], "distinct_shapes": len(plans), "arena": stats,
                "algorithmic_bytes": algo, "achieved_gb_s": round(gbps, 1), "hbm_peak_gb_s": HBM_PEAK_GBPS,
                "frac_of_peak": round(gbps / HBM_PEAK_GBPS, 4)})
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")
            del r, rc, out_a, out_c
        del plans, full, rgb_frames, ws_y, ws_uv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
