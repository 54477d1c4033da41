#!/usr/bin/env python3
"""Packed RGB / RGBA frames -> NV12 at another size, for an encoder: the packed resizers' resize_nv12 (the
resize, then one RGB -> YUV 4:2:0 kernel) against the composition available without it -- resize_tensor
followed by torch ops that compute the same integers (the int32 matrix for Y, the 2 x 2 sums, the matrix,
the shift and the min for U and V, the interleave and the casts).  Device-resident batches, rotated so
that no timed step reads a batch the previous step left in the caches.  Not the headline metric
(bench.py).

  python benchmark/rgb_nv12.py [--frames 64] [--steps 10] [--reps 5] [--only 1080p-720p] [--channels 3]

Prints one JSON line per configuration: ms per batch of both paths (the median of `reps` alternated
windows of `steps` batches between device events, and every window), their ratio, whether the new path's
slowest window beat the composition's fastest, resize_tensor alone, and -- as an estimate of the second
pass -- the difference of the new path and resize_tensor with the bytes it moves, beside the on-box
streaming probe of the pass's own read:write mix (libiqo_probe.so: C : 1.5, so 2 : 1 for RGB and 8 : 3
for RGBA; a probe, not a ceiling).  The two paths are compared bit for bit before they are timed.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"1080p-720p": (1920, 1080, 1280, 720), "2160p-1080p": (3840, 2160, 1920, 1080)}
METHODS = {"lanczos3": ("lanczos", 3), "area": ("area", 0)}
# IQO_CS_BT709_LIMITED (include/iqo_hip.h): yOff, cYR, cYG, cYB, cUR, cUG, cUB, cVR, cVG, cVB
BT709 = (16, 2991, 10064, 1016, 1649, 5547, 7196, 7196, 6536, 660)


def composition(r, src, out):
    """What a caller had before resize_nv12: the pixels from resize_tensor, the rest in torch (even sizes)."""
    import torch
    dw, dh = r.dstW, r.dstH
    cw, ch = dw // 2, dh // 2
    n = src.shape[0]
    yoff, cyr, cyg, cyb, cur, cug, cub, cvr, cvg, cvb = BT709
    rgb = r.resize_tensor(src)[..., :3].to(torch.int32)
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = (cyr * R + cyg * G + cyb * B + ((yoff << 14) + 8192)) >> 14
    s = rgb.view(n, ch, 2, cw, 2, 3).sum(dim=(2, 4))
    SR, SG, SB = s[..., 0], s[..., 1], s[..., 2]
    u = ((cub * SB - cur * SR - cug * SG + ((128 << 16) + 32768)) >> 16).clamp_(max=255)
    v = ((cvr * SR - cvg * SG - cvb * SB + ((128 << 16) + 32768)) >> 16).clamp_(max=255)
    out[:, :dw * dh] = y.view(n, -1).to(torch.uint8)
    out[:, dw * dh:] = torch.stack([u, v], dim=3).view(n, -1).to(torch.uint8)
    return out


def windows(step, stream, dev, steps):
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

    import bench
    import libiqo_amd

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="a shape name of SHAPES")
    ap.add_argument("--channels", type=int, default=0, help="3 or 4; default both")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    n = args.frames
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    probe = bench.probe_lib()
    for sname, (sw, sh, dw, dh) in SHAPES.items():
        if args.only and args.only != sname:
            continue
        for C in (3, 4):
            if args.channels and args.channels != C:
                continue
            # rotated batches: together beyond the 256 MiB of last-level cache
            nb = max(2, -(-(640 << 20) // (n * sw * sh * C)))
            srcs = [torch.randint(0, 256, (n, sh, sw, C), dtype=torch.uint8, device=dev, generator=g) for _ in range(nb)]
            nbytes = dw * dh + 2 * (dw // 2) * (dh // 2)
            for mname, (m, d) in METHODS.items():
                r = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, 1, channels=C)
                out = torch.empty((n, nbytes), dtype=torch.uint8, device=dev)
                old_out = torch.empty((n, nbytes), dtype=torch.uint8, device=dev)
                pixels = torch.empty((n, dh, dw, C), dtype=torch.uint8, device=dev)
                k = [0, 0, 0]

                def new():
                    k[0] += 1
                    r.resize_nv12(srcs[k[0] % nb], standard="bt709", out=out)

                def old():
                    k[1] += 1
                    composition(r, srcs[k[1] % nb], old_out)

                def first():
                    k[2] += 1
                    r.resize_tensor(srcs[k[2] % nb], pixels)

                # the same bits first
                same = bool(torch.equal(r.resize_nv12(srcs[0], standard="bt709"), composition(r, srcs[0], old_out)))
                for _ in range(args.warmup):
                    new()
                    old()
                    first()
                torch.cuda.synchronize(dev)
                t_new, t_old, t_first = [], [], []
                for _ in range(args.reps):  # alternated windows
                    t_new.append(windows(new, stream, dev, args.steps))
                    t_old.append(windows(old, stream, dev, args.steps))
                    t_first.append(windows(first, stream, dev, args.steps))
                ms_new, ms_old, ms_first = (statistics.median(t) for t in (t_new, t_old, t_first))
                # second pass: reads the resized pixels, writes 1.5 bytes per pixel
                pass2_bytes = n * (dw * dh * C + nbytes)
                pass2_ms = ms_new - ms_first
                line = {"workload": "%s %s %s -> NV12" % ("RGB" if C == 3 else "RGBA", sname, mname), "frames": n,
                        "kernel": r.describe()["kernel"], "bit_identical": same,
                        "new_ms": round(ms_new, 4), "torch_composition_ms": round(ms_old, 4),
                        "speedup": round(ms_old / ms_new, 2),
                        "slowest_new_window_beats_fastest_composition": max(t_new) < min(t_old),
                        "resize_tensor_ms": round(ms_first, 4),
                        "new_windows_ms": [round(t, 4) for t in t_new],
                        "composition_windows_ms": [round(t, 4) for t in t_old],
                        "resize_tensor_windows_ms": [round(t, 4) for t in t_first],
                        "second_pass_estimate": {
                            "ms": round(pass2_ms, 4), "bytes": pass2_bytes,
                            "gb_s": round(pass2_bytes / (pass2_ms / 1e3) / 1e9, 1) if pass2_ms > 0 else None,
                            "note": "new_ms - resize_tensor_ms; launch gaps included"}}
                # the streaming probe at the second pass's own mix (C : 1.5), on buffers of its size
                mix = (2, 1) if C == 3 else (8, 3)
                unit = pass2_bytes // (mix[0] + mix[1])
                rb, wb = unit * mix[0], unit * mix[1]
                ps = torch.empty((2, rb), dtype=torch.uint8, device=dev)
                pd = torch.empty((2, wb), dtype=torch.uint8, device=dev)
                sp = bench.stream_probe(probe, mix, ps, rb, pd, wb, dev, stream, 20)
                del ps, pd
                line["stream_probe"] = sp
                gbs = line["second_pass_estimate"]["gb_s"]
                line["second_pass_estimate"]["fraction_of_probe"] = round(gbs / sp["ceiling"], 3) if gbs else None
                print(json.dumps(line), flush=True)
                del r, out, old_out, pixels
            del srcs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
