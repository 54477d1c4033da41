#!/usr/bin/env python3
"""NV12 decode output -> normalised planar RGB tensors: Nv12Resizer.resize_normalized (the resize, then
one YUV -> RGB kernel) against the composition available without it -- Nv12Resizer.resize_frames
followed by torch ops that compute the same integers and the same normalisation (chroma replicated,
the int32 matrix, the clamps, float32(byte) * scale + bias, the cast).  Device-resident batches,
rotated so that no timed step reads a batch the previous step left in the caches.  Not the headline
metric (bench.py).

  python benchmark/nv12_rgb.py [--frames 64] [--steps 10] [--reps 5] [--only 1080p-224] [--chroma full]

Prints one JSON line per configuration: ms per batch of both paths (the median of `reps` alternated
windows of `steps` batches between device events, and every window), their ratio, the plane resize
alone, and -- as an estimate of the second pass -- the difference of the new path and the plane resize
with the bytes it moves, beside the on-box streaming probe of the pass's own read:write mix
(libiqo_probe.so: 1.5 : 6 = 1 : 4 for fp16, 1.5 : 12 = 1 : 8 for fp32; a probe, not a ceiling).  The
two paths are compared bit for bit before they are timed.

--chroma full times Nv12Resizer(chroma="full") -- chroma filtered to the full output grid -- against what
a caller can compose without it: a planar resizer for Y, a 2-channel packed resizer srcW/2 x srcH/2 ->
dstW x dstH for UV (pxScale 1), and the same integer matrix per pixel in torch.  Its lines carry
"chroma": "full", the two plane resizes alone instead of resize_frames, and whether every window of the
new path was faster than every window of the composition; no streaming probe.  The default, --chroma
replicate, prints the lines described above, unchanged.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"1080p-224": (1920, 1080, 224, 224), "2160p-1080p": (3840, 2160, 1920, 1080)}
METHODS = {"lanczos3": ("lanczos", 3), "area": ("area", 0)}
# IQO_CS_BT709_LIMITED (include/iqo_hip.h): yOff, cY, cRV, cGU, cGV, cBU
BT709 = (16, 19077, 29372, 3494, 8731, 34610)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def composition(r, src, scale_t, bias_t, dtype):
    """What a caller had before resize_normalized: the planes from resize_frames, the rest in torch."""
    import torch
    dw, dh = r.dstW, r.dstH
    cw, ch = dw // 2, dh // 2
    n = src.shape[0]
    planes = r.resize_frames(src)
    yoff, cy, crv, cgu, cgv, cbu = BT709
    y = planes[:, :dw * dh].view(n, dh, dw).to(torch.int32) - yoff
    uv = planes[:, dw * dh:].view(n, ch, cw, 2).to(torch.int32) - 128
    uv = uv.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)  # (even sizes: no clamp of the index)
    u, v = uv[..., 0], uv[..., 1]
    lum = cy * y + 8192
    rgb = torch.stack([lum + crv * v, lum - cgu * u - cgv * v, lum + cbu * u], dim=1)
    rgb = (rgb >> 14).clamp_(0, 255).to(torch.float32)
    return (rgb * scale_t + bias_t).to(dtype)


def composition_full(ry, ruv, src, ybuf, uvbuf, scale_t, bias_t, dtype, stream, planes_only=False):
    """chroma="full" without the library's entry: Y and the UV plane resized to dstW x dstH by two resizers
    straight from the NV12 frames (no copy), the rest in torch."""
    import torch
    sw, sh, dw, dh = ry.srcW, ry.srcH, ry.dstW, ry.dstH
    n, b = src.shape[0], src.data_ptr()
    ry.resize_device(n, sw, src.stride(0), b, dw, dw * dh, ybuf, stream)
    ruv.resize_device(n, 2 * (sw // 2), src.stride(0), b + sw * sh, 2 * dw, 2 * dw * dh, uvbuf, stream)
    if planes_only:
        return None
    yoff, cy, crv, cgu, cgv, cbu = BT709
    y = ybuf.to(torch.int32) - yoff
    uv = uvbuf.to(torch.int32) - 128
    u, v = uv[..., 0], uv[..., 1]
    lum = cy * y + 8192
    rgb = torch.stack([lum + crv * v, lum - cgu * u - cgv * v, lum + cbu * u], dim=1)
    rgb = (rgb >> 14).clamp_(0, 255).to(torch.float32)
    return (rgb * scale_t + bias_t).to(dtype)


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
    ap.add_argument("--chroma", choices=("replicate", "full"), default="replicate")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    n = args.frames
    scale = tuple(1.0 / (255.0 * s) for s in STD)
    bias = tuple(-m / s for m, s in zip(MEAN, STD))
    scale_t = torch.tensor(scale, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    bias_t = torch.tensor(bias, dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    probe = bench.probe_lib()
    for sname, (sw, sh, dw, dh) in SHAPES.items():
        if args.only and args.only != sname:
            continue
        ins = sw * sh + 2 * (sw // 2) * (sh // 2)
        # rotated batches: together beyond the 256 MiB of last-level cache
        nb = max(2, -(-(640 << 20) // (n * ins)))
        srcs = [torch.randint(0, 256, (n, ins), dtype=torch.uint8, device=dev, generator=g) for _ in range(nb)]
        for mname, (m, d) in METHODS.items():
            full = args.chroma == "full"
            r = libiqo_amd.Nv12Resizer(m, d, sw, sh, dw, dh, chroma=args.chroma)
            if full:
                ry = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh)
                ruv = libiqo_amd.make_resizer(m, d, sw // 2, sh // 2, dw, dh, 1, channels=2)
                ybuf = torch.empty((n, dh, dw), dtype=torch.uint8, device=dev)
                uvbuf = torch.empty((n, dh, dw, 2), dtype=torch.uint8, device=dev)
            planes_out = torch.empty((n, dw * dh + 2 * (dw // 2) * (dh // 2)), dtype=torch.uint8, device=dev)
            for dname, dtype in (("fp16", torch.float16), ("fp32", torch.float32)):
                out = torch.empty((n, 3, dh, dw), dtype=dtype, device=dev)
                k = [0, 0, 0]

                def new():
                    k[0] += 1
                    r.resize_normalized(srcs[k[0] % nb], scale, bias, standard="bt709", dtype=dtype, out=out)

                def old():
                    k[1] += 1
                    if full:
                        return composition_full(ry, ruv, srcs[k[1] % nb], ybuf, uvbuf, scale_t, bias_t, dtype, stream)
                    return composition(r, srcs[k[1] % nb], scale_t, bias_t, dtype)

                def first():
                    k[2] += 1
                    if full:
                        composition_full(ry, ruv, srcs[k[2] % nb], ybuf, uvbuf, scale_t, bias_t, dtype, stream, True)
                    else:
                        r.resize_frames(srcs[k[2] % nb], planes_out)

                # the same bits first
                a = r.resize_normalized(srcs[0], scale, bias, standard="bt709", dtype=dtype)
                b = (composition_full(ry, ruv, srcs[0], ybuf, uvbuf, scale_t, bias_t, dtype, stream) if full
                     else composition(r, srcs[0], scale_t, bias_t, dtype))
                bits = torch.int32 if dtype == torch.float32 else torch.int16
                same = bool(torch.equal(a.view(bits), b.view(bits)))
                del a, b
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
                elem = out.element_size()
                # second pass: reads the resized planes, writes three float planes
                pass2_bytes = n * ((3 * dw * dh if full else dw * dh + 2 * (dw // 2) * (dh // 2)) + 3 * dw * dh * elem)
                pass2_ms = ms_new - ms_first
                line = {"workload": "NV12 %s %s -> normalised RGB %s" % (sname, mname, dname), "frames": n,
                        "kernels": list(r.describe()), "bit_identical": same,
                        "new_ms": round(ms_new, 4), "torch_composition_ms": round(ms_old, 4),
                        "speedup": round(ms_old / ms_new, 2), "new_faster": ms_new < ms_old,
                        "resize_frames_ms": round(ms_first, 4),
                        "new_windows_ms": [round(t, 4) for t in t_new],
                        "composition_windows_ms": [round(t, 4) for t in t_old],
                        "second_pass_estimate": {
                            "ms": round(pass2_ms, 4), "bytes": pass2_bytes,
                            "gb_s": round(pass2_bytes / (pass2_ms / 1e3) / 1e9, 1) if pass2_ms > 0 else None,
                            "note": "new_ms - resize_frames_ms; launch gaps included"}}
                if full:
                    line["chroma"] = "full"
                    line["kernels"].append(r.chroma_kernel())
                    line["plane_resizes_ms"] = line.pop("resize_frames_ms")
                    line["every_new_window_faster"] = max(t_new) < min(t_old)
                    line["second_pass_estimate"]["note"] = "new_ms - plane_resizes_ms; launch gaps included"
                # the streaming probe at the second pass's own mix, on buffers of its size
                elif pass2_bytes >= (8 << 20):
                    mix = (1, 2 * elem)  # 1.5 bytes read per 3 * elem written
                    rb, wb = pass2_bytes // (1 + mix[1]), pass2_bytes // (1 + mix[1]) * mix[1]
                    ps = torch.empty((2, rb), dtype=torch.uint8, device=dev)
                    pd = torch.empty((2, wb), dtype=torch.uint8, device=dev)
                    line["stream_probe"] = bench.stream_probe(probe, mix, ps, rb, pd, wb, dev, stream, 20)
                    del ps, pd
                print(json.dumps(line), flush=True)
                del out
            del r, planes_out
            if full:
                del ry, ruv, ybuf, uvbuf
        del srcs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
