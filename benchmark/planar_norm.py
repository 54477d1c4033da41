#!/usr/bin/env python3
"""Planar U8 frames ([F, 3, H, W], as an image decoder leaves them) -> normalised planar float tensors:
resize_planes_normalized (the plan's resize into a workspace, then one kernel) against the composition
available without it -- resize_tensor on the [F * 3, H, W] view followed by
(x.to(float32) * scale + bias).to(dtype) with broadcast per-plane tensors.  Device-resident batches,
rotated so that no timed step reads a batch the previous step left in the caches.  Not the headline
metric (bench.py).

  python benchmark/planar_norm.py [--frames 64] [--steps 10] [--reps 5] [--only 1080p-224]

Prints one JSON line per configuration: ms per batch of both paths (the median of `reps` alternated
windows of `steps` batches between device events, and every window), their ratio, whether every window of
the new path was faster than every window of the composition, the resize alone, and -- as an estimate of
the second pass -- the difference of the new path and the resize alone with the bytes it moves, beside the
on-box streaming probe at the nearest read:write mix libiqo_probe.so has (1 : 4, the pass's own for fp32;
fp16 is 1 : 2; a probe, not a ceiling).  The two paths are compared bit for bit before they are timed.

The last line is the luma-only form, NV12 1080p -> 224 x 224 fp16, one plane:
Nv12Resizer.resize_luma_normalized against a planar resizer on the Y plane of the NV12 frames through
resize_device plus the same torch ops, with Nv12Resizer.resize_normalized (chroma resized, the colour matrix,
three planes) beside it for context only.
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
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ROTATE_BYTES = 640 << 20  # rotated batches: together beyond the 256 MiB of last-level cache


def windows(step, stream, dev, steps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        step()
    e1.record(stream)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / steps


def measure(args, dev, stream, new, old, first, extra=None):
    """Bit comparison of new() and old() on batch 0, warm-up, then alternated windows.  Each callable takes the
    batch index and returns its result."""
    import torch
    a, b = new(0), old(0)
    bits = torch.int32 if a.dtype == torch.float32 else torch.int16
    same = bool(a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(bits), b.contiguous().view(bits)))
    del a, b
    paths = [new, old, first] + ([extra] if extra else [])
    k = [0] * len(paths)

    def stepper(i):
        def step():
            k[i] += 1
            paths[i](k[i])
        return step

    steps = [stepper(i) for i in range(len(paths))]
    for _ in range(args.warmup):
        for s in steps:
            s()
    torch.cuda.synchronize(dev)
    times = [[] for _ in paths]
    for _ in range(args.reps):  # alternated windows
        for t, s in zip(times, steps):
            t.append(windows(s, stream, dev, args.steps))
    return same, times


def report(line, same, times, pass2_bytes, first_name):
    t_new, t_old, t_first = times[:3]
    ms_new, ms_old, ms_first = (statistics.median(t) for t in (t_new, t_old, t_first))
    pass2_ms = ms_new - ms_first
    line.update({
        "bit_identical": same, "new_ms": round(ms_new, 4), "torch_composition_ms": round(ms_old, 4),
        "speedup": round(ms_old / ms_new, 2), "new_faster": ms_new < ms_old,
        "every_new_window_faster": max(t_new) < min(t_old),
        "window_spread_ms": {"new": round(max(t_new) - min(t_new), 4), "composition": round(max(t_old) - min(t_old), 4)},
        first_name: round(ms_first, 4),
        "new_windows_ms": [round(t, 4) for t in t_new],
        "composition_windows_ms": [round(t, 4) for t in t_old],
        "second_pass_estimate": {
            "ms": round(pass2_ms, 4), "bytes": pass2_bytes,
            "gb_s": round(pass2_bytes / (pass2_ms / 1e3) / 1e9, 1) if pass2_ms > 0 else None,
            "note": "new_ms - %s; launch gaps included" % first_name}})
    return line


def probe_line(bench, probe, pass2_bytes, elem, dev, stream):
    """The streaming probe over as many bytes as the second pass moves, at the nearest read : write mix the
    probe library has: the pass reads 1 byte per `elem` written, 1 : 4 for fp32 and 1 : 2 for fp16, and the
    probe's 1 : 4 serves both (its other neighbour of 1 : 2 is 1 : 1, further off in the share of reads)."""
    import torch
    mix = (1, 4)
    rb, wb = pass2_bytes // 5, pass2_bytes // 5 * 4
    ps = torch.empty((2, rb), dtype=torch.uint8, device=dev)
    pd = torch.empty((2, wb), dtype=torch.uint8, device=dev)
    out = bench.stream_probe(probe, mix, ps, rb, pd, wb, dev, stream, 20)
    out["second_pass_mix_read_write"] = "1:%d" % elem
    return out


def main():
    import torch

    import bench
    import libiqo_amd

    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", help="a shape name of SHAPES, or luma")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: a timing without one says nothing"
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    n, P = args.frames, 3
    scale = tuple(1.0 / (255.0 * s) for s in STD)
    bias = tuple(-m / s for m, s in zip(MEAN, STD))
    scale_t = torch.tensor(scale, dtype=torch.float32, device=dev).view(1, P, 1, 1)
    bias_t = torch.tensor(bias, dtype=torch.float32, device=dev).view(1, P, 1, 1)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    probe = bench.probe_lib()
    for sname, (sw, sh, dw, dh) in SHAPES.items():
        if args.only and args.only != sname:
            continue
        nb = max(2, -(-ROTATE_BYTES // (n * P * sw * sh)))
        srcs = [torch.randint(0, 256, (n, P, sh, sw), dtype=torch.uint8, device=dev, generator=g) for _ in range(nb)]
        for mname, (m, d) in METHODS.items():
            r = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh)
            u8 = torch.empty((n * P, dh, dw), dtype=torch.uint8, device=dev)
            for dname, dtype in (("fp16", torch.float16), ("fp32", torch.float32)):
                out = torch.empty((n, P, dh, dw), dtype=dtype, device=dev)

                def new(k):
                    return r.resize_planes_normalized(srcs[k % nb], scale, bias, dtype=dtype, out=out)

                def first(k):
                    return r.resize_tensor(srcs[k % nb].view(n * P, sh, sw), out=u8)

                def old(k):
                    # what a caller has without the entry
                    x = first(k).view(n, P, dh, dw)
                    return (x.to(torch.float32) * scale_t + bias_t).to(dtype)

                same, times = measure(args, dev, stream, new, old, first)
                elem = out.element_size()
                pass2_bytes = n * P * dw * dh * (1 + elem)  # reads the resized planes, writes the float planes
                line = report({"workload": "planar %s %s -> normalised %s" % (sname, mname, dname), "frames": n,
                               "planes": P, "kernel": r.describe()["kernel"]}, same, times, pass2_bytes,
                              "resize_tensor_ms")
                if pass2_bytes >= (8 << 20):
                    line["stream_probe"] = probe_line(bench, probe, pass2_bytes, elem, dev, stream)
                print(json.dumps(line), flush=True)
                del out
            del r, u8
        del srcs
        torch.cuda.empty_cache()

    if args.only in ("", "luma"):
        sw, sh, dw, dh = SHAPES["1080p-224"]
        m, d = METHODS["lanczos3"]
        ins = sw * sh + 2 * (sw // 2) * (sh // 2)
        nb = max(2, -(-ROTATE_BYTES // (n * ins)))
        srcs = [torch.randint(0, 256, (n, ins), dtype=torch.uint8, device=dev, generator=g) for _ in range(nb)]
        r = libiqo_amd.Nv12Resizer(m, d, sw, sh, dw, dh)
        ry = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh)
        dtype = torch.float16
        u8 = torch.empty((n, 1, dh, dw), dtype=torch.uint8, device=dev)
        out = torch.empty((n, 1, dh, dw), dtype=dtype, device=dev)
        rgb = torch.empty((n, 3, dh, dw), dtype=dtype, device=dev)

        def new(k):
            return r.resize_luma_normalized(srcs[k % nb], scale[:1], bias[:1], dtype=dtype, out=out)

        def first(k):
            s = srcs[k % nb]
            ry.resize_device(n, sw, s.stride(0), s, dw, dw * dh, u8, stream)
            return u8

        def old(k):
            return (first(k).to(torch.float32) * scale_t[:, :1] + bias_t[:, :1]).to(dtype)

        def context(k):
            return r.resize_normalized(srcs[k % nb], scale, bias, standard="bt709", dtype=dtype, out=rgb)

        same, times = measure(args, dev, stream, new, old, first, context)
        line = report({"workload": "NV12 1080p-224 lanczos3 luma only -> normalised fp16", "frames": n, "planes": 1,
                       "kernel": ry.describe()["kernel"]}, same, times, n * dw * dh * 3, "resize_device_ms")
        line["context_nv12_resize_normalized_rgb_ms"] = round(statistics.median(times[3]), 4)
        line["context_windows_ms"] = [round(t, 4) for t in times[3]]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
