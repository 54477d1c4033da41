#!/usr/bin/env python3
"""Speed of the normalised planar float output of the packed resize on one MI355X, one JSON line
per shape, three legs in the same run:

  fused        resize_normalized: packed U8 frames -> [F, planes, H, W] floats in one launch;
  u8           the packed plan's U8 call alone (resize_tensor), for the cost of the float stores;
  workaround   what a caller did before: the U8 packed resize, then eager torch
               permute -> to(dtype) -> * scale + bias into a preallocated output.

Every leg runs three times, interleaved (fused, u8, workaround, fused, ...); the median is reported
and (max - min) / median is the spread the ratios are read against.  Timing is bench.py's:
device-resident batches rotated so that no launch reads data still in the 256 MiB Infinity Cache,
>= 150 ms of untimed launches, then HIP events around `--steps` launches.  GB/s counts the source
bytes and the output bytes of the leg's own result.

  python scripts/bench_norm.py [--steps 20] [--out profiles/norm_bench.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_packed import PEAK_GBS, gbs, rotating, settle_and_time  # noqa: E402

MEAN = (0.485, 0.456, 0.406, 0.5)
STD = (0.229, 0.224, 0.225, 0.25)
SHAPES = [  # name, method, channels, order, dtype, (sw, sh, dw, dh)
    ("rgb_1080p_720p_lanczos3_fp32", "lanczos", 3, (0, 1, 2), "float32", (1920, 1080, 1280, 720)),
    ("rgb_1080p_720p_lanczos3_fp16", "lanczos", 3, (0, 1, 2), "float16", (1920, 1080, 1280, 720)),
    ("rgba_1080p_720p_lanczos3_3planes_bf16", "lanczos", 4, (0, 1, 2), "bfloat16", (1920, 1080, 1280, 720)),
    ("rgb_480p_224_area_fp16", "area", 3, (0, 1, 2), "float16", (640, 480, 224, 224)),
]


def bench_shape(name, method, C, order, dtype_name, dims, steps, dev, stream):
    import torch

    import libiqo_amd
    sw, sh, dw, dh = dims
    dtype = getattr(torch, dtype_name)
    elem = 4 if dtype_name == "float32" else 2
    P = len(order)
    src_b, out_b, u8_b = sw * sh * C, dw * dh * P * elem, dw * dh * C
    frames = int(math.ceil(1.0e9 / (src_b + out_b)))
    moved = float(frames) * (src_b + out_b)
    moved_u8 = float(frames) * (src_b + u8_b)
    rot = max(2, int(math.ceil(2.5e9 / moved)))
    scale = [1.0 / (255.0 * STD[c]) for c in order]
    bias = [-MEAN[c] / STD[c] for c in order]
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    srcs = [torch.randint(0, 256, (frames, sh, sw, C), dtype=torch.uint8, device=dev, generator=g) for _ in range(rot)]
    outs = [torch.empty((frames, P, dh, dw), dtype=dtype, device=dev) for _ in range(rot)]
    u8s = [torch.empty((frames, dh, dw, C), dtype=torch.uint8, device=dev) for _ in range(rot)]
    r = libiqo_amd.make_resizer(method, 3 if method == "lanczos" else 0, sw, sh, dw, dh, device=dev.index, channels=C)
    assert r.describe()["kernel"] == "packed_tile"
    r.prepare()
    scale_t = torch.tensor(scale, dtype=dtype, device=dev).view(1, P, 1, 1)
    bias_t = torch.tensor(bias, dtype=dtype, device=dev).view(1, P, 1, 1)
    ident = tuple(order) == tuple(range(C))

    def fused(s, d, u):
        r.resize_normalized(s, scale, bias, dtype=dtype, order=order, out=d, stream=stream)

    def u8_only(s, d, u):
        r.resize_tensor(s, out=u, stream=stream)

    def workaround(s, d, u):
        r.resize_tensor(s, out=u, stream=stream)
        x = u.permute(0, 3, 1, 2)
        if not ident:
            x = x[:, :P] if tuple(order) == tuple(range(P)) else x[:, list(order)]
        f = x.to(dtype)
        f.mul_(scale_t)
        torch.add(f, bias_t, out=d)

    bufs = list(zip(srcs, outs, u8s))
    legs = {"fused": fused, "u8": u8_only, "workaround": workaround}
    ms = {k: [] for k in legs}
    for _ in range(3):
        for k, fn in legs.items():
            ms[k].append(settle_and_time(rotating(fn, bufs), dev, stream, steps))
    # the fused call and the workaround agree (fp32: bit for bit; the workaround's half arithmetic
    # rounds the product and the sum in the half type, so the half types agree to a few units in
    # the last place of the larger of the two)
    a = torch.empty_like(outs[0][:1])
    b = torch.empty_like(outs[0][:1])
    fused(srcs[0][:1], a, None)
    workaround(srcs[0][:1], b, torch.empty_like(u8s[0][:1]))
    torch.cuda.synchronize(dev)
    if dtype_name == "float32":
        assert torch.equal(a, b), "fused call and the torch workaround disagree"
    else:
        eps = 2.0 ** (-10 if dtype_name == "float16" else -7)
        assert ((a.float() - b.float()).abs() <= 4 * eps * b.float().abs().clamp_min(1.0)).all()

    def leg(k, nbytes):
        v = sorted(ms[k])
        return {"ms": [round(t, 4) for t in ms[k]], "ms_median": round(v[1], 4),
                "spread": round((v[2] - v[0]) / v[1], 4), "gbs": round(gbs(nbytes, v[1]), 1),
                "of_8tbs": round(gbs(nbytes, v[1]) / PEAK_GBS, 4)}

    res = {"shape": name, "method": method, "channels": C, "order": list(order), "dtype": dtype_name,
           "frames": frames, "rotated_buffers": rot, "bytes_per_launch": int(moved), "steps": steps,
           "fused": leg("fused", moved), "u8": leg("u8", moved_u8), "workaround": leg("workaround", moved)}
    fa, fb, fc = (res[k]["ms_median"] for k in ("fused", "u8", "workaround"))
    res["fused_over_workaround_ms"] = round(fa / fc, 4)
    res["fused_over_u8_ms"] = round(fa / fb, 4)
    res["workaround_over_fused_speedup"] = round(fc / fa, 4)
    # faster than the workaround by more than the recorded repeat spread
    res["faster_than_workaround"] = bool(max(ms["fused"]) < min(ms["workaround"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the lines as a JSON list")
    ap.add_argument("--only", default=None, help="substring of the shape names to run")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_norm.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    lines = []
    for shape in SHAPES:
        if args.only and args.only not in shape[0]:
            continue
        res = bench_shape(*shape, args.steps, dev, stream)
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res), flush=True)
        lines.append(res)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
