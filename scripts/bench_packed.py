#!/usr/bin/env python3
"""Speed of the packed (interleaved) resize on one MI355X, one JSON line per shape:

  packed_tile     the packed plan on a device-resident batch, GB/s of source + output bytes and as a
                  fraction of 8 TB/s;
  planar_tile     the planar tile kernel (every other kernel family switched off, as
                  tests/test_gpu_parity.py test_tile_streamer_matches_oracle does) on the same pixel
                  shape as one plane, frames * C planes so the launch moves the same bytes -- three
                  repeats in the same run, their spread is the noise the ratio is read against;
  workaround      what a caller did before packed plans, end to end on the same buffers: torch
                  de-interleave, C planar resize_device calls with the default kernels, torch
                  interleave.

Timing is bench.py's: device-resident batches rotated so that no launch reads data still in the
256 MiB Infinity Cache, >= 150 ms of untimed launches, then HIP events around `--steps` launches.

  python scripts/bench_packed.py [--steps 20] [--out profiles/packed_bench.json]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("IQO_HIP_TUNING", "1")  # the A/B keys that leave the planar tile kernel alone

PEAK_GBS = 8000.0
TILE_OFF = ("walk", "a32", "d32", "d31", "ryx", "ryg", "up2", "u23", "l23")
SHAPES = [  # name, channels, (sw, sh, dw, dh)
    ("rgba_1080p_720p_lanczos3", 4, (1920, 1080, 1280, 720)),
    ("rgb_1080p_720p_lanczos3", 3, (1920, 1080, 1280, 720)),
    ("nv12_2160p_1080p_lanczos3", 2, (3840, 2160, 1920, 1080)),
]


def settle_and_time(step, dev, stream, steps, settle_ms=150.0):
    """bench.py settle_and_time: ~settle_ms of untimed launches, then `steps` between two HIP events."""
    import torch
    t0 = time.perf_counter()
    n = 0
    while n < 3 or (time.perf_counter() - t0) * 1e3 < settle_ms:
        step()
        n += 1
        if n % 8 == 0:
            torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        step()
    e1.record(stream)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / steps


def rotating(fn, bufs):
    """step() that walks the rotated (src, dst) buffer sets."""
    state = {"i": 0}

    def step():
        fn(*bufs[state["i"] % len(bufs)])
        state["i"] += 1
    return step


def gbs(nbytes, ms):
    return nbytes / (ms * 1e-3) / 1e9


def bench_rgb(name, C, dims, steps, dev, stream):
    import torch

    import libiqo_amd
    sw, sh, dw, dh = dims
    per_frame = (sw * sh + dw * dh) * C
    frames = int(math.ceil(1.0e9 / per_frame))
    moved = float(frames) * per_frame
    rot = max(2, int(math.ceil(2.5e9 / moved)))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    srcs = [torch.randint(0, 256, (frames, sh, sw, C), dtype=torch.uint8, device=dev, generator=g) for _ in range(rot)]
    dsts = [torch.empty((frames, dh, dw, C), dtype=torch.uint8, device=dev) for _ in range(rot)]
    packed = libiqo_amd.LanczosResizer(3, sw, sh, dw, dh, device=dev.index, channels=C)
    assert packed.describe()["kernel"] == "packed_tile"
    packed.prepare()
    t_packed = settle_and_time(rotating(lambda s, d: packed.resize_tensor(s, out=d, stream=stream), list(zip(srcs, dsts))),
                               dev, stream, steps)
    # planar tile: the same buffers read as frames * C planes of sw x sh (same bytes per launch)
    tile = libiqo_amd.LanczosResizer(3, sw, sh, dw, dh, device=dev.index)
    for k in TILE_OFF:
        tile.set_option(k, 0)
    assert tile.describe()["kernel"] == "tile"
    tile.prepare()
    psrcs = [s.view(frames * C, sh, sw) for s in srcs]
    pdsts = [d.view(frames * C, dh, dw) for d in dsts]
    t_tile = [settle_and_time(rotating(lambda s, d: tile.resize_tensor(s, out=d, stream=stream), list(zip(psrcs, pdsts))),
                              dev, stream, steps) for _ in range(3)]
    # the workaround: de-interleave, C planar resizes (default kernels), interleave
    fast = libiqo_amd.LanczosResizer(3, sw, sh, dw, dh, device=dev.index)
    fast.prepare()
    planes_s = torch.empty((C, frames, sh, sw), dtype=torch.uint8, device=dev)
    planes_d = torch.empty((C, frames, dh, dw), dtype=torch.uint8, device=dev)

    def workaround(s, d):
        planes_s.copy_(s.permute(3, 0, 1, 2))
        for c in range(C):
            fast.resize_tensor(planes_s[c], out=planes_d[c], stream=stream)
        d.copy_(planes_d.permute(1, 2, 3, 0))
    t_work = settle_and_time(rotating(workaround, list(zip(srcs, dsts))), dev, stream, max(3, steps // 4))
    # same answer (frame 0, every rotation slot was written by the workaround last)
    check = torch.empty_like(dsts[0][:1])
    packed.resize_tensor(srcs[0][:1], out=check, stream=stream)
    torch.cuda.synchronize(dev)
    assert torch.equal(check, dsts[0][:1]), "packed plan and the planar workaround disagree"
    tile_gbs = sorted(gbs(moved, t) for t in t_tile)
    mid = tile_gbs[1]
    return {
        "shape": name, "channels": C, "frames": frames, "rotated_buffers": rot, "bytes_per_launch": int(moved),
        "steps": steps,
        "packed_tile": {"ms": round(t_packed, 4), "gbs": round(gbs(moved, t_packed), 1),
                        "of_8tbs": round(gbs(moved, t_packed) / PEAK_GBS, 4)},
        "planar_tile": {"ms": [round(t, 4) for t in t_tile], "gbs": [round(x, 1) for x in tile_gbs],
                        "gbs_median": round(mid, 1), "noise": round((tile_gbs[2] - tile_gbs[0]) / mid, 4)},
        "packed_over_planar_tile": round(gbs(moved, t_packed) / mid, 4),
        "workaround": {"kernel": fast.describe()["kernel"], "ms": round(t_work, 4),
                       "gbs_of_packed_bytes": round(gbs(moved, t_work), 1)},
        "packed_over_workaround": round(t_work / t_packed, 4),
    }


def bench_nv12(name, dims, steps, dev, stream):
    import torch

    import libiqo_amd
    sw, sh, dw, dh = dims
    cw, ch, cdw, cdh = sw // 2, sh // 2, dw // 2, dh // 2
    fs, fd = sw * sh + 2 * cw * ch, dw * dh + 2 * cdw * cdh
    frames = int(math.ceil(1.0e9 / (fs + fd)))
    moved = float(frames) * (fs + fd)
    moved_uv = float(frames) * 2 * (cw * ch + cdw * cdh)
    rot = max(2, int(math.ceil(2.5e9 / moved)))
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    srcs = [torch.randint(0, 256, (frames, fs), dtype=torch.uint8, device=dev, generator=g) for _ in range(rot)]
    dsts = [torch.empty((frames, fd), dtype=torch.uint8, device=dev) for _ in range(rot)]
    nv = libiqo_amd.Nv12Resizer("lanczos", 3, sw, sh, dw, dh, device=dev.index)
    ky, kuv = nv.describe()
    assert kuv == "packed_tile"
    t_nv = settle_and_time(rotating(lambda s, d: nv.resize_frames(s, out=d, stream=stream), list(zip(srcs, dsts))),
                           dev, stream, steps)
    # the UV plane alone through the packed plan
    uv = libiqo_amd.LanczosResizer(3, cw, ch, cdw, cdh, pxScale=2, device=dev.index, channels=2)
    uv.prepare()

    def uv_only(s, d):
        uv.resize_device(frames, 2 * cw, s.stride(0), s.data_ptr() + sw * sh, 2 * cdw, d.stride(0),
                         d.data_ptr() + dw * dh, stream)
    t_uv = settle_and_time(rotating(uv_only, list(zip(srcs, dsts))), dev, stream, steps)
    # the workaround: de-interleave UV into I420, the I420 resizer (default kernels), interleave
    yuv = libiqo_amd.Yuv420Resizer("lanczos", 3, sw, sh, dw, dh, device=dev.index)
    i420_s = torch.empty((frames, fs), dtype=torch.uint8, device=dev)
    i420_d = torch.empty((frames, fd), dtype=torch.uint8, device=dev)

    def workaround(s, d):
        i420_s[:, :sw * sh].copy_(s[:, :sw * sh])
        i420_s[:, sw * sh:].view(frames, 2, ch * cw).copy_(s[:, sw * sh:].view(frames, ch * cw, 2).permute(0, 2, 1))
        yuv.resize_frames(i420_s, out=i420_d, stream=stream)
        d[:, :dw * dh].copy_(i420_d[:, :dw * dh])
        d[:, dw * dh:].view(frames, cdh * cdw, 2).copy_(i420_d[:, dw * dh:].view(frames, 2, cdh * cdw).permute(0, 2, 1))
    t_work = settle_and_time(rotating(workaround, list(zip(srcs, dsts))), dev, stream, max(3, steps // 4))
    check = torch.empty_like(dsts[0][:1])
    nv.resize_frames(srcs[0][:1], out=check, stream=stream)
    torch.cuda.synchronize(dev)
    assert torch.equal(check, dsts[0][:1]), "NV12 plan and the I420 workaround disagree"
    return {
        "shape": name, "channels": 2, "frames": frames, "rotated_buffers": rot, "bytes_per_launch": int(moved),
        "steps": steps, "kernels": {"y": ky, "uv": kuv},
        "nv12": {"ms": round(t_nv, 4), "gbs": round(gbs(moved, t_nv), 1), "of_8tbs": round(gbs(moved, t_nv) / PEAK_GBS, 4)},
        "packed_tile": {"plane": "uv", "ms": round(t_uv, 4), "gbs": round(gbs(moved_uv, t_uv), 1),
                        "of_8tbs": round(gbs(moved_uv, t_uv) / PEAK_GBS, 4)},
        # a planar plan of the UV shape (integer ratio, one phase) runs lanczos_stream; no option
        # leaves it the tile kernel, so there is no planar tile figure for this shape
        "planar_tile": None,
        "workaround": {"ms": round(t_work, 4), "gbs_of_nv12_bytes": round(gbs(moved, t_work), 1)},
        "packed_over_workaround": round(t_work / t_nv, 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the lines as a JSON list")
    ap.add_argument("--only", default=None, help="substring of the shape names to run")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_packed.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    lines = []
    for name, C, dims in SHAPES:
        if args.only and args.only not in name:
            continue
        res = bench_nv12(name, dims, args.steps, dev, stream) if name.startswith("nv12") else \
            bench_rgb(name, C, dims, args.steps, dev, stream)
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
