"""Host cost of one resize_device call (a launch-bound tiny frame): microseconds per call, median of 7 x 4000 calls."""
import statistics, sys, time
import torch
sys.path.insert(0, ".")
import libiqo_amd
dev = torch.device("cuda:0")
out = []
for name, args, kw in (("tile 16x8->16x16", ("lanczos", 4, 16, 8, 16, 16, 1), {}),
                       ("up2 16x5->48x15", ("lanczos", 2, 16, 5, 48, 15, 1), {}),
                       ("ryx 17x36->16x16", ("area", 0, 17, 36, 16, 16, 1), {}),
                       ("symb 512x32->256x16", ("lanczos", 3, 512, 32, 256, 16, 1), {}),
                       ("packed_tile c3 40x24->27x17", ("lanczos", 3, 40, 24, 27, 17, 1), {"channels": 3})):
    r = libiqo_amd.make_resizer(*args, **kw)
    C = kw.get("channels", 1)
    sw, sh, dw, dh = args[2:6]
    src = torch.zeros((4, sh, sw * C), dtype=torch.uint8, device=dev)
    dst = torch.zeros((4, dh, dw * C), dtype=torch.uint8, device=dev)
    call = lambda: r.resize_device(4, sw * C, sw * C * sh, src, dw * C, dw * C * dh, dst)
    for _ in range(500):
        call()
    torch.cuda.synchronize()
    t = []
    for _ in range(7):
        t0 = time.perf_counter()
        for _ in range(4000):
            call()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) / 4000 * 1e6)
    out.append("%s %.2f" % (name.split()[0], statistics.median(t)))
print("us/call  " + "  ".join(out))
