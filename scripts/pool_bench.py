"""The six max-pooling entry points (dk_maxpool_*) at the stem-position shape 256 x 64 x 112 x 112,
stride 2, fp32 and bf16, beside dk_bn_apply_* (relu = 1) on the same tensor -- the pass the fused
_bnx forward replaces, and the yardstick: the fused forward reads the same x and writes a quarter of
y plus one location byte per output element, where the apply writes all of y.  The calls alternate
(every entry once per round), each timed with HIP events after a warm-up round; median and min-max
over the rounds, bytes moved from the shapes, and the share of the HBM peak (8.0 TB/s; a float4 copy
measures 6.29 TB/s).
    python scripts/pool_bench.py [--shape N C H W] [--stride S] [--rounds R]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dorknet_amd._hip import lib, stream_handle  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def bench(dtype, N, C, H, W, s, rounds):
    st = stream_handle()
    bf = dtype == torch.bfloat16
    e = 2 if bf else 4
    sfx = "bf16" if bf else "f32"
    OH, OW = H // s, W // s
    nin, nout = N * C * H * W, N * C * OH * OW
    torch.manual_seed(0)
    x = torch.randn((N, C, H, W), device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
    ya = torch.empty_like(x)
    dx = torch.empty_like(x)
    y = torch.empty((N, C, OH, OW), dtype=dtype, device="cuda", memory_format=torch.channels_last)
    dy = torch.randn((N, C, OH, OW), device="cuda").to(dtype).contiguous(memory_format=torch.channels_last)
    idx = torch.empty((N, C, OH, OW), dtype=torch.uint8, device="cuda", memory_format=torch.channels_last)
    bn = [torch.randn(C, device="cuda"), torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda"),
          torch.randn(C, device="cuda")]
    bnp = [t.data_ptr() for t in bn] + [1]
    fn = lambda name: getattr(lib, "{}_{}".format(name, sfx))  # noqa: E731
    xp, yp, ip = x.data_ptr(), y.data_ptr(), idx.data_ptr()
    pooled = N * C * OH * s * OW * s  # the input elements inside a window
    calls = [
        ("bn_apply (relu)", nin * e * 2,
         lambda: fn("dk_bn_apply")(xp, x.numel(), C, *bnp, ya.data_ptr(), 0, st)),
        ("maxpool_fwd (train)", pooled * e + nout * (e + 1),
         lambda: fn("dk_maxpool_fwd")(xp, N, H, W, C, s, yp, ip, st)),
        ("maxpool_fwd (test)", pooled * e + nout * e,
         lambda: fn("dk_maxpool_fwd")(xp, N, H, W, C, s, yp, 0, st)),
        ("maxpool_fwd_bnx (train)", pooled * e + nout * (e + 1),
         lambda: fn("dk_maxpool_fwd_bnx")(xp, N, H, W, C, s, *bnp, yp, ip, st)),
        ("maxpool_fwd_bnx (test)", pooled * e + nout * e,
         lambda: fn("dk_maxpool_fwd_bnx")(xp, N, H, W, C, s, *bnp, yp, 0, st)),
        ("maxpool_bwd", nout * (e + 1) + nin * e,
         lambda: fn("dk_maxpool_bwd")(dy.data_ptr(), ip, N, H, W, C, s, dx.data_ptr(), st)),
    ]
    times = {name: [] for name, _, _ in calls}
    for r in range(rounds + 1):  # round 0 is the warm-up
        for name, _, f in calls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            if r:
                times[name].append(1e3 * a.elapsed_time(b))
    print("{} x {} x {} x {} stride {} {}: median of {} alternating rounds".format(N, C, H, W, s, sfx, rounds))
    med = {}
    for name, nbytes, _ in calls:
        t = sorted(times[name])
        m = t[len(t) // 2]
        med[name] = m
        print("  {:26s} {:8.1f} us  (min {:8.1f}, max {:8.1f})  {:7.1f} MB  {:5.2f} TB/s  {:4.1f} % of peak".format(
            name, m, t[0], t[-1], nbytes / 1e6, nbytes / m / 1e6, 100 * nbytes / (m * 1e-6) / HBM_PEAK))
    print("  unfused bn_apply + maxpool_fwd (train): {:.1f} us; fused maxpool_fwd_bnx (train): {:.1f} us".format(
        med["bn_apply (relu)"] + med["maxpool_fwd (train)"], med["maxpool_fwd_bnx (train)"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[256, 64, 112, 112], metavar=("N", "C", "H", "W"))
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()
    for dtype in (torch.float32, torch.bfloat16):
        bench(dtype, *a.shape, a.stride, a.rounds)


if __name__ == "__main__":
    main()
