"""The six flatten entry points (dk_flatten_*) at 256 x 64 x 56 x 56 (the stem-position map) and
256 x 512 x 7 x 7 (the last map: HW = 49, no flat row 16-byte aligned), each beside a float4 device copy
of the same byte count (dk_debug_stream_mix, one read stream and one write stream) timed in the same
script -- the yardstick: the flatten is pure data movement, so what it can reach is what a copy of its
bytes reaches.  The calls alternate (every entry and its copy once per round), each timed with HIP
events after a warm-up round; median and min-max over the rounds, bytes moved from the shapes, and the
ratio of the entry's rate to its copy's.
    python scripts/reshape_bench.py [--shape N C H W] [--rounds R]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dorknet_amd._hip import lib, stream_handle  # noqa: E402

SHAPES = [(256, 64, 56, 56), (256, 512, 7, 7)]


def bench(N, C, H, W, rounds):
    st = stream_handle()
    HW, n = H * W, N * C * H * W
    torch.manual_seed(0)
    x32 = torch.randn((N, C, H, W), device="cuda").contiguous(memory_format=torch.channels_last)
    x16 = x32.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    flat = torch.randn((N, C * HW), device="cuda")
    y = torch.empty((N, C * HW), device="cuda")
    dx32, dx16 = torch.empty_like(x32), torch.empty_like(x16)
    bn = [torch.randn(C, device="cuda"), torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda"),
          torch.randn(C, device="cuda")]
    bnp = [t.data_ptr() for t in bn] + [1]
    src, dst = torch.randn(2 * n, device="cuda"), torch.empty(2 * n, device="cuda")  # the copy's streams

    def copy_of(nbytes):
        numel = nbytes // 8 // 4 * 4  # half the bytes read, half written, whole float4s
        return lambda: lib.dk_debug_stream_mix(src.data_ptr(), 0, 0, dst.data_ptr(), 0, 1, 1, numel, 0, st)

    yp, fp = y.data_ptr(), flat.data_ptr()
    entries = [
        ("flatten_fwd_f32", 8 * n, lambda: lib.dk_flatten_fwd_f32(x32.data_ptr(), N, HW, C, yp, st)),
        ("flatten_fwd_bf16", 6 * n, lambda: lib.dk_flatten_fwd_bf16(x16.data_ptr(), N, HW, C, yp, st)),
        ("flatten_fwd_bnx_f32", 8 * n, lambda: lib.dk_flatten_fwd_bnx_f32(x32.data_ptr(), N, HW, C, *bnp, yp, st)),
        ("flatten_fwd_bnx_bf16", 6 * n, lambda: lib.dk_flatten_fwd_bnx_bf16(x16.data_ptr(), N, HW, C, *bnp, yp, st)),
        ("flatten_bwd_f32", 8 * n, lambda: lib.dk_flatten_bwd_f32(fp, N, HW, C, dx32.data_ptr(), st)),
        ("flatten_bwd_bf16", 6 * n, lambda: lib.dk_flatten_bwd_bf16(fp, N, HW, C, dx16.data_ptr(), st)),
    ]
    calls = []
    for name, nbytes, f in entries:
        calls.append((name, nbytes, f))
        calls.append((name + " copy", nbytes, copy_of(nbytes)))
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
    print("{} x {} x {} x {}: median of {} alternating rounds".format(N, C, H, W, rounds))
    med = {}
    for name, nbytes, _ in calls:
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
    for name, nbytes, _ in entries:
        t, m, c = sorted(times[name]), med[name], med[name + " copy"]
        print("  {:22s} {:8.1f} us  (min {:8.1f}, max {:8.1f})  {:7.1f} MB  {:5.2f} TB/s   float4 copy of the same "
              "bytes {:8.1f} us  {:5.2f} TB/s   ratio {:4.2f}".format(name, m, t[0], t[-1], nbytes / 1e6,
                                                                     nbytes / m / 1e6, c, nbytes / c / 1e6, c / m))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=None, metavar=("N", "C", "H", "W"))
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()
    for shape in ([tuple(a.shape)] if a.shape else SHAPES):
        bench(*shape, a.rounds)


if __name__ == "__main__":
    main()
