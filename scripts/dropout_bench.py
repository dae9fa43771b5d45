"""The six dropout entry points (dk_dropout_*) at 256 x 64 x 56 x 56 (the stem-position map) and
256 x 512 x 7 x 7 (the last map), each beside a float4 device copy of the same byte count
(dk_debug_stream_mix, one read stream and one write stream) timed in the same script -- the yardstick:
the layer reads every element once and writes it once, so what it can reach is what a copy of its bytes
reaches, unless the generator's integer multiplies (forty per eight elements) bind
first.  The calls alternate (every entry and its copy once per round), each timed with HIP events after
a warm-up round; median and min-max over the rounds, bytes moved from the shapes, and the ratio of the
entry's rate to its copy's.
    python scripts/dropout_bench.py [--shape N C H W] [--rounds R] [--drop-prob P]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dorknet_amd._hip import lib, stream_handle  # noqa: E402

SHAPES = [(256, 64, 56, 56), (256, 512, 7, 7)]


def bench(N, C, H, W, rounds, p):
    st = stream_handle()
    n = N * C * H * W
    T = int(math.floor(p * 65536.0))
    torch.manual_seed(0)
    x32 = torch.randn((N, C, H, W), device="cuda").contiguous(memory_format=torch.channels_last)
    x16 = x32.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    y32, y16 = torch.empty_like(x32), torch.empty_like(x16)
    bn = [torch.randn(C, device="cuda"), torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda"),
          torch.randn(C, device="cuda")]
    bnp = [t.data_ptr() for t in bn] + [1]
    src, dst = torch.randn(n, device="cuda"), torch.empty(n, device="cuda")  # the copy's streams
    step = [0]

    def copy_of(nbytes):
        numel = nbytes // 8 // 4 * 4  # half the bytes read, half written, whole float4s
        return lambda: lib.dk_debug_stream_mix(src.data_ptr(), 0, 0, dst.data_ptr(), 0, 1, 1, numel, 0, st)

    def mask_args():
        step[0] += 1  # a new mask every call, as in training
        return (n, T, 2024, step[0], 0, 0)

    p32, p16, q32, q16 = x32.data_ptr(), x16.data_ptr(), y32.data_ptr(), y16.data_ptr()
    entries = [
        ("dropout_fwd_f32", 8 * n, lambda: lib.dk_dropout_fwd_f32(p32, *mask_args(), q32, st)),
        ("dropout_fwd_bf16", 4 * n, lambda: lib.dk_dropout_fwd_bf16(p16, *mask_args(), q16, st)),
        ("dropout_fwd_bnx_f32", 8 * n, lambda: lib.dk_dropout_fwd_bnx_f32(p32, *mask_args(), C, *bnp, q32, st)),
        ("dropout_fwd_bnx_bf16", 4 * n, lambda: lib.dk_dropout_fwd_bnx_bf16(p16, *mask_args(), C, *bnp, q16, st)),
        ("dropout_bwd_f32", 8 * n, lambda: lib.dk_dropout_bwd_f32(p32, *mask_args(), q32, st)),
        ("dropout_bwd_bf16", 4 * n, lambda: lib.dk_dropout_bwd_bf16(p16, *mask_args(), q16, st)),
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
    print("{} x {} x {} x {}, drop_prob {}: median of {} alternating rounds".format(N, C, H, W, p, rounds))
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
    ap.add_argument("--drop-prob", type=float, default=0.5)
    a = ap.parse_args()
    if not 0.0 <= a.drop_prob < 1.0:
        ap.error("--drop-prob must lie in [0, 1)")
    for shape in ([tuple(a.shape)] if a.shape else SHAPES):
        bench(*shape, a.rounds, a.drop_prob)


if __name__ == "__main__":
    main()
