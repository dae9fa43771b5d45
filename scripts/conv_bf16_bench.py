"""Dense convolution, bf16 activations against fp32: forward, input gradient and weight gradient of
BASELINE config 2's layer (3x3, 64 -> 64 on 256 x 64 x 56 x 56, stride 1, pad 1) through the unchanged
_f32 entries and the _bf16 entries in one process, the two alternating call by call.

Times are HIP events around single calls after warm-up (median and min/max of --reps calls); the
fraction is the entry's perfmodel bound (max(flops / its MFMA peak, compulsory bytes / HBM spec)) over
the measured time.  The bf16 results are compared with the fp32 ones on the same bf16-representable
inputs (normwise) before anything is timed.

    python scripts/conv_bf16_bench.py [--reps 20] [--out profiles/conv_bf16_bench.md]
    python scripts/conv_bf16_bench.py --sweep   # + every tile configuration for the bf16 entries
                                                # (dk_debug_set_gemm_config kind 0 / 1): the source of
                                                # the kRowConv / split-K bf16 rules in gemm_engine.h
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dorknet_amd import perfmodel  # noqa: E402
from dorknet_amd._hip import lib, stream_handle  # noqa: E402

BF16 = torch.bfloat16


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def time_pair(fns, reps, warmup=3):
    """Median / min / max microseconds of each callable, the callables alternating call by call."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
          for _ in fns]
    for r in range(reps):
        for i, f in enumerate(fns):
            a, b = ev[i][r]
            a.record()
            f()
            b.record()
    torch.cuda.synchronize()
    out = []
    for e in ev:
        t = sorted(1e3 * a.elapsed_time(b) for a, b in e)
        out.append((t[len(t) // 2], t[0], t[-1]))
    return out


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "conv_bf16_bench.md"))
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--shape", type=int, nargs=4, default=[256, 64, 56, 64], metavar=("N", "C", "HW", "K"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_bf16_bench.py times kernels on an MI355X; no HIP device is visible")
    N, C, H, K = a.shape
    W, R, S, stride, pad = H, 3, 3, 1, 1
    OH, OW = H, W
    st = stream_handle()
    torch.manual_seed(0)
    xh = nhwc(torch.randn(N, C, H, W, device="cuda").to(BF16))
    dyh = nhwc(torch.randn(N, K, OH, OW, device="cuda").to(BF16))
    xf, dyf = nhwc(xh.float()), nhwc(dyh.float())
    w = torch.randn(K, C, R, S, device="cuda") * 0.05
    w_krsc = torch.empty(K, R, S, C, device="cuda")
    w_crsk = torch.empty(C, R, S, K, device="cuda")
    lib.dk_conv_weight_krsc_f32(w.data_ptr(), K, C, R, S, C, w_krsc.data_ptr(), st)
    lib.dk_conv_weight_crsk_f32(w.data_ptr(), K, C, R, S, w_crsk.data_ptr(), st)
    yf, yh = nhwc(torch.empty(N, K, OH, OW, device="cuda")), nhwc(torch.empty(N, K, OH, OW, device="cuda", dtype=BF16))
    dxf, dxh = torch.empty_like(xf), torch.empty_like(xh)
    dwf, dwh = torch.empty_like(w), torch.empty_like(w)
    z = (0, 0, 0, 0, 0, 0)
    nbf = lib.dk_conv2d_wgrad_workspace_bytes(N, OH, OW, K, C, R, S)
    wsf = torch.empty(max(nbf, 256), dtype=torch.uint8, device="cuda")
    ws = {"h": None}

    def bf16_ws():  # (the bf16 split follows the split-K knob: query after setting it)
        nb = lib.dk_conv2d_wgrad_bf16_workspace_bytes(N, OH, OW, K, C, R, S)
        if ws["h"] is None or ws["h"].numel() < nb:
            ws["h"] = torch.empty(max(nb, 256), dtype=torch.uint8, device="cuda")
        return ws["h"].data_ptr(), nb

    calls = {
        "fwd": ("dk_conv2d_fwd_ex_f32", lambda: (xf.data_ptr(), N, H, W, C, w_krsc.data_ptr(), K, R, S, stride, pad, 0,
                                                 yf.data_ptr(), OH, OW, *z, st),
                "dk_conv2d_fwd_ex_bf16", lambda: (xh.data_ptr(), N, H, W, C, w_krsc.data_ptr(), K, R, S, stride, pad, 0,
                                                  yh.data_ptr(), OH, OW, *z, st)),
        "dgrad": ("dk_conv2d_dgrad_f32", lambda: (dyf.data_ptr(), N, OH, OW, K, w_crsk.data_ptr(), C, R, S, pad,
                                                  dxf.data_ptr(), H, W, st),
                  "dk_conv2d_dgrad_bf16", lambda: (dyh.data_ptr(), N, OH, OW, K, w_crsk.data_ptr(), C, R, S, pad,
                                                   dxh.data_ptr(), H, W, st)),
        "wgrad": ("dk_conv2d_wgrad_f32", lambda: (dyf.data_ptr(), xf.data_ptr(), N, H, W, C, C, K, R, S, stride, pad, OH,
                                                  OW, 0, 0.0, dwf.data_ptr(), wsf.data_ptr(), nbf, st),
                  "dk_conv2d_wgrad_bf16", lambda: (dyh.data_ptr(), xh.data_ptr(), N, H, W, C, C, K, R, S, stride, pad,
                                                   OH, OW, 0, 0.0, dwh.data_ptr(), *bf16_ws(), st)),
    }
    outs = {"fwd": (yh, yf), "dgrad": (dxh, dxf), "wgrad": (dwh, dwf)}
    lines = ["# Dense convolution: bf16 activations against fp32",
             "",
             "scripts/conv_bf16_bench.py{}: 3x3 stride 1 pad 1, {} -> {} channels on {} x {} x {} x {}{},"
             .format(" --sweep" if a.sweep else "", C, K, N, C, H, W,
                     " (BASELINE config 2's layer)" if a.shape == [256, 64, 56, 64] else ""),
             "device 0 ({}).  HIP-event time of single calls after 3 warm-up calls, median [min, max] of {}"
             .format(getattr(torch.cuda.get_device_properties(0), "gcnArchName", torch.cuda.get_device_name(0)), a.reps),
             "calls, the fp32 and bf16 entries alternating.  bound = perfmodel (max of flops over the entry's MFMA",
             "peak -- {:.0f} TF/s fp32, {:.0f} TF/s bf16 -- and compulsory bytes over {:.0f} GB/s); frac = bound / time."
             .format(perfmodel.PEAK_F32_TFLOPS, perfmodel.PEAK_BF16_TFLOPS, perfmodel.PEAK_HBM_GBS),
             "",
             "| pass | fp32 entry | us | bound us | frac | bf16 entry | us | bound us | frac | fp32 / bf16 | bf16 vs fp32 result |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, (nf, af, nh, ah) in calls.items():
        ff, fh = getattr(lib, nf), getattr(lib, nh)
        ff(*af())
        fh(*ah())
        torch.cuda.synchronize()
        err = rel(outs[name][0], outs[name][1])
        (tf, tf0, tf1), (th, th0, th1) = time_pair([lambda: ff(*af()), lambda: fh(*ah())], a.reps)
        bf_ = 1e6 * perfmodel.bound_time_s(*perfmodel.work(nf, af()), nf)
        bh_ = 1e6 * perfmodel.bound_time_s(*perfmodel.work(nh, ah()), nh)
        lines.append("| {} | {} | {:.1f} [{:.1f}, {:.1f}] | {:.1f} | {:.3f} | {} | {:.1f} [{:.1f}, {:.1f}] | {:.1f} | {:.3f} | "
                     "{:.2f} | {:.2e} normwise |".format(name, nf, tf, tf0, tf1, bf_, bf_ / tf, nh, th, th0, th1, bh_,
                                                         bh_ / th, tf / th, err))
        print(lines[-1], flush=True)
    if a.sweep:
        lines += ["", "## Tile sweep of the bf16 entries", "",
                  "dk_debug_set_gemm_config(0, id) (row configurations: forward, dgrad) and (1, id) (split-K",
                  "configurations: weight gradient); `default` = the built-in rule.  id: BM x BN x BK, WM x WN waves as",
                  "in DK_ROW_CONFIGS / DK_SPLITK_CONFIGS (gemm_engine.h).  us: median [min, max].", "",
                  "| pass | config | us |", "|---|---|---|"]
        nrow = lib.dk_debug_set_gemm_config(0, -1)
        nsplit = lib.dk_debug_set_gemm_config(1, -1)
        for name, kind, n in (("fwd", 0, nrow), ("dgrad", 0, nrow), ("wgrad", 1, nsplit)):
            _, _, nh, ah = calls[name]
            fh = getattr(lib, nh)
            for cfg in [-1] + list(range(n)):
                lib.dk_debug_set_gemm_config(kind, cfg)
                try:
                    (t, t0, t1), = time_pair([lambda: fh(*ah())], a.reps)
                    cell = "{:.1f} [{:.1f}, {:.1f}]".format(t, t0, t1)
                except Exception as e:
                    if "10001" not in str(e):  # anything but a refused configuration ends the run
                        raise
                    cell = "refused (bad arguments)"
                finally:
                    lib.dk_debug_set_gemm_config(kind, -1)
                lines.append("| {} | {} | {} |".format(name, "default" if cfg < 0 else cfg, cell))
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
