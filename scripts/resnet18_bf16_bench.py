"""ResNet-18-depsep with bf16 activation storage against fp32, in one process:

  * the training step (forward, backward, SGD-momentum update) at batch 256, fp32 input and bf16 input, the
    weights, batch and optimiser of bench.py's config 3; HIP events around --steps steps after --warmup
    untimed ones, the two storage types alternating round by round (--rounds);
  * the per-entry breakdown of one bf16 step (bench.py's Instrument: every C-ABI call bracketed by HIP
    events, single-stream), so the bf16 kernels that dominate are known;
  * the residual join pass alone at 256 x 64 x 56 x 56, both BatchNorms on load, ReLU, with mask:
    dk_bn_add_f32 against dk_bn_add_bf16, alternating call by call.  With a mask the bf16 join moves 7
    bytes per element against 13, so its time must not exceed the fp32 join's: the script exits non-zero
    if it does.

    python scripts/resnet18_bf16_bench.py [--batch 256] [--steps 10] [--warmup 10] [--out profiles/resnet18_bf16_bench.md]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
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


def make_step(batch, bf16):
    from examples.resnet18_depsep import ResNet18, synthetic_batch
    from dorknet_amd._tensor import as_device
    from dorknet_amd.optimisers.SGDMomentum import SGDMomentum
    np.random.seed(0)
    net = ResNet18("DogsImageNet225ResNet18DepSep")
    net.to_gpu()
    sgd = SGDMomentum(net, 0.05 * batch / 200.0, 0.9)
    X, _, onehot = synthetic_batch(batch, seed=1000)
    X, onehot = as_device(X), as_device(onehot)
    if bf16:
        X = X.to(BF16)
    last = []

    def step():
        last[:] = net.forward(X, onehot)
        net.backward()
        sgd.update_weights()
    return step, last


def time_steps(step, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def join_bench(reps):
    N, C, H = 256, 64, 56
    st = stream_handle()
    torch.manual_seed(0)
    ah, bh = (nhwc(torch.randn(N, C, H, H, device="cuda").to(BF16)) for _ in range(2))
    af, bf = nhwc(ah.float()), nhwc(bh.float())
    par = [torch.randn(C, device="cuda") * 0.3, torch.rand(C, device="cuda") + 0.5,
           1 + 0.3 * torch.randn(C, device="cuda"), 0.2 * torch.randn(C, device="cuda")]
    pa = tuple(t.data_ptr() for t in par) + (1,)
    pb = tuple(t.data_ptr() for t in par) + (0,)
    yf, yh = torch.empty_like(af), torch.empty_like(ah)
    mf = torch.empty(af.numel(), dtype=torch.uint8, device="cuda")
    mh = torch.empty(af.numel(), dtype=torch.uint8, device="cuda")
    n = af.numel()
    args32 = (af.data_ptr(), *pa, bf.data_ptr(), *pb, n, C, 1, yf.data_ptr(), mf.data_ptr(), st)
    args16 = (ah.data_ptr(), *pa, bh.data_ptr(), *pb, n, C, 1, yh.data_ptr(), mh.data_ptr(), st)
    lib.dk_bn_add_f32(*args32)
    lib.dk_bn_add_bf16(*args16)
    torch.cuda.synchronize()
    same = bool(torch.equal(yf.to(BF16), yh)) and bool(torch.equal(mf, mh))
    (t32, lo32, hi32), (t16, lo16, hi16) = time_pair([lambda: lib.dk_bn_add_f32(*args32),
                                                      lambda: lib.dk_bn_add_bf16(*args16)], reps)
    b32 = 1e6 * perfmodel.bound_time_s(*perfmodel.work("dk_bn_add_f32", args32), "dk_bn_add_f32")
    b16 = 1e6 * perfmodel.bound_time_s(*perfmodel.work("dk_bn_add_bf16", args16), "dk_bn_add_bf16")
    return dict(t32=(t32, lo32, hi32), t16=(t16, lo16, hi16), b32=b32, b16=b16, same=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet18_bf16_bench.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnet18_bf16_bench.py times kernels on an MI355X; no HIP device is visible")
    from bench import Instrument, single_stream
    torch.cuda.set_device(0)
    j = join_bench(a.reps)
    print("join: fp32 {:.1f} us, bf16 {:.1f} us, results agree: {}".format(j["t32"][0], j["t16"][0], j["same"]),
          flush=True)
    step32, last32 = make_step(a.batch, False)
    step16, last16 = make_step(a.batch, True)
    for _ in range(a.warmup):
        step32()
        step16()
    torch.cuda.synchronize()
    loss32, loss16 = float(last32[0]), float(last16[0])
    ms32, ms16 = [], []
    for _ in range(a.rounds):
        ms32.append(time_steps(step32, a.steps))
        ms16.append(time_steps(step16, a.steps))
        print("round: fp32 {:.3f} ms/step, bf16 {:.3f} ms/step".format(ms32[-1], ms16[-1]), flush=True)
    with single_stream():
        with Instrument(perfmodel.MODEL.keys()) as ins:
            step16()
    summ = ins.summary()
    tot = sum(s["ms"] for s in summ.values())
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    dev = getattr(torch.cuda.get_device_properties(0), "gcnArchName", torch.cuda.get_device_name(0))
    lines = ["# ResNet-18-depsep: bf16 activation storage against fp32",
             "",
             "scripts/resnet18_bf16_bench.py, device 0 ({}), one process.".format(dev),
             "",
             "## Training step, batch {}".format(a.batch),
             "",
             "Forward, backward and SGD-momentum update on bench.py's config 3 (weights seed 0, synthetic batch seed",
             "1000); fp32: the batch fed as fp32; bf16: the same batch fed as bf16 (every activation and activation",
             "gradient stored in bf16, parameters / statistics / weight gradients fp32).  HIP events around {} steps"
             .format(a.steps),
             "after {} untimed steps of each, the two alternating for {} rounds; ms per step, median [min, max] of"
             .format(a.warmup, a.rounds),
             "the rounds.  Loss after the warm-up steps: fp32 {:.5f}, bf16 {:.5f}.".format(loss32, loss16),
             "",
             "| storage | ms / step | images / s |",
             "|---|---|---|",
             "| fp32 | {:.3f} [{:.3f}, {:.3f}] | {:.0f} |".format(med(ms32), min(ms32), max(ms32),
                                                                  1e3 * a.batch / med(ms32)),
             "| bf16 | {:.3f} [{:.3f}, {:.3f}] | {:.0f} |".format(med(ms16), min(ms16), max(ms16),
                                                                  1e3 * a.batch / med(ms16)),
             "",
             "fp32 / bf16 step time: {:.3f}.".format(med(ms32) / med(ms16)),
             "",
             "## Per-entry breakdown of one bf16 step",
             "",
             "Every C-ABI call bracketed by HIP events (bench.py's Instrument), weight gradients and skip projections",
             "on the launch stream (single_stream) so an entry's events time only its own kernels; bound = perfmodel",
             "(max of flops over the entry's peak and compulsory bytes over {:.0f} GB/s); frac = bound / time.  Total"
             .format(perfmodel.PEAK_HBM_GBS),
             "instrumented: {:.3f} ms.".format(tot),
             "",
             "| entry | calls | ms | share | bound ms | frac |",
             "|---|---|---|---|---|---|"]
    for n, s in sorted(summ.items(), key=lambda kv: -kv[1]["ms"]):
        lines.append("| `{}` | {} | {:.3f} | {:.1%} | {:.3f} | {:.3f} |".format(
            n, s["calls"], s["ms"], s["ms"] / tot, s["bound_ms"], s["bound_ms"] / s["ms"] if s["ms"] else 0.0))
    ok = j["t16"][0] <= j["t32"][0]
    lines += ["",
              "## The residual join pass alone",
              "",
              "y = ReLU(bnA(a) + bnB(b)) with the mask stored, 256 x 64 x 56 x 56, both BatchNorms on load:",
              "`dk_bn_add_f32` (13 bytes per element) against `dk_bn_add_bf16` (7 bytes per element), HIP events",
              "around single calls after 3 warm-up calls, the two alternating; us, median [min, max] of {} calls."
              .format(a.reps),
              "y and the mask agree with the fp32 entry's (y rounded to bf16): {}.".format(j["same"]),
              "",
              "| entry | us | bound us | frac |",
              "|---|---|---|---|",
              "| `dk_bn_add_f32` | {:.1f} [{:.1f}, {:.1f}] | {:.1f} | {:.3f} |".format(*j["t32"], j["b32"],
                                                                                    j["b32"] / j["t32"][0]),
              "| `dk_bn_add_bf16` | {:.1f} [{:.1f}, {:.1f}] | {:.1f} | {:.3f} |".format(*j["t16"], j["b16"],
                                                                                     j["b16"] / j["t16"][0]),
              "",
              "Condition (the bf16 join moves 7 bytes per element against 13, so it must not take longer than the",
              "fp32 join measured in the same run): bf16 {:.1f} us <= fp32 {:.1f} us -- {}.".format(
                  j["t16"][0], j["t32"][0], "met" if ok else "NOT met")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[-14:]))
    print("wrote", a.out)
    if not (ok and j["same"]):
        raise SystemExit("the bf16 join is slower than the fp32 join, or its result differs")


if __name__ == "__main__":
    main()
