"""Evaluation on the GPU, measured:

(a) the counter kernel alone, dk_classify_accumulate_f32 at 60 x 120 (the reference's evaluation batch and
    the model's head), 256 x 120 and 2048 x 1000, with and without the confusion matrix;
(b) evaluation throughput: ResNet-18-depsep at 225 x 225 over 20 device-resident batches of 60 images,
    FeedForwardNetwork.evaluate (device-side counters, one read at the end) against FeedForwardNetwork.test
    (the reference's loop: every batch's scores copied to the host), alternating in the same process.

The rows of (a) take turns within a round, each timed with HIP events; (b) is timed with HIP events around
the whole call (it ends with its own synchronisation either way).  One warm-up round, then median and
min-max over the rounds.  The report is printed and written to --out.
    python scripts/eval_bench.py [--rounds R] [--batches B] [--batch N] [--bf16] [--out profiles/eval_bench.txt]
"""
import argparse
import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dorknet_amd._hip import lib, require_gpu, stream_handle  # noqa: E402


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)   # us


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--batch", type=int, default=60)
    ap.add_argument("--size", type=int, default=225)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.txt"))
    a = ap.parse_args()
    require_gpu()
    st = stream_handle()
    rng = np.random.RandomState(0)

    # (a) the kernel alone
    calls = []
    keep = []
    for N, classes in ((60, 120), (256, 120), (2048, 1000)):
        e = np.exp(2.0 * rng.standard_normal((N, classes)))
        s = torch.from_numpy((e / e.sum(axis=1, keepdims=True)).astype(np.float32)).cuda()
        y = torch.from_numpy(rng.randint(0, classes, size=N).astype(np.int32)).cuda()
        state = torch.zeros(22, dtype=torch.int64, device="cuda")
        conf = torch.zeros((classes, classes), dtype=torch.int64, device="cuda")
        keep.append((s, y, state, conf))
        for name, c in (("counters", 0), ("counters + confusion", conf.data_ptr())):
            calls.append(("{} x {}, {}".format(N, classes, name),
                          lambda s=s, y=y, state=state, c=c, N=N, classes=classes: lib.dk_classify_accumulate_f32(
                              s.data_ptr(), y.data_ptr(), N, classes, state.data_ptr(), c, 0, 0, 0, st)))
    times = {name: [] for name, _ in calls}
    for r in range(a.rounds + 1):   # round 0 is the warm-up
        for name, f in calls:
            t = timed(f)
            if r:
                times[name].append(t)
    lines = ["dk_classify_accumulate_f32: median (min - max) of {} alternating rounds".format(a.rounds)]
    for name, _ in calls:
        lines.append("  {:36s} {:8.1f} us  ({:.1f} - {:.1f})".format(name, *stats(times[name])))

    # (b) evaluate against test
    from examples.resnet18_depsep import ResNet18, synthetic_batch
    np.random.seed(0)
    net = ResNet18("eval_bench")
    net.to_gpu()
    loader = []
    for i in range(a.batches):
        X, y, onehot = synthetic_batch(a.batch, seed=i, size=a.size)
        X = torch.as_tensor(X, device="cuda")
        if a.bf16:
            X = X.to(torch.bfloat16)
        loader.append((X, y.tolist(), None))
        if i == 0:   # one training-mode pass: the running statistics exist from the first batch on
            net.forward(X, torch.as_tensor(onehot, device="cuda"))
    images = a.batch * a.batches
    results = {}

    def run_evaluate():
        results["evaluate"] = net.evaluate(loader).accuracy

    def run_test():
        with contextlib.redirect_stderr(io.StringIO()):   # test's progress bar
            results["test"] = net.test(loader, a.batch, images)

    rows = [("evaluate", run_evaluate), ("test", run_test)]
    times = {name: [] for name, _ in rows}
    for r in range(a.rounds + 1):
        for name, f in rows:
            t = timed(f)
            if r:
                times[name].append(t)
    lines.append("ResNet-18-depsep {0} x {0}, {1} device-resident batches of {2}{3}: median (min - max) of {4} "
                 "alternating rounds".format(a.size, a.batches, a.batch, ", bf16 input" if a.bf16 else "", a.rounds))
    for name, _ in rows:
        m, lo, hi = stats(times[name])
        lines.append("  net.{:10s} {:9.2f} ms  ({:.2f} - {:.2f})  {:9.1f} images/s  ({:.1f} - {:.1f})".format(
            name, m / 1e3, lo / 1e3, hi / 1e3, images / (m * 1e-6), images / (hi * 1e-6), images / (lo * 1e-6)))
    lines.append("  accuracy: evaluate {!r}, test {!r}".format(results["evaluate"], results["test"]))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
