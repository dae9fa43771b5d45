"""The device-resident image store's batch path, measured per mixup batch pair:

(a) same-size sources (375 x 500, the one case the older chain can run), batch 256, crop 225 of a
    pre-crop of 281: DeviceImageDataLoader.pull_batch(2) against the chain it replaces --
    DeviceImagePreprocessor.preprocess_batch twice, mixup_batches, and for bf16 the two casts -- both
    drawing their crop offsets on the host, fp32 and bf16;
(b) the same through a ragged store, sizes drawn around 375 x 500 (the chain cannot run this);
(c) the store kernel alone (dk_store_batch_nchw_f32 / dk_store_batch_nhwc_bf16 on tables already on the
    device) with the bytes the algorithm needs -- the source pixels under the two crop windows once and
    the two output batches once -- over its time.

The rows take turns within a round, each timed with HIP events around the whole call; one warm-up
round, then median and min-max over the rounds.  The report is printed and written to --out.
    python scripts/loader_bench.py [--rounds R] [--batch N] [--out profiles/loader_bench.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dorknet_amd._hip import lib, require_gpu, stream_handle  # noqa: E402
from dorknet_amd.data_loading.device_loader import DeviceImageDataLoader  # noqa: E402
from dorknet_amd.data_loading.device_pipeline import DeviceImagePreprocessor, mixup_batches  # noqa: E402
from dorknet_amd.data_loading.device_store import DeviceImageStore  # noqa: E402


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


def needed_bytes(store, plan, loader, out_bytes):
    """Source bytes under the crop windows of both batches, read once, plus both outputs written once."""
    (TH, TW), (OH, OW) = loader.target, loader.window
    src = 0.0
    for half in (plan.a, plan.b):
        hw = store.shapes[half.indices].astype(np.float64)
        src += float(np.sum(hw[:, 0] * (OH / TH) * hw[:, 1] * (OW / TW))) * store.channels
    return src + 2 * len(plan.a.indices) * store.channels * OH * OW * out_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=225)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loader_bench.txt"))
    a = ap.parse_args()
    require_gpu()
    N, classes = a.batch, 120
    rng = np.random.RandomState(0)
    same = rng.randint(0, 256, size=(2 * N, 375, 500, 3), dtype=np.uint8)
    labels = rng.randint(0, classes, size=2 * N)
    names = [str(c) for c in range(classes)]
    same_store = DeviceImageStore.from_arrays(list(same), labels, names)
    ragged = []
    for _ in range(2 * N):
        h, w = rng.randint(300, 451), rng.randint(400, 601)
        if rng.uniform() < 0.3:
            h, w = w, h
        ragged.append(rng.randint(0, 256, size=(h, w, 3), dtype=np.uint8))
    ragged_store = DeviceImageStore.from_arrays(ragged, labels, names)
    del ragged
    dense = torch.from_numpy(same).cuda()
    eye = torch.eye(classes, dtype=torch.float32, device="cuda")
    lab = torch.from_numpy(labels).cuda()
    y, y_m = eye[lab[:N]], eye[lab[N:]]   # the chain's one-hot labels, built outside the timed call
    pp = DeviceImagePreprocessor((a.size, a.size), crop_mode="random")
    draws = np.random.RandomState(1)
    keep = {}

    def chain(bf16):
        def run():
            X = pp.preprocess_batch(dense[:N], rng=draws)
            X_m = pp.preprocess_batch(dense[N:], rng=draws)
            out = mixup_batches(X, X_m, y, y_m, draws.uniform(0.0, 0.4))
            if bf16:
                out = (out[0].to(torch.bfloat16), out[1].to(torch.bfloat16)) + out[2:]
            keep["chain"] = out
        return run

    def loader_row(store, dtype):
        ld = DeviceImageDataLoader(store, N, pp, class_balance=False, mixup_range_tuple=(0.0, 0.4), out_dtype=dtype,
                                   rng=draws)

        def run():
            keep["loader"] = list(ld.pull_batch(2))
        return run

    def kernel_row(store, dtype):
        ld = DeviceImageDataLoader(store, N, pp, class_balance=False, mixup_range_tuple=(0.0, 0.4), out_dtype=dtype,
                                   rng=np.random.RandomState(2))
        plan = ld.plan_batch()
        tabs = torch.from_numpy(np.concatenate([plan.a.table, plan.b.table])).cuda()
        bf16 = dtype == torch.bfloat16
        fmt = torch.channels_last if bf16 else torch.contiguous_format
        X = [torch.empty((N, 3, a.size, a.size), dtype=dtype, device="cuda", memory_format=fmt) for _ in range(2)]
        entry = lib.dk_store_batch_nhwc_bf16 if bf16 else lib.dk_store_batch_nchw_f32
        (TH, TW), (OH, OW) = ld.target, ld.window
        p, q = float(np.float32(plan.prop)), float(np.float32(1 - plan.prop))
        keep[("k", id(store), bf16)] = (tabs, X)

        def run():
            entry(store.data.data_ptr(), store.table.data_ptr(), len(store), 3, tabs.data_ptr(), tabs[N:].data_ptr(), N,
                  TH, TW, OH, OW, 128.0, p, q, X[0].data_ptr(), X[1].data_ptr(), stream_handle())
        return run, needed_bytes(store, plan, ld, 2 if bf16 else 4)

    rows, nbytes = [], {}
    for tag, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        rows.append(("same size, {}: older chain".format(tag), chain(dtype == torch.bfloat16)))
        rows.append(("same size, {}: loader".format(tag), loader_row(same_store, dtype)))
        rows.append(("ragged,    {}: loader".format(tag), loader_row(ragged_store, dtype)))
        for what, store in (("same size", same_store), ("ragged,   ", ragged_store)):
            name = "{} {}: store kernel alone".format(what, tag)
            f, nbytes[name] = kernel_row(store, dtype)
            rows.append((name, f))
    times = {name: [] for name, _ in rows}
    for r in range(a.rounds + 1):   # round 0 is the warm-up
        for name, f in rows:
            t = timed(f)
            if r:
                times[name].append(t)
    lines = ["one mixup batch pair, batch {} x 3 x {} x {} from {} x 500-ish uint8 sources: median (min - max) of {} "
             "alternating rounds".format(N, a.size, a.size, 375, a.rounds)]
    for name, _ in rows:
        m, lo, hi = stats(times[name])
        line = "  {:40s} {:9.1f} us  ({:.1f} - {:.1f})".format(name, m, lo, hi)
        if name in nbytes:
            line += "  {:.1f} MB needed, {:.2f} TB/s".format(nbytes[name] / 1e6, nbytes[name] / (m * 1e-6) / 1e12)
        lines.append(line)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
