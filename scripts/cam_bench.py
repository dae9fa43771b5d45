"""The class activation map kernel at the reference's shape: 60 images x 3 classes, 8 x 8 x 512 features
enlarged to 225 x 225 (the flagship script's batch, one map per workgroup).  Rows:

    masks + overlays   dk_cam_f32 with both outputs (what FeedForwardNetwork.class_activation_maps runs);
    overlays alone     the mask store left out;
    masks alone        no image: the second sweep and the overlay stores left out;
    bf16 features      dk_cam_bf16 with both outputs;
    top-k              dk_topk_rows_f32, 60 x 120 scores, K = 3.

The calls alternate (every row once per round), each timed with HIP events after a warm-up round; median
and min-max over the rounds.  Bytes moved are counted from the shapes -- the features and the image read
twice (the second and third sweep; the three maps of an image share it, so most of those reads are served
on chip), the mask and the overlay written once -- and set against the HBM peak (8.0 TB/s; a float4 copy
measures 6.29 TB/s).  There is nothing to compare against: the reference does this on the host, one image
at a time.  The report is printed and written to --out.
    python scripts/cam_bench.py [--shape N K C h w H W] [--rounds R] [--out profiles/cam_bench.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dorknet_amd._hip import lib, require_gpu, stream_handle  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=7, default=[60, 3, 512, 8, 8, 225, 225],
                    metavar=("N", "K", "C", "h", "w", "H", "W"))
    ap.add_argument("--classes", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cam_bench.txt"))
    a = ap.parse_args()
    require_gpu()
    N, K, C, h, w, H, W = a.shape
    st = stream_handle()
    rng = np.random.RandomState(0)
    feat = torch.from_numpy(np.maximum(rng.standard_normal((N, h, w, C)), 0).astype(np.float32)).cuda()
    feat16 = feat.to(torch.bfloat16)
    wts = torch.from_numpy((rng.standard_normal((C, a.classes)) / np.sqrt(C)).astype(np.float32)).cuda()
    scores = torch.from_numpy(rng.standard_normal((N, a.classes)).astype(np.float32)).cuda()
    idx = torch.empty((N, K), dtype=torch.int32, device="cuda")
    img = torch.from_numpy(rng.uniform(-128, 127, size=(N, 3, H, W)).astype(np.float32)).cuda()
    mask = torch.empty((N, K, H, W), dtype=torch.float32, device="cuda")
    over = torch.empty((N, K, H, W, 3), dtype=torch.uint8, device="cuda")

    def topk():
        lib.dk_topk_rows_f32(scores.data_ptr(), N, a.classes, K, idx.data_ptr(), st)

    def cam(entry, f, image, m, o):
        entry(f.data_ptr(), N, h, w, C, wts.data_ptr(), a.classes, idx.data_ptr(), K, image, H, W, 128.0, m, o, st)

    px = N * K * H * W
    fbytes, ibytes = N * K * h * w * C * 4, 2 * px * 12
    calls = [
        ("masks + overlays", fbytes + ibytes + px * 4 + px * 3,
         lambda: cam(lib.dk_cam_f32, feat, img.data_ptr(), mask.data_ptr(), over.data_ptr())),
        ("overlays alone", fbytes + ibytes + px * 3, lambda: cam(lib.dk_cam_f32, feat, img.data_ptr(), 0, over.data_ptr())),
        ("masks alone", fbytes + px * 4, lambda: cam(lib.dk_cam_f32, feat, 0, mask.data_ptr(), 0)),
        ("bf16 features", fbytes // 2 + ibytes + px * 4 + px * 3,
         lambda: cam(lib.dk_cam_bf16, feat16, img.data_ptr(), mask.data_ptr(), over.data_ptr())),
        ("top-k", N * a.classes * 4 + N * K * 4, topk),
    ]
    topk()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in calls}
    for r in range(a.rounds + 1):  # round 0 is the warm-up
        for name, _, f in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if r:
                times[name].append(1e3 * e0.elapsed_time(e1))
    lines = ["{} images x {} classes, {} x {} x {} features -> {} x {}, {} classes: median of {} alternating rounds".format(
        N, K, h, w, C, H, W, a.classes, a.rounds)]
    for name, nbytes, _ in calls:
        t = sorted(times[name])
        m = t[len(t) // 2]
        lines.append("  {:18s} {:8.1f} us  (min {:8.1f}, max {:8.1f})  {:7.2f} MB  {:5.2f} TB/s  {:4.1f} % of the HBM peak".format(
            name, m, t[0], t[-1], nbytes / 1e6, nbytes / m / 1e6, 100 * nbytes / (m * 1e-6) / HBM_PEAK))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
