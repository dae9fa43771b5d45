"""The image augmentation entry points at the flagship input shape: a 256 x 281 x 281 x 3 uint8 batch
(the pre-crop size of 225 x 225 images), random 225 x 225 crop windows, the flagship script's augmenter
(HSV perturbation 0.9-1.1 / 0.5-2 / 0.5-2, rotation +-15 degrees, flip 0.5), fp32 NCHW out.  Rows:

    cast alone        dk_u8_nhwc_to_nchw_f32 (crop + cast + layout): the pipeline without augmentation,
                      and the yardstick -- that kernel is the one the pipeline has always run;
    augment, cast     dk_augment_u8 (crop + augment to a uint8 batch), then dk_u8_nhwc_to_nchw_f32 on it;
    fused             dk_augment_u8_to_nchw_f32 (crop + augment + cast in one kernel).

The calls alternate (every row once per round), each timed with HIP events after a warm-up round; median
and min-max over the rounds, bytes moved from the shapes, the share of the HBM peak (8.0 TB/s; a float4
copy measures 6.29 TB/s) and the share of the 7.73 ms fp32 training step.  The two augmented forms must
agree bit for bit; that is checked first.
--augmenter hsv / rotation / flip runs one step of the flagship augmenter alone (what each costs).
    python scripts/augment_bench.py [--shape N H W] [--crop R] [--rounds K] [--augmenter flagship]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dorknet_amd._hip import lib, require_gpu, stream_handle  # noqa: E402
from dorknet_amd.data_loading.device_augmentation import DeviceImageAugmenter  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s
STEP_MS = 7.73     # the fp32 ResNet-18-depsep training step at batch 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[256, 281, 281], metavar=("N", "H", "W"))
    ap.add_argument("--crop", type=int, default=225)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--augmenter", choices=["flagship", "hsv", "rotation", "flip"], default="flagship")
    a = ap.parse_args()
    require_gpu()
    N, H, W = a.shape
    R = a.crop
    st = stream_handle()
    rng = np.random.RandomState(0)
    x = torch.from_numpy(rng.randint(0, 256, size=(N, H, W, 3)).astype(np.uint8)).cuda()
    crop = torch.from_numpy(np.stack([rng.randint(0, H - R, N), rng.randint(0, W - R, N)], 1).astype(np.int32)).cuda()
    opts = dict(hsv_pert_tuples=((0.9, 1.1), (0.5, 2), (0.5, 2)), rotation_tuple=(-15, 15), horizontal_flip_prob=0.5)
    only = {"hsv": "hsv_pert_tuples", "rotation": "rotation_tuple", "flip": "horizontal_flip_prob"}.get(a.augmenter)
    aug = DeviceImageAugmenter(**({only: opts[only]} if only else opts))
    tab = torch.from_numpy(aug.pack(aug.draw(N, rng), R, R).view(np.uint8)).cuda()
    u8 = torch.empty((N, R, R, 3), dtype=torch.uint8, device="cuda")
    y_cast = torch.empty((N, 3, R, R), dtype=torch.float32, device="cuda")
    y_two = torch.empty_like(y_cast)
    y_fused = torch.empty_like(y_cast)
    xp, cp, tp = x.data_ptr(), crop.data_ptr(), tab.data_ptr()

    def cast_alone():
        lib.dk_u8_nhwc_to_nchw_f32(xp, N, H, W, 3, cp, R, R, 128.0, y_cast.data_ptr(), st)

    def augment_u8():
        lib.dk_augment_u8(xp, N, H, W, 3, cp, R, R, tp, u8.data_ptr(), st)

    def two_kernels():
        augment_u8()
        lib.dk_u8_nhwc_to_nchw_f32(u8.data_ptr(), N, R, R, 3, 0, R, R, 128.0, y_two.data_ptr(), st)

    def fused():
        lib.dk_augment_u8_to_nchw_f32(xp, N, H, W, 3, cp, R, R, tp, 128.0, y_fused.data_ptr(), st)

    px = N * R * R
    calls = [
        ("cast alone", px * 3 + px * 12, cast_alone),
        ("augment to uint8 alone", px * 3 + px * 3, augment_u8),
        ("augment, cast (2 kernels)", px * 3 + px * 3 + px * 3 + px * 12, two_kernels),
        ("fused augment + cast", px * 3 + px * 12, fused),
    ]
    two_kernels()
    fused()
    torch.cuda.synchronize()
    if not torch.equal(y_two, y_fused):
        raise SystemExit("the fused and the two-kernel outputs differ")
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
    print("{} x {} x {} x 3 uint8, {} x {} windows, {} augmenter, fp32 NCHW out: median of {} alternating rounds".format(
        N, H, W, R, R, a.augmenter, a.rounds))
    med = {}
    for name, nbytes, _ in calls:
        t = sorted(times[name])
        m = med[name] = t[len(t) // 2]
        print("  {:28s} {:8.1f} us  (min {:8.1f}, max {:8.1f})  {:6.1f} MB  {:5.2f} TB/s  {:4.1f} % of peak  "
              "{:5.2f} % of the {} ms step".format(name, m, t[0], t[-1], nbytes / 1e6, nbytes / m / 1e6,
                                                    100 * nbytes / (m * 1e-6) / HBM_PEAK, 100 * m / (STEP_MS * 1e3),
                                                    STEP_MS))
    f, t2, c = med["fused augment + cast"], med["augment, cast (2 kernels)"], med["cast alone"]
    print("  fused / two kernels: {:.2f}; fused - cast alone: {:+.1f} us; the fused form {} the two-kernel form".format(
        f / t2, f - c, "beat" if f < t2 else "did not beat"))


if __name__ == "__main__":
    main()
