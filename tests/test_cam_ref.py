"""Class activation maps, the numpy restatements of tests/_cam_ref.py on the CPU:
the colour table, known answers of the resize, the zero-mask branch, the fp32 restatement (a) against the
reference's code path in fp64 (b) within the bounds derived in the helper's docstring, and the top-k
order.  The GPU kernels are held to (a) bit for bit in tests/test_gpu_cam.py."""
import numpy as np
import pytest

from tests import _cam_ref as ref

import dorknet_amd.cam  # noqa: F401  (the module these restatements pin)


def test_jet_table():
    J = ref.JET
    assert J.shape == (256, 3) and J.dtype == np.uint8
    assert tuple(J[0]) == (128, 0, 0) and tuple(J[255]) == (0, 0, 128)
    assert np.array_equal(J, J[::-1, ::-1])            # JET[i] = JET[255 - i][::-1]
    s = int(np.abs(np.diff(J.astype(np.int64), axis=0)).max())
    assert s == ref.JET_STEP
    assert 1 <= s <= 4                                  # 255 / 64 per index, rounded
    # i = 128 by hand: b = 32/64 -> 127.5 -> 128 (tie to even), g = 1, r = b[127] = 33/64 -> 131.48
    assert J.max() == 255 and tuple(J[128]) == (128, 255, 131)


def test_resize_known_answers():
    rng = np.random.RandomState(0)
    S = rng.standard_normal((5, 7)).astype(np.float32)
    assert np.array_equal(ref.resize(S, 5, 7), S)                       # equal sizes: a copy
    # a constant stays: exactly where the products are exact (a power of two; fl(fl(1 - f) + f) = 1 for
    # every fp32 f in [0, 1)), and for any other constant within the roundings of the two passes (per pass
    # 1 - f, two products and a sum: below 4 u each way, so 8 u |c| in all)
    for c in (np.float32(2.0), np.float32(-0.25)):
        assert np.array_equal(ref.resize(np.full((3, 5), c), 37, 53), np.full((37, 53), c))
    c = np.float32(1.7)
    assert np.abs(ref.resize(np.full((3, 5), c), 37, 53).astype(np.float64) - c).max() <= 8 * ref.U32 * c
    a, b = np.float32(3.0), np.float32(-5.0)                            # exact in fp32 with quarter weights
    row = ref.resize(np.array([[a, b]], dtype=np.float32), 1, 4)
    assert np.array_equal(row, np.array([[a, .75 * a + .25 * b, .25 * a + .75 * b, b]], dtype=np.float32))
    S = rng.standard_normal((3, 5)).astype(np.float32)
    big = ref.resize(S, 37, 53)
    assert big.shape == (37, 53) and big.dtype == np.float32
    assert big.min() >= S.min() and big.max() <= S.max()


def test_map_without_a_positive_value():
    rng = np.random.RandomState(1)
    feat = np.abs(rng.standard_normal((1, 3, 5, 70))).astype(np.float32)
    weights = -np.abs(rng.standard_normal((70, 4))).astype(np.float32)
    image = rng.uniform(-128, 127, size=(1, 3, 11, 13)).astype(np.float32)
    idx = np.array([[2, 0]])
    masks, overlays = ref.cam_f32(feat, weights, idx, image)
    assert np.array_equal(masks, np.zeros((1, 2, 11, 13), dtype=np.float32))
    o = ref.JET[0].astype(np.float32) + (image[0].transpose(1, 2, 0) + np.float32(128))
    want = (np.float32(255) * (o / o.max())).astype(np.uint8)
    assert np.array_equal(overlays[0, 0], want) and np.array_equal(overlays[0, 1], want)


# (N, K, C, (h, w), (H, W)); seeds 0 and 1 each: for these the bounds' preconditions hold (the range of
# every map exceeds its error ER, and 255 * mask bound < 1) and (a), evaluated by numpy, lies inside them
AB_SHAPES = [(2, 3, 96, (3, 5), (37, 53)), (1, 3, 512, (8, 8), (225, 225)), (2, 2, 64, (8, 8), (5, 7))]
AB_SEEDS = [0, 1]


@pytest.mark.parametrize("seed", AB_SEEDS)
@pytest.mark.parametrize("shape", AB_SHAPES, ids=lambda s: "N{}K{}C{}".format(*s[:3]))
def test_fp32_restatement_against_the_fp64_reference(shape, seed):
    N, K, C, (h, w), (H, W) = shape
    rng = np.random.RandomState(100 + seed)
    feat = np.maximum(rng.standard_normal((N, h, w, C)), 0).astype(np.float32)      # a post-ReLU feature map
    weights = (rng.standard_normal((C, 10)) / np.sqrt(C)).astype(np.float32)
    idx = np.stack([rng.permutation(10)[:K] for _ in range(N)])
    images = rng.uniform(-128, 127, size=(N, 3, H, W)).astype(np.float32)
    ma, oa = ref.cam_f32(feat, weights, idx, images)
    mb, ob, aux = ref.cam_f64(feat, weights, idx, images)
    worst_m, worst_o = 0.0, 0.0
    for n in range(N):
        for k in range(K):
            bound, Rb, ER = ref.mask_bound(aux["S"][n, k], aux["A"][n, k], C, H, W, mb[n, k])
            assert Rb > ER and 255 * bound.max() + 255 * ref.U32 < 1, (n, k, Rb, ER, bound.max())
            err = np.abs(ma[n, k].astype(np.float64) - mb[n, k])
            worst_m = max(worst_m, float((err / bound).max()))
            assert np.all(err <= bound), (n, k, float((err / bound).max()))
            levels = ref.overlay_levels(aux["M"][n, k])
            diff = np.abs(oa[n, k].astype(np.int64) - ob[n, k].astype(np.int64)).max()
            worst_o = max(worst_o, diff / levels)
            assert diff <= levels, (n, k, int(diff), levels)
    print("mask error at most {:.3f} of its bound, overlay at most {:.3f} of its levels".format(worst_m, worst_o))


def test_topk_restatement():
    rng = np.random.RandomState(2)
    scores = rng.permutation(3 * 120).reshape(3, 120).astype(np.float32)           # distinct
    for k in (1, 3, 16):
        want = np.stack([np.argsort(r)[::-1][:k] for r in scores])
        assert np.array_equal(ref.topk_rows(scores, k), want)
    tie = np.array([[0.5, 2.0, 1.0, 2.0, -1.0, 2.0]], dtype=np.float32)
    assert ref.topk_rows(tie, 4).tolist() == [[5, 3, 1, 2]]                        # the higher index first
    assert ref.topk_rows(np.zeros((1, 5), np.float32), 5).tolist() == [[4, 3, 2, 1, 0]]
