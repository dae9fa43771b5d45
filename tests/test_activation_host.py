"""Host checks of the activations beyond ReLU (no GPU): the numpy float32 twin (tests/_activation_twin.py) against
torch CPU fp64 autograd within its derived per-element bounds, the special values it states, the kink margins of the
seeded cases, and the layers' host-only behaviour -- constructor and alpha validation, repr, the h5 + json round
trip, the C declarations and the perfmodel entries."""
import json
import os

import numpy as np
import pytest
import torch

from dorknet_amd import _hip
from dorknet_amd.layers.activations import HardSwish, LeakyReLu, ReLu, ReLu6, SiLu, checked_alpha
from tests import _activation_twin as T
from tests._convert import log_ratio

f32 = np.float32
NAMES = sorted(T.KINDS)
ALPHAS = (0.01, -0.3)


def _worst(got, ref, bound):
    """(err / bound at its worst, index); an error where the bound is 0 counts as infinite, as does a NaN."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    k = int(np.argmax(r))
    return float(r[k]), k


@pytest.fixture(scope="module")
def grid():
    return T.grid()


@pytest.mark.parametrize("name", NAMES)
def test_twin_within_derived_bounds_of_fp64(name, grid):
    """Forward and derivative over 2^20 points of [-30, 30], the bf16 values of [-100, 100] and the finite edge
    values (+-0, the kinks, +-1e4, +-80, +-87).  The bounds are the twin's docstring's; none is fitted."""
    kind = T.KINDS[name]
    assert grid.size >= 2 ** 20 + 1000 and grid.dtype == f32
    for alpha in (ALPHAS if kind == T.LEAKY else (0.01,)):
        y = T.forward(kind, grid, alpha)
        d = T.backward(kind, grid, np.ones_like(grid), alpha)
        ry, rd = T.reference(kind, grid, alpha)
        by, bd = T.bounds(kind, grid, alpha)
        for what, got, ref, bound in (("y", y, ry, by), ("d", d, rd, bd)):
            r, k = _worst(got, ref, bound)
            print("{} {} alpha {}: worst err / bound {:.4f} at v = {!r}".format(name, what, alpha, r, float(grid[k])))
            log_ratio("twin {} {}".format(name, what), r, "act")
            assert r <= 1.0, (name, what, float(grid[k]), float(got[k]), float(ref[k]), float(bound[k]))


def test_twin_constants_and_reduction():
    """The constants are the kernel's (act_math.h), k * C1 is exact and the reduced argument stays below 0.35."""
    assert float(T.SIXTH) == 0.16666667163372039794921875
    assert float(T.LOG2E) == 1.44269502162933349609375
    assert float(T.C2) == -2.12194441701285541057586669921875e-4
    assert float(T.POLY[0]) == 1.98412701138295233249664306640625e-4
    assert float(T.POLY[1]) == 1.388888922519981861114501953125e-3
    assert float(T.POLY[2]) == 8.333333767950534820556640625e-3
    assert float(T.POLY[3]) == 4.16666679084300994873046875e-2
    assert T.CLAMP >= np.exp(-80.0) and T.CLAMP < 1.01 * np.exp(-80.0)
    a = np.linspace(0, 80, 2 ** 18).astype(f32)
    kf = (a * T.LOG2E + T.SHIFT) - T.SHIFT
    assert np.array_equal(kf, np.rint(a * T.LOG2E)) and kf.max() <= 116
    assert np.array_equal((kf * T.C1).astype(np.float64), kf.astype(np.float64) * float(T.C1))
    r = (a - kf * T.C1) - kf * T.C2
    assert np.abs(r).max() <= 0.35
    z = T.exp_neg_abs(np.asarray([0.0, 80.0, 1e4, np.inf, -np.inf], dtype=f32))
    assert z[0] == 1.0 and z[1] == z[2] == z[3] == z[4] and z[1] >= 2.0 ** -126


def test_special_values_are_what_the_twin_states():
    v = np.asarray([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e4, -1e4], dtype=f32)
    dy = np.full(v.shape, 2.0, dtype=f32)
    al = f32(0.25)
    y, g = T.forward(T.LEAKY, v, al), T.backward(T.LEAKY, v, dy, al)
    assert np.isnan(y[0]) and g[0] == 0.5
    assert y[1] == 0 and not np.signbit(y[1]) and y[2] == 0 and np.signbit(y[2]) and g[1] == g[2] == 0.5
    assert y[3] == np.inf and y[4] == -np.inf and g[3] == 2.0 and g[4] == 0.5 and y[5] == 1e4 and y[6] == -2500.0
    y, g = T.forward(T.RELU6, v, al), T.backward(T.RELU6, v, dy, al)
    assert np.isnan(y[0]) and g[0] == 0
    assert y[1] == 0 and not np.signbit(y[1]) and np.signbit(y[2]) and y[3] == 6 and y[4] == 0 and y[5] == 6
    assert np.array_equal(g, np.zeros_like(g))
    y, g = T.forward(T.HARDSWISH, v, al), T.backward(T.HARDSWISH, v, dy, al)
    assert np.isnan(y[0]) and np.isnan(g[0])
    assert y[1] == 0 and not np.signbit(y[1]) and np.signbit(y[2]) and g[1] == g[2] == 1.0
    assert y[3] == np.inf and g[3] == 2.0 and y[4] == 0 and g[4] == 0 and y[5] == 1e4 and y[6] == 0 and g[6] == 0
    y, g = T.forward(T.SILU, v, al), T.backward(T.SILU, v, dy, al)
    assert np.isnan(y[0]) and np.isnan(g[0])
    assert y[1] == 0 and not np.signbit(y[1]) and np.signbit(y[2]) and g[1] == g[2] == 1.0
    assert y[3] == np.inf and np.isnan(g[3]) and y[4] == -np.inf and g[4] == -np.inf
    assert y[5] == 1e4 and g[5] == 2.0 and np.isfinite(y[6]) and np.isfinite(g[6]) and y[6] < 0 and abs(y[6]) < 1e-30
    # the kinks' derivatives are torch's
    for kind, pts in T.KINKS.items():
        if pts:
            p = np.asarray(pts, dtype=f32)
            assert np.array_equal(T.backward(kind, p, np.ones_like(p), 0.01).astype(np.float64),
                                  T.reference(kind, p, 0.01)[1])


def test_bf16_rounding_and_partial_rows():
    a = np.asarray([1.00390625, 1.01171875, -3.0e4, 0.0, 1e-30], dtype=f32)   # ties: to even
    assert np.array_equal(T.to_bf16(a), torch.as_tensor(a).to(torch.bfloat16).to(torch.float32).numpy())
    assert np.array_equal(T.from_bf16_bits(T.bf16_bits(T.to_bf16(a))), T.to_bf16(a))
    rng = np.random.RandomState(3)
    P, C, rows = 37, 4, 3
    x, dy = T.to_bf16(rng.randn(P, C)), T.to_bf16(rng.randn(P, C))
    bn = tuple(v.astype(f32) for v in (rng.randn(C) * 0.3, rng.rand(C) + 0.5, 1 + 0.3 * rng.randn(C), rng.randn(C)))
    for relu in (0, 1):
        g, part, apart = T.backward_bnx(T.SILU, x, dy, bn, relu, 0.0, False, rows)
        v, dead, xh = T.bn_v(x, bn, relu, False)
        assert bool(dead.any()) == bool(relu) and np.all(g[dead] == 0)
        assert np.array_equal(g[~dead], T.backward(T.SILU, v, dy)[~dead])
        assert part.shape == (rows, 2, C) and np.all(apart >= np.abs(part))
        np.testing.assert_allclose(part[:, 0].sum(axis=0), g.astype(np.float64).sum(axis=0), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(part[:, 1].sum(axis=0), (g.astype(np.float64) * xh).sum(axis=0), rtol=1e-13,
                                   atol=1e-13)
        assert np.array_equal(part[2, 0], g[26:].astype(np.float64).sum(axis=0))   # ppb = 13: rows 0-12, 13-25, 26-36


@pytest.mark.parametrize("name", NAMES)
def test_seeded_cases_keep_the_kink_margin(name):
    """The seed of a case is the first of 0, 1, 2, ... at which no value lies within KINK_MARGIN of a kink, so no fp32
    evaluation of v can decide a branch differently from fp64."""
    kind = T.KINDS[name]
    for shape in ((3, 37), (2, 8, 7, 7)):
        seed, (v, dy) = T.seeded(kind, lambda s: T.entry_inputs(kind, shape, s))
        assert T.kink_margin(kind, v) >= T.KINK_MARGIN
        for earlier in range(seed):
            assert T.kink_margin(kind, T.entry_inputs(kind, shape, earlier)[0]) < T.KINK_MARGIN
        assert np.array_equal(T.to_bf16(v), v) and np.array_equal(T.to_bf16(dy), dy)
    assert T.kink_margin(T.RELU6, np.asarray([1.0, 6.0 + 2.0 ** -11])) < T.KINK_MARGIN
    assert T.kink_margin(T.SILU, np.asarray([0.0])) == np.inf
    e = T.with_edges(np.ones((4, 5), dtype=f32))
    assert np.isnan(e.ravel()[9]) and e.ravel()[5] == np.inf and np.signbit(e.ravel()[1]) and e.ravel()[7] == 9984.0


# ---- the layers, host only ------------------------------------------------------------------------

def test_constructor_repr_and_validation():
    l = LeakyReLu("lk")
    assert (l.layer_name, l.alpha, l.kind) == ("lk", 0.01, 0) and type(l.alpha) is float
    assert repr(l) == "LeakyReLu(lk, alpha=0.01)" and repr(LeakyReLu("a", alpha=np.float32(0.5))) == "LeakyReLu(a, alpha=0.5)"
    assert LeakyReLu("n", -2).alpha == -2.0 and LeakyReLu("z", 0).alpha == 0.0
    assert repr(ReLu6("r")) == "ReLu6(r)" and repr(HardSwish("h")) == "HardSwish(h)" and repr(SiLu("s")) == "SiLu(s)"
    assert (ReLu6("r").kind, HardSwish("h").kind, SiLu("s").kind) == (1, 2, 3)
    for cls in (LeakyReLu, ReLu6, HardSwish, SiLu):
        assert cls.accepts_bn_input is True and not issubclass(cls, ReLu)
        m = cls("m")
        assert m.is_on_gpu is False and m.learned_params is None and m.grads is None and m._state is None
        x = torch.zeros(2, 3)
        with pytest.raises(RuntimeError):
            m.forward(x)  # not on the GPU: there is no CPU path
        with pytest.raises(RuntimeError):
            m.backward(x)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39):
        with pytest.raises(ValueError):
            LeakyReLu("d", bad)
    for bad in ("0.1", None, [0.1], True, False, 1j):
        with pytest.raises(TypeError):
            LeakyReLu("d", bad)
    assert checked_alpha("d", 3) == 3.0


def test_reference_alias_import():
    import dorknet_amd
    dorknet_amd.install_reference_aliases()
    from layers.activations import HardSwish as H, LeakyReLu as L, ReLu6 as R, SiLu as S
    assert (H, L, R, S) == (HardSwish, LeakyReLu, ReLu6, SiLu)


def _h5_available():
    from dorknet_amd.network import checkpoint
    try:
        checkpoint._backend().File  # noqa: B018
        from dorknet_amd.network import _h5lite
        if checkpoint._backend() is _h5lite:
            _h5lite._load()
        return True
    except ImportError:
        return False


@pytest.mark.skipif(not _h5_available(), reason="neither h5py nor the HDF5 C library is available")
def test_network_with_activations_round_trips(tmp_path):
    from dorknet_amd.layers.dense_layer import DenseLayer
    from dorknet_amd.layers.losses import SoftmaxWithCrossEntropy
    from dorknet_amd.layers.pointwise_convolution import PointwiseConvLayer
    from dorknet_amd.layers.residual_block import ResidualBlock
    from dorknet_amd.network.feed_forward_network import FeedForwardNetwork
    np.random.seed(5)
    net = FeedForwardNetwork("acts")
    net.add_layer(ResidualBlock("block", [PointwiseConvLayer("pw", filter_block_shape=(8, 8), with_bias=False),
                                          LeakyReLu("block_leaky", alpha=-0.125)],
                                post_skip_activation=ReLu("block_relu")))
    net.add_layer(DenseLayer("dense_1", incoming_chans=24, output_dim=16))
    net.add_layer(LeakyReLu("leaky", alpha=0.2))
    net.add_layer(ReLu6("relu6"))
    net.add_layer(HardSwish("hswish"))
    net.add_layer(SiLu("silu"))
    net.add_layer(DenseLayer("dense_2", incoming_chans=16, output_dim=5))
    net.set_loss_layer(SoftmaxWithCrossEntropy("softmax"))
    h5f, js = str(tmp_path / "w.h5"), str(tmp_path / "s.json")
    net.save_weights_to_h5(h5f)
    net.save_layer_structure_to_json(js)
    with open(js) as f:
        s = json.load(f)
    assert s["leaky"] == "LeakyReLu(leaky, alpha=0.2)" and s["relu6"] == "ReLu6(relu6)"
    assert s["hswish"] == "HardSwish(hswish)" and s["silu"] == "SiLu(silu)"
    fresh = FeedForwardNetwork("x")
    fresh.load_network_from_json_and_h5(js, h5f)   # layers are rebuilt by their type names
    assert [(type(l), l.layer_name) for l in fresh.layers] == [(type(l), l.layer_name) for l in net.layers]
    assert fresh.layers[2].alpha == 0.2 and type(fresh.layers[2].alpha) is float
    sub = fresh.layers[0].layer_list[1]
    assert type(sub) is LeakyReLu and sub.alpha == -0.125
    from dorknet_amd.network.checkpoint import open_h5
    for bad in (float("nan"), float("inf")):   # loading validates as the constructor does
        with open_h5(h5f, "r+") as f:
            f["leaky/layer_info"].attrs["alpha"] = bad
        with pytest.raises(ValueError):
            FeedForwardNetwork("y").load_network_from_json_and_h5(js, h5f)


ENTRIES = {  # name: argument count
    "dk_act_fwd_f32": 6, "dk_act_fwd_bf16": 6, "dk_act_fwd_bnx_f32": 12, "dk_act_fwd_bnx_bf16": 12,
    "dk_act_bwd_f32": 7, "dk_act_bwd_bf16": 7, "dk_act_bwd_bnx_f32": 15, "dk_act_bwd_bnx_bf16": 15,
}


def test_header_declarations():
    decls = _hip.parse_header()
    for name, argc in ENTRIES.items():
        ret, params = decls[name]
        assert ret == "int" and len(params) == argc, (name, params)
        assert params[-1] == ("void*", "stream") or params[-1][1] == "stream"
        assert ("float", "alpha") in [(t.strip(), n) for t, n in params] and "kind" in [n for _, n in params]


@pytest.mark.skipif(not os.path.exists(_hip.LIB_PATH), reason="run __graft_entry__.build() first")
def test_entries_resolve_and_refuse_bad_arguments():
    import ctypes
    lib = _hip.lib
    for name, argc in ENTRIES.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == argc and ctypes.c_float in fn.argtypes
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)  # non-NULL, so that it is the scalars that are refused (before any launch)
    bn = (p, p, p, p, 1)
    for sfx in ("_f32", "_bf16"):
        fwd, fbn, bwd, bbn = (getattr(lib, "dk_act_" + n + sfx) for n in ("fwd", "fwd_bnx", "bwd", "bwd_bnx"))
        for n, kind, alpha in ((0, 0, 0.1), (-8, 0, 0.1), (8, -1, 0.1), (8, 4, 0.1), (8, 0, float("nan")),
                               (8, 0, float("inf"))):
            with pytest.raises(_hip.HipError, match="bad arguments"):
                fwd(p, n, kind, alpha, p, None)
            with pytest.raises(_hip.HipError, match="bad arguments"):
                fbn(p, n, 4, *bn, kind, alpha, p, None)
            with pytest.raises(_hip.HipError, match="bad arguments"):
                bwd(p, p, n, kind, alpha, p, None)
            with pytest.raises(_hip.HipError, match="bad arguments"):
                bbn(p, p, max(n, -1) // 4, 4, *bn, kind, alpha, p, p, 1 << 20, None)
        for x, y in ((None, p), (p, None)):
            with pytest.raises(_hip.HipError, match="bad arguments"):
                fwd(x, 8, 0, 0.1, y, None)
        with pytest.raises(_hip.HipError, match="bad arguments"):
            bwd(p, None, 8, 0, 0.1, p, None)
        for C in (0, -4, 3):   # n % C != 0 too
            with pytest.raises(_hip.HipError, match="bad arguments"):
                fbn(p, 8, C, *bn, 0, 0.1, p, None)
        with pytest.raises(_hip.HipError, match="workspace too small"):
            bbn(p, p, 2, 4, *bn, 0, 0.1, p, p, lib.dk_bn_workspace_bytes(2, 4) - 1, None)
    with pytest.raises(_hip.HipError, match="bad arguments"):   # bf16 off the 4-channel route
        lib.dk_act_bwd_bnx_bf16(p, p, 2, 6, *bn, 0, 0.1, p, p, 1 << 20, None)
    with pytest.raises(_hip.HipError, match="bad arguments"):   # bf16 with a pointer off 16 bytes
        lib.dk_act_fwd_bf16(p + 2, 8, 0, 0.1, p, None)


def test_perfmodel_entries():
    from dorknet_amd import perfmodel
    n, P, C = 4096, 128, 32
    for sfx, e in (("_f32", 4), ("_bf16", 2)):
        assert perfmodel.work("dk_act_fwd" + sfx, (1, n, 3, 0.0, 2, 0))[1] == e * 2 * n
        assert perfmodel.work("dk_act_fwd_bnx" + sfx, (1, n, C, 1, 1, 1, 1, 0, 2, 0.0, 2, 0))[1] == e * 2 * n
        assert perfmodel.work("dk_act_bwd" + sfx, (1, 2, n, 1, 0.0, 3, 0))[1] == e * 3 * n
        rows = perfmodel.bn_partial_rows(P, C)
        fl, by = perfmodel.work("dk_act_bwd_bnx" + sfx, (1, 2, P, C, 1, 1, 1, 1, 0, 3, 0.0, 3, 4, 64, 0))
        assert by == e * 3 * P * C + rows * 2 * C * 8 and fl > 0
    from tests._bn_ref import CASES, bn_blocks
    for P, C in CASES.values():
        assert perfmodel.bn_partial_rows(P, C) == bn_blocks(P, C)
