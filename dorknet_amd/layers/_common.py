"""Small helpers shared by the parameterised layers."""
from __future__ import annotations

import numpy as np
import torch

from .._hip import lib, stream_handle, weight_grad_stream, workspace
from .._tensor import as_device


def l2_strength(reg):
    """Strength to fold into the weight-gradient kernel, or None when the regulariser
    is not an l2 (then its backward() is added separately)."""
    if reg is None:
        return 0.0
    if getattr(reg, "type", None) == "l2" and hasattr(reg, "strength"):
        return float(reg.strength)
    return None


def add_regulariser_grad(grad: torch.Tensor, weights: torch.Tensor, reg) -> None:
    """grads["weights"] += reg.backward(W) for a non-l2 regulariser (kept general like
    convolution.py:99-100)."""
    extra = as_device(reg.backward(weights)).contiguous()
    lib.dk_add_f32(grad.data_ptr(), extra.data_ptr(), grad.numel(), 0, grad.data_ptr(), 0, stream_handle())


def grad_buffer(layer, key: str, shape) -> torch.Tensor:
    """The layer's persistent gradient tensor for `key`, (re)allocated if missing or of
    the wrong shape.  Backward passes overwrite it in place: values follow the
    reference's "backward overwrites self.grads[k]" semantics while the tensor object
    stays stable for the optimiser table and data-parallel gradient buckets."""
    g = layer.grads.get(key)
    # fast path (every backward): the tensor this function handed out last time, same shape
    cache = layer.__dict__.setdefault("_grad_buffer_cache", {})
    hit = cache.get(key)
    if hit is not None and hit[0] is g and hit[1] == shape:
        return g
    shape_t = tuple(int(s) for s in shape)
    if not isinstance(g, torch.Tensor) or g.device.type != "cuda" or tuple(g.shape) != shape_t \
            or not g.is_contiguous():
        g = torch.empty(shape_t, dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
        layer.grads[key] = g
    cache[key] = (g, shape)
    return g


def weight_grad(layer, dy, x, P, K, shape, launch, colsum="dk_colsum_f32"):
    """The frame around a layer's weight-gradient launch, on the side stream
    (_hip.weight_grad_stream): the bias gradient (the column sums of dy as [P, K], `colsum`), then
    launch(w, strength, gw, stream) -- w / strength: the weights and the l2 strength the kernel
    folds in (0 / 0.0 without an l2 regulariser), gw: grads["weights"] of `shape` -- and any other
    regulariser's term added to gw after it.  The launch takes its workspace inside (workspace.get
    is per stream)."""
    w = layer.learned_params["weights"]
    with weight_grad_stream(dy, x, *layer._bn_tensors()):
        sst = stream_handle()
        if layer.with_bias:
            gb = grad_buffer(layer, "bias", (K,))
            nb = lib.dk_colsum_workspace_bytes(P, K)
            getattr(lib, colsum)(dy.data_ptr(), P, K, gb.data_ptr(), workspace.get(nb), nb, sst)
        gw = grad_buffer(layer, "weights", shape)
        s = l2_strength(layer.weight_regulariser)
        launch(w.data_ptr() if s else 0, s or 0.0, gw.data_ptr(), sst)
        if s is None:
            add_regulariser_grad(gw, w, layer.weight_regulariser)


def init_weights(shape, initialiser: str, fan_sum: float) -> np.ndarray:
    """Reference initialisers (convolution.py:24-28 and siblings), numpy's global RNG."""
    if initialiser == "glorot_uniform":
        limit = np.sqrt(6.0 / fan_sum)
        return np.random.uniform(low=-limit, high=limit, size=shape).astype(np.float32)
    elif initialiser == "normal":
        return 0.01 * np.random.randn(*shape).astype(np.float32)
    raise ValueError("unknown weight_initialiser {!r}".format(initialiser))


def patches_count(in_size: int, f: int, stride: int, padding: int):
    """The reference's output-size arithmetic: a float ((Hp - f)/stride) + 1
    (convolution.py:67-68), truncated by int() where used as a size."""
    full = ((in_size + 2 * padding - f) / stride) + 1
    return full, int(full)
