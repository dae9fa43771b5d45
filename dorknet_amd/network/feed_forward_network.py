"""Sequential network container (reference: network/feed_forward_network.py).

Same API: ``add_layer``, ``set_loss_layer``, ``to_gpu``, ``forward(X, y_one_hot,
test_mode=False, terminal_layer_name=None) -> (loss, X)``, ``backward()``, ``test``,
``save_weights_to_h5``, ``save_layer_structure_to_json``,
``load_network_from_json_and_h5``; beside ``test``, ``evaluate`` and ``predict`` keep the
counting and the arg-sort on the device (dorknet_amd/metrics.py).  The forward pass runs (BatchNormLayer, ReLu) pairs
fused (layers/_chain.py) and remembers the steps it took for ``backward``.
"""
from __future__ import annotations

import json

import numpy as np

from ..layers._bn_input import materialize
from ..layers._chain import chain_backward, execute
from ..layers.activations import ReLu  # noqa: F401  (re-exported names used by loaders)
from ..layers.batch_norm import BatchNormLayer  # noqa: F401
from ..layers.convolution import ConvLayer  # noqa: F401
from ..layers.dense_layer import DenseLayer  # noqa: F401
from ..layers.depthwise_convolution import DepthwiseConvLayer  # noqa: F401
from ..layers.losses import SoftmaxWithCrossEntropy  # noqa: F401
from ..layers.pointwise_convolution import PointwiseConvLayer  # noqa: F401
from ..layers.pooling import GlobalAveragePoolingLayer  # noqa: F401
from ..layers.residual_block import ResidualBlock  # noqa: F401
from .._hip import async_weight_grads
from .._tensor import act_dtype, as_device


class FeedForwardNetwork:
    def __init__(self, name):
        self.name = name
        self.is_on_gpu = False
        self.layers = []
        self.loss_layer = None
        self._steps = None

    def __repr__(self):
        out = "{}: \n".format(self.name)
        for l in self.layers:
            out += "\t" + l.__repr__() + "\n"
        return out

    def add_layer(self, layer):
        self.layers.append(layer)

    def set_loss_layer(self, loss_layer):
        self.loss_layer = loss_layer

    def to_gpu(self):
        if self.is_on_gpu:
            print("Model already on GPU, ignoring request")
            return
        layer = None
        try:
            for layer in self.layers:
                layer.to_gpu()
            if self.loss_layer is not None:
                self.loss_layer.is_on_gpu = True
            self.is_on_gpu = True
        except Exception as e:
            print("Error putting layer {} on GPU, error was: {}".format(layer, e))
            raise e

    def _l2_plan(self):
        """If every regularisation term the forward pass would add is a plain l2 on a
        layer's weights, return the (weights, strength) list (in the order
        feed_forward_network.py:55-60 and residual_block.py:78-84 visit them) so all terms
        are computed in one multi-tensor launch; None otherwise (per-layer fallback)."""
        from ..layers.layer import Layer
        from ..layers.residual_block import ResidualBlock
        from ..layers._common import l2_strength
        plan = []

        def visit(layer):
            rf = type(layer).regulariser_forward
            if rf is ResidualBlock.regulariser_forward:
                for l in layer.layer_list:
                    if hasattr(l, "regulariser_forward") and not visit(l):
                        return False
                return True
            if rf is not Layer.regulariser_forward:
                return False
            reg = layer.weight_regulariser
            if not reg:
                return True
            s = l2_strength(reg)
            w = layer.learned_params["weights"] if layer.learned_params else None
            if s is None or not (hasattr(w, "is_cuda") and w.is_cuda and w.is_contiguous()):
                return False
            plan.append((w, s))
            return True

        for layer in self.layers:
            if hasattr(layer, "regulariser_forward") and not visit(layer):
                return None
        return plan

    def _l2_total(self, plan, loss_tensor):
        """loss_tensor + sum of 0.5*s*sum(W^2) over `plan` (dk_l2_loss_multi_f32)."""
        import torch
        from .._hip import lib, stream_handle, workspace
        from .._table import DeviceTable, f32_word
        t = getattr(self, "_l2_table", None)
        if t is None:  # rows {w, n, first_block, strength}, 2048 elements per block
            t = self._l2_table = DeviceTable(2048, "FeedForwardNetwork", ("l2-regularised weights", "weight"), 1,
                                             hint="call forward after to_gpu()")
        t.ensure([(w, f32_word(s)) for w, s in plan])
        out = torch.empty((), dtype=torch.float32, device=loss_tensor.device)
        nb = lib.dk_l2_multi_workspace_bytes(t.blocks)
        lib.dk_l2_loss_multi_f32(t.ptr, t.ntens, t.blocks, loss_tensor.data_ptr(), out.data_ptr(), workspace.get(nb),
                                 nb, stream_handle())
        return out

    def forward(self, X, y_one_hot, test_mode=False, terminal_layer_name=None):
        loss = 0
        regularisation_terms = []
        steps = []
        self._steps = steps
        plan = None
        if not test_mode and self.loss_layer is not None and terminal_layer_name is None:
            plan = self._l2_plan()
            if plan is not None and not plan:
                plan = None
        keep = () if terminal_layer_name is None else (terminal_layer_name,)

        def visit(group, X):
            for l in group:
                if l.layer_name == terminal_layer_name:
                    return True
                if not test_mode and plan is None and hasattr(l, "regulariser_forward"):
                    regularisation_terms.append(l.regulariser_forward())
            return False

        X, steps, stopped = execute(self.layers, X, test_mode, keep=keep, visit=visit)
        self._steps = steps
        if stopped:
            return loss, materialize(X)
        if self.loss_layer is not None:
            this_loss, X = self.loss_layer.forward(X, y_one_hot, test_mode=test_mode)
            if plan is not None:
                return self._l2_total(plan, this_loss), X
            loss += this_loss
            loss += sum(regularisation_terms)
        return loss, X  # NB if test_mode=True, you get softmax scores ("logits")

    def backward(self, upstream_dx=None, input_grad=False):
        """Reference behaviour (feed_forward_network.py:62-70): backward from the loss layer.
        Extension: an explicit output gradient for a network without a loss layer (BASELINE
        config 5's stack is driven this way).  Like the reference this returns nothing, so the
        gradient w.r.t. the network input (which the reference computes and drops) is not
        computed; input_grad=True computes and returns it."""
        if upstream_dx is not None:
            pass
        elif self.loss_layer is not None:
            upstream_dx = self.loss_layer.backward()
        else:
            raise ValueError("Network doesn't have a loss, can't run backward pass.")
        with async_weight_grads():  # weight gradients on the side stream, joined on exit
            dx = chain_backward(self._steps, upstream_dx, need_input_grad=input_grad)
        return dx if input_grad else None

    def test(self, data_loader, batch_size, test_set_size):
        from tqdm import tqdm
        test_correct_total = 0
        for X_test_batch, y_test_batch, _ in tqdm(data_loader, total=test_set_size / batch_size):
            X_test_batch = as_device(X_test_batch)
            _, batch_scores = self.forward(X_test_batch, y_one_hot=None, test_mode=True)
            if hasattr(y_test_batch, "cpu"):  # labels on the device (DeviceImageDataLoader)
                y_test_batch = y_test_batch.cpu().numpy()
            test_correct_total += np.sum(np.asarray(y_test_batch) ==
                                         np.argmax(batch_scores.cpu().numpy(), axis=1))
        return float(test_correct_total) / test_set_size

    def evaluate(self, data_loader, top=(1, 5), confusion=False, num_batches=None):
        """Accuracy, top-k accuracy, loss and (confusion=True) the confusion matrix over the (X, y, _)
        triples of `data_loader`, the loader that `test` takes: X host or device, fp32 or bf16, y the
        integer labels (a list, an array or a tensor), batches of any sizes.  Per batch: as_device,
        forward(X, None, test_mode=True) and one counter launch (dorknet_amd/metrics.py; DESIGN.md
        section 16); nothing comes back to the host before the final read.  Returns a
        ClassificationReport; `top` lists the k (1 <= k <= min(classes, 16)) its repr prints;
        num_batches stops after that many batches.  A label outside [0, classes) leaves its row out."""
        from ..metrics import RANK_BINS, ClassificationMeter
        try:
            top = tuple(int(k) for k in ((top,) if np.isscalar(top) else top))
        except (TypeError, ValueError):
            raise ValueError("evaluate: top must be integers, got {!r}".format(top))
        if not top or min(top) < 1 or max(top) > RANK_BINS:
            raise ValueError("evaluate: top needs 1 <= k <= min(classes, {}), got {}".format(RANK_BINS, top))
        if num_batches is not None and int(num_batches) < 1:
            raise ValueError("evaluate: num_batches must be at least 1, got {}".format(num_batches))
        if self.loss_layer is None:
            raise ValueError("evaluate: the network has no loss layer, so no scores to evaluate")
        meter = None
        for i, (X, y, _) in enumerate(data_loader):
            if num_batches is not None and i >= int(num_batches):
                break
            _, scores = self.forward(as_device(X, act_dtype(X)), None, test_mode=True)
            if meter is None:
                classes = scores.shape[1]
                if max(top) > classes:
                    raise ValueError("evaluate: top needs 1 <= k <= min(classes, {}), got {} for {} classes".format(
                        RANK_BINS, top, classes))
                meter = ClassificationMeter(classes, confusion=confusion)
            meter.update(scores, y)
        if meter is None:
            raise ValueError("evaluate: the data loader gave no batch")
        return meter.result(top)

    def predict(self, X, top=5):
        """The `top` best classes of every image of the batch X and their scores, best first:
        (class_idx int32 (N, top), scores fp32 (N, top)), both on the GPU -- the
        ``np.argsort(scores)[::-1]`` loop of the reference's
        examples/imagenet_dogs_225_resnet_18_depsep_evaluate.py:41-46 for a whole batch
        (dk_topk_rows_vals_f32).  1 <= top <= min(classes, 16)."""
        from ..cam import MAX_TOP, top_classes_with_scores
        if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or not 1 <= top <= MAX_TOP:
            raise ValueError("predict: top must be an integer with 1 <= top <= min(classes, {}), got {!r}".format(
                MAX_TOP, top))
        if not hasattr(X, "shape") or len(X.shape) < 2 or X.shape[0] < 1:
            raise ValueError("predict: X must be a batch (N >= 1, ...) array or tensor, got {}".format(
                tuple(X.shape) if hasattr(X, "shape") else type(X)))
        _, scores = self.forward(as_device(X, act_dtype(X)), None, test_mode=True)
        return top_classes_with_scores(scores, int(top))

    def class_activation_maps(self, X, top=3, feature_layer="res8", dense_layer="dense1", feature_test_mode=True):
        """Class activation maps of the `top` best classes of every image of the batch X (fp32 or bf16
        (N, 3, H, W), channels B, G, R, minus 128 as the preprocessor delivers it), on the GPU
        (dorknet_amd/cam.py; the reference's examples/imagenet_dogs_225_resnet_18_depsep_CAM.py:62-87).
        Returns (class_idx int32 (N, top), masks fp32 (N, top, H, W), overlays uint8 (N, top, H, W, 3) BGR).

        The scores come from forward(X, None, test_mode=True), the features from
        forward(X, None, test_mode=feature_test_mode, terminal_layer_name=feature_layer), the weights
        from the DenseLayer named `dense_layer`.  The reference's script takes its features with
        test_mode=False, i.e. with the batch statistics of the single image it feeds; the default here
        is True (the running statistics, as for the scores).  feature_test_mode=False on a batch of one
        image gives the reference's behaviour (and updates the running statistics, as it does there)."""
        import torch
        from ..cam import class_activation_maps, top_classes
        dense = next((l for l in self.layers if l.layer_name == dense_layer), None)
        if not isinstance(dense, DenseLayer):
            raise ValueError("class_activation_maps: the network has no DenseLayer named {!r}".format(dense_layer))
        if not any(l.layer_name == feature_layer for l in self.layers):
            raise ValueError("class_activation_maps: the network has no layer named {!r}".format(feature_layer))
        X = as_device(X, act_dtype(X))
        _, scores = self.forward(X, None, test_mode=True)
        _, features = self.forward(X, None, test_mode=feature_test_mode, terminal_layer_name=feature_layer)
        if features.dim() != 4:
            raise ValueError("class_activation_maps: the output of layer {!r} is not a 4-D feature map".format(
                feature_layer))
        class_idx = top_classes(scores, top)
        images = X if X.dtype == torch.float32 else X.float()   # bf16 widens exactly
        masks, overlays = class_activation_maps(features, dense.learned_params["weights"], class_idx, images=images)
        return class_idx, masks, overlays

    def save_weights_to_h5(self, fname):
        from .checkpoint import open_h5
        with open_h5(fname, "w") as f:
            for layer in self.layers:
                layer.save_to_h5(f)
            if self.loss_layer is not None:
                self.loss_layer.save_to_h5(f)

    def save_layer_structure_to_json(self, fname):
        structure_dict = {"name": self.name}
        for layer in self.layers:
            structure_dict[layer.layer_name] = repr(layer)
        if self.loss_layer is not None:
            structure_dict[self.loss_layer.layer_name] = repr(self.loss_layer)
        with open(fname, "w") as f:
            json.dump(structure_dict, f, indent=4)

    def load_network_from_json_and_h5(self, json_fname, h5_fname):
        from .checkpoint import load_network
        load_network(self, json_fname, h5_fname)
