"""Drop-in for the hot-path part of the reference's ``train.py``: the inner training step
(train.py:119-142), ``trainable_params`` (train.py:283-303), the Adam / CrossEntropyLoss choice
(train.py:369-372), ``H5Loader`` (train.py:31-48) and the shell around them: the
``train_model`` epoch loop with early stopping, best-weights restore, checkpoint / resume, ``test_model`` with the
classification summary, ``save_model`` / ``load_model``. Checkpoints hold tensors and numbers only (the reference
pickles whole objects, train.py:249-262); the confusion-matrix plot is not reproduced.

``TrainStep`` fuses zero_grad -> forward -> CrossEntropyLoss -> backward -> Adam into HIP kernel
calls; under ``torch.distributed`` it shards nothing itself (each rank feeds its own bags) and
exchanges (a) BatchNorm statistics (SyncBN, so the result equals the reference's single-process
step on the global batch) and (b) ONE flat gradient buffer with an RCCL all-reduce over xGMI.
"""

import os
import time

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import Dataset

from . import cnn_train, mla_train, ops
from .params import *  # noqa: F401,F403
from .torchvggish.vggish import cache_stamp, weight_caches


class H5Loader(Dataset):
    """Dataset over array-likes (HDF5 datasets or ndarrays): train.py:31-48."""

    def __init__(self, X_desc, y_desc):
        self.X_desc, self.y_desc = X_desc, y_desc

    def __len__(self):
        return self.y_desc.shape[0]

    def __getitem__(self, idx):
        return (self.X_desc[idx], self.y_desc[idx])


def trainable_params(model, feature_extract):
    """train.py:283-303: the parameters to hand to the optimizer (prints their names)."""
    params_to_update = model.parameters()
    print("Params to learn:")
    if feature_extract:
        params_to_update = []
        for name, param in model.named_parameters():
            if param.requires_grad:
                params_to_update.append(param)
                print("\t", name)
    else:
        for name, param in model.named_parameters():
            if param.requires_grad:
                print("\t", name)
    return params_to_update


def parse_criterion(criterion, classes):
    """What the HIP loss with options (``ops.cross_entropy_opts``) needs of an ``nn.CrossEntropyLoss``, checked on the host without a
    device: {"weight": float32 CPU tensor of ``classes`` elements or None, "ignore_index", "label_smoothing", "reduction"}.
    Refused: another loss (TypeError); ``reduction="none"`` (the step returns a scalar), ``label_smoothing`` outside [0, 1], a
    weight that is not a finite, non-negative float tensor of ``classes`` elements with a positive entry (ValueError); more than
    1024 classes (NotImplementedError)."""
    if not isinstance(criterion, nn.CrossEntropyLoss):
        raise TypeError("the HIP training step implements nn.CrossEntropyLoss, not %s" % type(criterion).__name__)
    if criterion.reduction not in ("mean", "sum"):
        raise ValueError("reduction=%r: the HIP step returns a scalar loss, 'mean' or 'sum'" % (criterion.reduction,))
    eps = float(criterion.label_smoothing)
    if not 0.0 <= eps <= 1.0:
        raise ValueError("label_smoothing must lie in [0, 1], not %r" % (criterion.label_smoothing,))
    if classes > 1024:
        raise NotImplementedError("the HIP loss with options is built for up to 1024 classes, not %d" % classes)
    weight = criterion.weight
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or not weight.is_floating_point():
            raise ValueError("the class weights must be a float tensor")
        if weight.dim() != 1 or weight.numel() != classes:
            raise ValueError("the class weights have shape %s; the head has %d classes" % (tuple(weight.shape), classes))
        weight = weight.detach().to("cpu", torch.float32).contiguous()
        if not bool(torch.isfinite(weight).all()) or bool((weight < 0).any()):
            raise ValueError("the class weights must be finite and non-negative")
        if not bool((weight > 0).any()):
            raise ValueError("the class weights are all zero")
    return {"weight": weight, "ignore_index": int(criterion.ignore_index), "label_smoothing": eps, "reduction": criterion.reduction}


def parse_bce_criterion(criterion, classes):
    """What the HIP binary cross-entropy (``ops.bce_loss``) needs of an ``nn.BCELoss``, checked on the host without a device:
    {"weight": float32 CPU tensor of ``classes`` elements or None, "reduction"}. The weight is the per-class rescaling of
    ``nn.BCELoss(weight=)``, one entry per column. Refused as ``parse_criterion`` refuses: another loss (TypeError;
    ``nn.BCEWithLogitsLoss`` among them, the head's outputs are probabilities, not logits); ``reduction="none"``, a weight that is
    not a finite, non-negative float tensor of ``classes`` elements with a positive entry (ValueError); more than 1024 classes
    (NotImplementedError)."""
    if not isinstance(criterion, nn.BCELoss):
        raise TypeError("the HIP multi-label step implements nn.BCELoss, not %s" % type(criterion).__name__)
    if criterion.reduction not in ("mean", "sum"):
        raise ValueError("reduction=%r: the HIP step returns a scalar loss, 'mean' or 'sum'" % (criterion.reduction,))
    if classes > 1024:
        raise NotImplementedError("the HIP binary cross-entropy is built for up to 1024 classes, not %d" % classes)
    weight = criterion.weight
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or not weight.is_floating_point():
            raise ValueError("the class weights must be a float tensor")
        if weight.dim() != 1 or weight.numel() != classes:
            raise ValueError("the class weights have shape %s; the head has %d classes" % (tuple(weight.shape), classes))
        weight = weight.detach().to("cpu", torch.float32).contiguous()
        if not bool(torch.isfinite(weight).all()) or bool((weight < 0).any()):
            raise ValueError("the class weights must be finite and non-negative")
        if not bool((weight > 0).any()):
            raise ValueError("the class weights are all zero")
    return {"weight": weight, "reduction": criterion.reduction}


class TrainStep:
    """One fused training step of an ``Ensemble``: frozen CNN (the reference default
    ``cnn_trainable=False``; model.py:159-160) or finetune (every parameter trainable, train.py:96-97;
    f32 precision).

    All trainable parameters are re-seated as views of ONE flat float32 buffer (same for
    gradients and the two Adam moments), so the data-parallel exchange is a single all-reduce
    and Adam a single kernel. ``attention_modules.*.fcf.*`` never receive a gradient
    (model.py:237-238); like torch's Adam (which skips ``grad is None``) they are left untouched.
    """

    def __init__(self, clf, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, process_group=None, params=None, sync_bn=True, graph=None,
                 optimizer=None, max_grad_norm=None, criterion=None, trunk_data_parallel=False):
        """``params``: the parameters the caller's optimizer holds (``optimizer.param_groups[...]["params"]``); None =
        every parameter that requires grad. Exactly the tensors in ``params`` that require grad are updated, as
        ``optimizer.step()`` does in the reference (train.py:138; torch's Adam skips parameters whose ``.grad`` is None,
        i.e. the frozen ones). Gradients of parameters OUTSIDE that set are not computed: the reference computes and then
        never applies them (its ``__main__`` builds the Adam before ``set_requires_grad(clf, True)``, train.py:369-370 vs
        :96-97, so its "finetune" run only ever steps the MLA head) -- the updated model is the same.
        ``trunk_data_parallel``: allow ResNet trunk parameters in the update set under a process group (off: that combination is
        refused). The step then equals the single-process step on the global batch: SyncBN in the trunk's forward AND backward
        (``ops.rn_bn_bwd_sync``), gradients summed by one flat all-reduce. The head keeps its equal-shard contract.
        ``optimizer``: a ``torch.optim.Adam`` / ``AdamW`` whose ``param_groups`` define the update set (instead of ``params``) AND
        how each group is stepped: ``lr``, ``betas``, ``eps``, ``weight_decay`` (L2, or decoupled for AdamW), ``amsgrad``. The
        groups are read again at every call, so an LR scheduler or ``group["lr"] = ...`` acts on the next step, graph replays
        included; the torch optimizer itself is never stepped. All groups are stepped by ONE launch (``ops.adam_grouped_step``).
        ``max_grad_norm`` (needs ``optimizer``): ``clip_grad_norm_`` on the all-reduced flat gradient before the update;
        ``grad_norm`` / ``clip_coef`` are the device values of the last step, ``grads`` keep the unclipped gradients.
        ``criterion``: None = the plain mean cross-entropy (``ops.cross_entropy``), or an ``nn.CrossEntropyLoss`` whose ``weight``,
        ``ignore_index``, ``label_smoothing`` and ``reduction`` ("mean" | "sum") the step honours (``ops.cross_entropy_opts``). The
        weight is copied to the device once, here; the other three are read here and must not change afterwards. Under a process
        group the mean's denominator is the global batch's; ``last_counted`` holds the (global) number of rows whose label is not
        ``ignore_index``, a 1-element device tensor, after each step.
        An ``nn.BCELoss`` (``weight``, ``reduction`` "mean" | "sum") makes it a multi-label step (``ops.bce_loss``): labels are
        (B, classes) multi-hot or soft targets in [0, 1], the mean divides by global batch x classes, ``hits`` counts the rows
        with every class on the right side of 0.5, and ``last_cell_hits`` holds the (global) number of such cells, a 1-element
        device tensor, after each step; ``last_counted`` stays None."""
        self.clf, self.lr, self.betas, self.eps, self.t = clf, lr, betas, eps, 0
        self.criterion = criterion
        self._bce = isinstance(criterion, nn.BCELoss)
        parse = parse_bce_criterion if self._bce else parse_criterion
        self._crit = None if criterion is None else parse(criterion, clf.mla.classes)
        self._crit_weight, self._counted, self.last_counted = None, None, None
        self._cell_hits, self.last_cell_hits = None, None
        self.groups = None                                  # the optimizer's param_groups (the live list): the grouped step
        if optimizer is not None:
            if params is not None:
                raise ValueError("give either params= or optimizer= (its param_groups are the update set), not both")
            self.groups = self._check_optimizer(optimizer)
        elif max_grad_norm is not None:
            raise ValueError("max_grad_norm belongs to the grouped step: pass optimizer= (a torch.optim.Adam over the parameters will do)")
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError("max_grad_norm must be positive, not %r" % (max_grad_norm,))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        # sync_bn=False: per-shard BatchNorm statistics under data parallelism (DistributedDataParallel semantics) instead of the
        # global-batch statistics that reproduce the reference's single-process step; see ops.Dist
        self.dist = ops.Dist(process_group, sync_bn=sync_bn)
        self.exposed = None                                 # bench.py: list of (event, event) around the wait for the comm stream
        # use_graph: replay the whole step as one HIP graph from the second step of a batch shape on (single process only; env
        # MLA_TRAIN_GRAPH=0 or graph=False keeps every step eager)
        self.use_graph = (os.environ.get("MLA_TRAIN_GRAPH", "1") == "1") if graph is None else bool(graph)
        self._graph, self._eager_shape, self._dev_t = None, None, -1
        self.captures = 0                                   # graphs recorded so far (a re-capture after a disturbance counts)
        held = None if params is None else {id(p) for p in params}
        group_of = {}
        if self.groups is not None:
            for gi, grp in enumerate(self.groups):
                for q in grp["params"]:
                    if id(q) in group_of:
                        raise ValueError("a parameter is in two optimizer groups (%d and %d)" % (group_of[id(q)], gi))
                    group_of[id(q)] = gi
            held = set(group_of)
        named = [(n, p) for n, p in clf.named_parameters()
                 if p.requires_grad and ".fcf." not in n and (held is None or id(p) in held)]
        if not named:
            raise ValueError("no trainable parameter to update")
        self.resnet = getattr(clf, "cnn_type", "vggish") == "resnet"
        self.rn_fc = False
        self.rn_trunk = {}                                # id(trunk parameter) -> its gradient view (trunk backward on)
        trunk_names = set()
        if self.resnet:
            # the ResNet trunk runs its train-mode forward inside the step (batch statistics, running-statistics update); trained
            # are the head, with just_bottlenecks=False cnn.cnn_model.fc (model.py:148-149), and -- with the trunk backward on
            # (CNN.set_trunk_backward) -- the trunk parameters in the update set, through a tape of the forward
            self.rn_fc = any(n.startswith(self.RN_FC) for n, _ in named)
            trunk = [n for n, _ in named if n.startswith("cnn.") and not n.startswith(self.RN_FC)]
            trunk_names = set(trunk)
            if trunk and not getattr(clf.cnn, "trunk_backward", False):
                raise NotImplementedError("gradients into the ResNet trunk are off (parameter %s is in the update set); turn the HIP "
                                          "trunk backward on with clf.set_trunk_backward(True)" % trunk[0])
            # under a torch.distributed process group: opt-in (trunk_data_parallel=True). The trunk backward then all-reduces the
            # two batch sums of each BatchNorm2d it passes (SyncBN; none with sync_bn=False), and the trunk's gradients travel in
            # the one flat all-reduce after the backward -- no overlapped buckets: the per-layer collectives of the compute stream
            # and bucket all-reduces of a second stream would use the one communicator from two streams at once
            if trunk and (self.dist.active or self.dist.backend is not None) and not trunk_data_parallel:
                raise NotImplementedError("data-parallel training of the ResNet trunk is not built: its SyncBN backward needs sum(dy) "
                                          "and sum(dy * xhat) all-reduced per BatchNorm2d layer (parameter %s is in the update set); "
                                          "frozen-trunk data parallelism is supported" % trunk[0])
        # CNN gradients are needed iff the update set holds a CNN parameter; any subset of the CNN is fine (the backward
        # pass stops at the lowest layer that needs a gradient and skips the weight gradients nobody asked for)
        self.finetune = not self.resnet and any(n.startswith("cnn.") for n, _ in named)
        if self.finetune and clf.cnn.precision not in ("f32", "bf16"):
            raise NotImplementedError("CNN gradients are built for precision 'f32' (exact) and 'bf16' (bf16 arithmetic, f32 "
                                      "master weights), not %r" % clf.cnn.precision)
        dev = named[0][1].device
        assert dev.type == "cuda", "TrainStep needs the model on the GPU (train_model moves it there, train.py:101)"
        if self._crit is not None and self._crit["weight"] is not None:
            self._crit_weight = self._crit["weight"].to(dev)
        pad4 = lambda k: (k + 3) // 4 * 4                 # every tensor starts 16-byte aligned (GEMM operand rule)
        total = sum(pad4(p.numel()) for _, p in named)
        self.n_params = sum(p.numel() for _, p in named)
        self.flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_m = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(total, dtype=torch.float32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)       # completed steps: the dropout call counter of the graph-captured step
        self.adam_scal = torch.zeros(2, dtype=torch.float32, device=dev)    # Adam's step-dependent scalars, written in front of each replay
        if self.groups is not None:
            # the grouped step: which group owns which stretch of the flat buffers (built once, on the host), the per-group rows
            # (rewritten in front of every step), the amsgrad maximum (only when a group asks for it), clip_grad_norm_'s pair
            self._layout = [(p.numel(), group_of[id(p)]) for _, p in named]
            tab = ops.adam_groups_table([k for k, _ in self._layout], [g for _, g in self._layout], len(self.groups))
            assert tab["total"] == total
            self._table, self._n_runs, self._n_pads = tab["table"].to(dev), tab["runs"], tab["pads"]
            self.group_rows = torch.zeros(8 * len(self.groups), dtype=torch.float32, device=dev)
            self.flat_vmax = torch.zeros(total, dtype=torch.float32, device=dev) if any(g["amsgrad"] for g in self._group_scalars()) else None
            self._clip = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)           # [norm, coef] of the last step
            self.grad_norm, self.clip_coef = self._clip[0:1], self._clip[1:2]
            self._norm_ws = torch.zeros(1024, dtype=torch.float64, device=dev) if self.max_grad_norm is not None else None
        self.grads, self._seated, off = {}, [], 0
        spans = {}                                        # bucket id -> [first float, one past the last] of the flat buffers
        for n, p in named:
            k = p.numel()
            self.flat_p[off:off + k].copy_(p.detach().reshape(-1))
            p.data = self.flat_p[off:off + k].view(p.shape)
            self.grads[n] = self.flat_g[off:off + k].view(p.shape)
            self._seated.append((n, p, self.flat_p.data_ptr() + 4 * off))
            if n in trunk_names:
                self.rn_trunk[id(p)] = self.grads[n]
            b = "rn_trunk" if n in trunk_names else self._bucket_of(n)        # the ResNet trunk: one range (no overlap bucketing)
            spans[b] = [min(spans.get(b, [off, 0])[0], off), off + pad4(k)]
            off += pad4(k)
        # Gradient buckets of the data-parallel exchange: contiguous ranges of the flat gradient buffer that become final
        # at known points of the backward pass -- the head first, then the CNN from its last Linear down to conv1 -- so that
        # each range can be all-reduced on a second HIP stream while the layers below are still computing (the parameters
        # are laid out in named_parameters() order = forward order, so "the layers from position p upwards" is one range):
        #   "mla" 3.2 MB | "fc12" embeddings.2 + .4: 69 MB | "fc0" embeddings.0: 201 MB | "conv56" 14 MB | "conv14" 4 MB
        # xGMI rings are per-link bound, so a few large messages beat many small ones; the order above is the order in which
        # the backward pass finishes them.
        self.buckets = {b: tuple(v) for b, v in spans.items()}
        self.overlap = os.environ.get("MLA_DIST_OVERLAP", "1") == "1"
        self._comm_stream = None
        # MLA parameters outside the update set still need somewhere to write their gradient (the head's backward always
        # runs whole: it is 0.3 ms); those scratch tensors are never read
        self.mla_grads = {}
        for n, p in clf.mla.named_parameters():
            if ".fcf." in n:
                continue
            self.mla_grads[n] = self.grads["mla." + n] if "mla." + n in self.grads else torch.empty_like(p, dtype=torch.float32, device=dev)

    # layer position (cnn_train.backward's `pos`: 0..5 conv1..conv6, 6..8 the three Linear layers) at which a bucket is final
    BUCKET_TRIGGER = {"fc12": 7, "fc0": 6, "conv56": 4, "conv14": 0}

    RN_FC = "cnn.cnn_model.fc."

    @staticmethod
    def _bucket_of(name):
        if not name.startswith("cnn.") or name.startswith(TrainStep.RN_FC):
            return "mla"
        key = name.split(".")[-3:-1]                      # (..., "features" | "embeddings" | "0", index, "weight" | "bias")
        idx = int(key[1])
        if key[0] == "embeddings":
            return "fc0" if idx == 0 else "fc12"
        return "conv56" if idx >= 11 else "conv14"

    def _reduce_bucket(self, name):
        """All-reduce one finished gradient range on the communication stream (it first waits for the compute stream's work
        enqueued so far, i.e. for the kernels that produced the range)."""
        a, b = self.buckets[name]
        cur = torch.cuda.current_stream()
        if self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(device=self.flat_g.device)
        self._comm_stream.wait_stream(cur)
        with torch.cuda.stream(self._comm_stream):
            self.dist.all_reduce_sum(self.flat_g[a:b], "grad:" + name)

    def state_dict(self):
        """Optimizer state as plain tensors (Adam moments over the flat buffer + step count): what
        ``optimizer.state_dict()`` holds in the reference's checkpoints (train.py:249-258)."""
        if self.groups is not None:
            # the grouped step: per-group scalars (rows of lr, beta1, beta2, eps, weight_decay, decoupled, amsgrad), the layout
            # they belong to (numel and group of every tensor of the flat buffers) and, with amsgrad, the running maximum
            sd = {"adam_m": self.flat_m.clone(), "adam_v": self.flat_v.clone(), "step": torch.tensor(self.t),
                  "groups": torch.tensor([[g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], float(g["decoupled"]),
                                           float(g["amsgrad"])] for g in self._group_scalars()], dtype=torch.float64),
                  "layout": torch.tensor(self._layout, dtype=torch.int64)}
            if self.flat_vmax is not None:
                sd["adam_vmax"] = self.flat_vmax.clone()
            return sd
        return {"adam_m": self.flat_m.clone(), "adam_v": self.flat_v.clone(), "step": torch.tensor(self.t),
                "lr": torch.tensor(self.lr), "betas": torch.tensor(self.betas), "eps": torch.tensor(self.eps)}

    def load_state_dict(self, sd):
        if self.groups is not None:
            if "layout" not in sd or "groups" not in sd:
                raise ValueError("this checkpoint was written by a step without optimizer groups; this step was built with optimizer=")
            if sd["layout"].cpu().tolist() != [list(t) for t in self._layout] or sd["groups"].shape[0] != len(self.groups):
                raise ValueError("this checkpoint was written for another layout of optimizer groups (other trainable tensors, or "
                                 "tensors assigned to other groups): %d tensors in %d groups there, %d in %d here"
                                 % (sd["layout"].shape[0], sd["groups"].shape[0], len(self._layout), len(self.groups)))
            rows = sd["groups"].cpu().tolist()
            if ("adam_vmax" in sd) != (self.flat_vmax is not None):
                raise ValueError("this checkpoint %s the amsgrad maximum and this step %s it" % (
                    ("holds", "lacks") if "adam_vmax" in sd else ("lacks", "keeps")))
            for g, (lr, b1, b2, eps, wd, dec, ams) in zip(self.groups, rows):      # as optimizer.load_state_dict restores its groups
                g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"] = lr, (b1, b2), eps, wd, bool(ams)
                if "decoupled_weight_decay" in g or dec:
                    g["decoupled_weight_decay"] = bool(dec)
            self.flat_m.copy_(sd["adam_m"]); self.flat_v.copy_(sd["adam_v"]); self.t = int(sd["step"])
            if self.flat_vmax is not None:
                self.flat_vmax.copy_(sd["adam_vmax"])
            return
        if "layout" in sd:
            raise ValueError("this checkpoint was written by a step with optimizer groups; this step was built without optimizer=")
        assert sd["adam_m"].numel() == self.flat_m.numel(), "checkpoint was written for a different set of trainable parameters"
        self.flat_m.copy_(sd["adam_m"]); self.flat_v.copy_(sd["adam_v"]); self.t = int(sd["step"])
        self.lr, self.eps = float(sd["lr"]), float(sd["eps"])
        self.betas = tuple(float(b) for b in sd["betas"])

    @staticmethod
    def _check_optimizer(optimizer):
        """The live ``param_groups`` list of a torch Adam / AdamW the grouped HIP step can stand in for."""
        if not isinstance(optimizer, torch.optim.Adam):                    # AdamW is a subclass
            raise TypeError("the HIP step implements torch.optim.Adam and AdamW, not %s" % type(optimizer).__name__)
        if len(optimizer.param_groups) > 64:
            raise NotImplementedError("the grouped HIP Adam step takes up to 64 parameter groups, not %d" % len(optimizer.param_groups))
        for g in optimizer.param_groups:
            for key in ("maximize", "capturable", "differentiable"):
                if g.get(key, False):
                    raise NotImplementedError("%s=True is not implemented by the HIP Adam step" % key)
        return optimizer.param_groups

    def _group_scalars(self):
        """What each group asks for right now, as host numbers (read at every step: schedulers write ``lr`` between steps)."""
        out = []
        for i, g in enumerate(self.groups):
            if isinstance(g["lr"], torch.Tensor) or any(isinstance(b, torch.Tensor) for b in g["betas"]):
                raise NotImplementedError("a tensor lr / betas (group %d) is not implemented by the HIP Adam step: it would cost a "
                                          "device synchronisation per step" % i)
            for key in ("maximize", "capturable", "differentiable"):
                if g.get(key, False):
                    raise NotImplementedError("%s=True is not implemented by the HIP Adam step" % key)
            out.append({"lr": float(g["lr"]), "betas": (float(g["betas"][0]), float(g["betas"][1])), "eps": float(g["eps"]),
                        "weight_decay": float(g.get("weight_decay", 0.0)), "decoupled": bool(g.get("decoupled_weight_decay", False)),
                        "amsgrad": bool(g.get("amsgrad", False))})
        return out

    def _prepare_groups(self, t):
        """Enqueue the per-group rows of step t (in front of the eager step or the graph replay)."""
        scal = self._group_scalars()
        if self.flat_vmax is None and any(g["amsgrad"] for g in scal):
            raise RuntimeError("amsgrad was turned on after this TrainStep was built (it keeps no vmax buffer): build a new TrainStep")
        ops.adam_groups_prepare(self.group_rows, scal, t)

    def _check_criterion(self):
        """The criterion's scalars as they were when the step was built (a graph holds them as launch arguments)."""
        c, live = self._crit, self.criterion
        if self._bce:
            if live.reduction != c["reduction"]:
                raise RuntimeError("the criterion changed after this TrainStep was built (reduction: %r, was %r): build a new TrainStep"
                                   % (live.reduction, c["reduction"]))
            return
        now = (float(live.label_smoothing), int(live.ignore_index), live.reduction)
        if now != (c["label_smoothing"], c["ignore_index"], c["reduction"]):
            raise RuntimeError("the criterion changed after this TrainStep was built (label_smoothing, ignore_index, reduction: %r, was "
                               "%r): build a new TrainStep" % (now, (c["label_smoothing"], c["ignore_index"], c["reduction"])))

    def __call__(self, inputs, labels):
        """inputs (B, T, 1, 96, 64) (or whatever ``clf.input`` reshapes), labels (B,) int64.
        Returns (loss, hits) as device tensors (no host sync; train.py:141-142 syncs via .item()): hits = int32
        [n_correct, n_labels_out_of_range] over the global batch (``ops.raise_on_bad_labels(hits)`` -> n_correct or IndexError).
        With the HIP graph in use the two tensors (and ``last_out``) are the graph's own buffers: valid until the next step.
        ``inputs`` and ``labels`` are only read, and not kept: the graph works on private copies (one device copy per step).
        With an ``nn.BCELoss``: labels (B, classes) of a bool, integer or float dtype, values in [0, 1]; hits = int32 [rows in which
        every class lies on the right side of 0.5 (subset accuracy), bad cells] over the global batch
        (``ops.raise_on_bad_targets(hits)`` -> the row count or ValueError)."""
        clf = self.clf
        for n, p, ptr in self._seated:
            if p.data_ptr() != ptr:
                raise RuntimeError("parameter %s no longer lives in the flat buffer of this TrainStep (the model was moved or "
                                   "cast after the step was built): build a new TrainStep" % n)
        clf.train()
        if self._crit is None:
            ops.check_labels(labels, clf.mla.classes)
        elif self._bce:
            self._check_criterion()
            ops.check_targets(labels, clf.mla.classes)
        else:
            self._check_criterion()
            ops.check_labels_ignoring(labels, clf.mla.classes, self._crit["ignore_index"])
        if self._graph_usable(inputs) and not self._graph_disturbed():
            return self._graphed(inputs, labels)
        with torch.no_grad():
            loss, hits, out = self._body(inputs, self._device_labels(labels, inputs.device), captured=False)
        self._eager_shape = tuple(inputs.shape)
        self.last_out = out
        self.last_counted = self._counted
        self.last_cell_hits = self._cell_hits
        return loss, hits

    def _device_labels(self, labels, dev):
        """Class indices as int64, multi-label targets as float32: what the loss kernels read."""
        labels = labels.to(dev)
        return (labels.float() if self._bce else labels.long()).contiguous()

    # ---- the step as ONE HIP graph (no data-parallel group): ~130 small launches of the head's forward / backward / Adam and the
    # CNN's kernels become one graph launch; what the host used to pass per step -- Adam's step count, the dropout call number --
    # is read from device memory instead (mla_adam_prepare + mla_adam_step_dev, mla_dropout_mask_dev), so a replay is a real next step.

    def _dropouts(self):
        return [m for m in self.clf.mla.modules() if type(m).__name__ == "Dropout"]

    def _graph_usable(self, inputs):
        if not self.use_graph or self.dist.active or ops.profile is not None or not inputs.is_cuda or inputs.dtype != torch.float32:
            return False
        if not inputs.is_contiguous() or any(d.mask is not None for d in self._dropouts()):
            return False                      # injected masks change per step on the host: the eager path
        # first step of a shape runs eagerly: it sizes the library's workspaces and warms the weight caches outside any capture
        return self._eager_shape == tuple(inputs.shape)

    def _stamp(self):
        """What the recorded kernels read by address without the graph or this step owning it, as host values (no device sync):
        the model precision and the (data_ptr, _version) of every tensor outside the flat buffer that a cached weight copy derives
        from (the frozen VGGish's repacked / bf16 weights, the frozen ResNet trunk's repacks)."""
        lo = self.flat_p.data_ptr()
        hi = lo + 4 * self.flat_p.numel()
        cnn = self.clf.cnn
        return cnn.precision, cache_stamp(weight_caches(cnn), lambda p: lo <= p.data_ptr() < hi)

    def _graph_disturbed(self):
        """True (and the graph is dropped) when something the graph addresses was changed or replaced since the capture: frozen
        weights written in place (load_state_dict) or re-seated, set_precision, a library scratch buffer that grew. The step then
        runs eagerly, which derives fresh copies and sizes the scratch, and the next one is captured again -- the path a change
        of batch shape takes. Until it is dropped the graph holds the tensors it addresses (g["held"]), so none of them has gone
        back to the allocator by then."""
        g = self._graph
        if g is None:
            return False
        live = ops.scratch(self.flat_p.device)
        if self._stamp() == g["stamp"] and all(k in live and live[k].data_ptr() == ptr for k, ptr in g["scratch"].items()):
            return False
        self._graph = None
        return True

    def _graphed(self, inputs, labels):
        dev = inputs.device
        drops = self._dropouts()
        g = self._graph
        if g is not None and (g["shape"] != tuple(inputs.shape) or any(d.calls - self.t != g["bases"][id(d)] for d in drops)):
            g = self._graph = None                                 # another batch size, or somebody else drew masks in between
        if self._dev_t != self.t:
            self.step_dev.fill_(self.t)
            self._dev_t = self.t
        if g is None:
            # the static input and labels are the graph's own: the caller's tensors are never written and never kept
            g = {"shape": tuple(inputs.shape), "x": inputs.clone(), "y": self._device_labels(labels, dev).clone(),
                 "bases": {id(d): d.calls - self.t for d in drops}}
            torch.cuda.synchronize()
            g["graph"] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g["graph"], capture_error_mode="relaxed"), torch.no_grad():
                g["loss"], g["hits"], g["out"] = self._body(g["x"], g["y"], captured=True, bases=g["bases"])
            g["counted"], g["cell_hits"] = self._counted, self._cell_hits
            # what the recorded kernels address without having allocated it during the capture: compared before every replay
            # (_graph_disturbed) and kept alive for as long as this graph is
            scratch = ops.scratch(dev)
            g["stamp"], g["scratch"] = self._stamp(), {k: t.data_ptr() for k, t in scratch.items()}
            g["held"] = [t for c in weight_caches(self.clf.cnn) for t in c.tensors()] + list(scratch.values())
            if self._crit_weight is not None:
                g["held"].append(self._crit_weight)
            self._graph = g
            self.captures += 1
        else:
            g["x"].copy_(inputs, non_blocking=True)
            on_dev = labels.to(dev, non_blocking=True)
            g["y"].copy_(on_dev if self._bce else on_dev.long(), non_blocking=True)       # copy_ casts to the buffer's float32
        if self.groups is not None:
            self._prepare_groups(self.t + 1)
        else:
            ops.adam_prepare(self.adam_scal, self.lr, self.betas[0], self.betas[1], self.t + 1)
        g["graph"].replay()
        self.t += 1
        self._dev_t = self.t
        for d in drops:
            d.calls += 1
        rn = getattr(self.clf.cnn, "_rn_cache", None)
        if rn is not None:                         # the replay moved the ResNet running statistics on the device: eval coefficients are stale
            rn["bn"].key = None
            if self.rn_trunk:                      # and Adam the trunk weights, behind torch's version counters: so are the repacks
                rn["w"].key = None
        if self.finetune:                          # the graph re-derives its own weight copies; anything cached outside it is stale
            for m in self.clf.cnn.modules():
                if hasattr(m, "_cache"):
                    m._cache.key = None
        self.last_out = g["out"]
        self.last_counted, self.last_cell_hits = g["counted"], g["cell_hits"]
        return g["loss"], g["hits"]

    def _body(self, inputs, labels, captured, bases=None):
        """The kernel sequence of one step (train.py:124-138). captured: being recorded into the HIP graph."""
        clf = self.clf
        B_global = inputs.shape[0] * self.dist.world
        x = clf.input(inputs)
        rn_feats = None
        if self.finetune:
            feats, cnn_tape = cnn_train.forward(clf.cnn.cnn_model, x, clf.cnn.precision)
        elif self.resnet:                      # trunk in train mode; its SyncBN statistics go through self.dist
            from . import resnet
            m = clf.cnn.cnn_model
            rn_tape = {} if self.rn_trunk else None
            feats = resnet.trunk_forward(m, x, clf.cnn.precision, True, clf.cnn._rn_cache, dist=self.dist, tape=rn_tape)
            if self.rn_fc:                     # ResNet fc (just_bottlenecks=False): trunk features kept for the fc weight gradient
                rn_feats = feats
                feats = ops.linear_small(rn_feats, m.fc.weight.detach(), m.fc.bias.detach())
            elif not clf.cnn.just_bottlenecks:
                feats = resnet.fc_forward(m.fc, feats)
        else:
            feats = clf.cnn(x)
        ctx = mla_train.Ctx(tape=True, dist=self.dist, counter=self.step_dev if captured else None, bases=bases)
        out = mla_train.mla_forward(clf.mla, feats.reshape(-1, clf.mla.slots, clf.emb_input_size), ctx)
        if self._crit is None:
            loss, dout, hits = ops.cross_entropy(out, labels, 1.0 / B_global)
        elif self._bce:
            # every scalar of the loss is a launch argument: the mean's scale is the global batch's, known on the host
            loss, dout, hits, self._cell_hits = ops.bce_loss(out, labels, self._crit_weight, self._crit["reduction"],
                                                             inv_total=1.0 / (B_global * out.shape[1]))
        else:
            # the mean's denominator is all-reduced inside, on this (the compute) stream like the SyncBN sums, in front of the loss
            c = self._crit
            loss, dout, hits, self._counted = ops.cross_entropy_opts(out, labels, self._crit_weight, c["ignore_index"], c["label_smoothing"],
                                                                     c["reduction"], dist=self.dist)
        d_feats = mla_train.mla_backward(clf.mla, ctx, dout, self.mla_grads,
                                         need_input_grad=self.finetune or self.rn_fc or bool(self.rn_trunk))
        if self.rn_fc:
            fc = clf.cnn.cnn_model.fc
            gw = self.grads.get(self.RN_FC + "weight")
            gb = self.grads.get(self.RN_FC + "bias")
            d_feats = ops.linear_small_bwd(rn_feats, fc.weight.detach(), d_feats.contiguous(),
                                           gw if gw is not None else torch.empty_like(fc.weight, dtype=torch.float32),
                                           gb if gb is not None else torch.empty_like(fc.bias, dtype=torch.float32))
        if self.rn_trunk:                      # head -> fc -> trunk: the trunk's gradients land in the flat buffer
            from . import resnet
            resnet.trunk_backward(clf.cnn.cnn_model, rn_tape, d_feats.reshape(-1, 2048).contiguous(), self.rn_trunk, dist=self.dist)
        bucketed = self.dist.active and self.finetune and self.overlap
        if bucketed:
            # the head's gradients are final: reduce them while the CNN backward runs; each CNN bucket follows as soon as
            # the lowest layer it holds is done. No other collective is issued until the compute stream has waited for
            # the communication stream below, so the two streams never use the communicator at the same time.
            pending = [b for b in ("mla", "fc12", "fc0", "conv56", "conv14") if b in self.buckets]
            if "mla" in pending:
                self._reduce_bucket("mla"); pending.remove("mla")

            def after_layer(pos):
                for b in list(pending):
                    if self.BUCKET_TRIGGER[b] == pos:
                        self._reduce_bucket(b); pending.remove(b)
            cnn_train.backward(clf.cnn.cnn_model, cnn_tape, d_feats, self.grads, "cnn.cnn_model.", after_layer)
            for b in pending:                          # buckets whose trigger layer lies below the lowest trained layer
                self._reduce_bucket(b)
            if self.exposed is not None:               # how long the compute stream really waits for the exchange
                e0, e1 = ops._event(), ops._event()
                e0.record()
                torch.cuda.current_stream().wait_stream(self._comm_stream)
                e1.record()
                self.exposed.append((e0, e1))
            else:
                torch.cuda.current_stream().wait_stream(self._comm_stream)
        elif self.finetune:
            cnn_train.backward(clf.cnn.cnn_model, cnn_tape, d_feats, self.grads, "cnn.cnn_model.")
        if self.dist.active:
            if not bucketed:
                self.dist.all_reduce_sum(self.flat_g, "grad:flat")
            self.dist.all_reduce_sum(loss, "loss")
            self.dist.all_reduce_sum(hits, "hits")             # [running_corrects (train.py:142), #bad labels] over the global batch
            if self._bce:
                self.dist.all_reduce_sum(self._cell_hits, "cell_hits")
            elif self._crit is not None:
                self.dist.all_reduce_sum(self._counted, "counted")
        if self.groups is not None:
            # clip_grad_norm_ on the (all-reduced: the waits above are behind us) flat gradient, then every group in one launch.
            # One form, eager or captured: the rows and the coefficient are device memory either way.
            coef = None
            if self.max_grad_norm is not None:
                ops.grad_norm(self.flat_g, self.max_grad_norm, out=self._clip, workspace=self._norm_ws)
                coef = self.clip_coef
            if not captured:
                self.t += 1
                self._prepare_groups(self.t)
            ops.adam_grouped_step(self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.flat_vmax, self._table, self._n_runs,
                                  self._n_pads, self.group_rows, len(self.groups), coef, self.step_dev if captured else None)
            if not captured:
                self._invalidate_weight_copies()
        elif captured:
            ops.adam_step_dev(self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.betas[0], self.betas[1], self.eps, self.adam_scal, self.step_dev)
        else:
            self.t += 1
            ops.adam_step(self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.lr, self.betas[0], self.betas[1], self.eps, self.t)
            self._invalidate_weight_copies()
        return loss, hits, out

    def _invalidate_weight_copies(self):
        if self.finetune:                          # derived (repacked / bf16) weight copies are stale now
            for m in self.clf.cnn.modules():
                if hasattr(m, "_cache"):
                    m._cache.key = None
        if self.rn_trunk:                          # so are the ResNet trunk's repacked weights (Adam writes behind the version counters)
            self.clf.cnn._rn_cache["w"].key = None


def _evaluate(clf, loader, device, collect=False, criterion=None):
    """criterion: None = the plain mean cross-entropy, or the nn.CrossEntropyLoss to evaluate with (ops.cross_entropy_opts), as the
    reference calls ``criterion(outputs, labels)`` in every phase; the accuracy divides by all rows seen (train.py:145) either way.
    An nn.BCELoss: labels are (B, classes) targets, the loss is ops.bce_loss's, the accuracy is the subset accuracy (rows with every
    class on the right side of 0.5), and collect=True returns the outputs (N, K) and the targets (N, K) instead of predictions."""
    if isinstance(criterion, nn.BCELoss):
        return _evaluate_multilabel(clf, loader, device, collect, criterion)
    clf.eval()
    tot_loss, tot_hits, n, preds, trues = 0.0, 0, 0, [], []
    crit, crit_weight = None, None
    with torch.no_grad():
        for inputs, labels in loader:
            host_labels = labels
            inputs, labels = inputs.to(device).float(), labels.to(device).long()
            out = clf(inputs)
            if criterion is None:
                ops.check_labels(host_labels, out.shape[1])
                loss, _, hits = ops.cross_entropy(out, labels.contiguous(), 1.0 / inputs.shape[0], want_grad=False)
            else:
                if crit is None:
                    crit = parse_criterion(criterion, out.shape[1])
                    crit_weight = None if crit["weight"] is None else crit["weight"].to(device)
                ops.check_labels_ignoring(host_labels, out.shape[1], crit["ignore_index"])
                loss, _, hits, _ = ops.cross_entropy_opts(out, labels.contiguous(), crit_weight, crit["ignore_index"], crit["label_smoothing"],
                                                          crit["reduction"], want_grad=False)
            tot_loss += float(loss) * inputs.shape[0]
            tot_hits += ops.raise_on_bad_labels(hits)
            n += inputs.shape[0]
            if collect:
                preds.append(torch.max(out, 1)[1].cpu()); trues.append(labels.cpu())
    if collect:
        return tot_loss / max(n, 1), tot_hits / max(n, 1), torch.cat(preds), torch.cat(trues)
    return tot_loss / max(n, 1), tot_hits / max(n, 1)


def _evaluate_multilabel(clf, loader, device, collect, criterion):
    """_evaluate under an nn.BCELoss."""
    clf.eval()
    tot_loss, tot_hits, n, outs, trues = 0.0, 0, 0, [], []
    crit, crit_weight = None, None
    with torch.no_grad():
        for inputs, labels in loader:
            inputs = inputs.to(device).float()
            out = clf(inputs)
            if crit is None:
                crit = parse_bce_criterion(criterion, out.shape[1])
                crit_weight = None if crit["weight"] is None else crit["weight"].to(device)
            ops.check_targets(labels, out.shape[1])
            targets = labels.to(device).float().contiguous()
            loss, _, hits, _ = ops.bce_loss(out, targets, crit_weight, crit["reduction"], want_grad=False)
            tot_loss += float(loss) * inputs.shape[0]
            tot_hits += ops.raise_on_bad_targets(hits)
            n += inputs.shape[0]
            if collect:
                outs.append(out.cpu()); trues.append(targets.cpu())
    if collect:
        return tot_loss / max(n, 1), tot_hits / max(n, 1), torch.cat(outs), torch.cat(trues)
    return tot_loss / max(n, 1), tot_hits / max(n, 1)


def multilabel_summary(y_true, y_score, target_names=None):
    """The report of a multi-label run, from targets (N, K) (a cell is positive at >= 0.5) and scores (N, K). Per class: average
    precision = sum_n (R_n - R_{n-1}) P_n over the DISTINCT score thresholds in descending order (tied scores form one threshold),
    ROC AUC = the Mann-Whitney statistic with ties counted one half, and the support (positives). A class without a positive has
    AP = NaN; one without a positive or without a negative has AUC = NaN. "mAP", "mAUC" and "d_prime" = sqrt(2) ndtri(mAUC)
    average over the defined classes only; "classes_without_positives" and "classes_undefined_auc" say how many were left out.
    "subset_accuracy" (all K cells of a row right) and "micro avg" precision / recall / f1-score threshold the scores at 0.5.
    Plain numpy in float64: nothing here is on the GPU path."""
    y_true = np.asarray(y_true, dtype=np.float64) >= 0.5
    y_score = np.asarray(y_score, dtype=np.float64)
    if y_true.ndim != 2 or y_true.shape != y_score.shape:
        raise ValueError("targets %s and scores %s must both be (N, K)" % (y_true.shape, y_score.shape))
    n, k = y_true.shape
    if target_names is None:
        target_names = default_target_names(k)
    if len(target_names) != k:
        raise ValueError("%d target names for %d classes" % (len(target_names), k))
    ap, auc = np.full(k, np.nan), np.full(k, np.nan)
    for c in range(k):
        pos_total = int(y_true[:, c].sum())
        neg_total = n - pos_total
        order = np.argsort(-y_score[:, c], kind="stable")
        s, t = y_score[order, c], y_true[order, c]
        last = np.flatnonzero(np.append(s[1:] != s[:-1], True)) if n else np.zeros(0, dtype=np.int64)    # last row of each threshold
        tp = np.cumsum(t)[last].astype(np.float64)                 # positives at or above the threshold
        fp = (last + 1) - tp
        if pos_total > 0:
            recall = tp / pos_total
            ap[c] = float(np.sum(np.diff(np.append(0.0, recall)) * (tp / (tp + fp))))
        if pos_total > 0 and neg_total > 0:
            pos_g, neg_g = np.diff(np.append(0.0, tp)), np.diff(np.append(0.0, fp))
            auc[c] = float(np.sum(pos_g * ((neg_total - fp) + 0.5 * neg_g)) / (float(pos_total) * float(neg_total)))
    res = {name: {"average_precision": float(ap[i]), "roc_auc": float(auc[i]), "support": int(y_true[:, i].sum())}
           for i, name in enumerate(target_names)}
    res["mAP"] = float(np.mean(ap[~np.isnan(ap)])) if (~np.isnan(ap)).any() else float("nan")
    res["mAUC"] = float(np.mean(auc[~np.isnan(auc)])) if (~np.isnan(auc)).any() else float("nan")
    res["d_prime"] = float(np.sqrt(2.0) * torch.special.ndtri(torch.tensor(res["mAUC"], dtype=torch.float64)))
    res["classes_without_positives"] = int(np.isnan(ap).sum())
    res["classes_undefined_auc"] = int(np.isnan(auc).sum())
    pred = y_score >= 0.5
    res["subset_accuracy"] = float((pred == y_true).all(axis=1).mean()) if n else 0.0
    tp_all, n_pred, n_pos = float((pred & y_true).sum()), float(pred.sum()), float(y_true.sum())
    prec = tp_all / n_pred if n_pred else 0.0
    rec = tp_all / n_pos if n_pos else 0.0
    res["micro avg"] = {"precision": prec, "recall": rec, "f1-score": 2 * prec * rec / (prec + rec) if prec + rec else 0.0,
                        "support": int(n_pos)}
    return res


def classification_summary(y_true, y_pred, target_names=TARGET_NAMES):
    """Per-class precision / recall / f1 / support + accuracy and macro / weighted averages, laid out like
    sklearn's ``classification_report(output_dict=True)`` (train.py:246), and the row-normalised confusion
    matrix in percent (train.py:237-241). Plain numpy: nothing here is on the GPU path."""
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    k = len(target_names)
    cm = np.zeros((k, k), dtype=np.float64)
    np.add.at(cm, (y_true, y_pred), 1.0)
    tp, support, predicted = np.diag(cm), cm.sum(axis=1), cm.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.where(predicted > 0, tp / predicted, 0.0)
        rec = np.where(support > 0, tp / support, 0.0)
        f1 = np.where(prec + rec > 0, 2 * prec * rec / (prec + rec), 0.0)
        cm_pct = np.where(support[:, None] > 0, cm * 100.0 / support[:, None], 0.0).astype(np.float32)
    res = {name: {"precision": float(prec[i]), "recall": float(rec[i]), "f1-score": float(f1[i]), "support": int(support[i])}
           for i, name in enumerate(target_names)}
    total = float(support.sum())
    res["accuracy"] = float(tp.sum() / total) if total else 0.0
    for tag, wts in (("macro avg", np.ones(k)), ("weighted avg", support)):
        w = wts / wts.sum() if wts.sum() else wts
        res[tag] = {"precision": float((prec * w).sum()), "recall": float((rec * w).sum()), "f1-score": float((f1 * w).sum()),
                    "support": int(total)}
    return res, cm_pct


def default_target_names(classes):
    """Row names of the test report: the dataset's own for its 10 classes, else class_0, class_1, ..."""
    return list(TARGET_NAMES) if classes == len(TARGET_NAMES) else ["class_%d" % i for i in range(classes)]


def test_model(model, dataloader, criterion=None, optimizer=None, target_names=None):
    """train.py:182-247: final test pass -> (test accuracy, classification summary dict). The confusion-matrix
    plot of the reference is not reproduced; the matrix itself is returned under ``results["confusion_matrix_pct"]``.
    target_names: one name per class of the head; None = TARGET_NAMES for a 10-class head, else class_0, class_1, ...
    ``criterion`` is not read here: the test loss is the plain mean (``train_model(extended_criterion=True)`` tests with its criterion)."""
    return _test_model(model, dataloader, target_names, None)


def _test_model(model, dataloader, target_names, criterion):
    """test_model's body. criterion: None = the plain mean, or the nn.CrossEntropyLoss the test loss is taken with; rows whose label it
    ignores stay in the accuracy's denominator and are left out of the classification summary."""
    if dataloader is None:
        return None
    device = next(model.parameters()).device
    since = time.time()
    print("Testing"); print("-" * 10)
    loss, acc, preds, trues = _evaluate(model, dataloader, device, collect=True, criterion=criterion)
    if isinstance(criterion, nn.BCELoss):                  # preds: the outputs (N, K); the report is mAP / AUC, not a confusion matrix
        results = multilabel_summary(trues.numpy(), preds.numpy(), target_names)
        print("{} Loss: {:.4f}, subset Acc: {:.4f}, mAP: {:.4f}, mAUC: {:.4f}".format("test", loss, acc, results["mAP"], results["mAUC"]))
        print("Testing complete in {:.0f}s".format(time.time() - since))
        return results["mAP"], results
    if criterion is not None:
        keep = trues != int(criterion.ignore_index)
        preds, trues = preds[keep], trues[keep]
    print("{} Loss: {:.4f}, Acc: {:.4f}".format("test", loss, acc))
    print("Testing complete in {:.0f}s".format(time.time() - since))
    if target_names is None:
        mla = getattr(model, "mla", model)
        target_names = default_target_names(getattr(mla, "classes", len(TARGET_NAMES)))
    results, cm = classification_summary(trues.numpy(), preds.numpy(), target_names)
    results["confusion_matrix_pct"] = cm
    return acc, results


def _save_checkpoint(model, step, epoch, loss, accuracy, history, path):
    """train.py:249-258 with tensors and numbers only (the reference pickles whole objects; these files load with
    ``torch.load(weights_only=True)``): model ``state_dict`` + Adam state of the fused step + bookkeeping."""
    torch.save({"epoch": int(epoch), "model": model.state_dict(), "optimizer": step.state_dict(), "loss": float(loss),
                "accuracy": float(accuracy), "history": [float(h) for h in history]}, path)


def _resume_from_checkpoint(path, model, step):
    """train.py:260-262: restores `model` and `step` in place, returns (epoch, loss, accuracy, history)."""
    d = torch.load(path, map_location=next(model.parameters()).device, weights_only=True)
    model.load_state_dict(d["model"])
    step.load_state_dict(d["optimizer"])
    return d["epoch"], d["loss"], d["accuracy"], list(d["history"])


def save_model(model, path):
    """train.py:265-266."""
    torch.save(model.state_dict(), path)


def load_model(model_args, path):
    """train.py:268-271: build an Ensemble from its constructor arguments and load a ``save_model`` file."""
    from .model import Ensemble
    m = Ensemble(**model_args)
    m.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
    return m


def train_model(clf, dataloaders, criterion, optimizer, num_epochs=25, patience=10, save_model_path=None, resume=False,
                finetune=False, extended_optimizer=False, scheduler=None, max_grad_norm=None, extended_criterion=False):
    """Epoch loop with the reference's signature and return value (train.py:53-179):
    (model with the best-validation weights, validation accuracy history, test_model's result).
    ``criterion`` must be nn.CrossEntropyLoss and ``optimizer`` a one-group torch.optim.Adam without weight decay /
    amsgrad: its hyper-parameters AND its parameter list are read -- the fused HIP step updates exactly the tensors the
    optimizer holds (and that require grad), as ``optimizer.step()`` does; the torch optimizer object itself is not
    stepped (its ``state`` stays empty; the moments live in the checkpoint written here). Checkpoints hold tensors only
    (``_save_checkpoint``); ``resume=True`` continues from ``save_model_path`` (epoch, best accuracy, history,
    weights and Adam moments), as train.py:80-94 does from its pickled objects.
    ``extended_optimizer=True`` lifts the one-group rule: ``optimizer`` is a torch Adam or AdamW with any parameter groups (per-group
    lr / betas / eps / weight_decay / amsgrad), stepped by the grouped HIP step; ``scheduler`` (any torch LR scheduler over that
    optimizer) is stepped once per epoch after validation, a ``ReduceLROnPlateau`` with the validation loss; ``max_grad_norm``
    clips the gradient's L2 norm before each update. The last two need ``extended_optimizer=True``.
    ``extended_criterion=True``: ``criterion``'s ``weight``, ``ignore_index``, ``label_smoothing`` and ``reduction`` ("mean" | "sum") are
    honoured by the step (``TrainStep(criterion=)``) and by the validation and test loss; off, the criterion is the plain mean and
    a label of -100 is refused like any other label outside the classes.
    ``criterion=nn.BCELoss(weight, reduction)`` with ``extended_criterion=True`` trains a multi-label head: labels are (B, classes)
    targets in [0, 1], "train Acc" is the subset accuracy, validation computes ``multilabel_summary`` and its **mAP** is the number
    that enters the history, selects the best weights, is stored as the checkpoint's ``accuracy`` and drives ``patience``;
    ``scheduler`` still gets the validation loss, and the test phase returns ``(mAP, summary)``."""
    multilabel = extended_criterion and isinstance(criterion, nn.BCELoss)
    if not (isinstance(criterion, nn.CrossEntropyLoss) or multilabel) or not isinstance(optimizer, torch.optim.Adam):
        raise TypeError("the HIP training step implements CrossEntropyLoss + Adam (train.py:369-372), and with extended_criterion=True "
                        "BCELoss + Adam")
    if not extended_optimizer:
        if scheduler is not None or max_grad_norm is not None:
            raise ValueError("scheduler= and max_grad_norm= belong to the grouped HIP step: pass extended_optimizer=True")
        if len(optimizer.param_groups) != 1:
            raise NotImplementedError("the HIP Adam step takes ONE parameter group (train.py:369-370 builds one); "
                                      "extended_optimizer=True steps several")
        g = optimizer.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise NotImplementedError("weight_decay / amsgrad / maximize are not implemented by the HIP Adam step (train.py:369 uses "
                                      "none); extended_optimizer=True implements weight_decay and amsgrad")
    if finetune:
        from .model import set_requires_grad
        set_requires_grad(clf, True)                       # train.py:96-97 (AFTER the caller built the optimizer)
    import copy
    device = torch.device("cuda", torch.cuda.current_device())
    clf.to(device)                                         # train.py:101
    crit = criterion if extended_criterion else None
    if extended_optimizer:
        step = TrainStep(clf, optimizer=optimizer, max_grad_norm=max_grad_norm, criterion=crit)   # reads the groups at every step
    else:
        step = TrainStep(clf, lr=g["lr"], betas=g["betas"], eps=g["eps"], params=g["params"], criterion=crit)     # steps what the optimizer holds
    since, val_acc_history, best_acc, best_epoch, first_epoch = time.time(), [], 0.0, 0, 0
    if resume:
        assert save_model_path is not None
        if not os.path.exists(save_model_path):
            raise Exception("No such model file in the specified path.")
        ep, _, best_acc, val_acc_history = _resume_from_checkpoint(save_model_path, clf, step)
        first_epoch, best_epoch = ep + 1, ep
    best_wts = copy.deepcopy(clf.state_dict())
    test_loader = dataloaders.pop("test", None)
    for epoch in range(first_epoch, num_epochs):
        print("Epoch {}/{}".format(epoch + 1, num_epochs)); print("-" * 10)
        run_loss, run_hits, n = 0.0, 0, 0
        for inputs, labels in dataloaders["train"]:
            loss, hits = step(inputs.to(device).float(), labels)
            # under data parallelism the step returns the GLOBAL mean loss and the GLOBAL hit count (train.py:141-142 on the whole batch)
            seen = inputs.shape[0] * (step.dist.world if step.dist.active else 1)
            run_loss += float(loss) * seen; n += seen
            run_hits += ops.raise_on_bad_targets(hits) if multilabel else ops.raise_on_bad_labels(hits)
        print("train Loss: {:.4f}, Acc: {:.4f}".format(run_loss / max(n, 1), run_hits / max(n, 1)))
        if multilabel:                                     # the model-selection metric is the validation mAP
            v_loss, v_subset, v_out, v_true = _evaluate(clf, dataloaders["val"], device, collect=True, criterion=crit)
            v_sum = multilabel_summary(v_true.numpy(), v_out.numpy())
            v_acc = v_sum["mAP"]
            print("val Loss: {:.4f}, subset Acc: {:.4f}, mAP: {:.4f}, mAUC: {:.4f}".format(v_loss, v_subset, v_acc, v_sum["mAUC"]))
        else:
            v_loss, v_acc = _evaluate(clf, dataloaders["val"], device, criterion=crit)
            print("val Loss: {:.4f}, Acc: {:.4f}".format(v_loss, v_acc))
        val_acc_history.append(v_acc)
        if v_acc > best_acc:
            best_acc, best_epoch, best_wts = v_acc, epoch, copy.deepcopy(clf.state_dict())
            if save_model_path:
                _save_checkpoint(clf, step, epoch, v_loss, best_acc, val_acc_history, save_model_path)
                print("Model checkpoint saved successfully in the given path!")
        if scheduler is not None:                          # after the checkpoint: a resumed run steps the scheduler at the same point
            import warnings
            with warnings.catch_warnings():                # torch warns that optimizer.step() was never called: the HIP step stands in for it
                warnings.filterwarnings("ignore", message=r"Detected call of `lr_scheduler\.step\(\)` before")
                if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
                    scheduler.step(v_loss)
                else:
                    scheduler.step()
        if patience is not None and epoch - best_epoch >= patience:
            break
    print("Training complete in {:.0f}s; best val Acc: {:4f}".format(time.time() - since, best_acc))
    clf.load_state_dict(best_wts)
    tested = test_model(clf, test_loader) if crit is None else _test_model(clf, test_loader, None, crit)
    final = save_model_path or "best_weights.h5"
    root, ext = os.path.splitext(final)
    save_model(clf, root + ("_final_finetuned" if finetune else "_final") + ext)       # train.py:173-177
    return clf, val_acc_history, tested                    # test_model's (accuracy, summary) tuple or None, as train.py:179
