"""The CPU oracle's saliency gradients that tests/test_input_grad_gpu.py measures the HIP path against, computed once per
(just_bottlenecks, seed) and shared: the gradient of scores[b, target_b] with respect to the bags' examples through
oracle.model.ensemble_forward in float64 (the reference), in float32 (the yardstick of the f32 comparison) and under
torch.autocast("cpu", bfloat16) (the yardstick of the bf16 comparison). Device-free.

ReLU / pool routing makes this gradient discontinuous: a unit flipped anywhere in the stack changes one example's whole map, so
errors are taken per example and relative to the bag's gradient norm, and the f32 comparison uses seeds at which the f32 oracle
itself is flip-free (asserted by the test before it looks at the GPU result)."""

import functools
import importlib

import torch

from conftest import PKG
from oracle import model as OM

BAGS = 2
SEED_JB0 = 102            # the issue's seed for just_bottlenecks=False: the f32 oracle is flip-free there (R = 2.1e-5)
SEEDS_JB1 = range(100, 120)
SEED_JB1 = 108            # first_flip_free_seed(True): the first of SEEDS_JB1 with every r_i <= FLIP_FREE (100..107 have 2e-4 .. 6e-3)
FLIP_FREE = 1e-4          # every per-example r_i of the f32 oracle at or below this: no unit flipped


def state_dict(jb):
    W = importlib.import_module(PKG + ".weights")
    return {k: torch.as_tensor(v) for k, v in W.make_state_dict(7, W.ensemble_shapes((2, 1), jb)).items()}


def _grad(sd, x, jb, target, autocast=False):
    x = x.clone().requires_grad_(True)
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            scores = OM.ensemble_forward(sd, x, (2, 1), jb)
    else:
        scores = OM.ensemble_forward(sd, x, (2, 1), jb)
    scores = scores.double() if scores.dtype != torch.float64 else scores
    idx = scores.detach().argmax(dim=1) if target is None else target
    g, = torch.autograd.grad(scores.gather(1, idx.view(-1, 1)).sum(), [x])
    return scores.detach(), idx, g.detach().double()


@functools.lru_cache(maxsize=None)
def oracle(jb, seed):
    """dict: x (2, 10, 1, 96, 64) f32, target (2,) = the float64 arg-max, scores64, g64 and g32 (the float32 oracle's gradient for the
    same targets), gradients as float64 tensors of x's shape."""
    mk = importlib.import_module("make_golden")
    x = mk.synth_bags(seed, BAGS)[0].float()
    sd32 = state_dict(jb)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd32.items()}
    scores64, target, g64 = _grad(sd64, x.double(), jb, None)
    return dict(x=x, target=target, scores64=scores64, g64=g64, g32=_grad(sd32, x, jb, target)[2])


@functools.lru_cache(maxsize=None)
def oracle_autocast(jb, seed):
    """The float32 oracle under torch.autocast("cpu", bfloat16) on the same inputs and targets: its gradient, float64 of x's shape."""
    o = oracle(jb, seed)
    return _grad(state_dict(jb), o["x"], jb, o["target"], autocast=True)[2]


def first_flip_free_seed(jb):
    """The first seed of SEEDS_JB1 at which every per-example error of the f32 oracle is at most FLIP_FREE (about a second per
    seed: run by hand when the oracle or the weights change; the tests assert the property at the seed they use)."""
    for seed in SEEDS_JB1:
        o = oracle(jb, seed)
        if float(per_example_error(o["g32"], o["g64"]).max()) <= FLIP_FREE:
            return seed
    raise AssertionError("no flip-free seed")


def per_example_error(g, g64):
    """e_i = |g_i - g64_i|_2 / |g64 of the example's bag|_2 -> (2, 10)."""
    num = (g.double() - g64).flatten(2).norm(dim=2)
    return num / g64.flatten(1).norm(dim=1, keepdim=True)


def bag_error(g, g64):
    """|g - g64|_2 / |g64|_2 per bag -> (2,)."""
    return (g.double() - g64).flatten(1).norm(dim=1) / g64.flatten(1).norm(dim=1)


def one_minus_cos(g, g64):
    a, b = g.double().flatten(1), g64.flatten(1)
    return 1.0 - (a * b).sum(dim=1) / (a.norm(dim=1) * b.norm(dim=1))
