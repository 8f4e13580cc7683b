"""The launch order and operand wiring of the ResNet trunk walks (resnet.trunk_forward, trunk_backward, trunk_input_backward),
checked without a device: every ``ops.rn_*`` wrapper they call is replaced by a shape-only recorder (tests/resnet_walk_trace.py)
and the traces are compared with tests/golden/resnet_walk_trace.json (tests/golden/make_golden_resnet_walk.py)."""

import importlib
import json
import os

import pytest
import torch

import resnet_walk_trace as T
from conftest import GOLDEN, PKG

M = importlib.import_module(PKG + ".model")
RN = importlib.import_module(PKG + ".resnet")
ops = importlib.import_module(PKG + ".ops")

# calls per scenario: what a broken harness shows first (the fixture is what the traces are compared with)
COUNTS = {"eval_forward": 160, "eval_input_backward": 214, "train_forward": 213, "train_all": 425, "train_layer3_2_up": 248,
          "train_conv1": 321, "train_none": 161}


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "resnet_walk_trace.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("jb,precision", T.CONFIGS)
def test_walks_launch_what_the_fixture_records(jb, precision, fixture, monkeypatch):
    tracer = T.install(ops, monkeypatch.setattr)
    seen = []
    for tag, names, sha, tape in T.scenarios(M, RN, tracer, jb, precision):
        want = fixture[T.key(jb, precision, tag)]
        assert len(want["names"]) == COUNTS[tag], tag
        diverge = next((i for i, (a, b) in enumerate(zip(names, want["names"])) if a != b), min(len(names), len(want["names"])))
        assert names == want["names"], "%s: call %d is %s, the fixture has %s" % (tag, diverge, names[diverge:diverge + 3],
                                                                                  want["names"][diverge:diverge + 3])
        assert sha == want["sha256"], "%s: the same calls in the same order, on other operands" % tag
        assert tape is None or len(tape) == 0, "%s: the backward consumes its tape" % tag
        seen.append(tag)
    assert seen == list(COUNTS)


@pytest.mark.parametrize("jb,precision", T.CONFIGS)
def test_trunk_backward_refuses_an_eval_tape(jb, precision, monkeypatch):
    tracer = T.install(ops, monkeypatch.setattr)
    cnn = T.new_model(M, jb, precision, True).eval()
    tape = T.taped_eval_forward(RN, cnn, precision)
    grads = {id(p): torch.empty(p.shape) for _, p in RN.trunk_params(cnn.cnn_model)}
    tracer.begin()
    with pytest.raises(AssertionError, match="train-mode"):
        RN.trunk_backward(cnn.cnn_model, tape, torch.empty(T.N, 2048), grads)
    assert tracer.log == []
