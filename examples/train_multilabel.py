#!/usr/bin/env python3
"""Multi-label training through train_model: a synthetic 20-class multi-hot task (every tag adds its own spectral pattern to a bag of
log-mel examples; a bag carries one to three tags) trained with nn.BCELoss on the head's sigmoid outputs. The criterion runs in the
fused HIP step (TrainStep(criterion=nn.BCELoss(...)) under train_model(extended_criterion=True)); the validation mAP selects the
best weights and the test phase returns (mAP, summary).

    python examples/train_multilabel.py [epochs]

The VGGish weights are seeded, not pretrained, and stay frozen: the printed mAP only shows that the head learns the tags."""

import importlib
import os
import sys
import tempfile

import numpy as np
import torch
from torch.utils.data import DataLoader, TensorDataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"
M = importlib.import_module(PKG + ".model")
W = importlib.import_module(PKG + ".weights")
TR = importlib.import_module(PKG + ".train")

CLASSES, SLOTS = 20, 10


def synthetic(n, seed):
    """(n, 10, 1, 96, 64) bags in the front-end's value range and (n, 20) multi-hot targets: tag k adds pattern k to half of the slots."""
    rng = np.random.default_rng(seed)
    patterns = np.random.default_rng(1).normal(0.0, 1.0, (CLASSES, 96, 64)).astype(np.float32)
    y = np.zeros((n, CLASSES), dtype=np.float32)
    x = rng.normal(1.6, 1.0, (n, SLOTS, 1, 96, 64)).astype(np.float32)
    for b in range(n):
        tags = rng.choice(CLASSES, size=rng.integers(1, 4), replace=False)
        y[b, tags] = 1.0
        for k in tags:
            slots = rng.choice(SLOTS, size=SLOTS // 2, replace=False)
            x[b, slots, 0] += 1.5 * patterns[k]
    return torch.from_numpy(x), torch.from_numpy(y)


def main():
    epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    conf = dict(cnn_type="vggish", num_classes=10, use_pretrained=False, just_bottlenecks=False, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=1)
    torch.manual_seed(0)
    clf = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"), classes=CLASSES)
    shapes = W.mla_shapes([2, 1], 128, prefix="mla.", K=CLASSES)
    shapes.update(W.vggish_shapes("cnn.cnn_model."))
    clf.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(7, shapes).items()})
    clf.cuda()
    loaders = {split: DataLoader(TensorDataset(*synthetic(n, seed)), batch_size=32, shuffle=split == "train")
               for split, n, seed in (("train", 256, 10), ("val", 64, 11), ("test", 64, 12))}
    # rare tags may weigh more: one weight per class, as nn.BCELoss(weight=) broadcasts it over the batch
    criterion = torch.nn.BCELoss(weight=torch.ones(CLASSES))
    optimizer = torch.optim.Adam(TR.trainable_params(clf, True), lr=1e-3)
    with tempfile.TemporaryDirectory() as tmp:
        clf, history, tested = TR.train_model(clf, loaders, criterion, optimizer, num_epochs=epochs, patience=None,
                                              save_model_path=os.path.join(tmp, "multilabel.pt"), extended_criterion=True)
    m_ap, summary = tested
    print("validation mAP per epoch: %s" % " ".join("%.3f" % h for h in history))
    print("test mAP %.3f, mAUC %.3f, d' %.2f, subset accuracy %.3f, micro F1 %.3f (%d classes without positives)"
          % (m_ap, summary["mAUC"], summary["d_prime"], summary["subset_accuracy"], summary["micro avg"]["f1-score"],
             summary["classes_without_positives"]))


if __name__ == "__main__":
    main()
