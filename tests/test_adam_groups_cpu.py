"""CPU tests of the grouped Adam step's host side: the float64 restatement the GPU tests compare against (tests/adam_groups_cases.py)
pinned to torch.optim.Adam / AdamW, and the run-table builder of csrc/adam_groups.h through mla_adam_groups_table (no device)."""

import importlib

import numpy as np
import pytest
import torch

import adam_groups_cases as C
from conftest import PKG


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("opt", ["Adam", "AdamW"])
def test_restatement_equals_torch_in_float64(opt, amsgrad):
    """Two groups with different lr and weight_decay, clip_grad_norm_(..., 0.5), three steps, foreach=False: 1e-12."""
    rng = np.random.default_rng(11)
    shapes = [(7, 5), (13,), (4, 3, 2), (9,)]
    owner = [0, 1, 0, 1]
    params = [torch.nn.Parameter(torch.tensor(rng.uniform(-1, 1, s), dtype=torch.float64)) for s in shapes]
    hyper = [dict(lr=1e-3, weight_decay=1e-2), dict(lr=3e-4, weight_decay=0.0, betas=(0.8, 0.99), eps=1e-6)]
    cls = getattr(torch.optim, opt)
    torch_opt = cls([dict(params=[p for p, o in zip(params, owner) if o == g], **hyper[g]) for g in range(2)], amsgrad=amsgrad, foreach=False)
    groups = [dict(lr=h["lr"], betas=h.get("betas", (0.9, 0.999)), eps=h.get("eps", 1e-8), weight_decay=h["weight_decay"],
                   decoupled=opt == "AdamW", amsgrad=amsgrad) for h in hyper]
    layout = [(int(np.prod(s)), o) for s, o in zip(shapes, owner)]
    offs, total = C.offsets(layout)
    idx = C.group_index(layout)
    flat = np.zeros(total)
    for p, o in zip(params, offs):
        flat[o:o + p.numel()] = p.detach().numpy().ravel()
    state = C.fresh_state(flat)
    for t in range(1, 4):
        g = np.zeros(total)
        for p, o in zip(params, offs):
            p.grad = torch.tensor(rng.uniform(-1, 1, tuple(p.shape)) * 10.0 ** rng.uniform(0, 2), dtype=torch.float64)
            g[o:o + p.numel()] = p.grad.numpy().ravel()
        norm, coef = C.clip_coef(g, 0.5)
        got_norm = torch.nn.utils.clip_grad_norm_(params, 0.5, foreach=False)
        assert abs(float(got_norm) - norm) <= 1e-12 * norm and coef < 1.0
        torch_opt.step()
        C.restated_step(state, g, groups, idx, t, coef)
        for p, o in zip(params, offs):
            np.testing.assert_allclose(state["p"][o:o + p.numel()], p.detach().numpy().ravel(), rtol=0, atol=1e-12)
    assert not state["p"][~C.real_mask(layout)].any()


def test_clip_coefficient_edge_cases():
    assert C.clip_coef(np.array([3.0, 4.0]), 10.0) == (5.0, 1.0)
    norm, coef = C.clip_coef(np.array([1.0, np.nan]), 1.0)
    assert norm != norm and coef != coef
    assert C.clip_coef(np.array([1.0, np.inf]), 1.0) == (np.inf, 0.0)


def table_of(layout, n_groups):
    ops = importlib.import_module(PKG + ".ops")
    t = ops.adam_groups_table([k for k, _ in layout], [g for _, g in layout], n_groups)
    tab = t["table"].tolist()
    R, Cn, P = t["runs"], t["chunks"], t["pads"]
    assert len(tab) == 2 * R + 2 * Cn + 1 + 2 * P
    pads = tab[2 * R + 2 * Cn + 1:]
    return t, list(zip(tab[:R], tab[R:2 * R])), tab[2 * R:2 * R + Cn], tab[2 * R + Cn:2 * R + 2 * Cn + 1], list(zip(pads[0::2], pads[1::2]))


def test_interleaved_groups_merge_into_maximal_runs():
    # weights in group 0, biases in group 1, with neighbours of one group in between: w b | b | w w | b
    layout = [(64, 0), (8, 1), (6, 1), (32, 0), (12, 0), (10, 1)]
    t, runs, chunk_run, chunk_pad, pads = table_of(layout, 2)
    assert runs == C.expected_runs(layout) == [(64, 0), (80, 1), (124, 0), (136, 1)]
    assert t["total"] == 136 and t["chunks"] == 1 and chunk_run == [0]
    assert pads == [(72 + 4, 2), (124 + 8, 2)] and chunk_pad == [0, 2]
    # one group only: one run whatever the tensors
    _, runs, _, _, _ = table_of([(5, 0), (7, 0), (64, 0)], 1)
    assert runs == [(8 + 8 + 64, 0)]


def test_small_tensors_keep_their_pad4_offsets():
    layout = [(1, 0), (3, 1), (4, 0), (5, 1)]
    offs, total = C.offsets(layout)
    assert offs == [0, 4, 8, 12] and total == 20
    t, runs, chunk_run, chunk_pad, pads = table_of(layout, 2)
    assert t["total"] == total and runs == [(4, 0), (8, 1), (12, 0), (20, 1)]
    # the quad that ends a tensor of 4 k + r elements, and r: 1 element at 0, 3 at 4, none for the 4, 1 at 12 + 4
    assert pads == [(0, 1), (4, 3), (16, 1)] and chunk_pad == [0, 3]


def test_chunk_sections_follow_the_runs_across_a_sweep():
    layout = C.layout_wrapped()
    t, runs, chunk_run, chunk_pad, pads = table_of(layout, 3)
    offs, total = C.offsets(layout)
    past = sum(k for k, _ in layout) - C.ADAM_SWEEP
    assert t["total"] == total and past > 0 and past % 2 == 1          # beyond one sweep by an odd count
    assert runs == C.expected_runs(layout) and len(chunk_run) == (total + 2047) // 2048
    ends = [e for e, _ in runs]
    for c, r in enumerate(chunk_run):                              # the run that holds the chunk's first element
        assert (ends[r - 1] if r else 0) <= c * 2048 < ends[r]
    for c in range(len(chunk_run)):                                # the padding quads inside the chunk, and no others
        inside = [i for i, (q, _) in enumerate(pads) if c * 2048 <= q < (c + 1) * 2048]
        assert list(range(chunk_pad[c], chunk_pad[c + 1])) == inside
    assert any(ends[r] > C.ADAM_SWEEP > (ends[r - 1] if r else 0) for r in range(len(runs))) or C.ADAM_SWEEP in ends
    assert sum(1 for e in ends if e > C.ADAM_SWEEP) >= 2           # a group boundary inside the wrapped part


def test_more_than_64_groups_are_refused():
    ops = importlib.import_module(PKG + ".ops")
    lib = importlib.import_module(PKG + "._lib")
    assert ops.adam_groups_table([4] * 64, list(range(64)), 64)["runs"] == 64
    with pytest.raises(lib.MlaError) as e:
        ops.adam_groups_table([4] * 65, list(range(65)), 65)
    assert e.value.code == -2 and "65" in str(e.value)              # MLA_E_SHAPE
    with pytest.raises(lib.MlaError):
        ops.adam_groups_table([4, 4], [0, 2], 2)                     # a group index outside [0, n_groups)
    import ctypes
    rows = (lib.AdamGroup * 65)()
    fake = ctypes.c_void_p(0x1000)                                   # never dereferenced: refused before any launch
    assert lib.lib().mla_adam_groups_prepare(fake, rows, 65, 1, None) == -2
    assert lib.lib().mla_adam_grouped_step(fake, fake, fake, fake, None, 8, fake, 100, 1, 0, fake, 65, None, None) == -2
    assert lib.lib().mla_adam_grouped_step(fake, fake, fake, fake, None, 6, fake, 100, 1, 0, fake, 1, None, None) == -2    # n % 4
    assert lib.lib().mla_adam_grouped_step(fake, fake, fake, fake, None, 8, fake, 3, 1, 0, fake, 1, None, None) == -1      # table too short
