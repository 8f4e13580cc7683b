"""Which memory a HIP graph reads and writes when it is replayed: the captured training step (TrainStep(graph=True)) and the
captured inference forward (Ensemble.capture_waveforms) record raw device pointers -- of the batch, of derived weight copies
(repacked / bf16, torchvggish.vggish._Cache) and of the library's module-global scratch (ops._ws). Each scenario disturbs one of
them between replays the way a training loop does (device-resident batches reused across epochs, load_state_dict / set_precision /
an evaluation pass, an eager call that needs more scratch) and runs an eager twin (graph=False, same dropout ordinals) through the
identical calls. The tolerance is the graph path's contract: bit-for-bit equality of every loss, hit count, parameter, Adam moment
and buffer. The ownership checks read what both graph holders expose: ``held`` (the tensors the graph addresses without having
allocated them during the capture) and ``captures``."""

import importlib
import types

import pytest
import torch

from conftest import PKG
from test_train_graph_gpu import make

pytestmark = pytest.mark.gpu

M = importlib.import_module(PKG + ".model")
TR = importlib.import_module(PKG + ".train")
ops = importlib.import_module(PKG + ".ops")

BAGS = 8
CASES = [("bf16", False), ("f32", False), ("bf16", True)]            # (precision, finetune) as in test_train_graph_gpu.py


@pytest.fixture(scope="module")
def Wm(W):
    """The weights module with make_state_dict remembered per (seed, key set): 73 M portable-seeded values take seconds to draw,
    and load_state_dict copies them, so sharing the arrays between the models of this file is safe."""
    memo = {}

    def make_state_dict(seed, shapes):
        key = (seed, tuple(shapes))
        if key not in memo:
            memo[key] = W.make_state_dict(seed, shapes)
        return memo[key]
    return types.SimpleNamespace(make_state_dict=make_state_dict, ensemble_shapes=W.ensemble_shapes, waveform=W.waveform,
                                 uniform=W.uniform, stream_id=W.stream_id)


@pytest.fixture(scope="module")
def batches(mk):
    """Four host batches of 8 bags, drawn once and never written."""
    return [mk.synth_bags(300 + i, BAGS) for i in range(4)]


def twins(mk, Wm, precision, finetune):
    ens_e, step_e, ords = make(mk, Wm, precision, finetune, graph=False)
    ens_g, step_g, _ = make(mk, Wm, precision, finetune, graph=True, ordinals=ords)
    return (ens_e, step_e), (ens_g, step_g)


def result(pair):
    loss, hits = pair
    return float(loss), hits.tolist()


def assert_same_state(eager, graphed):
    (ens_e, step_e), (ens_g, step_g) = eager, graphed
    assert step_e._graph is None and step_e.captures == 0
    assert step_g.t == step_e.t
    assert torch.equal(step_g.flat_p, step_e.flat_p) and torch.equal(step_g.flat_m, step_e.flat_m) and torch.equal(step_g.flat_v, step_e.flat_v)
    for (k, a), (_, b) in zip(ens_g.state_dict().items(), ens_e.state_dict().items()):
        assert torch.equal(a, b), k


def other_cnn_weights(Wm, seed=8):
    """A second set of CNN weights in the key layout of Ensemble.cnn.load_state_dict."""
    sd = Wm.make_state_dict(seed, Wm.ensemble_shapes((2, 1), False))
    return {k[len("cnn."):]: torch.as_tensor(v) for k, v in sd.items() if k.startswith("cnn.")}


def eval_forward(ens, x):
    ens.eval()
    with torch.no_grad():
        return ens(x)


# ---- 1. device-resident batches reused across epochs --------------------------------------------------------------------------

@pytest.mark.parametrize("host_labels", [False, True])
@pytest.mark.parametrize("precision,finetune", CASES)
def test_preloaded_device_batches_two_epochs(mk, Wm, batches, precision, finetune, host_labels):
    """[b0, b1, b2, b3] live on the device for the whole run. The first step of the shape is eager on b0 and the capture happens on
    b1: a step that adopted b1 as its static input would copy b0, b2, b3 over it and then train on them under b1's labels."""
    def two_epochs(step):
        xs = [x.cuda() for x, _ in batches]
        ys = [y if host_labels else y.cuda() for _, y in batches]
        witness = [(x.clone(), y.clone()) for x, y in zip(xs, ys)]
        out = [result(step(xs[i], ys[i])) for _ in range(2) for i in range(4)]
        written = [i for i in range(4) if not (torch.equal(xs[i], witness[i][0]) and torch.equal(ys[i], witness[i][1]))]
        return out, written

    eager, graphed = twins(mk, Wm, precision, finetune)
    ref, written_e = two_epochs(eager[1])
    got, written_g = two_epochs(graphed[1])
    assert written_e == [] and written_g == [], "the step wrote the caller's batches %s" % written_g
    assert got == ref, (got, ref)
    assert_same_state(eager, graphed)
    assert graphed[1]._graph is not None and graphed[1].captures == 1


def test_one_batch_tensor_refilled_in_place(mk, Wm, batches):
    """The loader pattern that always worked: one device tensor, refilled in place, so every step sees the same pointer."""
    def two_epochs(step):
        x, y = torch.empty_like(batches[0][0], device="cuda"), torch.empty_like(batches[0][1], device="cuda")
        out = []
        for _ in range(2):
            for bx, by in batches:
                x.copy_(bx); y.copy_(by)
                out.append(result(step(x, y)))
        return out

    eager, graphed = twins(mk, Wm, "bf16", False)
    ref = two_epochs(eager[1])
    assert two_epochs(graphed[1]) == ref
    assert graphed[1].captures == 1
    assert_same_state(eager, graphed)


# ---- 2. frozen weights changed between replays ----------------------------------------------------------------------------------

def steps(step, batches, which):
    return [result(step(batches[i][0].cuda(), batches[i][1].cuda())) for i in which]


@pytest.mark.parametrize("eval_between", [False, True], ids=["straight", "eval_between"])
@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_frozen_cnn_reloaded_between_replays(mk, Wm, batches, precision, eval_between):
    """cnn.load_state_dict writes the frozen weights in place: the cache of repacked / bf16 copies notices through the version
    counters, a graph that recorded the old copies' addresses does not. straight: the old copies are still the cache's, with the
    old values. eval_between: an eval-mode forward has replaced them, and the recorded addresses are the allocator's again."""
    other = other_cnn_weights(Wm)
    x_eval = mk.synth_bags(999, 4)[0].cuda()

    def sequence(pair):
        ens, step = pair
        out = steps(step, batches, (0, 1, 2))
        ens.cnn.load_state_dict(other)
        if eval_between:
            out.append(eval_forward(ens, x_eval).tolist())
        return out + steps(step, batches, (3, 0))

    eager, graphed = twins(mk, Wm, precision, False)
    ref = sequence(eager)
    got = sequence(graphed)
    assert got == ref, (got, ref)
    assert graphed[1].captures == 2                                # steps 1-2 on the first graph, the last one on a second
    assert_same_state(eager, graphed)


def test_precision_switched_between_replays(mk, Wm, batches):
    """set_precision("f32") after a capture at "bf16": the frozen CNN of the next step runs the exact-f32 kernels on both twins."""
    def sequence(pair):
        ens, step = pair
        out = steps(step, batches, (0, 1, 2))
        ens.set_precision("f32")
        return out + steps(step, batches, (3, 0))

    eager, graphed = twins(mk, Wm, "bf16", False)
    ref = sequence(eager)
    got = sequence(graphed)
    assert got == ref, (got, ref)
    assert graphed[1].captures == 2
    assert_same_state(eager, graphed)


def test_resnet_frozen_trunk_reloaded_between_replays(Wm):
    """The ResNet branch (just_bottlenecks=False: the fc trains, the trunk is frozen): the step reads the trunk's repacked conv
    weights through resnet.new_cache()["w"]. 2 bags = 20 images, the smallest input of the ResNet step tests."""
    shapes = Wm.ensemble_shapes((2, 1), False, cnn_type="resnet", num_classes=10)
    conf = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=False, cnn_trainable=False,
                first_cnn_layer_trainable=False, in_channels=3)
    other = {k[len("cnn."):]: torch.as_tensor(v) for k, v in Wm.make_state_dict(22, shapes).items() if k.startswith("cnn.")}
    xs = [torch.from_numpy(Wm.uniform(10 + s, Wm.stream_id("rn_images"), 2 * 10 * 224 * 224, lo=0.0, hi=1.0).reshape(2, 10, 1, 224, 224))
          for s in range(5)]
    ys = [torch.tensor([(3 * i + s) % 10 for i in range(2)], dtype=torch.long) for s in range(5)]

    def build(graph, ordinals=None):
        torch.manual_seed(77)
        ens = M.Ensemble("repeat", conf, [2, 1], torch.device("cuda"), precision="bf16")
        ens.load_state_dict({k: torch.as_tensor(v) for k, v in Wm.make_state_dict(21, shapes).items()})
        ens.cuda()
        drops = [m for m in ens.mla.modules() if type(m).__name__ == "Dropout"]
        if ordinals is not None:
            for d, o in zip(drops, ordinals):
                d.ordinal = o
        return (ens, TR.TrainStep(ens, lr=1e-3, graph=graph)), [d.ordinal for d in drops]

    def sequence(pair):
        ens, step = pair
        out = [result(step(xs[s].cuda(), ys[s].cuda())) for s in range(3)]
        ens.cnn.load_state_dict(other)                             # trunk convs and BatchNorms, and the fc inside the flat buffer
        return out + [result(step(xs[s].cuda(), ys[s].cuda())) for s in (3, 4)]

    eager, ords = build(False)
    graphed, _ = build(True, ords)
    ref = sequence(eager)
    got = sequence(graphed)
    assert got == ref, (got, ref)
    assert graphed[1].captures == 2
    assert_same_state(eager, graphed)


# ---- 3. / 4. library scratch grown between replays ------------------------------------------------------------------------------

def shrink_scratch(*prefixes):
    """Scratch entries only ever grow, and they are the process's: forget the named ones, so that the next call sizes them at their
    floor again whatever ran before this test (a graph that still addressed one holds it itself)."""
    for k in [k for k in ops._ws if isinstance(k, str) and k.startswith(prefixes)]:
        del ops._ws[k]


def grow_ksplit():
    """The smallest problem on linear's K-split path that needs more than the 1 << 22 floats of the floor: 8 * 4104 * 128."""
    dev = torch.device("cuda")
    a, w, b = torch.ones((4104, 2048), device=dev), torch.ones((128, 2048), device=dev), torch.zeros(128, device=dev)
    assert float(ops.linear(a, w, b)[-1, -1]) == 2048.0


def grow_colsum():
    """A matrix with more than the 4096 columns of col_sum's floor."""
    x = torch.ones((8, 4104), device="cuda")
    assert float(ops.col_sum(x, torch.empty(4104, device="cuda"))[-1]) == 8.0


def entry(prefix):
    (key,) = [k for k in ops._ws if isinstance(k, str) and k.startswith(prefix)]
    return ops._ws[key]


def sentinel_like(old):
    """A tensor of the size of the scratch entry that has just been replaced: if the allocator hands out the old block, a replay
    that still writes there shows in it."""
    return torch.full((old["numel"] * old["itemsize"] // 4,), 12345.0, dtype=torch.float32, device="cuda")


def assert_sentinel(sentinel, old):
    if sentinel.data_ptr() == old["ptr"]:                          # elsewhere: the old block is not the allocator's to give, nothing to see
        assert bool((sentinel == 12345.0).all()), "a replay wrote into a block the allocator had handed out again"


def describe(t):
    return {"ptr": t.data_ptr(), "numel": t.numel(), "itemsize": t.element_size()}


@pytest.mark.parametrize("precision,finetune,grown", [("bf16", False, ("ksplit/",)), ("bf16", True, ("ksplit/", "colsum/"))],
                         ids=["frozen-ksplit", "finetune-ksplit-colsum"])
def test_scratch_grown_between_replays(mk, Wm, batches, precision, finetune, grown):
    """An eager call from outside the step (a validation forward on a larger batch, say) replaces a scratch entry whose address
    the graph recorded. The replay must not go through the old address unless the graph holds that tensor."""
    grow = {"ksplit/": grow_ksplit, "colsum/": grow_colsum}
    eager, graphed = twins(mk, Wm, precision, finetune)

    shrink_scratch(*grown)
    ref = steps(eager[1], batches, (0, 1, 2))
    for p in grown:
        grow[p]()
    ref += steps(eager[1], batches, (3, 0))

    shrink_scratch(*grown)
    step = graphed[1]
    got = steps(step, batches, (0, 1, 2))
    assert step.captures == 1
    old = {p: describe(entry(p)) for p in grown}
    for p in grown:
        grow[p]()
        assert entry(p).numel() > old[p]["numel"] and entry(p).data_ptr() != old[p]["ptr"]
    held = {t.data_ptr() for t in step._graph["held"]}
    assert all(old[p]["ptr"] in held for p in grown), "the live graph does not hold the scratch it addresses"
    sentinels = {p: sentinel_like(old[p]) for p in grown}
    for i in (3, 0):
        got.append(result(step(batches[i][0].cuda(), batches[i][1].cuda())))
        g = step._graph                                            # None: this step ran eagerly, nothing was replayed
        if g is not None:
            held = {t.data_ptr() for t in g["held"]}
            assert step.captures > 1 or all(old[p]["ptr"] in held for p in grown)
    assert got == ref, (got, ref)
    for p in grown:
        assert_sentinel(sentinels[p], old[p])
    assert_same_state(eager, graphed)


@pytest.fixture(scope="module")
def wave_model(mk, Wm):
    ens = M.Ensemble("repeat", dict(mk.CNN_CONF), [2, 1], torch.device("cuda"), precision="bf16")
    sd = {k: torch.as_tensor(v) for k, v in Wm.make_state_dict(6, Wm.ensemble_shapes((2, 1), False)).items()}
    ens.load_state_dict(sd)
    pcm = torch.from_numpy(Wm.waveform(31, 160000, 3)).cuda()
    return ens.cuda().eval(), sd, pcm


def test_graphed_waveforms_refuses_a_changed_model(Wm, wave_model):
    """The captured forward has a static output and cannot re-capture behind the caller's back: after load_state_dict, set_precision
    or a train() switch the next call must raise and say what changed. Scores of the old weights are the failure."""
    ens, sd, pcm = wave_model
    other = {k: torch.as_tensor(v) for k, v in Wm.make_state_dict(8, Wm.ensemble_shapes((2, 1), False)).items()}
    with torch.no_grad():
        g = ens.capture_waveforms(pcm)
        assert torch.equal(g(pcm), ens.forward_waveforms(pcm))
        ens.load_state_dict(other)
        with pytest.raises(RuntimeError, match="weights"):
            g(pcm)
        g = ens.capture_waveforms(pcm)                             # capturing again is the way on
        assert torch.equal(g(pcm), ens.forward_waveforms(pcm))
        ens.load_state_dict(sd)
        with pytest.raises(RuntimeError, match="weights"):
            g(pcm)

        g = ens.capture_waveforms(pcm)
        ens.set_precision("f32")
        with pytest.raises(RuntimeError, match="precision"):
            g(pcm)
        ens.set_precision("bf16")
        assert torch.equal(g(pcm), ens.forward_waveforms(pcm))      # switched back: the graph is the model's forward again

        ens.train()
        with pytest.raises(RuntimeError, match="mode"):
            g(pcm)
        ens.eval()
        assert torch.equal(g(pcm), ens.forward_waveforms(pcm))


def test_graphed_waveforms_keeps_its_scratch(Wm, wave_model):
    """The same K-split growth under a captured forward: it cannot re-capture, so it must own the block it recorded."""
    ens, _, pcm = wave_model
    ens.eval().set_precision("bf16")
    with torch.no_grad():
        shrink_scratch("ksplit/")
        g = ens.capture_waveforms(pcm)
        old = describe(entry("ksplit/"))
        grow_ksplit()
        assert entry("ksplit/").numel() > old["numel"] and entry("ksplit/").data_ptr() != old["ptr"]
        sentinel = sentinel_like(old)
        for seed in (31, 32):
            x = pcm if seed == 31 else torch.from_numpy(Wm.waveform(seed, 160000, 3)).cuda()
            assert g.captures == 1 and old["ptr"] in {t.data_ptr() for t in g.held}
            assert torch.equal(g(x), ens.forward_waveforms(x))
        assert_sentinel(sentinel, old)
