"""SHA-256 of every output of the VGGish finetune-backward kernels (f32 and bf16) and of two finetune steps, for bit comparison of two builds:
    python scripts/vggish_train_bits.py a.txt;  MLA_HIP_LIB=/path/to/other/libmla_hip.so python scripts/vggish_train_bits.py b.txt;  diff a.txt b.txt
Fixed seeds, one process per library. The kernels' reductions run in a fixed order, so the two lists must be equal."""
import hashlib, importlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
PKG = "audio-classification-using-a-deep-cnn-combined-with-multi-level-attention_amd"
ops, M, W, TR = (importlib.import_module(PKG + "." + m) for m in ("ops", "model", "weights", "train"))
from test_cnn_train_f32_gpu import WGRAD_CASES as WGRAD_F32        # noqa: E402
from test_finetune_bf16_gpu import SHAPES                            # noqa: E402
# the bf16 tests' cases (3 and 5 images: fewer than the one-split-per-CU count), and 9 images of 512 -> 512 (32 tiles: 8 splits on 256 CUs)
WGRAD_BF16 = [(s, 3) for s in SHAPES] + [((256, 256, 24, 16), 5), ((512, 512, 12, 8), 9)]
import make_golden as mk                                            # noqa: E402

out = open(sys.argv[1], "w")
DT = (torch.float32, torch.bfloat16)


def emit(name, t):
    h = hashlib.sha256(t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
    out.write("%s %s %s\n" % (name, tuple(t.shape), h))


def rnd(g, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=g).to(dtype).cuda()


for dt in DT:
    for n, H, Wd, C in ((3, 12, 8, 512), (3, 48, 32, 128)):
        g = torch.Generator().manual_seed(H * 1000 + C)
        a = rnd(g, n, H, Wd, C, dtype=dt).clamp_min(0)
        a[0, :2, :2, :] = 0.5                                          # a window of ties
        tag = " %s %s" % ((n, H, Wd, C), dt)
        emit("maxpool" + tag, ops.maxpool2x2(a))
        for pool in (0, 1):
            d = rnd(g, n, H >> pool, Wd >> pool, C, dtype=dt)
            db = torch.zeros(C, device="cuda")
            emit("relu_pool_bwd pool%d%s" % (pool, tag), ops.relu_pool_bwd(a, d, pool=bool(pool)))
            emit("relu_pool_bwd pool%d +db dz%s" % (pool, tag), ops.relu_pool_bwd(a, d, pool=bool(pool), db=db))
            emit("relu_pool_bwd pool%d +db db%s" % (pool, tag), db)
    cases = WGRAD_F32 if dt == torch.float32 else WGRAD_BF16
    for (cin, cout, H, Wd), n in cases:
        g = torch.Generator().manual_seed(cin + cout + n)
        dz, a = rnd(g, n, H, Wd, cout, dtype=dt), rnd(g, n, H, Wd, cin, dtype=dt)
        dw = torch.zeros(cout, cin, 3, 3, device="cuda")
        ops.conv_wgrad(dz, a, dw)
        emit("wgrad %d->%d n%d %s" % (cin, cout, n, dt), dw)
    for n in ((3, 172) if dt == torch.float32 else (3, 130)):
        g = torch.Generator().manual_seed(17 + n)
        x, w, b, d = rnd(g, n, 96, 64) * 2 + 1, rnd(g, 64, 1, 3, 3) * 0.3, rnd(g, 64) * 0.1, rnd(g, n, 48, 32, 64, dtype=dt)
        dw, db = torch.zeros(64, 1, 3, 3, device="cuda"), torch.zeros(64, device="cuda")
        ops.conv1_bwd(x, w, b, d, dw, db)
        emit("conv1_bwd dw n%d %s" % (n, dt), dw)
        emit("conv1_bwd db n%d %s" % (n, dt), db)
    for cin, cout in ((64, 128), (512, 512)):
        emit("repack_dgrad %d->%d %s" % (cin, cout, dt), ops.repack_dgrad(rnd(torch.Generator().manual_seed(cin), cout, cin, 3, 3), dt))
    x = rnd(torch.Generator().manual_seed(5), 1000, 200, dtype=dt)[:, 40:170]       # strided rows: (1000, 130) of (1000, 200)
    cs = torch.zeros(130, device="cuda")
    emit("transpose_padded %s" % dt, ops.transpose_padded(x))
    emit("col_sum %s" % dt, ops.col_sum(x, cs))

g = torch.Generator().manual_seed(23)                                # the last Linear: f32 output and gradient, bf16 dZ
h, d, db = rnd(g, 5, 128).clamp_min(0), rnd(g, 5, 128), torch.zeros(128, device="cuda")
emit("relu_bwd linear f32->bf16 dz", ops.relu_pool_bwd(h, d, pool=False, db=db, bf16=True))
emit("relu_bwd linear f32->bf16 db", db)
for cin, cout, H, Wd in ((64, 128, 48, 32), (256, 256, 24, 16), (512, 512, 12, 8)):      # window codes of the bf16 training forward
    g = torch.Generator().manual_seed(11 + cin)
    x = (torch.rand((6, H, Wd, cin), generator=g) * 2 - 0.6).clamp_min(0).to(torch.bfloat16).cuda()
    w = ((torch.rand((cout, cin, 3, 3), generator=g) - 0.5) * (2.0 / (9 * cin) ** 0.5)).cuda()
    b = ((torch.rand(cout, generator=g) - 0.5) * 0.1).cuda()
    d = (torch.rand((6, H // 2, Wd // 2, cout), generator=g) - 0.5).to(torch.bfloat16).cuda()
    codes, _ = ops.conv3x3_train_codes(x, ops.repack_conv_weight(w, torch.bfloat16), b, cout)
    db = torch.zeros(cout, device="cuda")
    emit("pool_bwd_codes dz %d->%d" % (cin, cout), ops.pool_bwd_codes(codes, d, db=db))
    emit("pool_bwd_codes db %d->%d" % (cin, cout), db)

for prec in ("f32", "bf16"):                                          # two finetune steps at the golden size
    ens = M.Ensemble("repeat", dict(mk.CNN_CONF), [2, 1], torch.device("cuda"), precision=prec)
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in W.make_state_dict(7, W.ensemble_shapes((2, 1), False)).items()})
    M.set_requires_grad(ens.cuda(), True)
    step = TR.TrainStep(ens, lr=1e-3)
    for s in range(2):
        x, y = mk.synth_bags(100 + s, 4)
        masks = mk.make_masks(200 + s, [2, 1], 4)
        for lvl, em in enumerate(ens.mla.embedded_mappings):
            for j, d in enumerate(em.dropouts):
                d.mask = masks["mla.embedded_mappings.%d.dropouts.%d" % (lvl, j)]
        loss, _ = step(x.cuda(), y.cuda())
        emit("finetune %s step %d loss" % (prec, s), loss)
    for k, v in ens.state_dict().items():
        emit("finetune %s %s" % (prec, k), v)
out.close()
print("wrote", sys.argv[1])
