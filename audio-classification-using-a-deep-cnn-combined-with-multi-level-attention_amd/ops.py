"""Tensor-level wrappers over the C ABI (include/mla_hip.h). PyTorch supplies device
buffers and the current stream; every number is produced by a HIP kernel of libmla_hip.so.
Nothing here falls back to torch ops."""

import ctypes
import os

import torch

from . import _lib

DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.int16: _lib.I16}
BN_EPS = 1e-5

# Optional per-kernel timing (bench.py): when `profile` is a list, every wrapped call appends
# (name, start_event, end_event) recorded on the current stream -- the stream the kernels run on.
profile = None
_ws = {}                  # per-device scratch buffers (statistics partials, column sums, split-K partials)


_event_pool = []


def reserve_events(n):
    """Create (and record once, which is what allocates them) n timing events ahead of a timed region: creating events inside
    it can stall the launching thread for tens of milliseconds when the runtime has to grow its event pool (measured: one
    60 ms stall in a 10-step region)."""
    while len(_event_pool) < n:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        _event_pool.append(e)
    torch.cuda.synchronize()


def _event():
    return _event_pool.pop() if _event_pool else torch.cuda.Event(enable_timing=True)


def _timed(name, fn, *args):
    if profile is None:
        return fn(*args)
    e0, e1 = _event(), _event()
    e0.record()
    rc = fn(*args)
    e1.record()
    profile.append((name, e0, e1))
    return rc


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _chk(t, dtype=None):
    assert t.is_cuda and t.is_contiguous(), "HIP ops need contiguous CUDA tensors"
    if dtype is not None:
        assert t.dtype == dtype, (t.dtype, dtype)
    return t


def _chk_rows(t, dtype=None):
    """A 2-D operand of an entry point that takes a row pitch: whatever _chk accepts, and rows that are strided (a column slice
    of a wider tensor)."""
    assert t.is_cuda and t.dim() == 2 and (t.is_contiguous() or (t.stride(1) == 1 and t.stride(0) >= t.shape[1])), \
        "HIP ops need CUDA matrices with contiguous rows"
    if dtype is not None:
        assert t.dtype == dtype, (t.dtype, dtype)
    return t


def repack_conv_weight(w, dtype):
    """(Cout, Cin, 3, 3) f32 -> (Cout, 9, Cin) in `dtype`."""
    _chk(w, torch.float32)
    cout, cin = w.shape[0], w.shape[1]
    out = torch.empty((cout, 9, cin), dtype=dtype, device=w.device)
    _lib.check(_lib.lib().mla_conv_repack_weights(_p(w), cout, cin, _p(out), DT[dtype], _lib.stream_ptr()))
    return out


def split_conv_weight(w):
    """(Cout, Cin, 3, 3) f32 -> (Cout, 9, 3 Cin) bf16 = [hi | lo | hi] per 64-channel chunk and tap (bf16x3 mode)."""
    packed = repack_conv_weight(w, torch.float32)
    cout, _, cin = packed.shape
    out = torch.empty((cout, 9, 3 * cin), dtype=torch.bfloat16, device=w.device)
    _lib.check(_lib.lib().mla_split_bf16x3(_p(packed), cout * 9, cin, cin, _p(out), 3 * cin, 64, 3, _lib.stream_ptr()))
    return out


def split_linear_weight(w, seg):
    """(N, K) f32 -> (N, 3 K) bf16 = [hi | lo | hi] per segment of `seg` input features (bf16x3 mode)."""
    _chk(w, torch.float32)
    n, k = w.shape
    out = torch.empty((n, 3 * k), dtype=torch.bfloat16, device=w.device)
    _lib.check(_lib.lib().mla_split_bf16x3(_p(w), n, k, k, _p(out), 3 * k, seg, 3, _lib.stream_ptr()))
    return out


def merge_split(x, seg):
    """(rows, 2 cols) bf16 [hi | lo] per segment -> (rows, cols) f32."""
    _chk(x, torch.bfloat16)
    rows, c2 = x.shape
    out = torch.empty((rows, c2 // 2), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().mla_merge_bf16x3(_p(x), rows, c2 // 2, c2, seg, _p(out), _lib.stream_ptr()))
    return out


def linear_split(a, w, b, seg, relu=True, out_split=True):
    """bf16x3 Linear: a (M, 2K) split activations, w (N, 3K) from split_linear_weight -> (M, 2N) split or (M, N) f32."""
    _chk(a, torch.bfloat16); _chk(w, torch.bfloat16)
    M, K = a.shape[0], a.shape[1] // 2
    N = w.shape[0]
    assert w.shape[1] == 3 * K
    out = torch.empty((M, 2 * N), dtype=torch.bfloat16, device=a.device) if out_split else torch.empty((M, N), dtype=torch.float32, device=a.device)
    _lib.check(_timed("linear_%dx%d" % (K, N), _lib.lib().mla_linear_bf16x3, _p(a), a.stride(0), _p(w), w.stride(0), _p(b), _p(out),
                      out.stride(0), M, N, K, seg, _lib.BF16X3 if out_split else _lib.F32, int(relu), _lib.stream_ptr()))
    return out


def to_bf16(w):
    _chk(w, torch.float32)
    out = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
    _lib.check(_lib.lib().mla_convert_f32(_p(w), _p(out), w.numel(), _lib.BF16, _lib.stream_ptr()))
    return out


def to_f32(x):
    _chk(x, torch.bfloat16)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().mla_convert_bf16_to_f32(_p(x), _p(out), x.numel(), _lib.stream_ptr()))
    return out


def conv1(x, w, b, dtype, split=False):
    """x (N, 96, 64) f32|bf16 -> (N, 48, 32, 64) NHWC; split (bf16x3): f32 in -> (N, 48, 32, 128) = [hi(64) | lo(64)]."""
    _chk(x); _chk(w, torch.float32); _chk(b, torch.float32)
    n = x.shape[0]
    assert tuple(x.shape[1:]) == (96, 64) and tuple(w.shape) == (64, 1, 3, 3)
    out = torch.empty((n, 48, 32, 128 if split else 64), dtype=dtype, device=x.device)
    _lib.check(_timed("conv1", _lib.lib().mla_vggish_conv1, _p(x), DT[x.dtype], n, _p(w), _p(b), _p(out),
                      _lib.BF16X3 if split else DT[dtype], _lib.stream_ptr()))
    return out


# MLA_FUSED_FRONT=0 (read once, here): Ensemble.forward_waveforms in bf16 runs the front-end and conv1 as two kernels again
# (A/B and bisecting). Tests flip the module variable.
FUSED_FRONT = os.environ.get("MLA_FUSED_FRONT", "1") != "0"


def logmel_conv1(pcm, w, b):
    """(W, n) device PCM (float32 or int16) -> (W * N, 48, 32, 64) NHWC bf16 = conv1(waveforms_to_examples(pcm, bf16)), bit for
    bit, in one kernel. Timed under the front-end's name ("logmel"); there is no "conv1" entry on this path."""
    from . import frontend
    assert pcm.dim() == 2 and pcm.is_cuda and pcm.stride(1) == 1 and pcm.dtype in (torch.float32, torch.int16)
    _chk(w, torch.float32); _chk(b, torch.float32)
    assert tuple(w.shape) == (64, 1, 3, 3)
    n_wave, n_samples = pcm.shape
    _, n_ex = frontend.counts(n_samples)
    out = torch.empty((n_wave * n_ex, 48, 32, 64), dtype=torch.bfloat16, device=pcm.device)
    if n_wave * n_ex == 0:
        return out
    tab = frontend.device_tables(pcm.device)
    _lib.check(_timed("logmel", _lib.lib().mla_logmel_conv1, _p(pcm), DT[pcm.dtype], n_wave, n_samples,
                      pcm.stride(0) if n_wave > 1 else n_samples, _p(tab), _p(w), _p(b), _p(out), _lib.stream_ptr()))
    return out


CONV_SHAPES = {2: ((48, 32, 64), (24, 16, 128)), 3: ((24, 16, 128), (24, 16, 256)), 4: ((24, 16, 256), (12, 8, 256)),
               5: ((12, 8, 256), (12, 8, 512)), 6: ((12, 8, 512), (6, 4, 512))}


def conv(layer, x, w_packed, b, split=False):
    """VGGish conv `layer` (2..6) with fused bias + ReLU (+ 2x2 max-pool for 2, 4, 6). NHWC. split (bf16x3): activations
    carry [hi | lo] planes (2 C channels), weights [hi | lo | hi] (3 Cin per tap)."""
    _chk(x); _chk(w_packed, x.dtype); _chk(b, torch.float32)
    shp_in, shp_out = CONV_SHAPES[layer]
    ka, kw, ko = (2, 3, 2) if split else (1, 1, 1)
    assert tuple(x.shape[1:]) == shp_in[:2] + (ka * shp_in[2],), (x.shape, shp_in)
    assert tuple(w_packed.shape) == (shp_out[2], 9, kw * shp_in[2])
    n = x.shape[0]
    out = torch.empty((n,) + shp_out[:2] + (ko * shp_out[2],), dtype=x.dtype, device=x.device)
    _lib.check(_timed("conv%d" % layer, _lib.lib().mla_vggish_conv, layer, _p(x), _p(w_packed), _p(b), _p(out), n,
                      _lib.BF16X3 if split else DT[x.dtype], _lib.stream_ptr()))
    return out


KSPLIT = 8          # fixed K ranges of the narrow forward layers (see linear)


def linear(a, w, b, relu=False, out_dtype=None, out=None, split_k=False):
    """a (M, K), w (N, K) same dtype (f32 | bf16), bias f32 -> (M, N) (optionally into `out`). split_k: allow K to be split
    over workgroups when there are few output tiles (weight gradients). Forward layers never split: the number of splits
    would depend on the batch size, and a bag's scores must not depend on which batch it is computed in."""
    _chk(a); _chk(w, a.dtype)
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K
    out_dtype = out_dtype or a.dtype
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=a.device)
    else:
        assert out.is_contiguous() and out.numel() == M * N and out.dtype == out_dtype
    # narrow outputs (the attention modules' 600 -> 10 fcv): a dedicated one-pass kernel instead of a nearly empty MFMA tile
    if (N <= 16 and a.dtype == torch.float32 and out_dtype == torch.float32 and not relu and not split_k and K % 4 == 0
            and K * N * 4 <= 65536 and a.stride(0) % 4 == 0 and w.stride(0) % 4 == 0
            and a.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0):
        _lib.check(_timed("linear_%dx%d" % (K, N), _lib.lib().mla_linear_narrow, _p(a), a.stride(0), _p(w), w.stride(0), _p(b), _p(out), N,
                          M, N, K, _lib.stream_ptr()))
        return out
    # narrow forward layers with a long reduction (VGGish's Linear(4096, 128): one column tile, so M / 128 workgroups for 256 CUs):
    # K always runs as KSPLIT fixed ranges whose partial sums are added in range order -- a per-LAYER constant, so a row's result
    # is the same in every batch (a split chosen by batch size would change the summation order)
    kc = 64 if a.dtype == torch.bfloat16 else 32
    if N <= 128 and K >= 2048 and K % (kc * KSPLIT) == 0 and not split_k and a.stride(0) % 8 == 0 and w.stride(0) % 8 == 0:
        key = "ksplit/" + str(a.device)
        if key not in _ws or _ws[key].numel() < KSPLIT * M * N:
            _ws[key] = torch.empty(max(KSPLIT * M * N, 1 << 22), dtype=torch.float32, device=a.device)
        ws = _ws[key]
        _lib.check(_timed("linear_%dx%d" % (K, N), _lib.lib().mla_linear_ksplit, _p(a), a.stride(0), _p(w), w.stride(0), _p(b), _p(out), N,
                          M, N, K, DT[a.dtype], DT[out_dtype], int(relu), KSPLIT, _p(ws), ws.numel(), _lib.stream_ptr()))
        return out
    # few output tiles but a long reduction (weight gradients): split K over workgroups
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    if split_k and a.dtype == torch.float32 and out_dtype == torch.float32 and tiles <= 64 and K >= 2048:
        splits = int(min(64, max(2, 256 // tiles), K // 512))
        key = "splitk/" + str(a.device)
        if key not in _ws or _ws[key].numel() < splits * M * N:
            _ws[key] = torch.empty(max(splits * M * N, 1 << 22), dtype=torch.float32, device=a.device)
        ws = _ws[key]
        _lib.check(_timed("linear_splitk_%dx%d" % (K, N), _lib.lib().mla_linear_splitk, _p(a), a.stride(0), _p(w), w.stride(0), _p(b),
                          _p(out), N, M, N, K, int(relu), splits, _p(ws), ws.numel(), _lib.stream_ptr()))
        return out
    _lib.check(_timed("linear_%dx%d" % (K, N), _lib.lib().mla_linear, _p(a), a.stride(0), _p(w), w.stride(0), _p(b), _p(out), N,
                      M, N, K, DT[a.dtype], DT[out_dtype], int(relu), _lib.stream_ptr()))
    return out


def linear_small(a, w, b):
    _chk(a, torch.float32); _chk(w, torch.float32)
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().mla_linear_small(_p(a), a.stride(0), _p(w), w.stride(0), _p(b), _p(out), N, M, N, K, _lib.stream_ptr()))
    return out


def _workspace(device):
    key = str(device)
    if key not in _ws:
        _ws[key] = torch.empty(int(_lib.lib().mla_bn_stats_workspace_bytes()) // 8, dtype=torch.float64, device=device)
    return _ws[key]


def bn_stats(x, mode, period, running_mean=None, running_var=None, momentum=-1.0):
    """Batch mean / biased variance per channel (mode 0: channel = row % period; 1: column);
    optionally updates running statistics in place (unbiased variance, torch semantics)."""
    _chk(x, torch.float32)
    rows, cols = x.shape
    ch = period if mode == 0 else cols
    mean = torch.empty(ch, dtype=torch.float32, device=x.device)
    var = torch.empty(ch, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().mla_bn_stats(_p(x), rows, cols, x.stride(0), mode, period, _p(_workspace(x.device)), _p(mean),
                                       _p(var), _p(running_mean), _p(running_var), float(momentum), _lib.stream_ptr()))
    return mean, var


def bn_apply(x, mode, period, mean, var, gamma, beta, act=0, keep_mask=None, drop_scale=1.0, out=None):
    _chk_rows(x, torch.float32)
    rows, cols = x.shape
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
    if keep_mask is not None:
        _chk(keep_mask, torch.uint8)
        assert keep_mask.numel() == rows * cols
    _lib.check(_lib.lib().mla_bn_apply(_p(x), x.stride(0), _p(out), out.stride(0), rows, cols, mode, period, _p(mean), _p(var),
                                       _p(gamma), _p(beta), BN_EPS, act, _p(keep_mask), float(drop_scale), _lib.stream_ptr()))
    return out


def attention_pool(z, bags, T, K, nv, nf, y, save=False):
    """z (bags*T, K); nv / nf = (mean, var, gamma, beta) of normv / normf; writes y (a (bags, K)
    column slice of the concatenated level outputs). Returns (att, cla) when save=True."""
    _chk(z, torch.float32)
    assert y.dtype == torch.float32 and y.stride(1) == 1
    att = torch.empty_like(z) if save else None
    cla = torch.empty_like(z) if save else None
    _lib.check(_lib.lib().mla_attention_pool(_p(z), bags, T, K, _p(nv[0]), _p(nv[1]), _p(nv[2]), _p(nv[3]), _p(nf[0]), _p(nf[1]),
                                             _p(nf[2]), _p(nf[3]), BN_EPS, _p(y), y.stride(0), _p(att), _p(cla), _lib.stream_ptr()))
    return att, cla


# ----------------------------------------------------------------- training-step kernels ----

def gather_bags(emb, first_rows, T):
    """(N, M) float32 embeddings (rows may be strided) and the first row of each of W windows -> the (W * T, M) head input
    out[w * T + t] = emb[first_rows[w] + t] in one launch (mla_gather_bags). Windows may overlap: a timeline's CNN runs once per
    distinct slot and its bags are gathered here. first_rows: host integers (a device tensor is read back first); they travel in
    one pinned buffer and one copy. A window that leaves emb raises before anything is launched."""
    import numpy as np
    _chk_rows(emb, torch.float32)
    if isinstance(first_rows, torch.Tensor):
        first_rows = first_rows.detach().cpu().numpy()
    fr = np.ascontiguousarray(np.asarray(first_rows), dtype=np.int64).reshape(-1)
    W, (N, M) = fr.shape[0], emb.shape
    out = torch.empty((W * int(T), M), dtype=torch.float32, device=emb.device)
    if W == 0:
        return out
    host = torch.empty(W, dtype=torch.int64, pin_memory=True)
    host.numpy()[:] = fr
    d = host.to(emb.device, non_blocking=True)
    _lib.check(_timed("gather_bags", _lib.lib().mla_gather_bags, _p(emb), N, emb.stride(0) if N > 1 else M, _p(d),
                      fr.ctypes.data_as(ctypes.c_void_p), W, int(T), M, _p(out), _lib.stream_ptr()))
    return out


class Dist:
    """Data-parallel context of the training step: SyncBN statistics, gradient buffer, loss and hit count are summed over
    the ranks of a ``torch.distributed`` process group.

    backend "nccl" (production: RCCL over xGMI): the sums run through the C ABI, ``mla_allreduce_flat`` on a communicator
    this object creates with ``mla_comm_init_rank`` (the 128-byte id travels from rank 0 through torch.distributed). The
    library binds the RCCL PyTorch has already loaded; MLA_DIST_COLLECTIVE=torch selects ``torch.distributed.all_reduce``
    on the same device buffers instead. backend "gloo" (CPU rehearsals, two ranks sharing one test GPU): host copy.
    world == 1: every all-reduce is a no-op unless ``always`` (or MLA_DIST_ALWAYS=1) asks for the collectives anyway --
    a one-rank sum leaves the data unchanged, so the production branch can be exercised on a one-GPU box."""

    def __init__(self, group=None, always=None, sync_bn=True):
        """sync_bn: train-mode BatchNorm statistics are summed over the ranks (the step then equals the reference's single-process
        step on the GLOBAL batch, train.py:119-142). False = per-shard statistics, the usual DistributedDataParallel semantics
        (SURVEY.md section 8e allows either): no statistics all-reduce, the result equals the reference run per shard with
        gradients averaged. trace: set to a list to record (tag, bytes, start event, end event) of every collective (bench.py)."""
        import os
        import torch.distributed as dist
        self.group, self.comm = group, None
        self.sync_bn, self.trace = sync_bn, None
        inited = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if inited else 1
        self.rank = dist.get_rank(group) if inited else 0
        self.backend = dist.get_backend(group) if inited else None
        always = (os.environ.get("MLA_DIST_ALWAYS") == "1") if always is None else always
        self.active = inited and (self.world > 1 or always)
        self.via = None
        self.fallback = None
        if self.active and self.backend == "nccl":
            self.via = os.environ.get("MLA_DIST_COLLECTIVE", "abi")
            if self.via == "abi":
                # every rank tries; the ranks then agree (one MIN all-reduce through torch.distributed) on whether ALL of them have a
                # communicator. If one could not make it (an RCCL without the entry points the library binds, a failed init), all of
                # them switch to torch.distributed.all_reduce on the same device buffers and say so (describe()["fallback"]): a
                # data-parallel run never ends up with ranks on different transports.
                err = None
                try:
                    self._init_comm(dist)
                except Exception as e:                      # noqa: BLE001 -- reported through describe(), the run continues on torch's transport
                    err = "%s: %s" % (type(e).__name__, e)
                ok = torch.tensor([0 if err else 1], dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))
                dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=self.group)
                if int(ok.item()) == 0:
                    self.close()
                    self.via = "torch"
                    self.fallback = err or "another rank could not create its communicator through the C ABI"
        elif self.active:
            self.via = "host"

    def _init_comm(self, dist):
        dev = torch.device("cuda", torch.cuda.current_device())
        uid, err0 = torch.zeros(128, dtype=torch.uint8), None
        if self.rank == 0:
            buf = (ctypes.c_char * 128)()
            try:
                _lib.check(_lib.lib().mla_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)))
                uid = torch.frombuffer(bytearray(buf.raw), dtype=torch.uint8).clone()
            except Exception as e:                          # noqa: BLE001 -- the other ranks are waiting in the broadcast below: send them zeros
                err0 = e
        uid = uid.to(dev)
        src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
        dist.broadcast(uid, src=src, group=self.group)
        raw = bytes(uid.cpu().numpy().tobytes())
        if err0 is not None or not any(raw):
            raise err0 or RuntimeError("rank 0 could not obtain an RCCL unique id through the C ABI")
        comm = ctypes.c_void_p()
        _lib.check(_lib.lib().mla_comm_init_rank(ctypes.byref(comm), self.world, ctypes.c_char_p(raw), self.rank))
        self.comm = comm
        # destroyed by close() or at interpreter exit while torch and RCCL are still loaded -- never from __del__, which may
        # run during teardown after either is gone
        import atexit
        import weakref
        ref = weakref.ref(self)
        atexit.register(lambda: ref() is not None and ref().close())

    def close(self):
        if self.comm is not None:
            torch.cuda.synchronize()
            _lib.check(_lib.lib().mla_comm_destroy(self.comm))
            self.comm = None


    def _reduce(self, t):
        """The collective itself, whatever the world size."""
        import torch.distributed as dist
        if self.via == "abi":
            assert t.is_cuda and t.is_contiguous()
            code = {torch.float32: _lib.F32, torch.float64: _lib.F64, torch.int32: _lib.I32}[t.dtype]
            _lib.check(_lib.lib().mla_allreduce_flat(_p(t), t.numel(), code, self.comm, _lib.stream_ptr()))
        elif self.via == "torch":
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        elif t.is_cuda:                                   # gloo: through the host
            host = t.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=self.group)
            t.copy_(host)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    def all_reduce_sum(self, t, tag="other"):
        """In-place sum over the group (see the class docstring for the transport)."""
        if not self.active:
            return t
        if self.trace is None:
            return self._reduce(t)
        e0, e1 = _event(), _event()
        e0.record()
        self._reduce(t)
        e1.record()
        self.trace.append((tag, t.numel() * t.element_size(), e0, e1))
        return t

    @property
    def bn_active(self):
        return self.active and self.sync_bn

    @property
    def bn_world(self):
        """Number of shards whose rows enter one BatchNorm statistic."""
        return self.world if self.bn_active else 1

    def ranks_reported(self):
        """The rank count as the TRANSPORT reports it (ncclCommCount of this object's communicator, or the process group's size):
        evidence that the collectives really span the ranks the launcher started."""
        if self.comm is not None:
            n = ctypes.c_int(-1)
            _lib.check(_lib.lib().mla_comm_count(self.comm, ctypes.byref(n)))
            return int(n.value)
        import torch.distributed as dist
        return dist.get_world_size(self.group) if self.active else 1

    def describe(self):
        origin = _lib.lib().mla_comm_library_origin().decode() if self.via == "abi" else None
        return {"active": bool(self.active), "backend": self.backend, "transport": {"abi": "mla_allreduce_flat (C ABI -> ncclAllReduce)",
                "torch": "torch.distributed.all_reduce", "host": "torch.distributed.all_reduce through host copies (gloo rehearsal)",
                None: None}[self.via], "rccl_library_origin": origin, "ranks": self.ranks_reported(), "sync_bn": bool(self.sync_bn),
                "fallback": getattr(self, "fallback", None)}


LOCAL = None          # set lazily (torch.distributed may not be initialised at import time)


def _local():
    global LOCAL
    if LOCAL is None:
        LOCAL = Dist.__new__(Dist)
        LOCAL.group, LOCAL.world, LOCAL.rank, LOCAL.active, LOCAL.comm, LOCAL.via = None, 1, 0, False, None, None
        LOCAL.sync_bn, LOCAL.trace, LOCAL.backend, LOCAL.fallback = True, None, None, None
    return LOCAL


def dropout_mask(n, seed, stream_id, offset, p_drop, device):
    """uint8 keep-mask from the counter-based generator of the library (mla_dropout_mask; numpy restatement: weights.keep_mask)."""
    out = torch.empty(n, dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().mla_dropout_mask(_p(out), n, int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 64 - 1), int(offset), float(p_drop),
                                           _lib.stream_ptr()))
    return out


def bn_stats_sync(x, mode, period, dist, running_mean=None, running_var=None, momentum=-1.0, also=(), tracked=None):
    """bn_stats with the (sum, sum of squares) all-reduced over the data-parallel group. `also`: further (running_mean,
    running_var, momentum) triples to update from the SAME statistics (two BatchNorms fed by one tensor, model.py:239-240:
    one pass over x and one all-reduce instead of two). tracked: the BatchNorm's num_batches_tracked (int64 device scalar), advanced
    by the finishing kernel; `also` entries are (running_mean, running_var, momentum, tracked)."""
    _chk(x, torch.float32)
    rows, cols = x.shape
    ch = period if mode == 0 else cols
    sums = torch.empty(2 * ch, dtype=torch.float64, device=x.device)
    L = _lib.lib()
    mean = torch.empty(ch, dtype=torch.float32, device=x.device)
    var = torch.empty(ch, dtype=torch.float32, device=x.device)
    count = (rows // period * cols if mode == 0 else rows) * dist.bn_world
    if dist.bn_active:
        _lib.check(L.mla_bn_stats_sums(_p(x), rows, cols, x.stride(0), mode, period, _p(_workspace(x.device)), _p(sums), _lib.stream_ptr()))
        dist.all_reduce_sum(sums, "syncbn_fwd")
        _lib.check(L.mla_bn_stats_finish(_p(sums), ch, float(count), _p(mean), _p(var), _p(running_mean), _p(running_var),
                                         float(momentum), _p(tracked), _lib.stream_ptr()))
    else:               # nothing to exchange between the two stages: one launch fewer (same bits)
        _lib.check(L.mla_bn_stats_fused(_p(x), rows, cols, x.stride(0), mode, period, _p(_workspace(x.device)), _p(sums), _p(mean), _p(var),
                                        _p(running_mean), _p(running_var), float(momentum), _p(tracked), _lib.stream_ptr()))
    for rm, rv, mom, trk in also:
        scratch_m, scratch_v = torch.empty_like(mean), torch.empty_like(var)
        _lib.check(L.mla_bn_stats_finish(_p(sums), ch, float(count), _p(scratch_m), _p(scratch_v), _p(rm), _p(rv), float(mom), _p(trk),
                                         _lib.stream_ptr()))
    return mean, var


def bn_backward(x, dy, yout, act, drop_scale, mode, period, mean, var, gamma, dist, dgamma, dbeta, want_dx=True,
                dx=None, accumulate=False, batch_stats=True, count=None):
    """BatchNorm backward through the fused activation/dropout. Writes dgamma/dbeta (local parts) and returns dx (global-batch
    exact under data parallelism). batch_stats=False: the forward normalised with FIXED statistics (eval mode: mean / var are the
    running buffers), so dx = gamma * rstd * g without the two batch-mean terms -- the same kernels with zero sums for dx.
    x, dy, yout: rows may be strided (the kernels take a pitch; 16-byte loads only where pitch and address allow).
    count: elements per channel in the GLOBAL batch; None = this shard's count times the number of shards (the training step's
    equal-shard contract). Shards of different sizes pass the true global count. Only this backward takes it: bn_stats_sync and
    the training step still assume equal shards, so unequal shards are NOT supported end to end."""
    _chk_rows(x, torch.float32); _chk_rows(dy, torch.float32)
    if yout is not None:
        _chk_rows(yout, torch.float32)
    rows, cols = x.shape
    ch = period if mode == 0 else cols
    L = _lib.lib()
    local = torch.empty(2 * ch, dtype=torch.float64, device=x.device)
    ld_y = yout.stride(0) if yout is not None else 0
    wide = mode == 1 and cols > 64                  # a head with more than 64 classes: the column-mode pair without the 64-column limit
    if wide:
        _lib.check(L.mla_bn_bwd_sums_wide(_p(x), x.stride(0), _p(dy), dy.stride(0), _p(yout), ld_y, act, float(drop_scale), rows, cols,
                                          _p(mean), _p(var), BN_EPS, _p(_workspace(x.device)), _p(local), _lib.stream_ptr()))
    else:
        _lib.check(L.mla_bn_bwd_sums(_p(x), x.stride(0), _p(dy), dy.stride(0), _p(yout), ld_y, act, float(drop_scale), rows, cols, mode,
                                     period, _p(mean), _p(var), BN_EPS, _p(_workspace(x.device)), _p(local), _lib.stream_ptr()))
    glob = local
    if not batch_stats:
        glob = torch.zeros_like(local)
    elif dist.bn_active:
        glob = dist.all_reduce_sum(local.clone(), "syncbn_bwd")
    if count is None:
        count = (rows // period * cols if mode == 0 else rows) * dist.bn_world
    if want_dx and dx is None:
        dx = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
    tail = (_p(mean), _p(var), _p(gamma), BN_EPS, _p(glob), _p(local), float(count), _p(dx) if want_dx else None,
            dx.stride(0) if want_dx else 0, int(accumulate), _p(dgamma), _p(dbeta), _lib.stream_ptr())
    head = (_p(x), x.stride(0), _p(dy), dy.stride(0), _p(yout), ld_y, act, float(drop_scale), rows, cols)
    _lib.check(L.mla_bn_bwd_apply_wide(*head, *tail) if wide else L.mla_bn_bwd_apply(*head, mode, period, *tail))
    return dx


def attention_pool_bwd(dy, att, cla, bags, T, K):
    du_v, du_f = torch.empty_like(att), torch.empty_like(att)
    _lib.check(_lib.lib().mla_attention_pool_bwd(_p(dy), dy.stride(0), _p(att), _p(cla), bags, T, K, _p(du_v), _p(du_f), _lib.stream_ptr()))
    return du_v, du_f


def linear_small_bwd(a, w, dz, dw, db):
    M, K = a.shape
    N = w.shape[0]
    da = torch.empty((M, K), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().mla_linear_small_bwd(_p(a), a.stride(0), _p(w), w.stride(0), _p(dz), dz.stride(0), M, N, K, _p(da), K,
                                               _p(dw), _p(db), _lib.stream_ptr()))
    return da


def transpose_padded(x):
    """(R, C) f32 | bf16 -> (C, R~) with zero padding (R~ = R rounded up to a 16-byte row), K-contiguous for the MFMA GEMM."""
    _chk_rows(x)
    R, C = x.shape
    if x.dtype == torch.bfloat16:
        ld = (R + 7) // 8 * 8
        out = torch.empty((C, ld), dtype=torch.bfloat16, device=x.device)
        _lib.check(_lib.lib().mla_transpose_bf16(_p(x), x.stride(0), _p(out), ld, R, C, _lib.stream_ptr()))
        return out
    _chk_rows(x, torch.float32)
    ld = (R + 3) // 4 * 4
    out = torch.zeros((C, ld), dtype=torch.float32, device=x.device) if ld != R else torch.empty((C, ld), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().mla_transpose_f32(_p(x), x.stride(0), _p(out), ld, R, C, _lib.stream_ptr()))
    return out


def col_sum(x, out):
    _chk_rows(x)
    rows, cols = x.shape
    key = "colsum/" + str(x.device)
    if key not in _ws or _ws[key].numel() < 64 * cols:
        _ws[key] = torch.empty(64 * max(cols, 4096), dtype=torch.float64, device=x.device)
    ws = _ws[key]
    fn = _lib.lib().mla_col_sum_bf16 if x.dtype == torch.bfloat16 else _lib.lib().mla_col_sum
    _lib.check(fn(_p(x), x.stride(0), rows, cols, _p(ws), _p(out), _lib.stream_ptr()))
    return out


def axpy(a, x, y):
    _lib.check(_lib.lib().mla_axpy(float(a), _p(x), _p(y), x.numel(), _lib.stream_ptr()))
    return y


def check_labels(labels, K):
    """nn.CrossEntropyLoss raises on a target outside [0, K) (train.py:372 keeps the default ignore_index=-100, a value the
    reference's dataset never produces -- labels are class indices, dataset.py:60-75 -- and which is refused here like any other
    negative label rather than silently dropped from the mean). Host tensors are checked
    here before the upload (no device sync); for device tensors the kernel refuses to index with such a label and reports
    it through its second counter (`hits[1]` = number of such labels) + a NaN loss, which `raise_on_bad_labels` turns into the
    same exception. The two counters are separate so that their sum over data-parallel ranks cannot cancel."""
    if not labels.is_cuda and labels.numel():
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi >= K:
            raise IndexError("Target %d is out of bounds." % (lo if lo < 0 else hi))


def raise_on_bad_labels(hits):
    """Call where the step's result is read on the host anyway (train.py:141-142): `hits` is cross_entropy's pair
    [n_correct, n_bad_labels] (summed over the ranks by a data-parallel step). Returns n_correct."""
    n, bad = (int(v) for v in hits.tolist())
    if bad > 0:
        raise IndexError("Target out of bounds: %d label(s) outside [0, num_classes)." % bad)
    return n


def cross_entropy(scores, labels, inv_total, want_grad=True):
    """CrossEntropyLoss(mean over the GLOBAL batch) on (B, K) scores: (loss, dscores, hits) with hits = int32 [n_correct,
    n_bad]; n_bad > 0 (and a NaN loss): that many labels were outside [0, K) -- see check_labels."""
    _chk_rows(scores, torch.float32); _chk(labels, torch.int64)
    B, K = scores.shape
    loss = torch.empty(1, dtype=torch.float32, device=scores.device)
    hits = torch.empty(2, dtype=torch.int32, device=scores.device)
    d = torch.empty((B, K), dtype=torch.float32, device=scores.device) if want_grad else None
    _lib.check(_lib.lib().mla_cross_entropy(_p(scores), scores.stride(0), _p(labels), B, K, float(inv_total), _p(loss), _p(d),
                                            K, _p(hits), _lib.stream_ptr()))
    return loss, d, hits


def check_labels_ignoring(labels, K, ignore_index):
    """check_labels for a criterion that honours ``ignore_index``: host labels equal to it pass (also when it is a class index),
    every other label outside [0, K) raises before the upload. Device labels are left to the kernel's counter, as there."""
    if not labels.is_cuda and labels.numel():
        kept = labels[labels != ignore_index]
        if kept.numel():
            lo, hi = int(kept.min()), int(kept.max())
            if lo < 0 or hi >= K:
                raise IndexError("Target %d is out of bounds." % (lo if lo < 0 else hi))


REDUCTIONS = {"mean": 0, "sum": 1}


def cross_entropy_opts(scores, labels, weight=None, ignore_index=-100, label_smoothing=0.0, reduction="mean", dist=None, want_grad=True):
    """nn.CrossEntropyLoss(weight, ignore_index=, label_smoothing=, reduction="mean" | "sum") on (B, K <= 1024) scores:
    (loss, dscores, hits, counted). hits = int32 [n_correct, n_bad] as cross_entropy's (raise_on_bad_labels reads it), counted =
    int32 [rows whose label is not ignore_index]; both are views of one 3-element tensor. Ignored rows add no loss, get exact zeros
    in dscores and are neither hits nor bad labels. The mean divides by the sum of weight[y] over the counted rows of the GLOBAL
    batch: with an active `dist` the denominator is all-reduced (on the current stream) in front of the main launch, so each
    rank's loss is its share of the global mean (sum the losses) and dscores is scaled for a summed gradient. With no counted
    row the mean is NaN, as torch's, and dscores all zero. Three launches (two for "sum"), graph-capturable, bit-reproducible."""
    _chk_rows(scores, torch.float32); _chk(labels, torch.int64)
    if reduction not in REDUCTIONS:
        raise ValueError("reduction must be 'mean' or 'sum' (the HIP loss returns a scalar), not %r" % (reduction,))
    B, K = scores.shape
    dev = scores.device
    if weight is not None:
        _chk(weight, torch.float32)
        assert weight.numel() == K, "weight holds %d elements for %d classes" % (weight.numel(), K)
    L = _lib.lib()
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    d = torch.empty((B, K), dtype=torch.float32, device=dev) if want_grad else None
    ws = torch.empty(int(L.mla_cross_entropy_opts_workspace_bytes(B)) // 8, dtype=torch.float64, device=dev)
    den = None
    if reduction == "mean":
        den = torch.empty(1, dtype=torch.float32, device=dev)
        _lib.check(L.mla_cross_entropy_den(_p(labels), B, K, _p(weight), int(ignore_index), _p(den), _lib.stream_ptr()))
        if dist is not None:
            dist.all_reduce_sum(den, "loss:den")
    _lib.check(_timed("cross_entropy_opts", L.mla_cross_entropy_opts, _p(scores), scores.stride(0), _p(labels), B, K, _p(weight),
                      int(ignore_index), float(label_smoothing), REDUCTIONS[reduction], _p(den), _p(loss), _p(d), K, _p(counts), _p(ws),
                      _lib.stream_ptr()))
    return loss, d, counts[0:2], counts[2:3]


def check_targets(targets, K):
    """nn.BCELoss raises on a target outside [0, 1] (a NaN included) and on a shape other than its input's. Host tensors are
    checked here before the upload (no device sync); for device tensors the kernel takes no logarithm of such a cell and reports
    it through its second counter (`hits[1]` = number of bad cells) + a NaN loss, which `raise_on_bad_targets` turns into the
    same exception -- as check_labels does for class indices."""
    if targets.dim() != 2 or targets.shape[1] != K:
        raise ValueError("multi-label targets must have shape (batch, %d), one column per class, not %s" % (K, tuple(targets.shape)))
    if not targets.is_cuda and targets.numel():
        t = targets.detach().float()
        if bool(torch.isnan(t).any()):
            raise ValueError("a target is NaN; BCELoss targets lie in [0, 1]")
        lo, hi = float(t.min()), float(t.max())
        if lo < 0.0 or hi > 1.0:
            raise ValueError("target %g lies outside [0, 1]" % (lo if lo < 0.0 else hi))


def raise_on_bad_targets(hits):
    """Call where the step's result is read on the host anyway: `hits` is bce_loss's pair [n_exact, n_bad_cells] (summed over the
    ranks by a data-parallel step). Returns n_exact, the rows in which every class lies on the right side of 0.5."""
    n, bad = (int(v) for v in hits.tolist())
    if bad > 0:
        raise ValueError("%d bad cell(s): a target that is NaN or outside [0, 1], or a probability outside [0, 1]" % bad)
    return n


def bce_loss(probs, targets, weight=None, reduction="mean", inv_total=None, want_grad=True):
    """nn.BCELoss(weight, reduction="mean" | "sum") on (B, K <= 1024) probabilities with float32 targets (B, K) in [0, 1], soft
    ones included: (loss, dprobs, hits, cell_hits). hits = int32 [rows with every class on the right side of 0.5 (subset accuracy),
    bad cells] (raise_on_bad_targets reads it), cell_hits = int32 [cells on the right side]; both are views of one 3-element
    tensor. ``inv_total``: the mean's scale, None = 1 / (B K); a data-parallel step passes 1 / (GLOBAL B * K), so that each rank's
    loss is its share of the global mean (sum the losses) and dprobs is scaled for a summed gradient. Both operands may be column
    slices with a pitch. Two launches, graph-capturable, bit-reproducible; see mla_bce for bad cells and NaN."""
    _chk_rows(probs, torch.float32); _chk_rows(targets, torch.float32)
    if reduction not in REDUCTIONS:
        raise ValueError("reduction must be 'mean' or 'sum' (the HIP loss returns a scalar), not %r" % (reduction,))
    B, K = probs.shape
    assert tuple(targets.shape) == (B, K), "targets %s for probabilities %s" % (tuple(targets.shape), (B, K))
    dev = probs.device
    if weight is not None:
        _chk(weight, torch.float32)
        assert weight.numel() == K, "weight holds %d elements for %d classes" % (weight.numel(), K)
    L = _lib.lib()
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    d = torch.empty((B, K), dtype=torch.float32, device=dev) if want_grad else None
    ws = torch.empty(int(L.mla_bce_workspace_bytes(B)) // 8, dtype=torch.float64, device=dev)
    scale = 1.0 / (B * K) if inv_total is None else float(inv_total)
    _lib.check(_timed("bce", L.mla_bce, _p(probs), probs.stride(0), _p(targets), targets.stride(0), B, K, _p(weight), REDUCTIONS[reduction],
                      scale, _p(loss), _p(d), K, _p(counts), _p(ws), _lib.stream_ptr()))
    return loss, d, counts[0:2], counts[2:3]


def dropout_mask_dev(n, seed, stream_base, counter, offset, p_drop, device, out=None):
    """dropout_mask with stream_id = stream_base + counter[0] + 1 read on the device (graph-captured training step)."""
    assert counter.dtype == torch.int64 and counter.is_cuda
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().mla_dropout_mask_dev(_p(out), n, int(seed) & (2 ** 64 - 1), int(stream_base) & (2 ** 64 - 1), _p(counter), int(offset),
                                               float(p_drop), _lib.stream_ptr()))
    return out


def adam_prepare(scal, lr, beta1, beta2, step):
    """Write Adam's step-dependent scalars for step `step` into the device pair adam_step_dev reads (an ordinary launch, enqueued in
    front of a graph replay)."""
    assert scal.dtype == torch.float32 and scal.is_cuda and scal.numel() == 2
    _lib.check(_lib.lib().mla_adam_prepare(_p(scal), float(lr), float(beta1), float(beta2), int(step), _lib.stream_ptr()))


def adam_step_dev(p, g, m, v, beta1, beta2, eps, scal, counter):
    """adam_step with its step-dependent scalars read from `scal` (adam_prepare), then counter += 1 (both graph-capturable)."""
    L = _lib.lib()
    _lib.check(L.mla_adam_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), float(beta1), float(beta2), float(eps), _p(scal), _lib.stream_ptr()))
    _lib.check(L.mla_counter_add(_p(counter), 1, _lib.stream_ptr()))


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step):
    _lib.check(_lib.lib().mla_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                                        int(step), _lib.stream_ptr()))


def adam_groups_table(numels, groups, n_groups):
    """The host half of the grouped Adam step (no device): tensor sizes (flat-buffer order) and their group indices -> dict with
    the padded `total`, the counts `runs`, `pads`, `chunks`, and `table`, the int64 CPU tensor mla_adam_grouped_step reads from
    device memory (run_end[runs] | run_group[runs] | chunk_run[chunks] | chunk_pad[chunks + 1] | (quad, valid)[pads])."""
    L = _lib.lib()
    n = len(numels)
    assert n == len(groups) and n >= 1
    numel = (ctypes.c_int64 * n)(*[int(k) for k in numels])
    grp = (ctypes.c_int32 * n)(*[int(k) for k in groups])
    counts = (ctypes.c_int64 * 5)()
    _lib.check(L.mla_adam_groups_table(numel, grp, n, int(n_groups), None, 0, counts))
    table = torch.zeros(counts[4], dtype=torch.int64)
    _lib.check(L.mla_adam_groups_table(numel, grp, n, int(n_groups), ctypes.c_void_p(table.data_ptr()), table.numel(), counts))
    return {"total": counts[0], "runs": counts[1], "pads": counts[2], "chunks": counts[3], "table": table}


def adam_groups_prepare(rows, groups, step):
    """Write the per-group rows of step `step` (an ordinary launch, enqueued in front of the step or the graph replay).
    rows: float32 device tensor of len(groups) * 8; groups: dicts with lr, betas, eps, weight_decay, decoupled, amsgrad."""
    assert rows.dtype == torch.float32 and rows.is_cuda and rows.numel() >= 8 * len(groups)
    arr = (_lib.AdamGroup * max(len(groups), 1))()
    for a, g in zip(arr, groups):
        a.lr, a.beta1, a.beta2, a.eps = float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])
        a.weight_decay, a.decoupled, a.amsgrad = float(g["weight_decay"]), int(bool(g["decoupled"])), int(bool(g["amsgrad"]))
    _lib.check(_lib.lib().mla_adam_groups_prepare(_p(rows), arr, len(groups), int(step), _lib.stream_ptr()))


def adam_grouped_step(p, g, m, v, vmax, table, n_runs, n_pads, rows, n_groups, coef=None, counter=None):
    """The Adam / AdamW step of every group in one launch (graph-capturable). table: adam_groups_table's tensor on the device;
    rows: adam_groups_prepare's; vmax: the amsgrad buffer or None; coef: None or the 1-element device tensor the gradient is
    scaled by (grad_norm's coefficient); counter: None or the device step counter, advanced by one."""
    assert table.dtype == torch.int64 and table.is_cuda and rows.is_cuda and rows.numel() >= 8 * n_groups
    assert all(t.dtype == torch.float32 and t.is_cuda and t.numel() == p.numel() for t in (p, g, m, v) + ((vmax,) if vmax is not None else ()))
    assert coef is None or (coef.is_cuda and coef.dtype == torch.float32 and coef.numel() == 1)
    L = _lib.lib()
    _lib.check(_timed("adam_grouped", L.mla_adam_grouped_step, _p(p), _p(g), _p(m), _p(v), _p(vmax), p.numel(), _p(table), table.numel(),
                      int(n_runs), int(n_pads), _p(rows), int(n_groups), _p(coef), _lib.stream_ptr()))
    if counter is not None:
        _lib.check(L.mla_counter_add(_p(counter), 1, _lib.stream_ptr()))


def grad_norm(g, max_norm, out=None, workspace=None):
    """-> float32 device pair [||g||_2, min(1, max_norm / (norm + 1e-6))]: torch.nn.utils.clip_grad_norm_'s norm and factor of a
    flat float32 gradient; deterministic (double-precision sums in a fixed order), graph-capturable, no host sync."""
    _chk(g, torch.float32)
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=g.device)
    if workspace is None:
        workspace = torch.empty(_lib.lib().mla_grad_norm_workspace_bytes() // 8, dtype=torch.float64, device=g.device)
    assert out.dtype == torch.float32 and out.numel() == 2 and workspace.numel() * workspace.element_size() >= _lib.lib().mla_grad_norm_workspace_bytes()
    _lib.check(_timed("grad_norm", _lib.lib().mla_grad_norm, _p(g), g.numel(), float(max_norm), _p(workspace), _p(out), _lib.stream_ptr()))
    return out


# ------------------------------------------------------------------ finetune (CNN gradients) ----

def conv3x3(x, w_packed, b, cout, pool, act):
    """Generic conv entry (training forward without fused pool, and dgrad), f32 or bf16. x NHWC."""
    _chk(x); _chk(w_packed, x.dtype)
    n, H, W_, cin = x.shape
    out = torch.empty((n, H // 2, W_ // 2, cout) if pool else (n, H, W_, cout), dtype=x.dtype, device=x.device)
    _lib.check(_timed("conv3x3_%d_%d" % (cin, cout), _lib.lib().mla_conv3x3, _p(x), _p(w_packed), _p(b), _p(out), n, H, W_, cin, cout,
                      int(pool), int(act), DT[x.dtype], _lib.stream_ptr()))
    return out


def conv3x3_train(x, w_packed, b, cout):
    """Training forward of a pooled layer: (pre-pool post-ReLU activation, its 2x2 max-pool) from one kernel."""
    _chk(x); _chk(w_packed, x.dtype)
    n, H, W_, cin = x.shape
    a = torch.empty((n, H, W_, cout), dtype=x.dtype, device=x.device)
    pooled = torch.empty((n, H // 2, W_ // 2, cout), dtype=x.dtype, device=x.device)
    _lib.check(_timed("conv3x3_%d_%d" % (cin, cout), _lib.lib().mla_conv3x3_train, _p(x), _p(w_packed), _p(b), _p(a), _p(pooled), n, H, W_,
                      cin, cout, DT[x.dtype], _lib.stream_ptr()))
    return a, pooled


def conv3x3_train_codes(x, w_packed, b, cout):
    """Training forward of a pooled layer, compact form: (window codes uint8 (n, H/2, W/2, cout), pooled activation). A code is the
    position 0..3 of the first maximum of the 2x2 window (MaxPool2d's order), or 4 where the ReLU is off -- one byte instead of the
    four pre-pool activations (8 bytes in bf16) that conv3x3_train keeps for the backward."""
    _chk(x); _chk(w_packed, x.dtype)
    n, H, W_, cin = x.shape
    codes = torch.empty((n, H // 2, W_ // 2, cout), dtype=torch.uint8, device=x.device)
    pooled = torch.empty((n, H // 2, W_ // 2, cout), dtype=x.dtype, device=x.device)
    _lib.check(_timed("conv3x3_%d_%d" % (cin, cout), _lib.lib().mla_conv3x3_train_codes, _p(x), _p(w_packed), _p(b), _p(codes), _p(pooled),
                      n, H, W_, cin, cout, DT[x.dtype], _lib.stream_ptr()))
    return codes, pooled


def _bias_ws(bf16, device):
    """The double-precision slots of the bias gradient, per device: "biasws16/" for the bf16 kernels (8 channels per lane), "biasws/" f32."""
    key = ("biasws16/" if bf16 else "biasws/") + str(device)
    if key not in _ws:
        nbytes = _lib.lib().mla_relu_pool_bwd_bf16_workspace_bytes() if bf16 else _lib.lib().mla_relu_pool_bwd_bias_workspace_bytes()
        _ws[key] = torch.empty(int(nbytes) // 8, dtype=torch.float64, device=device)
    return _ws[key]


def pool_bwd_codes(codes, d_out, db=None):
    """dZ (n, H, W, C) bf16 at the pre-pool resolution from the window codes and the pooled gradient; db: bias gradient on the way."""
    assert codes.dtype == torch.uint8 and codes.is_cuda and codes.is_contiguous()
    _chk(d_out, torch.bfloat16)
    n, HO, WO, C = codes.shape
    assert tuple(d_out.shape) == tuple(codes.shape)
    dz = torch.empty((n, 2 * HO, 2 * WO, C), dtype=torch.bfloat16, device=codes.device)
    _lib.check(_timed("relu_pool_bwd", _lib.lib().mla_pool_bwd_codes_bf16, _p(codes), _p(d_out), _p(dz), n, 2 * HO, 2 * WO, C,
                      _p(_bias_ws(True, codes.device)), _p(db), _lib.stream_ptr()))
    return dz


def repack_dgrad(w, dtype=torch.float32):
    """(Cout, Cin, 3, 3) f32 -> (Cin, 9, Cout) flipped, in `dtype`: weights of the transposed convolution."""
    _chk(w, torch.float32)
    cout, cin = w.shape[0], w.shape[1]
    out = torch.empty((cin, 9, cout), dtype=dtype, device=w.device)
    fn = _lib.lib().mla_conv_repack_dgrad_bf16 if dtype == torch.bfloat16 else _lib.lib().mla_conv_repack_dgrad
    _lib.check(fn(_p(w), cout, cin, _p(out), _lib.stream_ptr()))
    return out


def maxpool2x2(a):
    _chk(a)
    n, H, W_, C = a.shape
    out = torch.empty((n, H // 2, W_ // 2, C), dtype=a.dtype, device=a.device)
    fn = _lib.lib().mla_maxpool2x2_bf16 if a.dtype == torch.bfloat16 else _lib.lib().mla_maxpool2x2
    _lib.check(_timed("maxpool", fn, _p(a), _p(out), n, H, W_, C, _lib.stream_ptr()))
    return out


def relu_pool_bwd(a, d_out, pool, db=None, bf16=False):
    """dZ at a's resolution from the gradient of relu(.) [pool == 0] or maxpool(relu(.)) [pool == 1]; db (C,): also the
    bias gradient = column sums of dZ, accumulated in the same pass. bf16 (or a bf16 `a`): dZ in bf16 (a / d_out both bf16,
    or both f32 for the last Linear whose output is f32)."""
    _chk(a); _chk(d_out, a.dtype)
    a4 = a if a.dim() == 4 else a.reshape(a.shape[0], 1, 1, -1)
    n, H, W_, C = a4.shape
    if bf16 or a.dtype == torch.bfloat16:
        dz = torch.empty(a.shape, dtype=torch.bfloat16, device=a.device)
        _lib.check(_timed("relu_pool_bwd", _lib.lib().mla_relu_pool_bwd_bf16, _p(a), DT[a.dtype], _p(d_out), DT[d_out.dtype], _p(dz), n, H, W_, C,
                          int(pool), _p(_bias_ws(True, a.device)), _p(db), _lib.stream_ptr()))
        return dz
    _chk(a, torch.float32)
    dz = torch.empty_like(a)
    if db is None:
        _lib.check(_lib.lib().mla_relu_pool_bwd(_p(a), _p(d_out), _p(dz), n, H, W_, C, int(pool), _lib.stream_ptr()))
        return dz
    _chk(db, torch.float32)
    _lib.check(_timed("relu_pool_bwd", _lib.lib().mla_relu_pool_bwd_bias, _p(a), _p(d_out), _p(dz), n, H, W_, C, int(pool),
                      _p(_bias_ws(False, a.device)), _p(db), _lib.stream_ptr()))
    return dz


_wg_ws = {}


def scratch(device):
    """The live scratch entries of `device`, {key: tensor}. An entry is REPLACED when a call needs more room than it has, and
    the old tensor goes back to torch's allocator unless somebody else holds it: whoever records an entry's address in a HIP
    graph keeps the tensor from this dict (so the address stays the graph's) and compares data_ptr() before a replay."""
    return {(i, k): t for i, d in enumerate((_ws, _wg_ws)) for k, t in d.items() if t.device == device}


def conv_wgrad(dz, a_in, dw):
    _chk(dz); _chk(a_in, dz.dtype)
    n, H, W_, cout = dz.shape
    cin = a_in.shape[3]
    key = str(dz.device)
    if key not in _wg_ws:
        _wg_ws[key] = torch.empty(int(_lib.lib().mla_conv_wgrad_workspace_floats()), dtype=torch.float32, device=dz.device)
    ws = _wg_ws[key]
    assert dw.is_contiguous() and tuple(dw.shape) == (cout, cin, 3, 3) and dw.dtype == torch.float32
    fn = _lib.lib().mla_conv_wgrad_bf16 if dz.dtype == torch.bfloat16 else _lib.lib().mla_conv_wgrad
    _lib.check(_timed("wgrad_%d_%d" % (cin, cout), fn, _p(dz), _p(a_in), n, H, W_, cin, cout, _p(ws), ws.numel(), _p(dw), _lib.stream_ptr()))


def conv1_bwd(x, w, b, d_pooled, dw, db):
    _chk(x, torch.float32); _chk(d_pooled)
    n = x.shape[0]
    ws = torch.empty(int(_lib.lib().mla_conv1_bwd_workspace_floats()), dtype=torch.float32, device=x.device)
    fn = _lib.lib().mla_conv1_bwd_bf16 if d_pooled.dtype == torch.bfloat16 else _lib.lib().mla_conv1_bwd
    _lib.check(_timed("conv1_bwd", fn, _p(x), _p(w), _p(b), _p(d_pooled), n, _p(ws), _p(dw), _p(db), _lib.stream_ptr()))


def conv1_dgrad(x, w, b, d_pooled):
    """Gradient of conv1 + ReLU + max-pool with respect to its input: x (n, 96, 64) f32, d_pooled (n, 48, 32, 64) f32 or bf16 ->
    dx (n, 96, 64) f32 (mla_conv1_dgrad: the layer is recomputed, every element of dx is written once)."""
    _chk(x, torch.float32); _chk(w, torch.float32); _chk(b, torch.float32); _chk(d_pooled)
    n = x.shape[0]
    assert tuple(x.shape) == (n, 96, 64) and tuple(d_pooled.shape) == (n, 48, 32, 64) and tuple(w.shape) == (64, 1, 3, 3) and b.numel() == 64
    dx = torch.empty((n, 96, 64), dtype=torch.float32, device=x.device)
    _lib.check(_timed("conv1_dgrad", _lib.lib().mla_conv1_dgrad, _p(x), _p(w), _p(b), _p(d_pooled), DT[d_pooled.dtype], n, _p(dx),
                      _lib.stream_ptr()))
    return dx


# ---- ResNet-50 trunk (cnn_type="resnet"): NHWC activations in f32 / bf16, see include/mla_hip.h "ResNet-50 v1.5 trunk" ----

def rn_repack(w, dtype):
    """Conv2d weight (O, I, k, k) f32 -> (O, k, k, I) in `dtype`."""
    _chk(w, torch.float32)
    cout, cin, ks = w.shape[0], w.shape[1], w.shape[2]
    out = torch.empty((cout, ks, ks, cin), dtype=dtype, device=w.device)
    _lib.check(_lib.lib().mla_rn_repack(_p(w), cout, cin, ks, _p(out), DT[dtype], _lib.stream_ptr()))
    return out


def rn_stem(planes, single, w, dtype, scale=None, shift=None, relu=False):
    """(N, 224, 224) f32 planes -> NHWC (N, 112, 112, 64): Input normalisation + conv1 [+ eval bn1 + ReLU]."""
    _chk(planes, torch.float32); _chk(w, torch.float32)
    assert planes.dim() == 3, planes.shape
    n, H, W_ = planes.shape
    out = torch.empty((n, 112, 112, 64), dtype=dtype, device=planes.device)
    _lib.check(_timed("rn_stem", _lib.lib().mla_rn_stem, _p(planes), n, H, W_, int(single), _p(w), _p(scale), _p(shift), int(relu), _p(out),
                      DT[dtype], _lib.stream_ptr()))
    return out


def rn_conv(x, w_packed, stride, scale=None, shift=None, residual=None, relu=False):
    """NHWC x (N, H, W, Cin), packed weight (Cout, k, k, Cin) -> (N, Ho, Wo, Cout) [* scale + shift] [+ residual] [ReLU]."""
    _chk(x); _chk(w_packed, x.dtype)
    n, H, W_, cin = x.shape
    cout, ks = w_packed.shape[0], w_packed.shape[1]
    pad = ks // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W_ + 2 * pad - ks) // stride + 1
    out = torch.empty((n, Ho, Wo, cout), dtype=x.dtype, device=x.device)
    if residual is not None:
        _chk(residual, x.dtype)
        assert residual.shape == out.shape, (residual.shape, out.shape)
    _lib.check(_timed("rn_conv%dx%d" % (ks, ks), _lib.lib().mla_rn_conv, _p(x), n, H, W_, cin, _p(w_packed), cout, ks, stride,
                      _p(scale), _p(shift), _p(residual), int(relu), _p(out), DT[x.dtype], _lib.stream_ptr()))
    return out


def _rn_workspace(device, channels):
    key = ("rn_bn", str(device))
    need = int(_lib.lib().mla_rn_bn_workspace_bytes(channels)) // 8
    if key not in _ws or _ws[key].numel() < need:
        _ws[key] = torch.empty(need, dtype=torch.float64, device=device)
    return _ws[key]


def _rn_bn_finish(x, bn, running, want_stats, name, fn, *head):
    """What rn_bn_stats and rn_bn_stats_sync share: the outputs, the running buffers and the batch counter around the library
    call fn(*head, gamma, beta, eps, momentum, running_mean, running_var, mean, var, scale, shift, stream), timed as `name`."""
    C = x.shape[-1]
    dev = x.device
    scale = torch.empty(C, dtype=torch.float32, device=dev)
    shift = torch.empty(C, dtype=torch.float32, device=dev)
    mean = torch.empty(C, dtype=torch.float32, device=dev) if want_stats else None
    var = torch.empty(C, dtype=torch.float32, device=dev) if want_stats else None
    rm, rv = (bn.running_mean, bn.running_var) if running else (None, None)
    _lib.check(_timed(name, fn, *head, _p(bn.weight.detach()), _p(bn.bias.detach()), float(bn.eps), float(bn.momentum), _p(rm), _p(rv),
                      _p(mean), _p(var), _p(scale), _p(shift), _lib.stream_ptr()))
    if running:
        _lib.check(_lib.lib().mla_counter_add(_p(bn.num_batches_tracked), 1, _lib.stream_ptr()))
    return (scale, shift, mean, var) if want_stats else (scale, shift)


def rn_bn_stats(x, bn, running=True, want_stats=False):
    """Train-mode BatchNorm2d statistics of NHWC x: returns (scale, shift[, mean, var_biased]); updates bn's running
    statistics (and num_batches_tracked) when `running`."""
    _chk(x)
    C = x.shape[-1]
    return _rn_bn_finish(x, bn, running, want_stats, "rn_bn_stats", _lib.lib().mla_rn_bn_stats, _p(x), x.numel() // C, C, DT[x.dtype],
                         _p(_rn_workspace(x.device, C)))


def rn_bn_stats_sync(x, bn, dist, running=True, want_stats=False):
    """rn_bn_stats with the statistics of the data-parallel group's global batch (SyncBN): [sum x, sum x^2, rows] of the local
    shard, all-reduced (tag "syncbn_rn"), then finished on every rank. The row count travels in the message, so shards may
    differ in size. Without an active SyncBN group (no group, or sync_bn=False) this is rn_bn_stats itself, bit for bit."""
    if not dist.bn_active:
        return rn_bn_stats(x, bn, running, want_stats)
    _chk(x)
    C = x.shape[-1]
    L = _lib.lib()
    sums = torch.empty(2 * C + 1, dtype=torch.float64, device=x.device)
    _lib.check(_timed("rn_bn_sums", L.mla_rn_bn_sums, _p(x), x.numel() // C, C, DT[x.dtype], _p(_rn_workspace(x.device, C)), _p(sums),
                      _lib.stream_ptr()))
    dist.all_reduce_sum(sums, "syncbn_rn")
    return _rn_bn_finish(x, bn, running, want_stats, "rn_bn_finish", L.mla_rn_bn_finish, _p(sums), C)


def rn_bn_eval_coeffs(bn):
    C = bn.num_features
    dev = bn.weight.device
    scale = torch.empty(C, dtype=torch.float32, device=dev)
    shift = torch.empty(C, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().mla_rn_bn_eval_coeffs(_p(bn.weight.detach()), _p(bn.bias.detach()), _p(bn.running_mean), _p(bn.running_var),
                                                float(bn.eps), C, _p(scale), _p(shift), _lib.stream_ptr()))
    return scale, shift


def rn_bn_apply(x, scale, shift, residual=None, relu=False, out=None):
    _chk(x)
    C = x.shape[-1]
    out = x if out is None else out
    if residual is not None:
        _chk(residual, x.dtype)
        assert residual.shape == x.shape
    _lib.check(_timed("rn_bn_apply", _lib.lib().mla_rn_bn_apply, _p(x), x.numel() // C, C, _p(scale), _p(shift), _p(residual), int(relu),
                      _p(out), DT[x.dtype], _lib.stream_ptr()))
    return out


def rn_maxpool(x):
    _chk(x)
    n, H, W_, C = x.shape
    out = torch.empty((n, (H - 1) // 2 + 1, (W_ - 1) // 2 + 1, C), dtype=x.dtype, device=x.device)
    _lib.check(_timed("rn_maxpool", _lib.lib().mla_rn_maxpool, _p(x), n, H, W_, C, _p(out), DT[x.dtype], _lib.stream_ptr()))
    return out


def rn_avgpool(x):
    """NHWC (N, H, W, C) -> f32 (N, C)."""
    _chk(x)
    n, H, W_, C = x.shape
    out = torch.empty((n, C), dtype=torch.float32, device=x.device)
    _lib.check(_timed("rn_avgpool", _lib.lib().mla_rn_avgpool, _p(x), n, H * W_, C, _p(out), DT[x.dtype], _lib.stream_ptr()))
    return out


# ---- backward of the ResNet-50 trunk (csrc/resnet_bwd.hip): gradients NHWC in the activations' dtype, weight gradients f32 ----
# Workspaces are allocated per call from torch's caching allocator: inside a graph capture they belong to the graph's pool,
# so no later eager call of another size can free memory a captured step still uses.

def rn_repack_dgrad(w, dtype):
    """Conv2d weight (O, I, k, k) f32 -> (I, k, k, O) in `dtype` with the taps flipped (data-gradient weights)."""
    _chk(w, torch.float32)
    cout, cin, ks = w.shape[0], w.shape[1], w.shape[2]
    out = torch.empty((cin, ks, ks, cout), dtype=dtype, device=w.device)
    _lib.check(_lib.lib().mla_rn_repack_dgrad(_p(w), cout, cin, ks, _p(out), DT[dtype], _lib.stream_ptr()))
    return out


def rn_conv_dgrad(dy, w_dgrad, stride, in_hw, residual=None):
    """dy (N, Ho, Wo, Cout), dgrad weights (Cin, k, k, Cout) -> dx (N, H, W, Cin) [+ residual]; in_hw = (H, W)."""
    _chk(dy); _chk(w_dgrad, dy.dtype)
    n, Ho, Wo, cout = dy.shape
    cin, ks = w_dgrad.shape[0], w_dgrad.shape[1]
    H, W_ = in_hw
    out = torch.empty((n, H, W_, cin), dtype=dy.dtype, device=dy.device)
    if residual is not None:
        _chk(residual, dy.dtype)
        assert residual.shape == out.shape, (residual.shape, out.shape)
    _lib.check(_timed("rn_dgrad%dx%d_s%d" % (ks, ks, stride), _lib.lib().mla_rn_conv_dgrad, _p(dy), n, Ho, Wo, cout, _p(w_dgrad), cin, ks,
                      stride, H, W_, _p(residual), _p(out), DT[dy.dtype], _lib.stream_ptr()))
    return out


def rn_conv_wgrad(x, dy, stride, dw):
    """x (N, H, W, Cin), dy (N, Ho, Wo, Cout) in one dtype -> dw (Cout, Cin, k, k) f32, written."""
    _chk(x); _chk(dy, x.dtype); _chk(dw, torch.float32)
    n, H, W_, cin = x.shape
    cout, ks = dw.shape[0], dw.shape[2]
    assert tuple(dw.shape) == (cout, cin, ks, ks) and dy.shape[3] == cout
    L = _lib.lib()
    need = int(L.mla_rn_conv_wgrad_workspace_floats(n, dy.shape[1], dy.shape[2], cin, cout, ks, DT[x.dtype]))
    ws = torch.empty(max(need, 1), dtype=torch.float32, device=x.device)
    _lib.check(_timed("rn_wgrad%dx%d" % (ks, ks), L.mla_rn_conv_wgrad, _p(x), _p(dy), n, H, W_, cin, cout, ks, stride, _p(ws), ws.numel(),
                      _p(dw), DT[x.dtype], _lib.stream_ptr()))


def rn_stem_wgrad(planes, single, dy, dw):
    """Raw (N, 224, 224) f32 planes and dy (N, 112, 112, 64) -> dw (64, 3, 7, 7) f32 of the stem conv (normalisation folded in)."""
    _chk(planes, torch.float32); _chk(dy); _chk(dw, torch.float32)
    n = planes.shape[0]
    L = _lib.lib()
    ws = torch.empty(int(L.mla_rn_stem_wgrad_workspace_floats(n)), dtype=torch.float32, device=planes.device)
    _lib.check(_timed("rn_stem_wgrad", L.mla_rn_stem_wgrad, _p(planes), n, int(single), _p(dy), _p(ws), ws.numel(), _p(dw), DT[dy.dtype],
                      _lib.stream_ptr()))


def rn_bn_bwd(x, dy, mean, var, bn, y=None, want_dres=False, dgamma=None, dbeta=None):
    """Train-mode BatchNorm2d backward: x the BatchNorm input, mean / var its (biased) batch statistics, y the kept ReLU output
    (mask y > 0) or None. Returns (dx, dres): dres = the masked incoming gradient (residual path) when want_dres, else None.
    dgamma / dbeta: f32 tensors to write, or None."""
    _chk(x); _chk(dy, x.dtype)
    if y is not None:
        _chk(y, x.dtype)
    C = x.shape[-1]
    rows = x.numel() // C
    L = _lib.lib()
    ws = torch.empty(int(L.mla_rn_bn_bwd_workspace_bytes(C)) // 8, dtype=torch.float64, device=x.device)
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    _lib.check(_timed("rn_bn_bwd", L.mla_rn_bn_bwd, _p(x), _p(dy), _p(y), rows, C, _p(mean), _p(var), _p(bn.weight.detach()), float(bn.eps),
                      _p(ws), _p(dgamma), _p(dbeta), _p(dx), _p(dres), DT[x.dtype], _lib.stream_ptr()))
    return dx, dres


def rn_bn_bwd_sync(x, dy, mean, var, bn, dist, y=None, want_dres=False, dgamma=None, dbeta=None):
    """rn_bn_bwd under SyncBN: mean / var are the statistics of the data-parallel group's global batch (rn_bn_stats_sync with
    want_stats), and so are the two batch means of the backward: [sum g, sum g xhat, rows] of the local shard, all-reduced (tag
    "syncbn_rn_bwd"), then applied to the local rows. The row count travels in the message, so shards may differ in size. dgamma /
    dbeta receive this rank's part (from the local sums): the gradient all-reduce adds the ranks' parts. Without an active SyncBN
    group (no group, or sync_bn=False) this is rn_bn_bwd itself, bit for bit. The message's last element, the global row
    count, must come out > 0 (every rank contributes its own rows); stage 2 reads it on the device and answers anything else with
    an all-NaN dx, not with an exception."""
    if not dist.bn_active:
        return rn_bn_bwd(x, dy, mean, var, bn, y=y, want_dres=want_dres, dgamma=dgamma, dbeta=dbeta)
    _chk(x); _chk(dy, x.dtype)
    if y is not None:
        _chk(y, x.dtype)
    C = x.shape[-1]
    rows = x.numel() // C
    L = _lib.lib()
    ws = torch.empty(int(L.mla_rn_bn_bwd_workspace_bytes(C)) // 8, dtype=torch.float64, device=x.device)
    sums = torch.empty(2 * C + 1, dtype=torch.float64, device=x.device)
    _lib.check(_timed("rn_bn_bwd_sums", L.mla_rn_bn_bwd_sums, _p(x), _p(dy), _p(y), rows, C, _p(mean), _p(var), float(bn.eps), _p(ws), _p(sums),
                      _p(dgamma), _p(dbeta), DT[x.dtype], _lib.stream_ptr()))
    dist.all_reduce_sum(sums, "syncbn_rn_bwd")
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    _lib.check(_timed("rn_bn_bwd_apply", L.mla_rn_bn_bwd_apply, _p(x), _p(dy), _p(y), rows, C, _p(mean), _p(var), _p(bn.weight.detach()),
                      float(bn.eps), _p(sums), _p(ws), _p(dx), _p(dres), DT[x.dtype], _lib.stream_ptr()))
    return dx, dres


def rn_maxpool_bwd(x, dy):
    """MaxPool2d(3, 2, 1) backward: x the pooled input (N, H, W, C), dy (N, Ho, Wo, C) -> dx like x."""
    _chk(x); _chk(dy, x.dtype)
    n, H, W_, C = x.shape
    dx = torch.empty_like(x)
    _lib.check(_timed("rn_maxpool_bwd", _lib.lib().mla_rn_maxpool_bwd, _p(x), _p(dy), n, H, W_, C, _p(dx), DT[x.dtype], _lib.stream_ptr()))
    return dx


def rn_avgpool_bwd(d, shape, dtype):
    """AdaptiveAvgPool2d(1) backward: d (N, C) f32 -> (N, H, W, C) = d / (H W) in `dtype`; shape = (N, H, W, C)."""
    _chk(d, torch.float32)
    n, H, W_, C = shape
    dx = torch.empty((n, H, W_, C), dtype=dtype, device=d.device)
    _lib.check(_timed("rn_avgpool_bwd", _lib.lib().mla_rn_avgpool_bwd, _p(d), n, H * W_, C, _p(dx), DT[dtype], _lib.stream_ptr()))
    return dx


# ---- input gradient of the eval-mode trunk (saliency maps): the BatchNorm is a folded per-channel constant there ----

def rn_act_bwd(dy, scale, y=None, want_dres=False):
    """Backward of the eval epilogue y = [relu](conv * scale + shift [+ residual]): dy, y (the kept output; None = no ReLU) NHWC in
    one dtype, scale (C,) f32 -> (dpre = dy (y > 0) scale, dres = dy (y > 0) when want_dres, else None)."""
    _chk(dy); _chk(scale, torch.float32)
    if y is not None:
        _chk(y, dy.dtype)
        assert y.shape == dy.shape, (y.shape, dy.shape)
    C = dy.shape[-1]
    assert scale.numel() == C, (scale.shape, C)
    dpre = torch.empty_like(dy)
    dres = torch.empty_like(dy) if want_dres else None
    _lib.check(_timed("rn_act_bwd", _lib.lib().mla_rn_act_bwd, _p(dy), _p(y), _p(scale), dy.numel() // C, C, _p(dpre), _p(dres), DT[dy.dtype],
                      _lib.stream_ptr()))
    return dpre, dres


def rn_stem_dgrad(dy, w, single, y=None, scale=None):
    """dy (N, 112, 112, 64) f32 or bf16, stem weight (64, 3, 7, 7) f32 -> dx (N, 224, 224) f32, the gradient of the RAW planes
    Input receives (repeat / single and the normalisation folded in). y, scale: the stem's fused eval output and BatchNorm scale
    (both or neither); then dy is first masked by y > 0 and scaled."""
    _chk(dy); _chk(w, torch.float32)
    n = dy.shape[0]
    assert tuple(dy.shape) == (n, 112, 112, 64) and tuple(w.shape) == (64, 3, 7, 7), (dy.shape, w.shape)
    assert (y is None) == (scale is None), "y and scale come together"
    if y is not None:
        _chk(y, dy.dtype); _chk(scale, torch.float32)
        assert y.shape == dy.shape and scale.numel() == 64, (y.shape, scale.shape)
    dx = torch.empty((n, 224, 224), dtype=torch.float32, device=dy.device)
    _lib.check(_timed("rn_stem_dgrad", _lib.lib().mla_rn_stem_dgrad, _p(dy), n, _p(y), _p(scale), _p(w), int(single), _p(dx), DT[dy.dtype],
                      _lib.stream_ptr()))
    return dx
