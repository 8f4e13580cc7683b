"""Drop-in for the reference's ``model.py`` (vggish branch): ``Ensemble``, ``Input``, ``CNN``,
``CnnFlatten``, ``EmbeddedMapping``, ``AttentionModule``, ``MultiLevelAttention`` and
``set_requires_grad`` with the same constructor arguments, attribute names and ``state_dict``
keys (model.py:14, :68, :107, :179, :202, :228, :248, :272), executed by HIP kernels.

Reproduced on purpose (SURVEY.md section 7 "quirks"): ``fcv`` feeds both attention branches
and ``fcf`` is a dead parameter (model.py:230-238); BatchNorm1d(T) treats the time slot as
channel; the outputs are sigmoids that train.py feeds to CrossEntropyLoss; ``Input`` is a
reshape, never a transpose (model.py:98-99). The ``resnet`` branch (model.py:128-149) runs a frozen
ResNet-50 trunk on HIP kernels (``resnet.py``); its BatchNorm layers follow train / eval mode.
"""

from typing import Dict, List, Union

import numpy as np
import torch
from torch import nn

from . import differentiable, mla_train, ops, resnet
from .params import *  # noqa: F401,F403  (T, H, K, DR, M_VGGISH, M_VGGISH_JB, S_VGGISH_SHAPE: model.py:9)
from .torchvggish.vggish import Linear, PcmInput, VGGish, cache_stamp, weight_caches


class BatchNorm1d(nn.Module):
    """Parameter / buffer holder with torch.nn.BatchNorm1d's names (weight, bias, running_mean,
    running_var, num_batches_tracked), defaults eps 1e-5, momentum 0.1."""

    def __init__(self, num_features):
        super().__init__()
        self.num_features, self.eps, self.momentum = num_features, 1e-5, 0.1
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    def forward(self, x):
        raise RuntimeError("BatchNorm1d is executed by the fused HIP head of its parent module")


class Dropout(nn.Module):
    """nn.Dropout(p) stand-in. ``mask`` (uint8 keep-mask, 1 = keep) may be injected for reproducible runs; otherwise a
    fresh mask is drawn per training forward by the library's counter-based generator (``mla_dropout_mask``): element i
    of the GLOBAL batch is kept iff hash24(seed, stream, i) >= p * 2^24, with seed = ``torch.initial_seed()`` at
    construction (so ``torch.manual_seed`` makes runs repeatable, as with nn.Dropout) and stream = (this module's
    ordinal, call count). A data-parallel rank passes the offset of its shard: N ranks draw the masks of one process."""

    _instances = 0

    def __init__(self, p=0.5):
        super().__init__()
        self.p, self.mask = p, None
        self.seed, self.calls = torch.initial_seed(), 0
        Dropout._instances += 1
        self.ordinal = Dropout._instances

    def keep_mask(self, numel, device, offset=0):
        if self.mask is not None:
            m = self.mask.to(device=device, dtype=torch.uint8).reshape(-1).contiguous()
            assert m.numel() == numel
            return m
        self.calls += 1
        return ops.dropout_mask(numel, self.seed, (self.ordinal << 32) + self.calls, offset, self.p, device)

    def keep_mask_dev(self, numel, device, offset, counter, base):
        """The mask of call number base + counter[0] + 1 of this module, the call number read ON THE DEVICE: what a HIP graph of
        the training step records, so that every replay draws the next mask of the sequence keep_mask() would have drawn."""
        return ops.dropout_mask_dev(numel, self.seed, (self.ordinal << 32) + base, counter, offset, self.p, device)

    def forward(self, x):
        raise RuntimeError("Dropout is fused into the HIP BatchNorm/ReLU kernel of its parent module")


def check_head_shape(classes, slots, hidden):
    """The head's accepted range, checked by every constructor before anything is allocated: the wide pooling and column-mode
    BatchNorm kernels take up to 1024 classes, the row-mode BatchNorm up to 64 time slots (its period limit), the GEMM wants
    16-byte rows (hidden a multiple of 4)."""
    for name, v in (("classes", classes), ("slots", slots), ("hidden", hidden)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError("%s must be an int, got %r" % (name, v))
    if not 1 <= classes <= 1024:
        raise ValueError("classes must be in 1..1024, got %d" % classes)
    if not 1 <= slots <= 64:
        raise ValueError("slots must be in 1..64, got %d" % slots)
    if hidden < 4 or hidden % 4:
        raise ValueError("hidden must be a multiple of 4 and at least 4, got %d" % hidden)


class Ensemble(nn.Module):
    def __init__(self, input_conf: str, cnn_conf: Dict[str, Union[str, int]], model_conf: List[int], device,
                 precision: str = "f32", trunk_backward: bool = False, classes: int = K, slots: int = T, hidden: int = H,
                 input_grad: bool = False):
        check_head_shape(classes, slots, hidden)
        super().__init__()
        self.classes, self.slots, self.hidden = classes, slots, hidden
        self.cnn_type = cnn_conf["cnn_type"]
        self.just_bottlenecks = cnn_conf["just_bottlenecks"]
        self.num_classes = cnn_conf["num_classes"]
        if self.cnn_type == "vggish" and self.just_bottlenecks:
            self.emb_input_size = M_VGGISH_JB
        elif self.cnn_type == "vggish" and not self.just_bottlenecks:
            self.emb_input_size = M_VGGISH
        elif self.cnn_type == "resnet" and self.just_bottlenecks:
            self.emb_input_size = M_RESNET
        elif self.cnn_type == "resnet" and not self.just_bottlenecks:
            self.emb_input_size = self.num_classes
        else:
            raise Exception("CNN type is not valid.")
        self.input = Input(input_conf=input_conf, cnn_type=self.cnn_type, device=device)
        self.mla = MultiLevelAttention(model_conf, self.emb_input_size, classes=classes, slots=slots, hidden=hidden)
        self.cnn = CNN(**cnn_conf, precision=precision, trunk_backward=trunk_backward, input_grad=input_grad)

    def set_precision(self, precision):
        self.cnn.set_precision(precision)
        return self

    def set_trunk_backward(self, flag):
        self.cnn.set_trunk_backward(flag)
        return self

    def set_input_grad(self, flag):
        """Switch the gradient with respect to the input examples on or off (VGGish branch; default off): while on, an input
        of forward() that requires grad receives its gradient from loss.backward() / torch.autograd.grad. Returns self."""
        self.cnn.set_input_grad(flag)
        return self

    def forward(self, x):
        x_proc = self.input(x)
        features = self.cnn(x_proc)
        out = self.mla(features.reshape(-1, self.slots, self.emb_input_size))
        return out

    def _ten_window_bags(self, what):
        if self.slots != T:
            raise ValueError("%s builds the dataset's bags of %d windows, the model takes slots = %d; feed (B, slots, ...) inputs "
                             "through forward()" % (what, T, self.slots))

    def _waveforms_only_vggish(self):
        if self.cnn_type != "vggish":
            raise NotImplementedError("the waveform paths feed VGGish log-mel examples; cnn_type 'resnet' takes 224 x 224 "
                                      "spectrogram images (dataset.py:175-178 of the reference) through forward(), or 4 s clips "
                                      "of 22 050 Hz PCM through forward_clips()")

    def forward_waveforms(self, pcm):
        """Fused online path of the north star: (B, n_samples) 16 kHz PCM on the device (float32
        or int16), one bag per row with exactly T examples -> (B, K) scores. The front-end writes
        the examples directly in the CNN's compute dtype."""
        self._waveforms_only_vggish()
        from . import frontend
        dtype = torch.bfloat16 if self.cnn.precision == "bf16" else torch.float32
        feats = self.cnn.cnn_model[0] if self.just_bottlenecks else self.cnn.cnn_model.features
        if ops.FUSED_FRONT and dtype == torch.bfloat16 and not differentiable.wants_grad(feats):
            # bf16 inference: front-end + conv1 in one kernel, the examples tensor is never written
            assert pcm.dim() == 2 and frontend.counts(pcm.shape[1])[1] == self.slots, "each waveform must yield exactly T examples"
            features = self.cnn(PcmInput(pcm))
            return self.mla(features.reshape(-1, self.slots, self.emb_input_size))
        ex = frontend.waveforms_to_examples(pcm, out_dtype=dtype)
        assert ex.shape[0] == pcm.shape[0] * self.slots, "each waveform must yield exactly T examples"
        features = self.cnn(ex)
        return self.mla(features.reshape(-1, self.slots, self.emb_input_size))

    def forward_clips(self, pcm, overlap=True):
        """The ResNet branch's wave -> scores entry: (B, SAMPLES_NUM_RESNET) float32 PCM at 22 050 Hz on the device -> the
        (B, T, 1, 224, 224) mel-dB images of dataset.clips_to_images (two HIP kernels) -> forward(). input_conf, precision and
        just_bottlenecks act as in forward()."""
        if self.cnn_type != "resnet":
            raise NotImplementedError("forward_clips feeds the ResNet branch's mel-dB images; cnn_type 'vggish' takes 16 kHz PCM "
                                      "through forward_waveforms(), or 4 s clips of it through forward_clips_librosa()")
        self._ten_window_bags("forward_clips")
        from . import dataset
        return self.forward(dataset.clips_to_images(pcm, overlap))

    def _recordings_only_resnet(self, what):
        if self.cnn_type != "resnet":
            raise NotImplementedError("%s cuts and zero-fills 4 s clips for the ResNet branch; cnn_type 'vggish' does not zero-fill "
                                      "the waveform (its native path pads missing 0.96 s slots of the spectrogram with 0.0): use "
                                      "%s_native(), or forward_waveforms() for 16 kHz PCM; the librosa dataset path, which does "
                                      "zero-fill, is %s_librosa()" % (what, what, what))

    def forward_recordings(self, recordings, rates, overlap=True):
        """The ResNet branch from recordings as they are decoded: a sequence of host arrays, (n,) or (n, channels), int16 or
        floating, of any rates and lengths -> dataset.recordings_to_clips (one HIP launch: channel mean, resampling to 22 050 Hz,
        cut at 4 s, zero fill) -> forward_clips() -> (B, K) scores."""
        self._recordings_only_resnet("forward_recordings")
        self._ten_window_bags("forward_recordings")
        from . import dataset
        return self.forward_clips(dataset.recordings_to_clips(recordings, rates), overlap)

    def forward_wavfiles(self, paths, overlap=True):
        """forward_recordings for 16-bit WAV files (dataset.wavfiles_to_clips)."""
        self._recordings_only_resnet("forward_wavfiles")
        self._ten_window_bags("forward_wavfiles")
        from . import dataset
        return self.forward_clips(dataset.wavfiles_to_clips(paths), overlap)

    def forward_audiofiles(self, paths, overlap=True):
        """forward_recordings for WAV files of any PCM width or IEEE float, mixed in one batch: dataset.audiofiles_to_clips uploads
        the files' bytes and decodes them in the clips launch."""
        self._recordings_only_resnet("forward_audiofiles")
        self._ten_window_bags("forward_audiofiles")
        from . import dataset
        return self.forward_clips(dataset.audiofiles_to_clips(paths), overlap)

    def _native_bags(self, what, frames_fn, source, overlap):
        """The VGGish branch from recordings: the reference's native dataset path (load_hdf5(cnn_type="vggish", use_librosa=False),
        mnemonic vggish_native_10_s) in two launches, the bags written in the CNN's compute dtype, then the CNN and the head as
        forward_waveforms runs them."""
        if self.cnn_type != "vggish":
            raise NotImplementedError("%s builds the VGGish branch's log-mel bags (the reference's native dataset path); cnn_type "
                                      "'resnet' always takes the librosa path (dataset.py:176-178): use %s()"
                                      % (what, what[:-len("_native")]))
        self._ten_window_bags(what)
        if not overlap:
            raise ValueError("%s: overlap=False gives 4 frames per bag, the model takes T = %d; the dataset functions "
                             "(dataset.recordings_to_frames, ...) support it" % (what, T))
        dtype = torch.bfloat16 if self.cnn.precision == "bf16" else torch.float32
        frames = frames_fn(*source, overlap=True, out_dtype=dtype)
        features = self.cnn(frames.view(frames.shape[0] * T, S_VGGISH_SHAPE[0], S_VGGISH_SHAPE[1]))        # Input's reshape (model.py:98-99), not a transpose
        return self.mla(features.reshape(-1, T, self.emb_input_size))

    def forward_recordings_native(self, recordings, rates, overlap=True):
        """The VGGish branch from recordings as they are decoded (host arrays, (n,) or (n, channels), int16 or floating, any rates,
        at most 4 whole 0.96 s examples each) -> dataset.recordings_to_frames -> (B, K) scores."""
        from . import dataset
        return self._native_bags("forward_recordings_native", dataset.recordings_to_frames, (recordings, rates), overlap)

    def forward_wavfiles_native(self, paths, overlap=True):
        """forward_recordings_native for 16-bit WAV files (dataset.wavfiles_to_frames)."""
        from . import dataset
        return self._native_bags("forward_wavfiles_native", dataset.wavfiles_to_frames, (paths,), overlap)

    def forward_audiofiles_native(self, paths, overlap=True):
        """forward_recordings_native for WAV files of any PCM width or IEEE float (dataset.audiofiles_to_frames)."""
        from . import dataset
        return self._native_bags("forward_audiofiles_native", dataset.audiofiles_to_frames, (paths,), overlap)

    def _timeline(self, what, slots_fn, source, hop_slots, max_slots):
        """Recordings of any length scored over time: the distinct slots of all windows in two launches (dataset.recordings_to_slots),
        the CNN once per distinct slot in chunks of at most max_slots, the windows' bags gathered from the embeddings
        (ops.gather_bags), then the head. BatchNorm1d(T) of the head is per slot position, so only the CNN is shared."""
        if self.cnn_type != "vggish":
            raise NotImplementedError("%s scores the VGGish branch's log-mel bags over time; cnn_type 'resnet' has no timeline path: "
                                      "crop 4 s pieces on the host and use forward_recordings(), or score its mel-dB images over time "
                                      "with %s()" % (what, what.replace("score_timeline", "score_image_timeline")))
        self._ten_window_bags(what)
        if self.training:
            raise RuntimeError("%s runs in eval mode only: batch statistics over the windows of one recording are no defined training "
                               "step, and the chunks of max_slots would change them; call eval() first" % what)
        if int(max_slots) < 1:
            raise ValueError("%s: max_slots must be >= 1, got %r" % (what, max_slots))
        dtype = torch.bfloat16 if self.cnn.precision == "bf16" else torch.float32
        slots, first_rows, index, starts = slots_fn(*source, hop_slots=hop_slots, out_dtype=dtype)
        if first_rows.shape[0] == 0:
            return torch.empty((0, self.classes), dtype=torch.float32, device=slots.device), index, starts
        ex = slots.view(slots.shape[0], S_VGGISH_SHAPE[0], S_VGGISH_SHAPE[1])        # Input's reshape (model.py:98-99), not a transpose
        parts = [self.cnn(ex[at:at + int(max_slots)]) for at in range(0, ex.shape[0], int(max_slots))]
        emb = parts[0] if len(parts) == 1 else torch.cat(parts)
        return self.mla(ops.gather_bags(emb, first_rows, T).view(-1, T, self.emb_input_size)), index, starts

    def score_timeline(self, recordings, rates, hop_slots=3, max_slots=8192):
        """The VGGish branch over recordings of ANY length (host arrays, (n,) or (n, channels), int16 or floating, any rates): one
        score vector per window of four 0.96 s examples, the windows hop_slots * 0.32 s apart (dataset.recordings_to_slots states
        which). -> (scores (windows of all recordings, K) on the device, recording_index (int64, host), start_seconds (float64,
        host)), recordings in order and windows in order of time. A recording shorter than one window gives the one row
        forward_recordings_native gives. The CNN runs once per distinct 0.96 s slot, max_slots of them at a time (which bounds its
        activations); eval mode only."""
        from . import dataset
        return self._timeline("score_timeline", dataset.recordings_to_slots, (recordings, rates), hop_slots, max_slots)

    def score_timeline_wavfiles(self, paths, hop_slots=3, max_slots=8192):
        """score_timeline for 16-bit WAV files (dataset.wavfiles_to_slots)."""
        from . import dataset
        return self._timeline("score_timeline_wavfiles", dataset.wavfiles_to_slots, (paths,), hop_slots, max_slots)

    def score_timeline_audiofiles(self, paths, hop_slots=3, max_slots=8192):
        """score_timeline for WAV files of any PCM width or IEEE float (dataset.audiofiles_to_slots)."""
        from . import dataset
        return self._timeline("score_timeline_audiofiles", dataset.audiofiles_to_slots, (paths,), hop_slots, max_slots)

    def _image_timeline(self, what, tracks_fn, source, hop_images, max_images):
        """Recordings of any length scored over time on the ResNet branch: every recording's spectrogram once (dataset.recordings_to_tracks),
        then per chunk of at most max_images DISTINCT images the images launch, Input and the CNN, the windows' bags gathered from the
        embeddings (ops.gather_bags), then the head. BatchNorm1d(T) of the head is per slot position, so only the CNN is shared."""
        if self.cnn_type != "resnet":
            raise NotImplementedError("%s scores the ResNet branch's mel-dB images over time; cnn_type 'vggish' scores its log-mel bags "
                                      "over time with %s()" % (what, what.replace("score_image_timeline", "score_timeline")))
        self._ten_window_bags(what)
        if self.training:
            raise RuntimeError("%s runs in eval mode only: batch statistics over the windows of one recording are no defined training "
                               "step, and the chunks of max_images would change them; call eval() first" % what)
        if int(max_images) < 1:
            raise ValueError("%s: max_images must be >= 1, got %r" % (what, max_images))
        from . import frontend
        track, starts = tracks_fn(*source, hop_images=hop_images)
        if track is None:
            return torch.empty((0, self.classes), dtype=torch.float32, device="cuda" if torch.cuda.is_available() else "cpu"), \
                np.zeros(0, dtype=np.int64), starts
        parts = []
        for at in range(0, track.descriptors.images, int(max_images)):
            chunk = frontend.melspec_track_images(track, at, min(int(max_images), track.descriptors.images - at))
            parts.append(self.cnn(self.input(chunk.view(-1, 1, 1, S_RESNET_SHAPE[0], S_RESNET_SHAPE[1]))))
        emb = parts[0] if len(parts) == 1 else torch.cat(parts)
        return self.mla(ops.gather_bags(emb, track.first_rows, T).view(-1, T, self.emb_input_size)), track.recording_index, starts

    def score_image_timeline(self, recordings, rates, hop_images=3, max_images=256):
        """The ResNet branch over recordings of ANY length (host arrays, (n,) or (n, channels), int16 or floating, any rates): one
        score vector per 4 s window, the windows hop_images / 3 s apart (dataset.recordings_to_track_images states which, and how the
        images differ from cropping 4 s pieces on the host: reflection at the track's ends only, the floor against the track-wide
        maximum). -> (scores (windows of all recordings, classes) on the device, recording_index (int64, host), start_seconds
        (float64, host)), recordings in order and windows in order of time. A recording of at most one window gives the one row
        forward_recordings gives. The spectrogram is computed once and the CNN runs once per DISTINCT image, 3 W + 7 of them for W
        windows at the default hop where cropping needs 10 W, max_images of them at a time: that bounds the image tensor (200 KB
        each) and the trunk's activations; it is a bound on memory, not a tuned value. input_conf, precision and just_bottlenecks
        act as in forward(); eval mode only."""
        from . import dataset
        return self._image_timeline("score_image_timeline", dataset.recordings_to_tracks, (recordings, rates), hop_images, max_images)

    def score_image_timeline_wavfiles(self, paths, hop_images=3, max_images=256):
        """score_image_timeline for 16-bit WAV files (dataset.wavfiles_to_tracks)."""
        from . import dataset
        return self._image_timeline("score_image_timeline_wavfiles", dataset.wavfiles_to_tracks, (paths,), hop_images, max_images)

    def score_image_timeline_audiofiles(self, paths, hop_images=3, max_images=256):
        """score_image_timeline for WAV files of any PCM width or IEEE float (dataset.audiofiles_to_tracks)."""
        from . import dataset
        return self._image_timeline("score_image_timeline_audiofiles", dataset.audiofiles_to_tracks, (paths,), hop_images, max_images)

    def _saliency_target(self, target, bags, device):
        """The `target` argument of the saliency entries -> None (each bag's top class, known after the forward) or (bags,) int64
        class indices on `device`."""
        if target is None:
            return None
        if isinstance(target, int) and not isinstance(target, bool):
            if not 0 <= target < self.classes:
                raise ValueError("target %d is outside the %d classes" % (target, self.classes))
            return torch.full((bags,), target, dtype=torch.long, device=device)
        if torch.is_tensor(target):
            if target.dim() != 1 or target.shape[0] != bags or target.dtype.is_floating_point or target.dtype in (torch.bool, torch.complex64, torch.complex128):
                raise ValueError("target must hold one class index per bag: (%d,) integers, got %s %s" % (bags, tuple(target.shape), target.dtype))
            idx = target.to(device=device, dtype=torch.long)
            if bags and bool(((idx < 0) | (idx >= self.classes)).any()):
                raise ValueError("target holds a class outside the %d classes" % self.classes)
            return idx
        raise ValueError("target must be None, an int or a (B,) integer tensor, got %r" % (target,))

    def saliency(self, x, target=None, times_input=False):
        """Which time-frequency cells made the model say so: x (B, slots, 1, 96, 64) log-mel examples -> (scores (B, classes),
        detached; grad float32 of x's shape = d scores[b, target_b] / d x[b], multiplied by x with times_input). target: None
        (each bag's top class), an int, or a (B,) integer tensor. Eval mode only: the bags are then independent, so ONE backward
        of the sum of the picked scores gives every bag's map. The gradient is taken with respect to x alone
        (torch.autograd.grad): no parameter's .grad, no buffer and no switch of the module is changed, and a frozen conv stack
        launches no weight gradient."""
        if self.cnn_type != "vggish":
            raise NotImplementedError("saliency differentiates the VGGish branch down to its log-mel examples; cnn_type 'resnet' has no "
                                      "input gradient behind autograd: its trunk's backward there exists for train-mode BatchNorm only "
                                      "and its stem has no backward-data step in it; the eval-mode maps of the ResNet branch are "
                                      "saliency_images() / saliency_clips()")
        if self.training:
            raise RuntimeError("saliency runs in eval mode only: batch statistics would couple the bags of a batch (one backward "
                               "could not give per-bag maps) and the running statistics would move; call eval() first")
        if x.dim() != 5 or tuple(x.shape[1:]) != (self.slots, 1) + tuple(S_VGGISH_SHAPE):
            raise ValueError("saliency takes (B, %d, 1, %d, %d) examples, got %s" % ((self.slots,) + tuple(S_VGGISH_SHAPE) + (tuple(x.shape),)))
        idx = self._saliency_target(target, x.shape[0], x.device)
        feats = self.cnn.cnn_model[0] if self.just_bottlenecks else self.cnn.cnn_model.features
        xg = x.detach().requires_grad_(True)
        was = feats.input_grad
        feats.input_grad = True
        try:
            with torch.enable_grad():
                scores = self.forward(xg)
                if idx is None:
                    idx = scores.detach().argmax(dim=1)
                grad, = torch.autograd.grad(scores.gather(1, idx.view(-1, 1)).sum(), [xg])
        finally:
            feats.input_grad = was
        grad = grad.float()
        if times_input:
            grad = grad * x.detach().float()
        return scores.detach(), grad

    def saliency_waveforms(self, pcm, target=None, times_input=False):
        """saliency from (B, n_samples) 16 kHz PCM on the device, one bag of `slots` examples per row: the front-end of
        forward_waveforms (float32 examples), then saliency -> (scores, examples (B, slots, 1, 96, 64), grad): the map is plotted
        over the examples."""
        self._waveforms_only_vggish()
        from . import frontend
        ex = frontend.waveforms_to_examples(pcm, out_dtype=torch.float32)
        assert ex.shape[0] == pcm.shape[0] * self.slots, "each waveform must yield exactly T examples"
        ex = ex.view(pcm.shape[0], self.slots, 1, S_VGGISH_SHAPE[0], S_VGGISH_SHAPE[1])
        scores, grad = self.saliency(ex, target, times_input)
        return scores, ex, grad

    def waveform_saliency(self, pcm, target=None, times_input=False):
        """Which SAMPLES made the model say so: (B, n_samples) 16 kHz PCM on the device (float32, or int16 meaning pcm / 32768), one
        bag of `slots` examples per row -> (scores (B, classes), detached; grad (B, n_samples) float32 = d scores[b, target_b] /
        d pcm[b], multiplied by the float waveform with times_input). It is saliency_waveforms' map over the float32 examples carried
        one link further by the log-mel backward kernel (frontend.waveforms_to_examples_backward, which also states how the
        gradient is conditioned); scores, target and the eval-mode / VGGish-only rules are saliency's. No parameter's .grad, no
        buffer and no switch of the module is changed. The ResNet branch's counterpart is clip_saliency()."""
        self._waveforms_only_vggish()
        if self.training:
            raise RuntimeError("waveform_saliency runs in eval mode only, as saliency does: batch statistics would couple the bags of a "
                               "batch; call eval() first")
        from . import frontend
        scores, _, grad = self.saliency_waveforms(pcm, target, False)
        grad = frontend.waveforms_to_examples_backward(pcm, grad.reshape(-1, S_VGGISH_SHAPE[0], S_VGGISH_SHAPE[1]))
        if times_input:
            grad = grad * (pcm.float() / 32768.0 if pcm.dtype == torch.int16 else pcm.float())
        return scores, grad

    def saliency_images(self, x, target=None, times_input=False):
        """saliency for the ResNet branch: x (B, slots, 1, 224, 224) spectrogram images -> (scores (B, classes), detached; grad
        float32 of x's shape = d scores[b, target_b] / d x[b], multiplied by x with times_input). target as in saliency(). Eval mode
        only, for saliency()'s reason. The trunk runs its eval-mode forward with a tape and is walked back by hand
        (resnet.trunk_input_backward: the reverse walk trunk_backward uses, with BatchNorm as the folded per-channel constant it is
        in eval mode, the stem's backward-data kernel last); only the head (and the fc of just_bottlenecks=False) sits behind autograd, differentiated with respect to the
        features alone. No parameter's .grad, no buffer and no switch of the module is changed, whatever requires grad; no weight
        gradient is launched. The tape holds every activation of the batch: the caller splits large batches."""
        if self.cnn_type != "resnet":
            raise NotImplementedError("saliency_images differentiates the ResNet branch down to its 224 x 224 images; cnn_type 'vggish' "
                                      "takes log-mel examples through saliency(), or 16 kHz PCM through saliency_waveforms()")
        if self.training:
            raise RuntimeError("saliency_images runs in eval mode only: batch statistics would couple the bags of a batch (one backward "
                               "could not give per-bag maps) and the running statistics would move; call eval() first")
        if x.dim() != 5 or tuple(x.shape[1:]) != (self.slots, 1) + tuple(S_RESNET_SHAPE):
            raise ValueError("saliency_images takes (B, %d, 1, %d, %d) images, got %s" % ((self.slots,) + tuple(S_RESNET_SHAPE) + (tuple(x.shape),)))
        idx = self._saliency_target(target, x.shape[0], x.device)
        cnn_model = self.cnn.cnn_model
        tape = {}
        with torch.no_grad():
            feats = resnet.trunk_forward(cnn_model, self.input(x), self.cnn.precision, False, self.cnn._rn_cache, tape=tape)
        leaf = feats.detach().requires_grad_(True)
        with torch.enable_grad():
            emb = leaf if self.just_bottlenecks else differentiable.FcFn.apply(leaf, cnn_model.fc.weight, cnn_model.fc.bias)
            scores = self.mla(emb.reshape(-1, self.slots, self.emb_input_size))
            if idx is None:
                idx = scores.detach().argmax(dim=1)
            d_feats, = torch.autograd.grad(scores.gather(1, idx.view(-1, 1)).sum(), [leaf])
        grad = resnet.trunk_input_backward(cnn_model, tape, d_feats.float().contiguous()).view(x.shape)
        if times_input:
            grad = grad * x.detach().float()
        return scores.detach(), grad

    def saliency_clips(self, pcm, target=None, times_input=False, overlap=True):
        """saliency_images from (B, SAMPLES_NUM_RESNET) float32 PCM at 22 050 Hz on the device: the mel-dB images of
        forward_clips (dataset.clips_to_images), then saliency_images -> (scores, images (B, T, 1, 224, 224), grad): the map is
        plotted over the images."""
        if self.cnn_type != "resnet":
            raise NotImplementedError("saliency_clips feeds the ResNet branch's mel-dB images; cnn_type 'vggish' takes log-mel examples "
                                      "through saliency(), or 16 kHz PCM through saliency_waveforms()")
        self._ten_window_bags("saliency_clips")
        from . import dataset
        images = dataset.clips_to_images(pcm, overlap)
        scores, grad = self.saliency_images(images, target, times_input)
        return scores, images, grad

    def clip_saliency(self, pcm, target=None, times_input=False, overlap=True, floor_grad=True):
        """Which SAMPLES made the ResNet branch say so: (B, SAMPLES_NUM_RESNET) float32 PCM at 22 050 Hz on the device -> (scores
        (B, classes), detached; grad (B, SAMPLES_NUM_RESNET) float32 = d scores[b, target_b] / d pcm[b], multiplied by the waveform
        with times_input). It is saliency_clips' map over the mel-dB images carried one link further by the mel-dB backward kernels
        (dataset.clips_to_images_backward; floor_grad=False treats power_to_db's top_db floor as a constant instead of passing its
        gradient to the clip's loudest cell). scores, target and the eval-mode / ResNet-only rules are saliency_images'; the
        front-end and its backward are float32 in every precision mode. No parameter's .grad, no buffer and no switch of the
        module is changed."""
        if self.cnn_type != "resnet":
            raise NotImplementedError("clip_saliency differentiates the ResNet branch down to its 22 050 Hz clips; cnn_type 'vggish' takes "
                                      "16 kHz PCM through waveform_saliency()")
        if self.training:
            raise RuntimeError("clip_saliency runs in eval mode only, as saliency_images does: batch statistics would couple the bags of a "
                               "batch; call eval() first")
        from . import dataset
        scores, _, grad = self.saliency_clips(pcm, target, False, overlap)
        grad = dataset.clips_to_images_backward(pcm, grad, overlap, floor_grad)
        if times_input:
            grad = grad * pcm.float()
        return scores, grad

    def _librosa_bags(self, what, frames_fn, source, overlap):
        """The VGGish branch on the reference's librosa dataset path (load_hdf5(cnn_type="vggish", use_librosa=True), mnemonic
        vggish_10_s): HTK mel-dB bags written in the CNN's compute dtype, then the CNN and the head as _native_bags runs them."""
        if self.cnn_type != "vggish":
            raise NotImplementedError("%s builds the VGGish branch's HTK mel-dB bags (64 bands, unpadded frames); cnn_type 'resnet' "
                                      "takes librosa's default spectrogram: use %s()" % (what, what[:-len("_librosa")]))
        self._ten_window_bags(what)
        if not overlap:
            raise ValueError("%s: overlap=False is not defined on the VGGish librosa path (388 columns do not split into whole "
                             "96-column frames; the reference's split refuses it)" % what)
        dtype = torch.bfloat16 if self.cnn.precision == "bf16" else torch.float32
        frames = frames_fn(*source, out_dtype=dtype)
        features = self.cnn(frames.view(frames.shape[0] * T, S_VGGISH_SHAPE[0], S_VGGISH_SHAPE[1]))        # Input's reshape (model.py:98-99), not a transpose
        return self.mla(features.reshape(-1, T, self.emb_input_size))

    def forward_clips_librosa(self, pcm, overlap=True):
        """The VGGish branch's wave -> scores entry on the librosa path: (B, 64 000) float32 PCM at 16 kHz on the device ->
        dataset.clips_to_frames_librosa (two HIP kernels) -> (B, K) scores."""
        from . import dataset
        return self._librosa_bags("forward_clips_librosa", dataset.clips_to_frames_librosa, (pcm,), overlap)

    def forward_recordings_librosa(self, recordings, rates, overlap=True):
        """forward_clips_librosa from recordings as they are decoded (host arrays, (n,) or (n, channels), int16 or floating, any
        rates and lengths): dataset.recordings_to_frames_librosa cuts at 4 s and zero-fills."""
        from . import dataset
        return self._librosa_bags("forward_recordings_librosa", dataset.recordings_to_frames_librosa, (recordings, rates), overlap)

    def forward_wavfiles_librosa(self, paths, overlap=True):
        """forward_recordings_librosa for 16-bit WAV files (dataset.wavfiles_to_frames_librosa)."""
        from . import dataset
        return self._librosa_bags("forward_wavfiles_librosa", dataset.wavfiles_to_frames_librosa, (paths,), overlap)

    def forward_audiofiles_librosa(self, paths, overlap=True):
        """forward_recordings_librosa for WAV files of any PCM width or IEEE float (dataset.audiofiles_to_frames_librosa)."""
        from . import dataset
        return self._librosa_bags("forward_audiofiles_librosa", dataset.audiofiles_to_frames_librosa, (paths,), overlap)

    def stream_waveforms(self, host_batches):
        """Host-resident PCM: iterate over (B, n_samples) float32 / int16 tensors in PINNED host memory and yield the
        (B, K) scores of each. The copy of batch i+1 runs on its own HIP stream while batch i computes (two device
        buffers), so a steady stream is bound by max(copy, compute), not their sum. Scores are yielded after the batch's
        compute has been enqueued; they are ordinary tensors on the current stream."""
        self._waveforms_only_vggish()
        dev = next(self.parameters()).device
        cur = torch.cuda.current_stream(dev)
        copy = torch.cuda.Stream(device=dev)
        it = iter(host_batches)

        def upload(host):
            assert host.is_pinned(), "stream_waveforms overlaps asynchronous copies: the host tensors must be pinned"
            with torch.cuda.stream(copy):
                d = host.to(dev, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy)
            return d, ev

        nxt = next(it, None)
        pending = upload(nxt) if nxt is not None else None
        while pending is not None:
            d, ev = pending
            nxt = next(it, None)
            pending = upload(nxt) if nxt is not None else None      # in flight while `d` computes
            cur.wait_event(ev)
            out = self.forward_waveforms(d)
            d.record_stream(cur)                                     # the caching allocator must not recycle `d` early
            yield out

    def capture_waveforms(self, pcm):
        """Capture forward_waveforms for inputs shaped like `pcm` into a HIP graph (eval mode only) and return a
        callable that replays it: ~45 kernel launches per step become one graph launch, which is what small
        batches (about 1 000 clips, where a step is ~1.5 ms of GPU work) need."""
        self._waveforms_only_vggish()
        return GraphedWaveforms(self, pcm)


class GraphedWaveforms:
    """forward_waveforms of an eval-mode Ensemble captured once into a HIP graph. The C-ABI kernels are plain
    launches on torch's current stream, so torch's capture records them; scratch tensors allocated while
    capturing live in the graph's private pool. Call with a tensor of the captured shape/dtype.

    The recorded kernels also address memory the capture did not allocate: the cached weight copies (repacked / bf16) and the
    library's scratch buffers. Those tensors are kept in ``held`` for as long as this object lives, so their addresses stay the
    graph's even after the cache or ``ops`` has moved on to newer ones; a grown scratch buffer therefore changes nothing. What
    would make a replay compute something else than ``forward_waveforms`` does now -- weights changed in place or re-seated
    (load_state_dict), set_precision, a train() switch -- is compared on the host before every replay and raises RuntimeError:
    the output buffer is static, so the caller has to capture again. ``captures`` counts the graphs recorded (always 1)."""

    def __init__(self, model, pcm):
        assert not model.training, "graph capture covers the eval-mode forward (train-mode statistics sync with the host)"
        self.model = model
        self.captures = 0
        self.static_in = pcm.clone()
        side = torch.cuda.Stream(device=pcm.device)
        side.wait_stream(torch.cuda.current_stream(pcm.device))
        with torch.cuda.stream(side), torch.no_grad():       # weight repacks / caches / workspaces are built here
            for _ in range(2):
                model.forward_waveforms(self.static_in)
        torch.cuda.current_stream(pcm.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode="relaxed"), torch.no_grad():
            self.static_out = model.forward_waveforms(self.static_in)
        self.captures += 1
        self.stamp = self._stamp()
        self.held = [t for c in weight_caches(model.cnn) for t in c.tensors()] + list(ops.scratch(pcm.device).values())

    def _stamp(self):
        m = self.model
        return {"train / eval mode": m.training, "precision": m.cnn.precision,
                "CNN weights (written in place or re-seated, e.g. by load_state_dict)": cache_stamp(weight_caches(m.cnn))}

    def __call__(self, pcm):
        now = self._stamp()
        if now != self.stamp:
            raise RuntimeError("the captured forward_waveforms graph no longer matches the model: %s changed since the capture; "
                               "call capture_waveforms() again" % ", ".join(k for k in now if now[k] != self.stamp[k]))
        if pcm.data_ptr() != self.static_in.data_ptr():
            assert pcm.shape == self.static_in.shape and pcm.dtype == self.static_in.dtype
            self.static_in.copy_(pcm, non_blocking=True)
        self.graph.replay()
        return self.static_out


class Input(nn.Module):
    def __init__(self, input_conf, cnn_type, device):
        super().__init__()
        self.conf, self.device, self.cnn_type = input_conf, device, cnn_type

    def forward(self, x):
        if self.cnn_type == "vggish":
            return x.reshape((-1, 1, S_VGGISH_SHAPE[0], S_VGGISH_SHAPE[1]))
        elif self.cnn_type == "resnet":
            # model.py:84-99: repeat / single channels, ImageNet normalisation and the (-1, 3, 224, 224) reshape all happen in
            # the stem kernel, which needs the raw planes (the conv's zero padding applies to the normalised channels)
            if self.conf not in ("repeat", "single"):
                raise Exception("Invalid input type")
            if x.dim() != 5 or x.shape[2] != 1 or tuple(x.shape[3:]) != S_RESNET_SHAPE:
                raise ValueError("cnn_type 'resnet' takes (B, T, 1, %d, %d) inputs, got %s" % (S_RESNET_SHAPE + (tuple(x.shape),)))
            planes = x.detach().reshape(-1, S_RESNET_SHAPE[0], S_RESNET_SHAPE[1])
            if planes.dtype != torch.float32 or not planes.is_contiguous():
                planes = planes.float().contiguous()
            return resnet.StemInput(planes, self.conf == "single")
        else:
            raise Exception("CNN type is not valid.")


class CNN(nn.Module):
    def __init__(self, cnn_type="vggish", num_classes=10, use_pretrained=True, just_bottlenecks=False,
                 cnn_trainable=False, first_cnn_layer_trainable=False, in_channels=3, precision="f32", trunk_backward=False,
                 input_grad=False):
        super().__init__()
        self.precision = precision
        # cnn_type="resnet": gradients into the trunk (cnn_trainable / first_cnn_layer_trainable, model.py:131-136) run on the
        # HIP trunk backward only when this is on; while off, a trunk parameter that requires grad raises. No-op for VGGish.
        self.trunk_backward = bool(trunk_backward)
        if cnn_type == "vggish":
            model_urls = {"vggish": "https://github.com/harritaylor/torchvggish/releases/download/v0.1/vggish-10086976.pth"}
            self.cnn_model = VGGish(urls=model_urls, pretrained=use_pretrained, preprocess=False, postprocess=False,
                                    progress=True, precision=precision)
            if not cnn_trainable:
                set_requires_grad(self.cnn_model, False)
            if just_bottlenecks:
                self.cnn_model = nn.Sequential(list(self.cnn_model.children())[0], CnnFlatten(cnn_type))
        elif cnn_type == "resnet":
            if precision not in ("f32", "bf16"):
                raise NotImplementedError("cnn_type 'resnet' runs in precision 'f32' or 'bf16', not %r" % precision)
            self.cnn_model = resnet.resnet50(pretrained=use_pretrained)
            if not cnn_trainable:
                set_requires_grad(self.cnn_model, False)
            if first_cnn_layer_trainable:
                if in_channels == 3:
                    set_requires_grad(self.cnn_model.conv1, True)
                else:
                    self.cnn_model.conv1 = resnet.Conv2d(in_channels, 64, 7, stride=2, padding=3)
            if just_bottlenecks:
                modules = list(self.cnn_model.children())[:-1]       # model.py:142-146: drop fc, flatten
                modules.append(CnnFlatten(cnn_type))
                self.cnn_model = nn.Sequential(*modules)
            else:
                self.cnn_model.fc = resnet.Linear(self.cnn_model.fc.in_features, num_classes)   # after the freeze: trainable
            self._rn_cache = resnet.new_cache()
        else:
            raise Exception("Invalid CNN model name specified.")
        self.cnn_type = cnn_type
        self.just_bottlenecks = just_bottlenecks
        self.set_input_grad(input_grad)

    def set_precision(self, precision):
        if self.cnn_type == "resnet" and precision not in ("f32", "bf16"):
            raise NotImplementedError("cnn_type 'resnet' runs in precision 'f32' or 'bf16', not %r" % precision)
        self.precision = precision
        for m in self.cnn_model.modules():
            if hasattr(m, "precision"):
                m.precision = precision
        return self

    def set_trunk_backward(self, flag):
        """Turn the HIP backward of the ResNet-50 trunk on or off (models built by the reference's own constructor call or by
        load_model); returns self. No effect for cnn_type="vggish", whose finetuning always runs."""
        self.trunk_backward = bool(flag)
        return self

    def set_input_grad(self, flag):
        """Switch the gradient with respect to the input examples on or off (VGGFeatures.set_input_grad; default off); returns
        self. cnn_type="resnet" has none behind autograd (Ensemble.saliency_images walks its eval-mode trunk by hand)."""
        if self.cnn_type == "resnet":
            if flag:
                raise NotImplementedError("cnn_type 'resnet' has no input gradient behind autograd: the trunk's backward there exists "
                                          "for train-mode BatchNorm only and the stem has no backward-data step in it; eval-mode maps: "
                                          "Ensemble.saliency_images()")
            return self
        feats = self.cnn_model[0] if self.just_bottlenecks else self.cnn_model.features
        feats.set_input_grad(flag)
        return self

    def forward(self, x):
        if self.cnn_type == "resnet":
            if self.trunk_backward and torch.is_grad_enabled() and resnet.trunk_requires_grad(self.cnn_model):
                if not self.training:
                    raise NotImplementedError("the ResNet trunk backward differentiates the train-mode forward (batch statistics); "
                                              "run eval-mode forwards under torch.no_grad() as _evaluate / test_model do")
                params = [p for _, p in resnet.trunk_params(self.cnn_model)]
                feats = differentiable.TrunkFn.apply(self.cnn_model, x, self.precision, self._rn_cache, *params)
            else:
                feats = resnet.trunk_forward(self.cnn_model, x, self.precision, self.training, self._rn_cache)
            return feats if self.just_bottlenecks else resnet.fc_forward(self.cnn_model.fc, feats)
        x = self.cnn_model(x)
        if x.dtype == torch.bfloat16:      # bf16 bottlenecks (just_bottlenecks=True) feed the f32 head
            if x.requires_grad:
                return differentiable.CastFn.apply(x)
            x = ops.merge_split(x.contiguous(), 512) if self.precision == "bf16x3" else ops.to_f32(x.contiguous())
        return x


class CnnFlatten(nn.Module):
    def __init__(self, cnn_type):
        super().__init__()
        self.cnn_type = cnn_type

    def forward(self, x):
        if self.cnn_type == "resnet":
            x = torch.flatten(x, 1)
        elif self.cnn_type == "vggish":
            x = torch.transpose(x, 1, 3)
            x = torch.transpose(x, 1, 2)
            x = x.contiguous()           # no copy: VGGFeatures returns an NCHW view of NHWC memory
            x = x.view(x.size(0), -1)
        else:
            raise Exception("Invalid CNN model name specified.")
        return x


class EmbeddedMapping(nn.Module):
    def __init__(self, n_fc, is_first, emb_input_size, *, slots=T, hidden=H):
        check_head_shape(1, slots, hidden)
        super().__init__()
        self.n_fc, self.slots, self.hidden = n_fc, slots, hidden
        self.norm0 = BatchNorm1d(slots)
        if is_first:
            self.fc = nn.ModuleList([Linear(emb_input_size, hidden)] + [Linear(hidden, hidden) for _ in range(n_fc - 1)])
        else:
            self.fc = nn.ModuleList([Linear(hidden, hidden) for _ in range(n_fc)])
        self.dropouts = nn.ModuleList([Dropout(p=DR) for _ in range(n_fc)])
        self.norms = nn.ModuleList([BatchNorm1d(slots) for _ in range(n_fc)])

    def forward(self, x):
        return mla_train.embedded_mapping_forward(self, x, None)


class AttentionModule(nn.Module):
    def __init__(self, *, classes=K, slots=T, hidden=H):
        check_head_shape(classes, slots, hidden)
        super().__init__()
        self.classes, self.slots, self.hidden = classes, slots, hidden
        self.fcv = Linear(hidden, classes)
        self.fcf = Linear(hidden, classes)          # never used by forward (model.py:237-238); kept for the state_dict
        self.normv = BatchNorm1d(slots)
        self.normf = BatchNorm1d(slots)

    def forward(self, h):
        y = torch.empty((h.shape[0], self.classes), dtype=torch.float32, device=h.device)
        mla_train.attention_forward(self, h, y, None)
        return y


class MultiLevelAttention(nn.Module):
    def __init__(self, model_conf, emb_input_size, *, classes=K, slots=T, hidden=H):
        check_head_shape(classes, slots, hidden)
        super().__init__()
        self.model = model_conf
        self.classes, self.slots, self.hidden = classes, slots, hidden
        shape = dict(slots=slots, hidden=hidden)
        self.embedded_mappings = nn.ModuleList(
            [EmbeddedMapping(model_conf[0], is_first=True, emb_input_size=emb_input_size, **shape)] +
            [EmbeddedMapping(n_layers, is_first=False, emb_input_size=emb_input_size, **shape) for n_layers in model_conf[1:]])
        self.attention_modules = nn.ModuleList([AttentionModule(classes=classes, **shape) for _ in model_conf])
        self.fc = Linear(len(model_conf) * classes, classes)
        self.norm = BatchNorm1d(classes)

    def forward(self, x):
        if differentiable.wants_grad(self, x):
            # train.py:124-138 on the drop-in: outputs = clf(inputs); loss.backward() -- the head's HIP backward runs behind autograd,
            # in train mode (batch statistics, dropout) and in eval mode (running statistics) alike
            return differentiable.HeadFn.apply(self, x.float(), *self.parameters())
        return mla_train.mla_apply(self, x)


def set_requires_grad(model, value):
    for param in model.parameters():
        param.requires_grad = value
