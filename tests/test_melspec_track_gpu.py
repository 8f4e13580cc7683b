"""The ResNet branch's image timeline on the GPU (melspec_track_* in csrc/melspec.hip, dataset.recordings_to_track_images,
Ensemble.score_image_timeline) on the ragged batch of tests/test_melspec_track_cpu.py: the tracks against the float64 restatement
(tests/librosa_restated.py) at test_melspec_cpu.py's (REL, FLOOR), and bit for bit: interior columns against the 4 s crops, the
images against the floored gather of the kernel's own D, one window against the crop route, batch and chunk invariance, what lies
behind a track's end. The deviation from cropping on the host is pinned, and the scores are the head's on the gathered bags."""

import importlib
import wave

import numpy as np
import pytest
import torch

import librosa_restated as R
from conftest import PKG
from test_melspec_cpu import FLOOR, REL, SR
from test_melspec_track_cpu import BATCH, HOP, IMAGE_STEP, IMAGE_W, MELS, Q, STEP, WINDOW, kept_images

pytestmark = pytest.mark.gpu

CONF = dict(cnn_type="resnet", num_classes=10, use_pretrained=False, just_bottlenecks=True, cnn_trainable=False,
            first_cnn_layer_trainable=False, in_channels=3)


@pytest.fixture(scope="module")
def fe():
    return importlib.import_module(PKG + ".frontend")


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module(PKG + ".dataset")


@pytest.fixture(scope="module")
def ops():
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def recs():
    return [R.waveform(name, n) for name, n in BATCH]


@pytest.fixture(scope="module")
def made(ds, fe, recs):
    """The batch once: its clips rows, its Track, all of its images and the windows' start seconds. Nothing below writes to them."""
    lengths = [len(x) for x in recs]
    clips = ds.recordings_to_clips(recs, SR, SR, max(lengths))
    track, starts = ds.recordings_to_tracks(recs, SR, Q)
    images = fe.melspec_track_images(track, 0, track.descriptors.images)
    return clips, track, images, starts


def blocks(track):
    """[(224, C_r) view of D_r] per recording."""
    return [track.db[off:off + MELS * C].view(MELS, C) for _, C, _, off, _, _ in track.descriptors.host.tolist()]


def test_batch_layout(made):
    clips, track, images, starts = made
    d = track.descriptors
    assert d.windows.tolist() == [4, 1, 1, 2] and d.host[:, 1].tolist() == [1576, 901, 901, 1126] and d.images == 52
    assert tuple(images.shape) == (52, 1, 224, 224) and images.dtype == torch.float32 and tuple(clips.shape) == (4, 154350)
    assert track.first_rows.tolist() == [0, 3, 6, 9, 19, 29, 39, 42] and track.recording_index.tolist() == [0, 0, 0, 0, 1, 2, 3, 3]
    assert starts.tolist() == [0.0, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 1.0] and starts.dtype == np.float64


def test_tracks_match_restatement(made, recs):
    _, track, _, _ = made
    for i, Dr in enumerate(blocks(track)):
        L_ = int(track.descriptors.host[i, 0])
        x = np.zeros(L_, dtype=np.float32)
        x[:min(len(recs[i]), L_)] = recs[i][:L_]
        D = Dr.cpu().numpy()
        assert np.isfinite(D).all() and float(track.maxima[i]) == D.max()
        ok, ratio = R.power_close(R.db_to_power(D), R.mel_power(x, SR, MELS, HOP), REL, FLOOR)
        print("%s, %d samples: worst error / bound %.3f" % (BATCH[i][0], BATCH[i][1], ratio))
        assert ok, (BATCH[i], ratio)


def test_interior_columns_are_the_crops_bits(made, fe):
    clips, track, _, _ = made
    d = track.descriptors
    crops = torch.stack([clips[r, STEP * Q * j:STEP * Q * j + WINDOW] for r in range(4) for j in range(d.windows[r])])
    D, _ = fe.melspec_db_unclipped(crops, SR, MELS, HOP)
    assert tuple(D.shape) == (8, MELS, 901)
    w = 0
    for r, Dr in enumerate(blocks(track)):
        for j in range(d.windows[r]):
            at = IMAGE_STEP * Q * j
            assert torch.equal(D[w][:, 11:890], Dr[:, at + 11:at + 890]), (r, j)
            w += 1
    # a track of one window is the crop itself, edges included
    assert torch.equal(D[4], blocks(track)[1]) and torch.equal(D[5], blocks(track)[2])


def test_images_are_the_floored_gather(made):
    _, track, images, _ = made
    d = track.descriptors
    for r, Dr in enumerate(blocks(track)):
        floored = torch.maximum(Dr, Dr.max() - 80.0)
        first = int(d.host[r, 4])
        for k, u in enumerate(kept_images(int(d.windows[r]), Q)):
            assert torch.equal(images[first + k, 0], floored[:, IMAGE_STEP * u:IMAGE_STEP * u + IMAGE_W]), (r, u)
    burst = images[:19]
    on_floor = float((burst == blocks(track)[0].max() - 80.0).float().mean())
    assert 0.10 <= on_floor <= 0.90, on_floor


def test_one_window_is_the_crop_route(made, ds, recs):
    _, track, images, _ = made
    want = ds.clips_to_images(ds.recordings_to_clips(recs[1:3], SR))
    for i, r in enumerate((1, 2)):
        first = int(track.descriptors.host[r, 4])
        assert torch.equal(images[first:first + 10], want[i]), r


def test_rows_do_not_depend_on_the_batch(made, ds, fe, recs):
    _, track, images, _ = made
    d = track.descriptors
    rev, _ = ds.recordings_to_tracks(recs[::-1], SR, Q)
    rev_images = fe.melspec_track_images(rev, 0, rev.descriptors.images)
    for r in range(4):
        alone, _ = ds.recordings_to_tracks(recs[r:r + 1], SR, Q)
        alone_images = fe.melspec_track_images(alone, 0, alone.descriptors.images)
        first, n = int(d.host[r, 4]), alone.descriptors.images
        assert torch.equal(alone.db, blocks(track)[r].reshape(-1)) and torch.equal(alone.maxima, track.maxima[r:r + 1]), r
        assert torch.equal(alone_images, images[first:first + n]), r
        at = int(rev.descriptors.host[3 - r, 4])
        assert torch.equal(blocks(rev)[3 - r], blocks(track)[r]) and torch.equal(rev_images[at:at + n], images[first:first + n]), r


def test_nothing_behind_a_track_is_read(made, fe):
    clips, track, images, _ = made
    wide = torch.full((4, clips.shape[1] + 1000), float("nan"), device="cuda")
    for r in range(4):
        L_ = int(track.descriptors.host[r, 0])
        wide[r, :L_] = clips[r, :L_]
    again = fe.melspec_track_db(wide, [n for _, n in BATCH], Q)
    assert torch.equal(again.db, track.db) and torch.equal(again.maxima, track.maxima)
    view = fe.melspec_track_db(wide[:, :clips.shape[1]], [n for _, n in BATCH], Q)        # rows with a stride of their own
    assert torch.equal(view.db, track.db)


def test_images_in_chunks(made, fe):
    _, track, images, _ = made
    parts = [fe.melspec_track_images(track, at, min(7, 52 - at)) for at in range(0, 52, 7)]
    assert [p.shape[0] for p in parts] == [7] * 7 + [3] and torch.equal(torch.cat(parts), images)
    with pytest.raises(ValueError, match="leave the 52 kept images"):
        fe.melspec_track_images(track, 50, 3)


def test_deviation_from_host_crops_is_what_the_definition_says(made, ds, fe):
    """burst, 154 350 samples, q = 3: the burst at sample 51 450 lies outside window 3, which starts at 66 150. The crop route floors
    that window against its own, much lower maximum and reflects at its ends: the images differ (test_melspec_track_cpu.py asserts on
    the restatement that the track's floor cuts through 10..90 % of it), the unclipped interior columns do not."""
    clips, track, images, _ = made
    crop = clips[0:1, 3 * Q * STEP:3 * Q * STEP + WINDOW].contiguous()
    by_crop = ds.clips_to_images(crop)[0]
    ours = images[int(track.first_rows[3]):int(track.first_rows[3]) + 10]
    assert not torch.equal(ours, by_crop)
    D0 = blocks(track)[0]
    Dc, _ = fe.melspec_db_unclipped(crop, SR, MELS, HOP)
    assert torch.equal(Dc[0][:, 11:890], D0[:, 675 + 11:675 + 890])
    assert float(Dc[0].max()) < float(D0.max()) - 3.0
    assert not torch.equal(Dc[0][:, :11], D0[:, 675:675 + 11])          # the crop reflects at sample 66 150, the track does not
    assert torch.equal(Dc[0][:, 890:], D0[:, 675 + 890:])               # window 3 ends where the track ends: the same reflection
    # where neither floor is active and no frame reads reflected samples, the two routes' images are the same bits
    both = (ours > D0.max() - 80.0) & (by_crop > Dc[0].max() - 80.0)
    both[0, :, :, :11] = False
    both[9, :, :, 890 - 675:] = False
    assert bool(both.any()) and torch.equal(ours[both], by_crop[both])


def test_nan_sample_stays_in_its_recording(made, ds, fe, recs):
    _, track, images, _ = made
    bad = [x.copy() for x in recs]
    bad[3][1000] = np.nan
    t, _ = ds.recordings_to_tracks(bad, SR, Q)
    got = fe.melspec_track_images(t, 0, 52)
    assert bool(torch.isnan(t.maxima[3])) and bool(torch.isnan(got[39:]).all())
    assert torch.equal(got[:39], images[:39]) and torch.equal(t.maxima[:3], track.maxima[:3])


def test_launch_count(ds, ops, recs):
    saved = ops.profile
    try:
        for batch in (recs, recs[2:3]):
            ops.profile = []
            ds.recordings_to_track_images(batch, SR, Q)
            names = [p[0] for p in ops.profile]
            assert names[0] == "clips_prepare" and len(names) <= 4 and names[1:] == ["melspec_track_db", "melspec_track_images"]
    finally:
        ops.profile = saved


def ensemble(ds, input_conf, precision):
    """test_melspec_gpu.py's test_forward_clips model: seeded weights, the head's running statistics moved to dB images by thirty
    train-mode passes over two other clips."""
    M = importlib.import_module(PKG + ".model")
    W = importlib.import_module(PKG + ".weights")
    ens = M.Ensemble(input_conf, CONF, [2, 1], torch.device("cuda"), precision=precision)
    sd = W.make_state_dict(11, W.ensemble_shapes((2, 1), True, cnn_type="resnet"))
    ens.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    ens.cuda()
    calib = ds.clips_to_images(torch.from_numpy(np.stack([R.waveform("noise", WINDOW), R.waveform("tones", WINDOW)])).cuda())
    ens.train()
    with torch.no_grad():
        for _ in range(30):
            ens(calib)
    return ens.eval()


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_trunk_embeddings_do_not_depend_on_the_batch(made, ds, precision):
    """What makes the score identities below bit-exact: rn_conv_kernel has no split-K and one K order per output pixel, and eval
    BatchNorm is a folded constant. 19 images as one batch, in chunks of 7 and one at a time."""
    _, _, images, _ = made
    ens = ensemble(ds, "repeat", precision)
    x = images[:19].view(-1, 1, 1, 224, 224)
    with torch.no_grad():
        whole = ens.cnn(ens.input(x))
        chunks = torch.cat([ens.cnn(ens.input(x[at:at + 7])) for at in range(0, 19, 7)])
        single = torch.cat([ens.cnn(ens.input(x[at:at + 1])) for at in range(19)])
    assert tuple(whole.shape) == (19, 2048) and bool(torch.isfinite(whole).all())
    assert torch.equal(whole, chunks) and torch.equal(whole, single)


def write_wav16(path, pcm):
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(SR)
        wf.writeframes(pcm.tobytes())
    return str(path)


@pytest.mark.parametrize("input_conf", ["repeat", "single"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_score_image_timeline(made, ds, recs, tmp_path, input_conf, precision):
    _, track, images, starts = made
    ens = ensemble(ds, input_conf, precision)
    idx = torch.from_numpy(track.first_rows)[:, None] + torch.arange(10)
    with torch.no_grad():
        scores, index, seconds = ens.score_image_timeline(recs, SR, hop_images=Q)
        want = ens(images[idx.cuda()])
        chunked, _, _ = ens.score_image_timeline(recs, SR, hop_images=Q, max_images=7)
        one = ens.forward_recordings(recs[1:3], SR)
    assert tuple(scores.shape) == (8, 10) and bool(torch.isfinite(scores).all())
    assert index.tolist() == [0, 0, 0, 0, 1, 2, 3, 3] and seconds.tolist() == starts.tolist() == [0.0, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 1.0]
    assert torch.equal(scores, want)
    assert torch.equal(chunked, scores)
    assert torch.equal(scores[4:6], one)
    # files: the int16 form of two of the recordings through the recordings entry and through both file entries
    pcm16 = [np.round(recs[r] * 32767.0).astype(np.int16) for r in (3, 2)]
    paths = [write_wav16(tmp_path / ("%d.wav" % i), x) for i, x in enumerate(pcm16)]
    with torch.no_grad():
        from_arrays, index, seconds = ens.score_image_timeline(pcm16, SR, hop_images=Q)
        for entry in (ens.score_image_timeline_wavfiles, ens.score_image_timeline_audiofiles):
            got, i2, s2 = entry(paths, hop_images=Q)
            assert torch.equal(got, from_arrays) and i2.tolist() == index.tolist() == [0, 0, 1] and s2.tolist() == seconds.tolist() == [0.0, 1.0, 0.0]
    assert tuple(from_arrays.shape) == (3, 10) and bool(torch.isfinite(from_arrays).all())
