"""Songs and outputs at any sample rate without a host pass: audio_io.load_device against audio_io.load_wav, a 48 kHz song through
the one-call cover and through the file-by-file route (the comparisons of tests/test_cover_pipeline.py, run on that song), and
VC.pipeline's resample_sr branch on the device against the host computation it replaces."""
import filecmp
import math
import os
import struct
import types

import numpy as np
import pytest
import torch
from scipy import signal
from scipy.io import wavfile

import test_cover_pipeline as tcp
from aicovergen_amd import audio_io, cover, ops
from aicovergen_amd.vc_infer_pipeline import VC, change_rms
from synthetic import weights
from synthetic.inputs import song_like, vocal_like
from test_cover_pipeline import world      # noqa: F401  (the module's fixture: model directories, one session, the 44.1 kHz song's cover)
from test_pipeline import GOLD, build, noise_fn_for
from test_resample_mc import d32


def _write_song(path, sr, channels, seconds=3.0, seed=9):
    x = song_like(seconds, sr, seed=seed).astype(np.float32) * 0.6
    audio_io.write_wav_pcm16(path, (x if channels == 2 else x[:1]).T, sr)
    return path


def _write_pcm24(path, sr, x, junk=b""):
    """(C, n) float -> a 24-bit PCM WAV file (3-byte containers, what a DAW exports), optionally with a JUNK chunk in front of fmt."""
    q = np.ascontiguousarray(np.clip(np.rint(x.T.astype(np.float64) * 2 ** 23), -2 ** 23, 2 ** 23 - 1), dtype="<i4")
    body = q.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    c = x.shape[0]
    chunks = b""
    if junk:
        chunks += b"JUNK" + struct.pack("<I", len(junk)) + junk + b"\0" * (len(junk) & 1)
    chunks += b"fmt " + struct.pack("<IHHIIHH", 16, 1, c, sr, sr * c * 3, c * 3, 24) + b"data" + struct.pack("<I", len(body)) + body
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)
    return path


class _Launches:
    """Counts the resample kernel's launches through ops._call."""

    def __init__(self, monkeypatch):
        self.n, real = 0, ops._call

        def call(name, *a):
            self.n += name == "aicg_resample_poly_mc"
            return real(name, *a)
        monkeypatch.setattr(ops, "_call", call)


@pytest.mark.parametrize("sr,channels", [(48000, 2), (22050, 1)])
def test_loader_parity(dev, tmp_path, monkeypatch, sr, channels):
    path = _write_song(str(tmp_path / "in.wav"), sr, channels)
    want, want_sr = audio_io.load_wav(path, 44100, mono=False)
    count = _Launches(monkeypatch)
    got = audio_io.load_device(path, 44100, dev.device)
    assert count.n == 1 and want_sr == 44100
    assert got.dtype == torch.float32 and got.device.type == dev.device.type and tuple(got.shape) == want.shape == (channels, math.ceil(3 * sr * 44100 / sr))
    dist = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print("load_device vs load_wav at %d Hz: %.3e (4 d32 = %.3e)" % (sr, dist, 4 * d32()))
    assert 0 < dist <= 4 * d32()


def test_loader_at_the_requested_rate_is_exact_and_launches_nothing(dev, tmp_path, monkeypatch):
    path = _write_song(str(tmp_path / "in.wav"), 44100, 2, seconds=1.0)
    count = _Launches(monkeypatch)
    got = audio_io.load_device(path, 44100, dev.device)
    assert count.n == 0 and np.array_equal(got.cpu().numpy(), audio_io.load_wav(path, 44100, mono=False)[0])
    assert audio_io.wav_rate(path) == 44100 and audio_io.wav_rate(__file__) is None


def test_float_wav_and_other_encodings_go_through_to_float(dev, tmp_path):
    x = (song_like(0.5, 32000, seed=3).astype(np.float32) * 0.5).T
    for name, data in (("f32.wav", x), ("i32.wav", np.rint(x.astype(np.float64) * 2 ** 30).astype(np.int32)),
                       ("u8.wav", np.rint(x * 100 + 128).astype(np.uint8)), ("i24.wav", None)):
        path = str(tmp_path / name)
        wavfile.write(path, 32000, data) if data is not None else _write_pcm24(path, 32000, x.T)
        want = audio_io.load_wav(path, 44100, mono=False)[0]
        got = audio_io.load_device(path, 44100, dev.device).cpu().numpy()
        assert got.shape == want.shape and np.abs(got - want).max() <= 4 * d32(), name


def test_wav_rate_reads_the_header_whatever_the_encoding(tmp_path):
    """The rate that decides between the loaders comes from the fmt chunk alone: every encoding scipy reads (24-bit PCM, which it
    cannot map, among them), chunks in front of fmt, nothing for a file that is no WAVE file."""
    x = (song_like(0.05, 48000, seed=4).astype(np.float32) * 0.5)
    for name, sr, data in (("i16.wav", 22050, np.rint(x.T * 32767).astype(np.int16)), ("f32.wav", 96000, x.T), ("f64.wav", 8000, x.T.astype(np.float64)),
                           ("u8.wav", 11025, np.rint(x.T * 100 + 128).astype(np.uint8)), ("i24.wav", 48000, None), ("i24_junk.wav", 88200, None)):
        path = str(tmp_path / name)
        wavfile.write(path, sr, data) if data is not None else _write_pcm24(path, sr, x, junk=b"abc" if "junk" in name else b"")
        assert audio_io.wav_rate(path) == wavfile.read(path)[0] == sr, name
    assert wavfile.read(str(tmp_path / "i24.wav"))[1].dtype == np.int32
    for name, content in (("empty.wav", b""), ("riff_only.wav", b"RIFF\x04\0\0\0WAVE"), ("other.wav", b"RIFF\x04\0\0\0AVI "), ("cut.wav", b"RIFF\x10\0\0\0WAVEfmt \x10\0\0\0\x01\0")):
        (tmp_path / name).write_bytes(content)
        assert audio_io.wav_rate(str(tmp_path / name)) is None, name
    assert audio_io.wav_rate(__file__) is None and audio_io.wav_rate(str(tmp_path)) is None and audio_io.wav_rate(str(tmp_path / "absent.wav")) is None


def test_24_bit_48k_song_takes_the_device_loader_in_both_routes(world, tmp_path, monkeypatch):
    """A 24-bit 48 kHz file (the usual DAW export) through CoverSession._separate and through run_mdx: each reads it with
    audio_io.load_device, once, neither with load_wav, and the stems of the first model are the same bytes."""
    from aicovergen_amd import mdx
    w = world
    song = _write_pcm24(str(tmp_path / "daw.wav"), 48000, song_like(1.0, 48000, seed=11).astype(np.float32) * 0.6)
    device, host = [], []
    real_device, real_host = audio_io.load_device, audio_io.load_wav
    monkeypatch.setattr(audio_io, "load_device", lambda *a, **k: device.append(a[0]) or real_device(*a, **k))
    monkeypatch.setattr(audio_io, "load_wav", lambda *a, **k: host.append(a[0]) or real_host(*a, **k))
    one_call, direct = str(tmp_path / "one_call"), str(tmp_path / "direct")
    os.makedirs(one_call)
    os.makedirs(direct)
    fetch = cover._Fetch(w.kind == "hip")
    w.session._separate(song, one_call, True, fetch)
    fetch.flush()
    assert device == [song] and song not in host
    mdx.run_mdx(w.params, direct, os.path.join(w.mdx_dir, cover.MDX_MODEL_FILES[0]), song, denoise=True, keep_orig=True)
    assert device == [song, song] and song not in host
    for name in ("daw_Vocals.wav", "daw_Instrumental.wav"):
        assert filecmp.cmp(os.path.join(one_call, name), os.path.join(direct, name), shallow=False), name
    sr, stem = wavfile.read(os.path.join(direct, "daw_Vocals.wav"))
    assert sr == 44100 and stem.shape == (44100, 2) and np.abs(stem).max() > 30


@pytest.fixture(scope="module")
def song48(world, tmp_path_factory):
    """A 1.5 s song as a 48 kHz file of the fixture song's name, its keep_files=True cover through the session, and how often each
    route took the device loader."""
    w = world
    tmp = str(tmp_path_factory.mktemp("rate48_" + w.kind))
    song = _write_song(os.path.join(tmp, "song.wav"), 48000, 2, seconds=1.5)
    calls, real = [], audio_io.load_device
    audio_io.load_device = lambda *a, **k: calls.append(a[0]) or real(*a, **k)
    w.session.output_dir = os.path.join(tmp, "song_output")
    os.makedirs(w.session.output_dir)
    try:
        path = w.session.song_cover_pipeline(song, "Voice", 0, True, **tcp.KW)
        one_call = len(calls)
        w48 = types.SimpleNamespace(**dict(vars(w), tmp=tmp, song=song, cover=path, dir=os.path.dirname(path), out_dir=w.session.output_dir))
        yield w48, calls, one_call
    finally:
        audio_io.load_device = real
        w.session.output_dir = w.out_dir


def test_48k_song_one_call_equals_file_by_file(song48):
    """Every file of the 48 kHz song's cover, byte for byte, against run_mdx x 3 / VC.pipeline / the file functions: the
    comparisons of tests/test_cover_pipeline.py.  Both routes read the song through audio_io.load_device, once each."""
    w48, calls, one_call = song48
    assert one_call == 1 and calls == [w48.song]
    tcp.test_1_separation_stems_equal_three_chained_run_mdx(w48)
    assert calls == [w48.song, w48.song]           # run_mdx on the song; the stem files it chains through are 44.1 kHz: load_wav
    tcp.test_2_ai_vocals_equal_a_separate_pipeline_call(w48)
    tcp.test_3_effects_pitch_shift_and_mix_equal_the_file_functions(w48)
    sr, stem = wavfile.read(os.path.join(w48.dir, tcp.STEMS[0]))
    assert sr == 44100 and stem.shape == (66150, 2)


def test_44k_song_is_untouched_and_resample_sr_reaches_the_conversion(world, tmp_path, monkeypatch):
    """The 44.1 kHz song: no route takes the device loader, and a session made with resample_sr=0 leaves the files of one made without
    the argument (the module fixture's), which are the files of the file-by-file route (load_wav, untouched).  Then the same
    session with resample_sr=16000: the song's cached part is reused as it is (the rate acts behind the voice-independent front), the
    AI vocals come out at 16 kHz."""
    from aicovergen_amd import mdx
    w = world
    calls, real = [], audio_io.load_device
    monkeypatch.setattr(audio_io, "load_device", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    s = cover.CoverSession(w.mdx_dir, w.rvc_dir, str(tmp_path / "out"), resample_sr=0)
    path = s.song_cover_pipeline(w.song, "Voice", 0, True, **tcp.KW)
    d = os.path.dirname(path)
    files = tcp._chain(w, w.song, str(tmp_path / "direct"))
    assert calls == [] and sorted(os.listdir(d)) == sorted(os.listdir(w.dir))
    for name in os.listdir(w.dir):
        assert filecmp.cmp(os.path.join(w.dir, name), os.path.join(d, name), shallow=False), name
    for f in files:
        assert filecmp.cmp(f, os.path.join(w.dir, os.path.basename(f)), shallow=False), f

    os.remove(path)
    os.remove(os.path.join(d, tcp.VOCALS))
    separations, fronts = [], []
    real_mdx, real_front = mdx.run_mdx_device, VC.front
    monkeypatch.setattr(mdx, "run_mdx_device", lambda *a, **k: separations.append(1) or real_mdx(*a, **k))
    monkeypatch.setattr(VC, "front", lambda *a, **k: fronts.append(1) or real_front(*a, **k))
    s.resample_sr = 16000
    assert s.song_cover_pipeline(w.song, "Voice", 0, False, **tcp.KW) == path
    assert separations == [] and fronts == []
    sr, got = wavfile.read(os.path.join(d, tcp.VOCALS))
    sr0, base = wavfile.read(os.path.join(w.dir, tcp.VOCALS))
    assert (sr0, sr) == (8000, 16000) and got.dtype == np.int16 and len(got) == 2 * len(base) and np.abs(got).max() > 100
    assert wavfile.read(path)[0] == 44100
    assert vars(cover.build_parser().parse_args(["-i", "a", "-dir", "V", "-p", "0", "-osr", "48000"]))["resample_sr"] == 48000


def test_pipeline_resample_sr_stays_on_the_device(dev, monkeypatch):
    """VC.pipeline(resample_sr=32000, device_out=True) on the 2.6 s fixture: an int16 device tensor of ceil(n 32000 / tgt_sr) samples,
    no Tensor.cpu() inside _post, and the samples of the host branch this replaces (change_rms and scipy's resample_poly in numpy,
    computed here from the float track of the resample_sr=0 call): one more fp32 rounding in front of the truncating int16 cast,
    the project's bound for that -- <= 1 LSB on >= 99.9 % of the samples, never more than 3."""
    gold = np.load(os.path.join(GOLD, "pipeline_small_resample32k.npz"))
    nets = weights.small_model_set(int(gold["seed"][0]))
    audio = vocal_like(float(gold["seconds"][0]), 16000, int(gold["seed"][0]) + 5)
    vc, hub, net_g, tgt_sr = build(dev, nets)
    resample_sr, seen, real_post, real_cpu = int(gold["resample_sr"][0]), {}, vc._post, torch.Tensor.cpu

    def post(audio_opt, audio16k, *a, **k):
        seen["track"], seen["audio"] = real_cpu(audio_opt).numpy().copy(), real_cpu(audio16k).numpy().copy()
        seen["cpu_calls"] = 0

        def cpu(t, *aa, **kk):
            seen["cpu_calls"] += 1
            return real_cpu(t, *aa, **kk)
        with monkeypatch.context() as m:
            m.setattr(torch.Tensor, "cpu", cpu)
            return real_post(audio_opt, audio16k, *a, **k)
    vc._post = post
    args = (hub, net_g, 0, audio, "x.wav", [0, 0, 0], 0, "rmvpe", "", 0.5, 1, 3, tgt_sr)
    tail = (0.25, "v2", 0.33, 128)
    base = vc.pipeline(*args, 0, *tail, noise_fn=noise_fn_for(nets))
    track, audio16k = seen["track"], seen["audio"]
    out = vc.pipeline(*args, resample_sr, *tail, noise_fn=noise_fn_for(nets), device_out=True)
    assert seen["cpu_calls"] == 0
    assert isinstance(out, torch.Tensor) and out.dtype == torch.int16 and out.device.type == dev.device.type
    assert out.shape == (math.ceil(len(base) * resample_sr / tgt_sr),) == gold["audio"].shape

    # the host branch as it stood (reference :639-651 in numpy)
    a = change_rms(audio16k, 16000, track, tgt_sr, 0.25)
    g = math.gcd(tgt_sr, resample_sr)
    a = signal.resample_poly(a, resample_sr // g, tgt_sr // g).astype(np.float32)
    audio_max = float(np.abs(a).max()) / 0.99
    want = (a * (32768 / audio_max if audio_max > 1 else 32768)).astype(np.int16)
    diff = np.abs(out.cpu().numpy().astype(np.int32) - want.astype(np.int32))
    print("resample_sr on the device vs the host branch: max %d LSB, %.5f within 1 LSB, %.5f equal" % (diff.max(), (diff <= 1).mean(), (diff == 0).mean()))
    assert diff.max() <= 3 and (diff <= 1).mean() >= 0.999
