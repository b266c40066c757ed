"""The three-stem mix of combine_audio (reference src/main.py:229-233) on the device: aicovergen_amd.cover.mix_stems against the
same composition written with the stdlib audioop calls pydub makes (apply_gain = audioop.mul, _sync = audioop.tostereo +
audioop.ratecv, overlay = a millisecond-length slice of the first operand + audioop.add).  16-bit PCM, byte for byte."""
import audioop
import os
import wave

import numpy as np
import pytest
import torch

from aicovergen_amd import cover


# ---- pydub's arithmetic, restated on audioop ---------------------------------------------------------
class Seg:
    def __init__(self, data, channels, rate):
        self.data, self.channels, self.rate = data, channels, rate

    @staticmethod
    def of(arr, rate):
        arr = arr if arr.ndim == 2 else arr[:, None]
        return Seg(arr.astype("<i2").tobytes(), arr.shape[1], rate)

    def gain(self, db):                                            # AudioSegment.apply_gain
        return Seg(audioop.mul(self.data, 2, 10 ** (float(db) / 20)), self.channels, self.rate)

    def converted(self, channels, rate):                           # set_channels, then set_frame_rate
        s = self
        if s.channels == 1 and channels == 2:
            s = Seg(audioop.tostereo(s.data, 2, 1, 1), 2, s.rate)
        if s.rate != rate and s.data:
            s = Seg(audioop.ratecv(s.data, 2, s.channels, s.rate, rate, None)[0], s.channels, rate)
        return Seg(s.data, s.channels, rate)

    def overlay(self, other):
        ch, rate = max(self.channels, other.channels), max(self.rate, other.rate)
        a, b = self.converted(ch, rate), other.converted(ch, rate)
        fw = 2 * ch
        n = len(a.data) // fw
        keep = int(round(1000 * (n / rate)) * (rate / 1000.0))    # seg1[position:] slices in whole milliseconds
        d = a.data[: keep * fw]
        d += b"\0" * (keep * fw - len(d))
        bd = b.data[: len(d)]
        return Seg(audioop.add(d[: len(bd)], bd, 2) + d[len(bd):], ch, rate)


def ref_mix(main, msr, backup, bsr, inst, isr, mg, bg, ig):
    m = Seg.of(main, msr).gain(-4).gain(mg)
    b = Seg.of(backup, bsr).gain(-6).gain(bg)
    i = Seg.of(inst, isr).gain(-7).gain(ig)
    out = m.overlay(b).overlay(i)
    return np.frombuffer(out.data, "<i2").reshape(-1, out.channels), out.rate


def _pcm(seconds, rate, channels, seed, amp=0.5):
    rng = np.random.default_rng(seed)
    n = int(round(seconds * rate))
    t = np.arange(n) / rate
    x = np.stack([amp * np.sin(2 * np.pi * (300 + 50 * c) * t) + 0.2 * amp * rng.standard_normal(n) for c in range(channels)], 1)
    return np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)


def _mix(dev, main, msr, backup, bsr, inst, isr, mg, bg, ig):
    t = lambda a: dev.t(torch.from_numpy(np.ascontiguousarray(a)))
    out, sr = cover.mix_stems(t(main), msr, t(backup), bsr, t(inst), isr, mg, bg, ig)
    dev.sync()
    return out.cpu().numpy(), sr


CASES = {
    # name: (vocals (s, rate, ch), backup, inst, gains)
    "40k_mono_vocals_44k1_stereo_stems": ((1.0, 40000, 1), (1.0, 44100, 2), (1.0, 44100, 2), (0, 0, 0)),
    "48k_vocals": ((0.9, 48000, 1), (0.9, 44100, 2), (0.9, 44100, 2), (0, 0, 0)),
    "32k_vocals": ((0.9, 32000, 1), (0.9, 44100, 2), (0.9, 44100, 2), (2, -3, 1)),
    "vocals_longer": ((1.3, 40000, 1), (0.7, 44100, 2), (1.0, 44100, 2), (0, 0, 0)),
    "vocals_shorter": ((0.4, 40000, 1), (1.1, 44100, 2), (0.8, 44100, 2), (0, 0, 0)),
    "saturating_gains": ((0.6, 40000, 1), (0.6, 44100, 2), (0.6, 44100, 2), (12, 9, 10)),
    "non_integer_gains": ((0.6, 40000, 1), (0.6, 44100, 2), (0.6, 44100, 2), (1.7, -2.35, 0.4)),
    "mono_stems_upmixed_late": ((0.5, 40000, 1), (0.5, 40000, 1), (0.5, 44100, 2), (0, 0, 0)),
    "odd_rates": ((0.37, 22051, 2), (0.41, 16000, 1), (0.3, 11025, 1), (-1, 3, 0.5)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_mix_stems_byte_identical_to_audioop(dev, name):
    (vs, vr, vc), (bs, br, bc), (is_, ir, ic), (mg, bg, ig) = CASES[name]
    main, backup, inst = _pcm(vs, vr, vc, 1, 0.8), _pcm(bs, br, bc, 2), _pcm(is_, ir, ic, 3)
    got, sr = _mix(dev, main, vr, backup, br, inst, ir, mg, bg, ig)
    want, wsr = ref_mix(main, vr, backup, br, inst, ir, mg, bg, ig)
    assert sr == wsr and got.shape == want.shape
    assert got.tobytes() == want.tobytes()
    if name == "saturating_gains":
        assert (np.abs(got.astype(np.int32)) >= 32767).sum() > 100


def test_mix_with_an_empty_stem(dev):
    main, inst = _pcm(0.3, 40000, 1, 4), _pcm(0.3, 44100, 2, 5)
    empty = np.zeros((0, 2), np.int16)
    got, sr = _mix(dev, main, 40000, empty, 44100, inst, 44100, 0, 0, 0)
    want, wsr = ref_mix(main, 40000, empty, 44100, inst, 44100, 0, 0, 0)
    assert sr == wsr and got.tobytes() == want.tobytes()
    got, _ = _mix(dev, np.zeros((0, 1), np.int16), 40000, inst, 44100, inst, 44100, 0, 0, 0)
    assert got.shape == (0, 2)


def test_combine_audio_writes_what_pydub_exports(dev, tmp_path):
    from scipy.io import wavfile
    paths = []
    for name, (s, r, c), seed in (("v", (0.5, 40000, 1), 6), ("b", (0.5, 44100, 2), 7), ("i", (0.5, 44100, 2), 8)):
        p = str(tmp_path / (name + ".wav"))
        wavfile.write(p, r, _pcm(s, r, c, seed)[:, 0] if c == 1 else _pcm(s, r, c, seed))
        paths.append(p)
    out = str(tmp_path / "cover.wav")
    cover.combine_audio(paths, out, 1, -1, 0, "wav")
    stems = [wavfile.read(p) for p in paths]
    want, sr = ref_mix(stems[0][1], stems[0][0], stems[1][1], stems[1][0], stems[2][1], stems[2][0], 1, -1, 0)
    with wave.open(out, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (2, 2, sr, want.shape[0])
        assert w.readframes(w.getnframes()) == want.tobytes()
    if not __import__("shutil").which("ffmpeg"):
        with pytest.raises(RuntimeError, match="ffmpeg"):
            cover.combine_audio(paths, str(tmp_path / "cover.mp3"), 0, 0, 0, "mp3")
        assert not os.path.exists(str(tmp_path / "cover.mp3"))


def test_bad_mix_arguments(dev):
    from aicovergen_amd import _lib
    lib = _lib.get()
    a = dev.t(torch.zeros(16, 1, dtype=torch.int16))
    out = dev.t(torch.zeros(16, 2, dtype=torch.int16))
    assert lib.aicg_pcm16_mix(a.data_ptr(), 1, 0, 16, 1.0, 1.0, a.data_ptr(), 1, 44100, 16, 1.0, 1.0, out.data_ptr(), 16, 0) == -2
    assert lib.aicg_pcm16_mix(a.data_ptr(), 1, 40000, 16, 1.0, 1.0, None, 1, 44100, 16, 1.0, 1.0, out.data_ptr(), 16, 0) == -2
    assert lib.aicg_pcm16_mix(a.data_ptr(), 3, 40000, 16, 1.0, 1.0, a.data_ptr(), 1, 44100, 16, 1.0, 1.0, out.data_ptr(), 16, 0) == -1
    with pytest.raises(TypeError):
        cover.mix_stems(a.float(), 40000, a, 40000, a, 40000, 0, 0, 0)


@pytest.mark.gpu
def test_240s_mix_byte_identical_on_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import conftest
    conftest._bind("hip")
    main, backup, inst = _pcm(240, 40000, 1, 21, 0.8), _pcm(240, 44100, 2, 22), _pcm(240, 44100, 2, 23)
    c = lambda a: torch.from_numpy(a).cuda()
    got, sr = cover.mix_stems(c(main), 40000, c(backup), 44100, c(inst), 44100, 0, 0, 0)
    want, wsr = ref_mix(main, 40000, backup, 44100, inst, 44100, 0, 0, 0)
    assert sr == wsr and got.cpu().numpy().tobytes() == want.tobytes()
