"""Settles the constants that DESIGN 8.1 lists as assumed from memory of sox (the `tempo` music profile 82 / 14.68 / 12 ms, the
linear cross-fade, pitch = tempo then rate): where pysox and the sox binary are installed, real sox and pitch_shift_signal shift the
same seeded signal and must agree in what two implementations with different resampling filters and search details can agree in.
Skipped where sox is absent (it is on neither the build machine nor the GPU machine of this project)."""
import shutil

import numpy as np
import pytest
import torch

import pitch_restated as R

sox = pytest.importorskip("sox")


def _envelope(y, sr):
    w = int(0.02 * sr)
    k = len(y) // w
    return np.sqrt((y[: k * w].reshape(k, w).astype(np.float64) ** 2).mean(1))


@pytest.mark.parametrize("semitones", [2, -3])
def test_real_sox_agrees_on_pitch_and_envelope(dev, semitones):
    if shutil.which("sox") is None:
        pytest.skip("the sox binary is not on PATH")
    from aicovergen_amd import cover
    sr = 44100
    x = R.stems(10.0, sr, 2, 71)
    t = np.arange(x.shape[1]) / sr
    x = (0.6 * x + 0.3 * np.sin(2 * np.pi * 440.0 * t)[None, :]).astype(np.float32)
    tfm = sox.Transformer()
    tfm.pitch(semitones)
    want = np.asarray(tfm.build_array(input_array=np.ascontiguousarray(x.T), sample_rate_in=sr), np.float64).T
    got, offs = cover.pitch_shift_signal(dev.t(torch.from_numpy(x)), sr, semitones)
    got = got.cpu().numpy()
    n = min(want.shape[1], got.shape[1])
    nwin = 65536
    mid = n // 2
    f = np.fft.rfftfreq(nwin, 1.0 / sr)
    band = (f > 440.0 * 2 ** (semitones / 12.0) * 0.9) & (f < 440.0 * 2 ** (semitones / 12.0) * 1.1)
    peaks = []
    for y in (want[0, :n], got[0, :n]):
        sp = np.abs(np.fft.rfft(y[mid - nwin // 2: mid + nwin // 2] * np.hanning(nwin)))
        peaks.append(float(f[band][np.argmax(sp[band])]))
    corr = float(np.corrcoef(_envelope(want[0, :n], sr), _envelope(got[0, :n], sr))[0, 1])
    print("N %+d: tone peak sox %.2f Hz, device %.2f Hz; 20 ms envelope correlation %.4f; %d WSOLA steps, mean offset %.1f frames"
          % (semitones, peaks[0], peaks[1], corr, offs.numel(), float(offs.float().mean())))
    assert abs(peaks[0] - peaks[1]) <= sr / nwin
    assert abs(peaks[1] - 440.0 * 2 ** (semitones / 12.0)) <= sr / nwin
    # both follow the input's slow envelope (0.7 Hz): the correlation of the 20 ms RMS envelopes is recorded above; a wrong segment
    # or overlap length would still pass 0.9, a wrong stretch factor (envelope drifting by seconds) would not
    assert corr >= 0.9
