"""Pins aicovergen_amd.cover against the libraries the reference's add_audio_effects and combine_audio call (src/main.py:206-233),
where they are installed: pedalboard's HighpassFilter -> Compressor(ratio=4, threshold_db=-15) -> Reverb on a seeded 10 s input,
and pydub's gain / overlay chain.  Settles the pedalboard details DESIGN 9 lists as assumed (parameter smoothing at the first
block, denormal handling): after the first 10 ms, at least 99.9 % of the samples within one 16-bit step."""
import os

import numpy as np
import pytest
import torch

pedalboard = pytest.importorskip("pedalboard")
pydub = pytest.importorskip("pydub")

from aicovergen_amd import cover  # noqa: E402


def _vocals(sr, seconds=10.0, seed=17):
    rng = np.random.default_rng(seed)
    n = int(sr * seconds)
    t = np.arange(n) / sr
    x = 0.5 * np.sin(2 * np.pi * 196 * t) * (0.2 + 0.8 * np.sin(2 * np.pi * 0.5 * t) ** 2) + 0.08 * rng.standard_normal(n)
    return np.clip(x, -1, 1).astype(np.float32).reshape(1, -1)


def test_effects_within_one_lsb_of_pedalboard(dev):
    sr = 40000
    x = _vocals(sr)
    board = pedalboard.Pedalboard([pedalboard.HighpassFilter(), pedalboard.Compressor(ratio=4, threshold_db=-15),
                                   pedalboard.Reverb(room_size=0.15, dry_level=0.8, wet_level=0.2, damping=0.7)])
    want = np.concatenate([board(x[:, i:i + sr], sr, reset=False) for i in range(0, x.shape[1], sr)], axis=1)
    got, _ = cover.vocal_effects(dev.t(torch.from_numpy(x)), sr, 0.15, 0.2, 0.8, 0.7)
    dev.sync()
    got = got.cpu().numpy()
    skip = round(0.01 * sr)
    lsb = np.abs(got[:, skip:].astype(np.float64) - want[:, skip:]) * 32767.0
    assert np.mean(lsb <= 1.0) >= 0.999, np.quantile(lsb, [0.5, 0.999, 1.0])


def test_mix_byte_identical_to_pydub(dev, tmp_path):
    from scipy.io import wavfile
    rng = np.random.default_rng(3)
    paths = []
    for name, sr, ch in (("v", 40000, 1), ("b", 44100, 2), ("i", 44100, 2)):
        d = np.clip(rng.standard_normal((sr * 10, ch)) * 6000, -32768, 32767).astype(np.int16)
        p = str(tmp_path / (name + ".wav"))
        wavfile.write(p, sr, d[:, 0] if ch == 1 else d)
        paths.append(p)
    ref = str(tmp_path / "pydub.wav")
    AS = pydub.AudioSegment
    (AS.from_wav(paths[0]) - 4 + 1).overlay(AS.from_wav(paths[1]) - 6 - 2).overlay(AS.from_wav(paths[2]) - 7 + 0.5).export(
        ref, format="wav")
    out = str(tmp_path / "cover.wav")
    cover.combine_audio(paths, out, 1, -2, 0.5, "wav")
    assert open(out, "rb").read() == open(ref, "rb").read()
    assert os.path.getsize(out) > 44
