"""pitch_shift on the device (csrc/pitch.hip, aicovergen_amd.cover.pitch_shift_signal) against the float64 restatement of its
definition in tests/pitch_restated.py: the WSOLA offsets obey the tie model, the arithmetic matches with the offsets
injected, the resampler matches the exact filter to the table's resolution, the filter meets the target derived from 16-bit output,
and the end-to-end properties of a pitch shift hold.  Every parity test exists on the emulator and, marked gpu, on the MI355X."""
import numpy as np
import pytest
import torch

import conftest
import pitch_restated as R
from aicovergen_amd import cover, ops

SEMITONES = (-12, -5, -1, 1, 2, 7, 12)


def _ratio(n):
    return 2.0 ** (n / 12.0)


def _tie_model(dev, seconds, sr, channels, semitones, seed):
    x = R.stems(seconds, sr, channels, seed)
    f = 1.0 / _ratio(semitones)
    y, offs = ops.tempo_wsola(dev.t(torch.from_numpy(x)), sr, f)
    offs = offs.cpu().numpy()
    ref = R.wsola(x, sr, f, offsets=offs)
    g = ref["geom"]
    assert tuple(ops.tempo_wsola_geometry(sr, f, x.shape[1])) == (g["seg"], g["search"], g["ovl"], g["skip"], g["steps"], g["n_out"])
    assert offs.shape == (g["steps"],) and offs[0] == 0 and offs.min() >= 0 and offs.max() < g["search"]
    eps = R.tie_eps(g["ovl"], channels)
    differ = float(np.mean(offs[1:] != ref["argmin"][1:]))
    excess = ref["chosen"][1:] / np.maximum(ref["best"][1:], 1e-300) - 1.0
    msg = "%d steps, %.2f %% choose another offset than the float64 argmin, worst cost excess %.3g (eps %.3g)" % (
        g["steps"], 100 * differ, excess.max(), eps)
    print(msg)
    assert np.all(ref["chosen"][1:] <= ref["best"][1:] * (1.0 + eps)), msg
    return y


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("semitones", [2, -3])
def test_offsets_obey_the_tie_model(dev, channels, semitones):
    """Free search on the device; the float64 restatement walks along the device's offsets: at every step the offset taken costs at
    most the float64 minimum times 1 + 2 (ovl C + 3) 2^-24."""
    seconds, sr = (6.0, 44100) if dev.big else (1.5, 8000)
    _tie_model(dev, seconds, sr, channels, semitones, 11 + channels)


@pytest.mark.gpu
def test_offsets_obey_the_tie_model_on_a_240_s_stereo_stem():
    conftest._bind("hip")
    _tie_model(conftest.Dev("hip"), 240.0, 44100, 2, 2, 21)
    torch.cuda.synchronize()


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("semitones", [2, -3])
def test_arithmetic_with_offsets_injected(dev, channels, semitones):
    """The offsets of an independent float64 run are injected, so no near-tie can move a segment.  Frames copied from the input are
    bit-identical.  A cross-faded frame is fl(fl(o fl(1 - a)) + fl(x a)) with a = fl(fl(1 / ovl) j): a carries 2 u, 1 - a at most
    2 u absolute, each product one more u, the sum one u of at most max(|o|, |x|): 6 u max(|o|, |x|) to first order (u = 2^-24)."""
    seconds, sr = (3.0, 44100) if dev.big else (1.5, 8000)
    x = R.stems(seconds, sr, channels, 31 + channels)
    f = 1.0 / _ratio(semitones)
    ref = R.wsola(x, sr, f)
    inj = torch.from_numpy(ref["offsets"].astype(np.int32))
    y, used = ops.tempo_wsola(dev.t(torch.from_numpy(x)), sr, f, dev.t(inj))
    y = y.cpu().numpy()
    assert np.array_equal(used.cpu().numpy(), ref["offsets"])
    assert y.shape == ref["y"].shape
    cp = ref["copied"]
    assert np.array_equal(y[:, cp], ref["y"][:, cp].astype(np.float32)), "copied frames must be the input's bits"
    err = np.abs(y[:, ~cp].astype(np.float64) - ref["y"][:, ~cp])
    bound = 6.0 * R.U * (1.0 + 1e-6) * ref["scale"][:, ~cp]
    worst = float((err / np.maximum(ref["scale"][:, ~cp], 1e-30)).max() / R.U)
    print("cross-fade: worst error %.2f u of the larger operand" % worst)
    assert np.all(err <= bound), "worst %.2f u" % worst


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("semitones", SEMITONES)
def test_resampler_against_the_exact_filter(dev, channels, semitones):
    """Device (float32 table, linear interpolation between 1024 phases, float64 sums) against the float64 evaluation of the same
    filter definition: the float output within the bound that follows from the table (pitch_restated.table_error_bound) plus the
    output's own float32 rounding; as 16-bit PCM no sample differs by more than one step."""
    seconds, sr = (1.0, 44100) if dev.big else (0.4, 8000)
    x = R.stems(seconds, sr, channels, 41 + channels)
    d = _ratio(semitones)
    n_out = int(round(x.shape[1] / d))
    y = ops.resample_ratio(dev.t(torch.from_numpy(x)), d, n_out).cpu().numpy()
    ref = R.resample(x, d, n_out)
    assert y.shape == ref.shape
    err = np.abs(y.astype(np.float64) - ref)
    bound = R.table_error_bound(d) * float(np.abs(x).max()) + R.U * np.abs(ref)
    flips = float(np.mean(R.to_int16(y) != R.to_int16(ref)))
    msg = "N %+d: max error %.3g (bound %.3g), %.4f %% of the 16-bit samples flip" % (semitones, err.max(), bound.min(), 100 * flips)
    print(msg)
    assert np.all(err <= bound), msg
    assert np.abs(R.to_int16(y).astype(np.int32) - R.to_int16(ref)).max() <= 1, msg


@pytest.mark.parametrize("semitones", [-12, 12])
def test_filter_design_meets_the_derived_target(semitones):
    """CPU only, on the host-built table: its rows are the filter sampled 1024 times per input sample.  From that response: deviation
    from 1 at most 2^-16 up to 0.90 of the narrower Nyquist frequency, at most 2^-16 (-96.3 dB) from that Nyquist frequency on."""
    d = _ratio(semitones)
    table, half = ops.resample_ratio_table(d)
    P = ops.RESAMPLE_PHASES
    assert (P, half) == (R.PHASES, R.design(d)["half"]) and table.shape == (P + 1, 2 * half + 1) and table.dtype == np.float32
    want = R.h(np.arange(P + 1)[:, None] / P + np.arange(-half, half + 1)[None, :], d)
    assert np.array_equal(table, want.astype(np.float32))
    assert np.array_equal(table[P, :-1], table[0, 1:]) and table[0, 0] == 0 and np.all(table[1:, -1] == 0)
    # h(q / P - half) for q = 0 .. 2 half P: row r, column j holds q = (j + half) P + r
    fine = table[:P].astype(np.float64).T.reshape(-1)[: 2 * half * P + 1]
    nfft = 1 << 23
    H = np.abs(np.fft.rfft(fine, nfft)) / P
    f = np.arange(len(H)) * (P / nfft)                  # cycles per input sample
    nyq = 0.5 * min(1.0, 1.0 / d)
    dev_pass = float(np.abs(H[f <= 0.90 * nyq] - 1.0).max())
    stop = float(H[f >= nyq].max())
    print("N %+d: passband deviation %.3g, stopband %.1f dB" % (semitones, dev_pass, 20 * np.log10(stop)))
    assert dev_pass <= 2.0 ** -16
    assert 20 * np.log10(stop) <= -96.3


def _peak_hz(y, sr, nwin):
    seg = y[len(y) // 2 - nwin // 2: len(y) // 2 + nwin // 2].astype(np.float64)
    return float(np.argmax(np.abs(np.fft.rfft(seg * np.hanning(nwin)))) * sr / nwin)


@pytest.mark.parametrize("semitones", [-12, -3, -1, 2, 7, 12])
def test_a_steady_tone_moves_by_the_ratio(dev, semitones):
    """A steady tone at f0 comes out with its spectral peak at f0 2^(N/12), within one bin of a Hann-windowed FFT over 8192 frames
    (32768 on the hardware's 44.1 kHz signal) from the middle of the output; and the output has exactly the input's frames."""
    seconds, sr, nwin, f0 = (4.0, 44100, 32768, 440.0) if dev.big else (2.0, 8000, 8192, 310.0)
    t = np.arange(int(seconds * sr)) / sr
    x = (0.5 * np.sin(2 * np.pi * f0 * t)).astype(np.float32)
    y, offs = cover.pitch_shift_signal(dev.t(torch.from_numpy(x)), sr, semitones)
    assert y.shape == x.shape and y.dtype == torch.float32 and offs.dtype == torch.int32
    got = _peak_hz(y.cpu().numpy(), sr, nwin)
    assert abs(got - f0 * _ratio(semitones)) <= sr / nwin, (got, f0 * _ratio(semitones), sr / nwin)


def test_stereo_stays_aligned_and_calls_repeat_bit_for_bit(dev):
    sr = 44100 if dev.big else 8000
    m = R.stems(1.5, sr, 1, 51)
    x = dev.t(torch.from_numpy(np.concatenate([m, m])))
    y, offs = cover.pitch_shift_signal(x, sr, 2)
    assert y.shape == x.shape and torch.equal(y[0], y[1])
    y2, offs2 = cover.pitch_shift_signal(x, sr, 2)
    assert torch.equal(y, y2) and torch.equal(offs, offs2)
    # the offsets returned reproduce the output when passed back in
    y3, _ = cover.pitch_shift_signal(x, sr, 2, offsets=offs)
    assert torch.equal(y, y3)
    # a batch of two stems is the two stems
    xs = dev.t(torch.from_numpy(np.stack([R.stems(1.0, sr, 2, 52), R.stems(1.0, sr, 2, 53)])))
    zb, ob = ops.tempo_wsola(xs, sr, 1.0 / _ratio(-3))
    for s in range(2):
        z1, o1 = ops.tempo_wsola(xs[s].contiguous(), sr, 1.0 / _ratio(-3))
        assert torch.equal(zb[s], z1) and torch.equal(ob[s], o1)
    rb = ops.resample_ratio(zb, _ratio(-3), xs.shape[2])
    assert torch.equal(rb[1], ops.resample_ratio(zb[1].contiguous(), _ratio(-3), xs.shape[2]))


def test_zero_semitones_is_the_identity_and_bad_input_raises(dev):
    x = dev.t(torch.from_numpy(R.stems(0.5, 8000, 2, 61)))
    y, _ = cover.pitch_shift_signal(x, 8000, 0)
    assert torch.equal(y, x) and y.data_ptr() != x.data_ptr()
    y1, _ = cover.pitch_shift_signal(x[0].contiguous(), 8000, -2)
    assert y1.shape == (x.shape[1],)
    with pytest.raises(ValueError):
        cover.pitch_shift_signal(dev.t(torch.zeros(3, 4000)), 8000, 2)
    with pytest.raises(TypeError):
        cover.pitch_shift_signal(dev.t(torch.zeros(2, 4000, dtype=torch.float64)), 8000, 2)
    with pytest.raises(RuntimeError, match="tempo"):
        ops.tempo_wsola(x, 8000, 8.0)
    e, _ = cover.pitch_shift_signal(dev.t(torch.zeros(2, 0)), 8000, 2)
    assert e.shape == (2, 0)
