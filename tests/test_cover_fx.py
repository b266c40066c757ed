"""The vocal effects chain of add_audio_effects (reference src/main.py:206-226) on the device: aicovergen_amd.cover over
csrc/fx.hip, each stage against a per-sample float32 restatement of the JUCE recurrences pedalboard wraps (written here,
operation for operation, no fused multiply-add).  Single-segment calls are the sequential recurrence and must match bit for bit
(the compressor's powf may differ by 2 ulp between platforms); segmented calls within 1e-6 of the signal's peak."""

import numpy as np
import pytest
import torch

from aicovergen_amd import _lib, cover, ops

f32 = np.float32


def _signal(sr, seconds, channels, seed):
    rng = np.random.default_rng(seed)
    n = int(sr * seconds)
    t = np.arange(n) / sr
    env = 0.15 + 0.85 * (0.5 + 0.5 * np.sin(2 * np.pi * 1.3 * t))
    x = np.stack([env * (0.6 * np.sin(2 * np.pi * (220 + 37 * c) * t) + 0.35 * rng.standard_normal(n)) for c in range(channels)])
    x[:, : n // 10] *= 0.02                      # a quiet stretch: the envelope sits below the threshold there
    return np.clip(x, -1, 1).astype(np.float32)


# ---- float32 restatements ------------------------------------------------------------------------
def ref_highpass(x, sr, s0=None):
    b0, b1, a1 = cover.highpass_coefs(sr)
    y = np.empty_like(x)
    st = np.zeros((x.shape[0], 2), np.float32) if s0 is None else s0.copy()
    for c in range(x.shape[0]):
        s = f32(st[c, 0])
        for i in range(x.shape[1]):
            v = x[c, i]
            o = b0 * v + s
            s = b1 * v - a1 * o
            y[c, i] = o
        st[c, 0] = s
    return y, st


def ref_compressor(x, sr, thr_db, ratio, s0=None, gains=None):
    cat, crl, thr, thr_inv, rinv = cover.compressor_coefs(sr, thr_db, ratio)
    y = np.empty_like(x)
    gains = np.empty_like(x) if gains is None else gains
    st = np.zeros((x.shape[0], 2), np.float32) if s0 is None else s0.copy()
    e1 = rinv - f32(1)
    for c in range(x.shape[0]):
        env = f32(st[c, 1])
        for i in range(x.shape[1]):
            v = x[c, i]
            a = abs(v)
            env = a + (cat if a > env else crl) * (env - a)
            g = f32(1) if env < thr else np.power(env * thr_inv, e1)
            gains[c, i] = g
            y[c, i] = g * v
        st[c, 1] = env
    return y, st


class RefReverb:
    """juce::Reverb, processMono / processStereo, parameters at their targets from the first sample."""

    def __init__(self, sr, channels, room, damping, wet, dry, width=1.0):
        self.gain, self.damp, self.fb, self.wet1, self.wet2, self.dry = cover.reverb_coefs(room, damping, wet, dry, width)
        self.C = channels
        self.cl = [cover.comb_lengths(sr, c) for c in range(channels)]
        self.al = [cover.allpass_lengths(sr, c) for c in range(channels)]
        self.cb = [[np.zeros(L, np.float32) for L in ls] for ls in self.cl]
        self.ab = [[np.zeros(L, np.float32) for L in ls] for ls in self.al]
        self.ci = [[0] * 8 for _ in range(channels)]
        self.ai = [[0] * 4 for _ in range(channels)]
        self.last = [[f32(0)] * 8 for _ in range(channels)]

    def _wet(self, c, inp):
        out = f32(0)
        d1 = f32(1) - self.damp
        for j in range(8):
            buf, k = self.cb[c][j], self.ci[c][j]
            o = buf[k]
            self.last[c][j] = o * d1 + self.last[c][j] * self.damp
            buf[k] = inp + self.last[c][j] * self.fb
            self.ci[c][j] = (k + 1) % len(buf)
            out = out + o
        for j in range(4):
            buf, k = self.ab[c][j], self.ai[c][j]
            b = buf[k]
            buf[k] = out + b * f32(0.5)
            self.ai[c][j] = (k + 1) % len(buf)
            out = b - out
        return out

    def process(self, x):
        y = np.empty_like(x)
        for i in range(x.shape[1]):
            if self.C == 1:
                w = self._wet(0, x[0, i] * self.gain)
                y[0, i] = w * self.wet1 + x[0, i] * self.dry
            else:
                inp = (x[0, i] + x[1, i]) * self.gain
                wl, wr = self._wet(0, inp), self._wet(1, inp)
                y[0, i] = (wl * self.wet1 + wr * self.wet2) + x[0, i] * self.dry
                y[1, i] = (wr * self.wet1 + wl * self.wet2) + x[1, i] * self.dry
        return y


def _run(dev, fn, x, *a, **k):
    y, st = fn(dev.t(torch.from_numpy(x)), *a, **k)
    dev.sync()
    return y.cpu().numpy(), st


def _ulps(a, b):
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int(np.abs(ia - ib).max()) if a.size else 0


CASES = [(32000, 1), (40000, 1), (48000, 1), (44100, 2)]


# ---- each stage, one segment: bit-identical ----------------------------------------------------------
@pytest.mark.parametrize("sr,ch", CASES)
def test_highpass_bit_identical(dev, sr, ch):
    x = _signal(sr, 0.5, ch, 1)
    y, st = _run(dev, cover.highpass, x, sr, segment=0)
    ry, rst = ref_highpass(x, sr)
    assert np.array_equal(y.view(np.int32), ry.view(np.int32))
    assert np.array_equal(st.cpu().numpy()[:, 0], rst[:, 0])


@pytest.mark.parametrize("sr,ch", CASES)
def test_compressor_within_2_ulp(dev, sr, ch):
    x = _signal(sr, 0.5, ch, 2)
    y, _ = _run(dev, cover.compressor, x, sr, -15.0, 4.0, segment=0)
    g = np.empty_like(x)
    ry, _ = ref_compressor(x, sr, -15.0, 4.0, gains=g)
    # the envelope is exact; the gain powf(env / thr, 1/ratio - 1) may sit up to 2 ulp away: y must be g' x for such a g'
    ok = np.zeros(x.shape, bool)
    for k in range(-2, 3):
        gk = g.copy()
        for _ in range(abs(k)):
            gk = np.nextafter(gk, np.float32(np.inf if k > 0 else -np.inf)).astype(np.float32)
        ok |= (gk * x).view(np.int32) == y.view(np.int32)
    assert ok.all(), np.argwhere(~ok)[:5]
    assert (g < 1).sum() > x.size // 4          # the compressor is working on most of the signal
    quiet = slice(0, x.shape[1] // 20)           # below the threshold the gain is exactly 1
    assert np.array_equal(y[:, quiet], x[:, quiet])


@pytest.mark.parametrize("sr,ch", CASES)
def test_reverb_bit_identical(dev, sr, ch):
    x = _signal(sr, 0.5, ch, 3)
    y, _ = _run(dev, cover.reverb, x, sr, 0.15, 0.7, 0.2, 0.8, segment=0)
    ry = RefReverb(sr, ch, 0.15, 0.7, 0.2, 0.8).process(x)
    assert np.array_equal(y.view(np.int32), ry.view(np.int32))


@pytest.mark.parametrize("room,damping", [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0)])
def test_reverb_room_and_damping_limits(dev, room, damping):
    sr = 40000
    x = _signal(sr, 0.3, 1, 4)
    y, _ = _run(dev, cover.reverb, x, sr, room, damping, 0.3, 0.6, segment=0)
    ry = RefReverb(sr, 1, room, damping, 0.3, 0.6).process(x)
    assert np.array_equal(y.view(np.int32), ry.view(np.int32))


def test_reverb_wet_zero_is_dry_times_x(dev):
    for sr, ch in ((40000, 1), (44100, 2)):
        x = _signal(sr, 0.3, ch, 5)
        y, _ = _run(dev, cover.reverb, x, sr, 0.5, 0.5, 0.0, 0.8)
        assert np.array_equal(y, x * (f32(0.8) * f32(2)))


def test_compressor_above_peak_is_identity(dev):
    x = _signal(40000, 0.3, 1, 6)
    y, _ = _run(dev, cover.compressor, x, 40000, 1.0, 4.0)    # threshold +1 dB > peak 1.0
    assert np.array_equal(y, x)


def test_chain_single_segment_matches_stages(dev):
    sr = 40000
    x = _signal(sr, 0.5, 1, 7)
    y, _ = _run(dev, cover.vocal_effects, x[0], sr, 0.15, 0.2, 0.8, 0.7, segment=0)
    z, _ = ref_highpass(x, sr)
    z, _ = ref_compressor(z, sr, -15.0, 4.0)
    ry = RefReverb(sr, 1, 0.15, 0.7, 0.2, 0.8).process(z)[0]
    # the compressor's gain may sit an ulp or two away (powf); everything after it is linear in its output
    assert np.abs(y - ry).max() <= 1e-6 * np.abs(x).max()


# ---- segments and pieces ----------------------------------------------------------------------------
@pytest.mark.parametrize("sr,ch", [(40000, 1), (44100, 2)])
def test_segmented_matches_single_segment(dev, sr, ch):
    x = _signal(sr, 8.0, ch, 8)               # longer than the reverb's warm-up (3.8 s here): segments start from zero state
    xs = x[0] if ch == 1 else x
    assert x.shape[1] > cover.warmup_reverb(sr, cover.reverb_coefs(0.15, 0.7, 0.2, 0.8)) + 20000
    one, _ = _run(dev, cover.vocal_effects, xs, sr, 0.15, 0.2, 0.8, 0.7, segment=0)
    seg, _ = _run(dev, cover.vocal_effects, xs, sr, 0.15, 0.2, 0.8, 0.7, segment=20000)
    assert np.isfinite(seg).all()
    assert np.abs(seg - one).max() <= 1e-6 * np.abs(x).max()
    assert not np.array_equal(seg, x.reshape(seg.shape))


@pytest.mark.parametrize("sr,ch", [(40000, 1), (44100, 2)])
def test_pieces_with_carried_state_equal_one_call(dev, sr, ch):
    x = _signal(sr, 2.3, ch, 9)
    xs = x[0] if ch == 1 else x
    one, _ = _run(dev, cover.vocal_effects, xs, sr, 0.15, 0.2, 0.8, 0.7, segment=0)
    parts, state = [], None
    for i0 in range(0, x.shape[1], sr):   # main.py reads one second at a time
        piece = xs[..., i0:i0 + sr]
        y, state = cover.vocal_effects(dev.t(torch.from_numpy(np.ascontiguousarray(piece))), sr, 0.15, 0.2, 0.8, 0.7,
                                       state=state, segment=0)
        parts.append(y.cpu().numpy())
    got = np.concatenate(parts, axis=-1)
    assert np.array_equal(got.view(np.int32), one.view(np.int32))


def test_empty_input_keeps_state(dev):
    sr = 40000
    x = _signal(sr, 0.2, 1, 10)[0]
    _, st = cover.vocal_effects(dev.t(torch.from_numpy(x)), sr, 0.15, 0.2, 0.8, 0.7, segment=0)
    y, st2 = cover.vocal_effects(dev.t(torch.zeros(0)), sr, 0.15, 0.2, 0.8, 0.7, state=st)
    dev.sync()
    assert y.shape == (0,)
    assert torch.equal(st.dyn.cpu(), st2.dyn.cpu()) and torch.equal(st.rev.cpu(), st2.rev.cpu())
    y, st3 = cover.vocal_effects(dev.t(torch.zeros(0)), sr, 0.15, 0.2, 0.8, 0.7)
    assert y.shape == (0,) and not st3.rev.cpu().any()


def test_bad_arguments_return_error_codes(dev):
    lib = _lib.get()
    x = dev.t(torch.zeros(2, 64))
    y = torch.empty_like(x)
    st = dev.t(torch.zeros(2, ops.fx_reverb_state_size(40000)))
    st2 = torch.empty_like(st)
    p, s = x.data_ptr(), 0
    # null pointers, the same state buffer in and out, unknown flags -> AICG_E_ARG (-2)
    assert lib.aicg_fx_dynamics(p, None, None, st.data_ptr(), 2, 64, 0, 0, *([0.5] * 8), 3, s) == -2
    assert lib.aicg_fx_dynamics(p, y.data_ptr(), st.data_ptr(), st.data_ptr(), 2, 64, 0, 0, *([0.5] * 8), 3, s) == -2
    assert lib.aicg_fx_dynamics(p, y.data_ptr(), None, st.data_ptr(), 2, 64, 0, 0, *([0.5] * 8), 4, s) == -2
    assert lib.aicg_fx_reverb(p, y.data_ptr(), None, st2.data_ptr(), 2, 64, 100, 0, 0, *([0.5] * 6), s) == -2
    # three channels, negative length / warm-up -> AICG_E_SHAPE (-1)
    assert lib.aicg_fx_dynamics(p, y.data_ptr(), None, st.data_ptr(), 3, 64, 0, 0, *([0.5] * 8), 3, s) == -1
    assert lib.aicg_fx_reverb(p, y.data_ptr(), None, st2.data_ptr(), 2, -1, 40000, 0, 0, *([0.5] * 6), s) == -1
    assert lib.aicg_fx_reverb(p, y.data_ptr(), None, st2.data_ptr(), 1, 64, 40000, 0, -5, *([0.5] * 6), s) == -1
    assert b"aicg_fx_reverb" in lib.aicg_last_error()
    # the delay lines of a very high rate do not fit the LDS -> AICG_E_LDS (-4)
    big = dev.t(torch.zeros(2, ops.fx_reverb_state_size(192000)))
    assert lib.aicg_fx_reverb(p, y.data_ptr(), None, big.data_ptr(), 2, 64, 192000, 0, 0, *([0.5] * 6), s) == -4
    with pytest.raises(ValueError):
        cover.vocal_effects(dev.t(torch.zeros(3, 16)), 40000, 0.15, 0.2, 0.8, 0.7)
    with pytest.raises(RuntimeError, match="aicg_fx_reverb"):
        cover.reverb(dev.t(torch.zeros(16)), 1000)


def test_warmup_rule():
    coefs = cover.reverb_coefs(0.15, 0.7, 0.2, 0.8)
    w = cover.warmup_reverb(40000, coefs)
    fb = float(coefs[2])
    # the longest comb's state after the warm-up has decayed below 2^-30 of itself
    assert fb ** ((w - 30 * sum(cover.allpass_lengths(40000, 1))) / max(cover.comb_lengths(40000, 1)) - 1) < 2.0 ** -30
    assert 8e4 < w < 2e5
    assert cover.warmup_reverb(40000, cover.reverb_coefs(1.0, 0.7, 0.2, 0.8)) > 10 * w
    hp = cover.highpass_coefs(40000)
    assert abs(float(hp[2])) ** cover.warmup_dynamics(hp=hp) < 2.0 ** -30


# ---- at size, on the GPU: 240 s of 40 kHz mono ------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("room", [0.15, 1.0])
def test_240s_segmented_vs_single_segment_on_gpu(room):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import conftest
    conftest._bind("hip")
    sr = 40000
    rng = np.random.default_rng(11)
    n = 240 * sr
    t = np.arange(n, dtype=np.float64) / sr
    x = (0.5 * np.sin(2 * np.pi * 180 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 0.7 * t)) + 0.1 * rng.standard_normal(n))
    x = torch.from_numpy(np.clip(x, -1, 1).astype(np.float32)).cuda()
    one, _ = cover.vocal_effects(x, sr, room, 0.2, 0.8, 0.7, segment=0)
    seg, _ = cover.vocal_effects(x, sr, room, 0.2, 0.8, 0.7)
    torch.cuda.synchronize()
    assert torch.isfinite(seg).all() and torch.isfinite(one).all()
    assert float((seg - one).abs().max()) <= 1e-6 * float(x.abs().max())
