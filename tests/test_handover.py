"""The stem hand-over kernels (csrc/handover.hip) against numpy restatements of the lines of run_mdx they replace
(aicovergen_amd/mdx.py:288-303, reference src/mdx.py:257-280), byte for byte: the peak, wave / peak, and the two 16-bit PCM stems
with soundfile's rounding.  numpy rounds after every operation there; the inverted stem is built so that a fused multiply-subtract
gives another int16, which is the check that the kernel is compiled without contraction.

Rejections: a dtype the library does not read reaches it as an unknown format and comes back with aicg_last_error's text; arguments
the C ABI cannot describe (non-contiguous tensors, float64 signals for the stem pass) are refused by the ops wrapper before the call."""
import numpy as np
import pytest
import torch

from aicovergen_amd import _lib, ops

f32 = np.float32
LENGTHS = [1, 7, 4096, 4099, 65537]      # tails of every vector width, n % 4 == 0 (row 1 aligned) and not, more than one workgroup


# ---- numpy restatements ------------------------------------------------------------------------------
def ref_normalise(x):
    """audio_io.load_wav's sample conversion, then mdx.py:289-292."""
    if x.dtype == np.int16:
        d = x.astype(np.float32) / 32768.0
        wave = np.ascontiguousarray((d[:, None] if d.ndim == 1 else d).T)
    else:
        wave = x.copy()
    if wave.shape[0] == 1:
        wave = np.concatenate([wave, wave], 0)
    peak = max(np.max(wave), abs(np.min(wave)))
    wave /= peak
    return wave, peak


def ref_pcm16(data):
    """audio_io.write_wav_pcm16's samples."""
    y = np.clip(np.asarray(data, dtype=np.float64), -1.0, 32767.0 / 32768.0)
    return np.rint(y * 32768.0).astype(np.int16)


def ref_stems(wave, sep, peak, compensation):
    """mdx.py:293-303: `separated = ... * peak`; the main stem; `wave.T - separated.T * model.compensation`."""
    separated = sep * peak
    assert separated.dtype == np.float32
    inv = wave.T - separated.T * compensation
    assert inv.dtype == np.float32
    return ref_pcm16(separated.T), ref_pcm16(inv)


def _pcm(n, ch, seed, lo=-20000, hi=15000):
    rng = np.random.default_rng(seed)
    x = rng.integers(lo, hi + 1, size=(n, ch)).astype(np.int16)
    return x


# ---- stem_normalise ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("ch", [1, 2])
def test_normalise_pcm16(dev, n, ch):
    x = _pcm(n, ch, n + ch)
    x[n // 2, ch - 1] = -20000                     # the negative peak is the larger one
    x[0, 0] = 15000 if n > 1 else x[0, 0]
    wave, peak = ops.stem_normalise(dev.t(torch.from_numpy(x)))
    dev.sync()
    rw, rp = ref_normalise(x)
    assert peak.dtype == torch.float32 and peak.shape == (1,) and wave.shape == (2, n)
    assert f32(peak.cpu().numpy()[0]).view(np.int32) == f32(rp).view(np.int32) and rp == f32(20000 / 32768)
    assert np.array_equal(wave.cpu().numpy().view(np.int32), rw.view(np.int32))


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("ch", [1, 2])
def test_normalise_float(dev, n, ch):
    rng = np.random.default_rng(100 + n + ch)
    x = (rng.standard_normal((ch, n)) * 0.3).astype(np.float32)
    x[ch - 1, n - 1] = -1.7                         # a float file may exceed full scale; the peak is negative and in the tail
    wave, peak = ops.stem_normalise(dev.t(torch.from_numpy(x)))
    dev.sync()
    rw, rp = ref_normalise(x)
    assert f32(peak.cpu().numpy()[0]) == f32(rp) == f32(1.7)
    assert np.array_equal(wave.cpu().numpy().view(np.int32), rw.view(np.int32))


def test_normalise_peak_at_minus_32768_and_positive_peak(dev):
    x = _pcm(4099, 2, 5)
    x[4098, 1] = -32768
    wave, peak = ops.stem_normalise(dev.t(torch.from_numpy(x)))
    rw, rp = ref_normalise(x)
    assert float(peak.cpu()[0]) == 1.0 == rp and np.array_equal(wave.cpu().numpy(), rw)
    y = _pcm(4099, 2, 6, lo=-9000, hi=9000)
    y[17, 0] = 31111                                # the positive peak is the larger one
    wave, peak = ops.stem_normalise(dev.t(torch.from_numpy(y)))
    rw, rp = ref_normalise(y)
    assert f32(peak.cpu().numpy()[0]) == f32(rp) == f32(31111 / 32768)
    assert np.array_equal(wave.cpu().numpy().view(np.int32), rw.view(np.int32))


def test_normalise_division_is_ieee(dev):
    """x / peak against x * (1 / peak): the inputs are chosen among those where the two differ."""
    rng = np.random.default_rng(8)
    x = rng.uniform(-0.7, 0.7, size=(2, 65537)).astype(np.float32)
    x[0, 0] = 0.7300000190734863
    p = f32(x[0, 0])
    differ = (x / p).view(np.int32) != (x * (f32(1) / p)).view(np.int32)
    assert differ.sum() > 1000
    wave, _ = ops.stem_normalise(dev.t(torch.from_numpy(x)))
    assert np.array_equal(wave.cpu().numpy().view(np.int32), ref_normalise(x)[0].view(np.int32))


def test_normalise_silence_is_numpys(dev):
    x = np.zeros((9, 2), np.int16)
    wave, peak = ops.stem_normalise(dev.t(torch.from_numpy(x)))
    with np.errstate(invalid="ignore", divide="ignore"):
        rw, rp = ref_normalise(x)
    assert float(peak.cpu()[0]) == 0.0 == rp
    assert np.isnan(rw).all() and torch.isnan(wave.cpu()).all()


# ---- mdx_stems_pcm16 ----------------------------------------------------------------------------------
def _fused_differs(compensation, count=64):
    """(wave, separated) pairs (peak = 1) for which wave - separated * compensation lands on another int16 when the product is not
    rounded before the subtraction: the two-rounding result sits exactly on k + 0.5, the exact one beside it."""
    rng = np.random.default_rng(31)
    c = f32(compensation)
    ws, ss = [], []
    for _ in range(200):
        if len(ws) >= count:
            break
        s = rng.uniform(-0.9, 0.9, 4096).astype(np.float32)
        t = s * c                                                    # float32 product, rounded
        exact = s.astype(np.float64) * np.float64(c)                 # 24 x 24 bits: exact in float64
        k = rng.integers(-3000, 3000, 4096)
        w = (t.astype(np.float64) + (k + 0.5) / 32768.0).astype(np.float32)
        two = w - t                                                  # float32 subtraction, rounded
        fused = (w.astype(np.float64) - exact).astype(np.float32)    # one rounding
        pick = (two.astype(np.float64) * 32768.0 == k + 0.5) & (ref_pcm16(two) != ref_pcm16(fused)) & (np.abs(w) < 1)
        ws += list(w[pick])
        ss += list(s[pick])
    assert len(ws) >= count, "no frame found where contraction changes the int16"
    return np.array(ws[:count], np.float32), np.array(ss[:count], np.float32)


def _corner_inputs(n, compensation, peak):
    """wave, separated (2, n): random signal with the corners written over its head (as far as n reaches)."""
    rng = np.random.default_rng(n)
    wave = rng.uniform(-1, 1, (2, n)).astype(np.float32)
    sep = rng.uniform(-1.3, 1.3, (2, n)).astype(np.float32) / f32(peak)
    k = np.array([0, 1, 2, 3, 100, 101, -1, -2, -3, -101, 32766, -32767, -32768], np.float64)
    ties = ((k + 0.5) / 32768.0 / peak).astype(np.float32)            # peak is a power of two: separated * peak is exactly k + 0.5
    edges = (np.array([1.0, 1.0 + 2.0 ** -20, 1.5, 32767.0 / 32768.0, 32767.25 / 32768.0, -1.0, -1.0 - 2.0 ** -20, -1.5]) / peak).astype(np.float32)
    head = np.concatenate([ties, edges])
    m = min(n, len(head))
    sep[0, :m] = head[:m]
    sep[1, :m] = head[::-1][:m]
    wave[:, :m] = 0                                                  # the inverted stem sees -(k + 0.5) * compensation there
    if peak == 1.0 and compensation != 1.0 and n >= 2 * len(head) + 64:
        fw, fs = _fused_differs(compensation)
        wave[0, m:m + 64], sep[0, m:m + 64] = fw, fs
        wave[1, n - 64:], sep[1, n - 64:] = fw, fs                    # and in the last frames, past the vector body when n % 4 != 0
    return wave, sep


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("compensation", [1.0, 1.035])
@pytest.mark.parametrize("peak", [1.0, 0.5])
def test_stems_pcm16(dev, n, compensation, peak):
    wave, sep = _corner_inputs(n, compensation, peak)
    rmain, rinv = ref_stems(wave, sep, f32(peak), compensation)
    if n >= 4096:
        assert {32767, -32768} <= set(rmain.reshape(-1).tolist()) and {0, 2, 100, 102, -2, -32768} <= set(rmain[:13, 0].tolist())
    w, s, p = (dev.t(torch.from_numpy(a)) for a in (wave, sep, np.array([peak], np.float32)))
    main, inv = ops.mdx_stems_pcm16(w, s, p, compensation)
    dev.sync()
    assert main.shape == inv.shape == (n, 2) and main.dtype == inv.dtype == torch.int16
    assert np.array_equal(main.cpu().numpy(), rmain)
    assert np.array_equal(inv.cpu().numpy(), rinv)
    # each output left out in turn (exclude_main / exclude_inversion)
    m2, i2 = ops.mdx_stems_pcm16(w, s, p, compensation, want_main=False)
    assert m2 is None and np.array_equal(i2.cpu().numpy(), rinv)
    m3, i3 = ops.mdx_stems_pcm16(w, s, p, compensation, want_inverted=False)
    assert i3 is None and np.array_equal(m3.cpu().numpy(), rmain)


def test_fused_multiply_subtract_would_differ(dev):
    """The contract-off check on its own: every one of these frames rounds to another int16 when the product keeps its exact value."""
    w1, s1 = _fused_differs(1.035, 64)
    wave, sep = np.stack([w1, w1[::-1]]).copy(), np.stack([s1, s1[::-1]]).copy()
    c = f32(1.035)
    fused = ref_pcm16((wave.astype(np.float64) - sep.astype(np.float64) * np.float64(c)).astype(np.float32).T)
    _, rinv = ref_stems(wave, sep, f32(1.0), 1.035)
    assert (fused != rinv).all()
    _, inv = ops.mdx_stems_pcm16(*(dev.t(torch.from_numpy(a)) for a in (wave, sep, np.ones(1, np.float32))), 1.035, want_main=False)
    assert np.array_equal(inv.cpu().numpy(), rinv)


def test_chain_of_both_kernels_equals_run_mdx_lines(dev):
    """normalise -> (a stand-in separation) -> stems, the peak never leaving the device."""
    x = _pcm(4099, 2, 77, lo=-30000, hi=30000)
    wave, peak = ops.stem_normalise(dev.t(torch.from_numpy(x)))
    sep = (wave * 0.83).flip(0).contiguous()
    main, inv = ops.mdx_stems_pcm16(wave, sep, peak, 1.021)
    rw, rp = ref_normalise(x)
    rsep = np.ascontiguousarray((rw * f32(0.83))[::-1])
    rmain, rinv = ref_stems(rw, rsep, rp, 1.021)
    assert np.array_equal(main.cpu().numpy(), rmain) and np.array_equal(inv.cpu().numpy(), rinv)


# ---- rejections ----------------------------------------------------------------------------------------
def test_bad_arguments(dev):
    lib = _lib.get()
    x = dev.t(torch.zeros(64, 2, dtype=torch.int16))
    out = dev.t(torch.zeros(2, 64))
    pk = dev.t(torch.ones(1))
    o16 = dev.t(torch.zeros(64, 2, dtype=torch.int16))
    # a dtype the library does not read arrives as an unknown format: AICG_E_ARG (-2) and the text ops raises with
    with pytest.raises(RuntimeError, match="aicg_stem_normalise: input format"):
        ops.stem_normalise(dev.t(torch.zeros(2, 64, dtype=torch.float64)))
    with pytest.raises(RuntimeError, match="aicg_stem_normalise: input format"):
        ops.stem_normalise(dev.t(torch.zeros(64, 2, dtype=torch.int32)))
    assert lib.aicg_stem_normalise(x.data_ptr(), 7, 2, 64, out.data_ptr(), pk.data_ptr(), 0) == -2
    assert b"aicg_stem_normalise" in lib.aicg_last_error()
    # three channels, a negative length -> AICG_E_SHAPE (-1); null pointers -> AICG_E_ARG (-2)
    assert lib.aicg_stem_normalise(x.data_ptr(), 0, 3, 64, out.data_ptr(), pk.data_ptr(), 0) == -1
    assert lib.aicg_stem_normalise(x.data_ptr(), 0, 2, -1, out.data_ptr(), pk.data_ptr(), 0) == -1
    assert lib.aicg_stem_normalise(None, 0, 2, 64, out.data_ptr(), pk.data_ptr(), 0) == -2
    assert lib.aicg_stem_normalise(x.data_ptr(), 0, 2, 64, out.data_ptr(), None, 0) == -2
    assert lib.aicg_mdx_stems_pcm16(out.data_ptr(), out.data_ptr(), pk.data_ptr(), 1.0, 64, None, None, 0) == -2
    assert b"aicg_mdx_stems_pcm16" in lib.aicg_last_error()
    assert lib.aicg_mdx_stems_pcm16(out.data_ptr(), out.data_ptr(), pk.data_ptr(), 1.0, 64, o16.data_ptr(), o16.data_ptr(), 0) == -2
    assert lib.aicg_mdx_stems_pcm16(out.data_ptr(), None, pk.data_ptr(), 1.0, 64, o16.data_ptr(), None, 0) == -2
    assert lib.aicg_mdx_stems_pcm16(out.data_ptr(), out.data_ptr(), pk.data_ptr(), 1.0, -5, o16.data_ptr(), None, 0) == -1
    with pytest.raises(ValueError, match="contiguous"):
        ops.stem_normalise(dev.t(torch.zeros(2, 64)).t())
    with pytest.raises(ValueError, match="contiguous"):
        ops.mdx_stems_pcm16(dev.t(torch.zeros(64, 2)).t(), out, pk, 1.0)
    with pytest.raises(TypeError, match="float32"):
        ops.mdx_stems_pcm16(out.double(), out, pk, 1.0)
    with pytest.raises(TypeError, match="peak"):
        ops.mdx_stems_pcm16(out, out, pk.double(), 1.0)
    with pytest.raises(ValueError, match="shape"):
        ops.mdx_stems_pcm16(out, dev.t(torch.zeros(2, 32)), pk, 1.0)
    # an empty stem is an empty result
    w, p = ops.stem_normalise(dev.t(torch.zeros(0, 2, dtype=torch.int16)))
    assert w.shape == (2, 0) and float(p.cpu()[0]) == 0.0
