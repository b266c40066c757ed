"""STFT / iSTFT (csrc/stft.hip) at the forms tests/test_stft.py leaves open: a window that is not symmetric (the periodic Hann is, so
a mirrored window index passes there), the frame-major inverse MDXModel.istft_tf uses, both overlap-add kernels with the ends looked
at separately, tonal input judged per bin and per sample (an error confined to a few bins disappears in a whole-tensor RMS of
white noise), batches of 1 / 3 / 5 signals that share workgroups, and the truncated band.

Reference: torch.stft / torch.istft in float64 on the CPU, on the same fp32 signal, spectrum and window.

Bar: torch's own float32 transform has an error `e32` against float64; the kernel may have 4 x that (another FFT factorisation of
the same length), in both measures:
  whole   relative RMS over the tensor;
  point   forward: max over (signal, bin, frame) of |got - ref| / (largest |ref| of that frame);
          inverse: max over samples of |got - ref| / (largest |ref| of that signal).
Bit-equality takes no tolerance."""
import pytest
import torch

from aicovergen_amd import ops
from conftest import rel_rms

FACTOR = 4.0

# n_fft, hop, L (2 signals): one compile-time plan per family -- 8 x 8 x 8 with four frames per workgroup (RMVPE), 16 x 16 x 8,
# 16 x 16 x 10, 16 x 16 x 15 -- and both run-time-radix lengths (4 * 3 * 5, 16 frames per workgroup; 4 * 2 * 5 * 5 * 5, four).  L is
# the shortest that exceeds n_fft / 2 (reflect padding) and, where a workgroup holds several frames, leaves the last one ragged:
# 2 x 5 frames in fours, 2 x 9 in sixteens, 2 x 7 in fours.
SIZES = [(1024, 160, 640), (4096, 1024, 3072), (5120, 1024, 3072), (7680, 1024, 4096), (60, 16, 128), (2000, 250, 1500)]


def asym_window(n_fft):
    """smooth, positive (but for w[0] = 0), w[i] != w[N - i]: rises to 1.34 at 0.6 N"""
    i = torch.arange(n_fft, dtype=torch.float64)
    return (torch.hann_window(n_fft, periodic=True, dtype=torch.float64) ** 0.5 * (1 + 0.5 * i / n_fft)).float()


def ref_stft(x, n_fft, hop, nb, window, dtype=torch.float64):
    """(n_sig, 2, nb, n_frames), the layout of ops.stft"""
    s = torch.stft(x.to(dtype), n_fft=n_fft, hop_length=hop, window=window.to(dtype), center=True, return_complex=True)
    return torch.view_as_real(s).permute(0, 3, 1, 2)[:, :, :nb].contiguous()


def ref_istft(sp, n_fft, hop, L, window, dtype=torch.float64):
    """sp (n_sig, 2, nb, n_frames) fp32; bins from nb up are zero; Im(DC) and Im(Nyquist) are ignored (a C2R transform), said here
    explicitly so that the reference does not depend on what torch's FFT backend does with them"""
    sp = sp.to(dtype).clone()
    nb = sp.shape[2]
    sp[:, 1, 0] = 0
    if nb == n_fft // 2 + 1:
        sp[:, 1, -1] = 0
    pad = torch.zeros(sp.shape[0], 2, n_fft // 2 + 1 - nb, sp.shape[3], dtype=dtype)
    c = torch.view_as_complex(torch.cat([sp, pad], 2).permute(0, 2, 3, 1).contiguous())
    return torch.istft(c, n_fft=n_fft, hop_length=hop, window=window.to(dtype), center=True, length=L)


def point_fwd(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    err = (got - ref).pow(2).sum(1).sqrt()                       # (n_sig, nb, n_frames)
    peak = ref.pow(2).sum(1).sqrt().amax(1, keepdim=True)        # per signal and frame
    return float((err / peak).max())


def point_inv(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    return float(((got - ref).abs() / ref.abs().amax(1, keepdim=True)).max())


def check(got, ref, f32, point, what):
    whole, pt, e_whole, e_pt = rel_rms(got, ref), point(got, ref), rel_rms(f32, ref), point(f32, ref)
    print("%s: whole %.3g (e32 %.3g), worst point %.3g (e32 %.3g)" % (what, whole, e_whole, pt, e_pt))
    assert got.shape == ref.shape and not torch.isnan(got).any(), what
    assert whole <= FACTOR * e_whole, (what, whole, e_whole)
    assert pt <= FACTOR * e_pt, (what, pt, e_pt)


def check_fwd(dev, x, n_fft, hop, nb, w, what):
    got = ops.stft(dev.t(x), n_fft, hop, nb, window=dev.t(w)).cpu()
    check(got, ref_stft(x, n_fft, hop, nb, w), ref_stft(x, n_fft, hop, nb, w, torch.float32), point_fwd, what)
    return got


def check_inv(dev, sp, n_fft, hop, L, w, what):
    got = ops.istft(dev.t(sp), n_fft, hop, L, window=dev.t(w)).cpu()
    check(got, ref_istft(sp, n_fft, hop, L, w), ref_istft(sp, n_fft, hop, L, w, torch.float32), point_inv, what)
    return got


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def noise(n_sig, L, seed):
    return torch.randn(n_sig, L, generator=torch.Generator().manual_seed(seed))


def spectrum(n_sig, L, n_fft, hop, nb, w, seed):
    """the fp32 spectrum of noise, with Im(DC) (and Im(Nyquist) in a full band) non-zero as the U-Net's output has them"""
    sp = ref_stft(noise(n_sig, L, seed), n_fft, hop, nb, w).float()
    sp[:, 1, 0, :] = 0.37
    if nb == n_fft // 2 + 1:
        sp[:, 1, -1, :] = -0.21
    return sp


# ---- asymmetric window -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,L", SIZES)
def test_asymmetric_window_forward(dev, n_fft, hop, L):
    """Noise through a window with w[i] != w[N - i], full band; the frame-major output is the same bits.
    Measured whole / worst point (e32 in brackets), in the order of SIZES:
      emulator  1.17e-7 (1.17e-7) / 1.31e-7 (1.31e-7); 1.29e-7 (1.27e-7) / 1.82e-7 (1.48e-7); 1.30e-7 (1.53e-7) / 1.54e-7 (1.91e-7);
                1.36e-7 (1.54e-7) / 1.82e-7 (1.68e-7); 9.63e-8 (9.29e-8) / 1.45e-7 (1.49e-7); 1.32e-7 (1.66e-7) / 1.69e-7 (2.18e-7)
      MI355X    1.15e-7 (1.18e-7) / 1.48e-7 (1.36e-7); 1.28e-7 (1.38e-7) / 1.53e-7 (1.94e-7); 1.29e-7 (1.32e-7) / 1.54e-7 (1.71e-7);
                1.35e-7 (1.39e-7) / 1.63e-7 (1.64e-7); 9.65e-8 (8.86e-8) / 1.42e-7 (1.37e-7); 1.32e-7 (1.34e-7) / 1.90e-7 (1.62e-7)"""
    w = asym_window(n_fft)
    x = noise(2, L, n_fft + 1)
    got = check_fwd(dev, x, n_fft, hop, n_fft // 2 + 1, w, "stft %d" % n_fft)
    fm = ops.stft(dev.t(x), n_fft, hop, window=dev.t(w), frame_major=True)
    assert torch.equal(bits(fm.transpose(2, 3)), bits(got))


@pytest.mark.parametrize("n_fft,hop,L", SIZES)
def test_asymmetric_window_inverse(dev, n_fft, hop, L):
    """The inverse multiplies by the same window and divides by its overlap-added square; full band.
    Measured whole / worst point (e32 in brackets), in the order of SIZES:
      emulator  8.88e-8 (9.48e-8) / 1.50e-7 (1.50e-7); 9.54e-8 (9.98e-8) / 1.51e-7 (1.82e-7); 8.82e-8 (9.62e-8) / 1.40e-7 (1.33e-7);
                9.45e-8 (1.05e-7) / 1.36e-7 (2.01e-7); 1.07e-7 (9.64e-8) / 1.80e-7 (1.29e-7); 1.13e-7 (1.50e-7) / 1.98e-7 (2.60e-7)
      MI355X    9.07e-8 (8.39e-8) / 1.51e-7 (1.52e-7); 9.57e-8 (1.08e-7) / 1.45e-7 (1.79e-7); 8.77e-8 (9.33e-8) / 1.40e-7 (1.72e-7);
                9.41e-8 (9.88e-8) / 1.88e-7 (1.36e-7); 9.44e-8 (9.38e-8) / 1.31e-7 (1.27e-7); 1.14e-7 (1.15e-7) / 2.00e-7 (1.95e-7)"""
    w = asym_window(n_fft)
    check_inv(dev, spectrum(2, L, n_fft, hop, n_fft // 2 + 1, w, n_fft + 2), n_fft, hop, L, w, "istft %d" % n_fft)


# ---- frame-major inverse ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,L", SIZES + [(1024, 150, 777), (60, 15, 131), (4096, 1001, 3075)])
def test_frame_major_inverse_is_the_bin_major_inverse(dev, n_fft, hop, L):
    """istft(frame_major=True) of the transposed planes (MDXModel.istft_tf's layout: bins contiguous) = the bin-major call, bit for bit;
    the six sizes, and an odd L with a hop that is no multiple of 4 (the scalar overlap-add) on three kernels; band cut to 3/4."""
    w = asym_window(n_fft)
    nb = 3 * (n_fft // 2) // 4
    sp = dev.t(spectrum(2, L, n_fft, hop, nb, w, n_fft + 3))
    a = ops.istft(sp, n_fft, hop, L, window=dev.t(w))
    b = ops.istft(sp.transpose(2, 3).contiguous(), n_fft, hop, L, frame_major=True, window=dev.t(w))
    assert a.shape == (2, L) and not torch.isnan(a).any() and torch.equal(bits(a), bits(b))


# ---- overlap-add variants --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [4096, 4097, 4098])
def test_both_overlap_add_kernels(dev, L):
    """n_fft = 64, hop = 16: L = 4096 takes istft_ola4_kernel (L, hop multiples of 4, n_fft of 8: four samples per thread, eight
    workgroups); L = 4097 and 4098 take the scalar kernel over the same 257 frames.  Against float64 over the whole signal and over the
    first and the last n_fft samples alone, where fewer frames overlap.
    Measured: every figure between 6.2e-8 and 8.1e-8 (whole) and 9.5e-8 and 1.5e-7 (worst point) on the emulator and on the MI355X; the
    worst ratio to e32 is 1.32 (emulator, L = 4097, head, point: 1.45e-7 against 1.10e-7) and 1.37 (MI355X, L = 4096, head, point:
    1.36e-7 against 9.93e-8)."""
    n_fft, hop = 64, 16
    w = asym_window(n_fft)
    sp = spectrum(2, L, n_fft, hop, n_fft // 2 + 1, w, L)
    got = ops.istft(dev.t(sp), n_fft, hop, L, window=dev.t(w)).cpu()
    ref, f32 = ref_istft(sp, n_fft, hop, L, w), ref_istft(sp, n_fft, hop, L, w, torch.float32)
    for name, sl in (("whole", slice(None)), ("head", slice(0, n_fft)), ("tail", slice(L - n_fft, L))):
        check(got[:, sl], ref[:, sl], f32[:, sl], point_inv, "ola L %d %s" % (L, name))


# ---- tonal input, per-bin bar ----------------------------------------------------------------------------------------------------
def tones(n_fft, nb, L, seed):
    """bin-centred, between two bins, two bins under the top of the kept band; DC offset; noise 60 dB under the tones"""
    n = torch.arange(L, dtype=torch.float64)
    k1, k2, k3 = nb // 5, nb // 2 + 0.5, nb - 3 + 0.3
    s = [torch.cos(2 * torch.pi * k * n / n_fft + ph) for k, ph in ((k1, 0.3), (k2, 1.1), (k3, 2.0))]
    x = 0.25 + s[0] + 0.5 * s[1] + 0.8 * s[2] + 1e-3 * torch.randn(2, L, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    x[1] = x[1].flip(0) * 0.7
    return x.float()


@pytest.mark.parametrize("n_fft,hop,L,nb", [(7680, 1024, 5120, 3072), (1024, 160, 800, 513), (2000, 250, 1500, 600)])
def test_tonal_input_per_bin_and_per_sample(dev, n_fft, hop, L, nb):
    """Three sinusoids + DC + a noise floor at -60 dB, the asymmetric window, the band the models keep (Voc_FT's 3072 of 3841 bins,
    RMVPE's full 513, 600 of 1001).  Forward: every (bin, frame) against the frame's spectral peak -- the floor between the tones is
    60 dB below it, so an error there that white noise would hide stands out.  Inverse of that spectrum, Im(DC) / Im(Nyquist) set
    non-zero: every sample against the signal's peak.
    Measured whole / worst point (e32 in brackets), forward then inverse:
      emulator  7680: 1.23e-7 (1.36e-7) / 1.11e-7 (9.22e-8), 9.31e-8 (1.10e-7) / 2.81e-7 (2.07e-7); 1024: 1.16e-7 (1.15e-7) / 1.26e-7
                (1.13e-7), 8.84e-8 (8.92e-8) / 1.54e-7 (1.50e-7); 2000: 1.01e-7 (1.26e-7) / 1.48e-7 (1.20e-7), 1.03e-7 (1.30e-7) / 2.21e-7 (2.38e-7)
      MI355X    7680: 1.20e-7 (1.31e-7) / 1.15e-7 (1.53e-7), 9.26e-8 (9.57e-8) / 1.99e-7 (1.86e-7); 1024: 1.18e-7 (1.23e-7) / 1.37e-7
                (1.30e-7), 9.17e-8 (8.36e-8) / 1.98e-7 (1.45e-7); 2000: 1.04e-7 (1.01e-7) / 1.48e-7 (1.28e-7), 1.05e-7 (1.03e-7) / 2.21e-7 (2.06e-7)"""
    w = asym_window(n_fft)
    x = tones(n_fft, nb, L, n_fft)
    check_fwd(dev, x, n_fft, hop, nb, w, "tonal stft %d" % n_fft)
    sp = ref_stft(x, n_fft, hop, nb, w).float()
    sp[:, 1, 0, :] = 0.37
    if nb == n_fft // 2 + 1:
        sp[:, 1, -1, :] = -0.21
    check_inv(dev, sp, n_fft, hop, L, w, "tonal istft %d" % n_fft)


# ---- batches that share workgroups -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames", [5, 6, 7])
@pytest.mark.parametrize("n_sig", [1, 3, 5])
def test_signals_of_a_batch_equal_single_calls(dev, n_sig, n_frames):
    """RMVPE's plan (n_fft 1024, hop 160: four frames per workgroup) with 5, 6, 7 frames per signal: a workgroup holds frames of two
    signals and the last one is ragged.  Signal s of the batch = the call with that signal alone, bit for bit, forward and inverse;
    the batch against float64.
    Measured over the nine cases, emulator and MI355X alike: forward 1.13e-7 .. 1.18e-7 whole, 1.32e-7 .. 2.34e-7 worst point; inverse
    8.6e-8 .. 9.2e-8 whole, 1.16e-7 .. 1.93e-7 worst point; the worst ratio to e32 is 1.59 (emulator, 1 x 7, forward, point: 2.34e-7
    against 1.47e-7) and 1.37 (MI355X, 1 x 7, inverse, point: 1.62e-7 against 1.18e-7)."""
    n_fft, hop = 1024, 160
    L = hop * (n_frames - 1) + 37
    w, wd = asym_window(n_fft), dev.t(asym_window(n_fft))
    x = noise(n_sig, L, 10 * n_sig + n_frames)
    got = check_fwd(dev, x, n_fft, hop, 513, w, "batch stft %d x %d" % (n_sig, n_frames))
    assert got.shape == (n_sig, 2, 513, n_frames)
    sp = spectrum(n_sig, L, n_fft, hop, 513, w, 20 * n_sig + n_frames)
    inv = check_inv(dev, sp, n_fft, hop, L, w, "batch istft %d x %d" % (n_sig, n_frames))
    for s in range(n_sig):
        assert torch.equal(bits(ops.stft(dev.t(x[s:s + 1]), n_fft, hop, 513, window=wd)), bits(got[s:s + 1])), s
        assert torch.equal(bits(ops.istft(dev.t(sp[s:s + 1]), n_fft, hop, L, window=wd)), bits(inv[s:s + 1])), s


# ---- truncated band --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,L,nb", [(7680, 1024, 4096, 3072), (1024, 160, 640, 300), (2000, 250, 1500, 600), (60, 16, 128, 1)])
def test_truncated_band_is_the_zero_padded_full_band(dev, n_fft, hop, L, nb):
    """istft with n_bins_in < n_fft / 2 + 1 = istft of the same planes padded with zero bins to the full band, bit for bit (both layouts)."""
    w = asym_window(n_fft)
    sp = spectrum(2, L, n_fft, hop, nb, w, n_fft + nb)
    full = torch.cat([sp, torch.zeros(2, 2, n_fft // 2 + 1 - nb, sp.shape[3])], 2)
    a = ops.istft(dev.t(sp), n_fft, hop, L, window=dev.t(w))
    b = ops.istft(dev.t(full), n_fft, hop, L, window=dev.t(w))
    c = ops.istft(dev.t(full).transpose(2, 3).contiguous(), n_fft, hop, L, frame_major=True, window=dev.t(w))
    assert not torch.isnan(a).any() and torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c))
