"""aicg_resample_poly_mc / ops.resample_poly: the per-channel polyphase resampler (csrc/dsp.hip) against scipy.signal.resample_poly.

Reference: scipy in float64 on the float64 signal.  Tolerance: d32, the largest distance of scipy's OWN float32 run (float32 signal,
hence float32 filter and sums) from that reference over all the cases below, times 4 -- the kernel sums the same <= 22 float32
products per output in another, fixed order.  d32 is computed here, once per session, never taken from the kernel."""
import functools
import math

import numpy as np
import pytest
import torch
from scipy import signal

from aicovergen_amd import _lib, ops

RATIOS = [(147, 160), (160, 147), (441, 320), (6, 5), (4, 5), (2, 1), (1, 3)]
LENGTHS = [1, 7, 4097, 50001]
CHANNELS = [1, 2, 3]


@functools.lru_cache(maxsize=None)
def signal_of(c, n):
    """Seeded white noise under a slow envelope, peak 1.0: (c, n) float64 holding float32 values on the 16-bit PCM grid (so that the
    PCM form of the same samples exists)."""
    rng = np.random.default_rng(1000 * c + n)
    t = np.arange(n) / 44100.0
    x = rng.standard_normal((c, n)) * (0.55 + 0.45 * np.sin(2 * np.pi * 1.5 * t + np.arange(c)[:, None]))
    x /= np.abs(x).max()
    pcm = np.clip(np.rint(x * 32767.0), -32768, 32767).astype(np.int16)
    pcm.flat[np.abs(pcm).argmax()] = -32768            # peak exactly 1.0
    pcm.setflags(write=False)
    return pcm


def as_f32(pcm):
    return pcm.astype(np.float32) / np.float32(32768.0)


@functools.lru_cache(maxsize=None)
def reference(c, n, up, down):
    y = signal.resample_poly(as_f32(signal_of(c, n)).astype(np.float64), up, down, axis=1)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def d32_of(up, down):
    """scipy's float32 run against the float64 reference, for one ratio over every shape."""
    return max(float(np.abs(signal.resample_poly(as_f32(signal_of(c, n)), up, down, axis=1).astype(np.float64) - reference(c, n, up, down)).max())
               for c in CHANNELS for n in LENGTHS)


@functools.lru_cache(maxsize=None)
def d32():
    return max(d32_of(up, down) for up, down in RATIOS)


def run(dev, x, up, down):
    """The rates only matter through their ratio: (sr_in, sr_out) = (down, up)."""
    return ops.resample_poly(dev.t(torch.from_numpy(np.array(x, order="C"))), down, up).cpu().numpy()


@pytest.mark.parametrize("up,down", RATIOS)
def test_against_scipy(dev, up, down):
    worst = 0.0
    for c in CHANNELS:
        for n in LENGTHS:
            pcm = signal_of(c, n)
            want = reference(c, n, up, down)
            got = run(dev, as_f32(pcm), up, down)
            assert got.dtype == np.float32 and got.shape == want.shape == (c, math.ceil(n * up / down)), (c, n)
            dist = float(np.abs(got - want).max())
            worst = max(worst, dist)
            assert dist <= 4 * d32(), "(%d, %d) at %d/%d: %.3e from scipy float64, d32 %.3e" % (c, n, up, down, dist, d32())
            assert np.array_equal(got, run(dev, as_f32(pcm), up, down)), "two runs differ"
            assert np.array_equal(got, run(dev, pcm.T, up, down)), "PCM-16 and fp32 forms of the same samples differ"
    print("resample_poly %d/%d: kernel %.3e, scipy float32 %.3e at this ratio, d32 %.3e over all" % (up, down, worst, d32_of(up, down), d32()))
    assert worst > 0 or up == down      # the comparison saw two different computations


@pytest.mark.parametrize("c,n,up,down,why", [
    (3, 800001, 147, 160, "718 tiles of 1024 outputs a channel on 682 workgroups: a workgroup's second tile"),
    (3, 520001, 441, 320, "700 tiles on 682 workgroups, the large table"),
    (2, 50001, 1, 40, "the input of 1024 outputs does not fit beside the table: tiles of 512"),
    (2, 50001, 1, 100, "tiles of 256, the smallest"),
], ids=["second_tile", "second_tile_large_table", "tile_512", "tile_256"])
def test_other_paths_of_the_launch(dev, c, n, up, down, why):
    """Sizes at which the launch takes a path the cases above do not reach; same reference, same tolerance (d32 of those cases)."""
    x = as_f32(signal_of(c, n))
    want = signal.resample_poly(x.astype(np.float64), up, down, axis=1)
    got = run(dev, x, up, down)
    assert got.shape == want.shape
    dist = float(np.abs(got - want).max())
    print("resample_poly %d/%d (%d, %d): kernel %.3e, d32 %.3e" % (up, down, c, n, dist, d32()))
    assert dist <= 4 * d32(), why
    assert np.array_equal(got[c - 1], run(dev, x[c - 1:], up, down)[0]), why


@pytest.mark.parametrize("up,down", RATIOS)
def test_channels_are_independent(dev, up, down):
    for n in LENGTHS:
        x = as_f32(signal_of(3, n))
        all3 = run(dev, x, up, down)
        for c in range(3):
            assert np.array_equal(all3[c], run(dev, x[c:c + 1], up, down)[0]), (n, c)


@pytest.mark.parametrize("up,down", RATIOS)
def test_impulses_land_where_scipy_puts_them(dev, up, down):
    """`pre` and n_out: an impulse at sample 0 and one at n - 1 give scipy's (float32-rounded) filter taps at scipy's positions."""
    for n in LENGTHS:
        for pos in {0, n - 1}:
            x = np.zeros((1, n), np.float32)
            x[0, pos] = 1.0
            want = signal.resample_poly(x.astype(np.float64), up, down, axis=1)
            got = run(dev, x, up, down)
            assert got.shape == want.shape
            # one product per output, so the only error is the float32 filter's: two roundings (firwin's value, then its product
            # with `up`) of a tap below 2, half an ulp = 2^-24 each.  A shift by one sample would show as ~the tap height.
            assert np.abs(want).max() > 0.01 and np.abs(got - want).max() <= 2.0 ** -23, (n, pos)


def test_same_rate_launches_nothing(dev, monkeypatch):
    monkeypatch.setattr(ops, "_call", lambda *a, **k: pytest.fail("a kernel was launched"))
    pcm = signal_of(2, 7)
    x = dev.t(torch.from_numpy(as_f32(pcm)))
    assert ops.resample_poly(x, 44100, 44100) is x
    y = ops.resample_poly(dev.t(torch.from_numpy(np.ascontiguousarray(pcm.T))), 48000, 48000)
    assert y.dtype == torch.float32 and y.is_contiguous() and np.array_equal(y.cpu().numpy(), as_f32(pcm))


def test_error_codes(dev):
    """Through the return code; nothing is launched (the buffers are far too small for what the arguments claim)."""
    lib = _lib.get()
    x = dev.t(torch.zeros(2, 64))
    y = dev.t(torch.zeros(2, 64))
    hp = dev.t(torch.zeros(4, 4))

    def rc(xp=x.data_ptr(), fmt=1, yp=y.data_ptr(), c=2, n_in=64, n_out=64, up=1, down=1, hpp=hp.data_ptr(), taps=4, pre=0):
        return lib.aicg_resample_poly_mc(xp, fmt, yp, c, n_in, n_out, up, down, hpp, taps, pre, None)
    assert rc() == 0
    dev.sync()
    E_SHAPE, E_ARG, E_LDS = -1, -2, -4
    assert rc(c=0) == E_SHAPE and b"aicg_resample_poly_mc" in lib.aicg_last_error()
    assert rc(up=0) == E_ARG and rc(down=0) == E_ARG and rc(taps=0) == E_ARG and rc(pre=-1) == E_ARG
    assert rc(fmt=2) == E_ARG
    assert rc(n_out=65) == E_SHAPE                      # ceil(64 * 1 / 1) = 64
    assert rc(up=2, down=3, n_out=44) == E_SHAPE        # ceil(128 / 3) = 43
    assert rc(n_in=-1) == E_SHAPE
    assert rc(xp=None) == E_ARG and rc(yp=None) == E_ARG and rc(hpp=None) == E_ARG
    assert rc(up=48000, down=44101, taps=21, n_out=8) == E_LDS and b"LDS" in lib.aicg_last_error()
    # the ends of the argument range: nothing the geometry multiplies can leave its type
    big = 2 ** 31 - 1
    assert rc(down=2 ** 20 + 1) == E_ARG and rc(down=big, n_in=2 ** 40 - 1, pre=2 ** 40 - 1) == E_ARG
    assert rc(up=big, n_in=2 ** 40 - 1, n_out=8) == E_LDS and rc(taps=big) == E_LDS
    assert rc(n_in=2 ** 40) == E_SHAPE and rc(pre=2 ** 40) == E_SHAPE and rc(n_in=2 ** 40 - 1, up=2, n_out=2 ** 40) == E_SHAPE
    # the binding reaches the same code for a pair of rates whose table cannot fit
    with pytest.raises(RuntimeError, match=r"aicg_resample_poly_mc failed \(-4\)"):
        ops.resample_poly(x, 44101, 48000)
    with pytest.raises(TypeError):
        ops.resample_poly(dev.t(torch.zeros(2, 8, dtype=torch.float64)), 48000, 44100)
    with pytest.raises(ValueError, match="contiguous"):
        ops.resample_poly(dev.t(torch.zeros(8, 2)).t(), 48000, 44100)
    assert ops.resample_poly(dev.t(torch.zeros(2, 0)), 48000, 44100).shape == (2, 0)
