"""csrc/select.hip: exact order statistics of |x| (radix select), numpy's quantile on top of them, the division by a device scalar and
the nan-median over a few rows.  The bar is numpy's bits.  Where numpy itself gives NaN (a NaN in the data, or an infinite neighbour
the interpolation subtracts from: inf - inf, inf * 0) a NaN is asked for, whatever its payload; everything else is compared as bit
patterns.  The quantile comparison needs numpy 2.x, whose index arithmetic ops.quantile_plan restates."""
import warnings

import numpy as np
import pytest
import torch

from aicovergen_amd import _lib, ops

TILE = 2048                 # kSelectTile: the elements a workgroup histograms per step
LENGTHS = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 1001, TILE - 1, TILE, TILE + 1, 65537, 160001)
BIG = (3840000, (1 << 24) + 3)          # a 240 s track; where float32(n - 1) * float32(0.999) moves the rank
KINDS = ("gauss", "equal", "levels", "mix", "nan")
_inputs = {}

needs_numpy2 = pytest.mark.skipif(not ops.numpy_quantile_mirrored(), reason="ops.quantile_plan restates numpy 2.x")


def make(kind, n):
    """One array per (kind, n), shared by the tests and never written to."""
    if (kind, n) not in _inputs:
        rng = np.random.default_rng(n % 100003 + 7 * KINDS.index(kind))
        if kind == "gauss":
            x = rng.standard_normal(n).astype(np.float32)
        elif kind == "equal":
            x = np.full(n, -0.37, dtype=np.float32)
        elif kind == "levels":      # 8 levels, long runs of duplicates; the levels differ in every digit the passes look at
            x = (np.array([0.0, 1e-30, 3e-5, 0.11, 0.5, 0.5000001, 1.0, 77.0], dtype=np.float32)[rng.integers(0, 8, n)]
                 * rng.choice(np.array([-1, 1], dtype=np.float32), n))
        elif kind == "mix":         # negatives, -0.0, denormals, one +inf
            x = rng.standard_normal(n).astype(np.float32)
            x[rng.random(n) < 0.2] = -0.0
            d = rng.random(n) < 0.2
            x[d] = (rng.integers(1, 1 << 23, n).astype(np.uint32).view(np.float32) * rng.choice(np.array([-1, 1], dtype=np.float32), n))[d]
            x[rng.integers(0, n)] = np.inf
        else:
            x = rng.standard_normal(n).astype(np.float32)
            x[rng.integers(0, n)] = np.nan
        _inputs[kind, n] = x
    return _inputs[kind, n]


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return got.shape == want.shape and bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))


def lengths(dev):
    return LENGTHS + (BIG if dev.big else ())


def np_quantile(x, q):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")         # inf - inf inside numpy's _lerp
        want = np.quantile(np.abs(x), q)
    assert want.dtype == np.float32
    return want


@pytest.mark.parametrize("kind", KINDS)
def test_abs_select_equals_the_sorted_array(dev, kind):
    for n in lengths(dev):
        x = make(kind, n)
        s = np.sort(np.abs(x))
        lo, hi, _ = ops.quantile_plan(n, 0.999)
        for a, b in {(lo, hi), (0, min(1, n - 1)), (n // 2, n // 2), (n - 1, n - 1)}:
            got = ops.abs_select(dev.t(torch.from_numpy(x)), a, b).cpu().numpy()
            want = np.full(2, np.nan, dtype=np.float32) if kind == "nan" else s[[a, b]]
            assert same_bits(got, want), (n, a, b, got, want)
        if kind == "nan":
            assert np.isnan(s[-1])


@needs_numpy2
@pytest.mark.parametrize("kind", KINDS)
def test_abs_quantile_has_numpys_bits(dev, kind):
    for n in lengths(dev):
        x = make(kind, n)
        got = ops.abs_quantile(dev.t(torch.from_numpy(x)), 0.999)
        assert got.dim() == 0 and got.dtype == torch.float32 and got.device.type == dev.device.type
        want = np_quantile(x, 0.999)
        assert same_bits(got.cpu().numpy(), want), (n, got, want)
        if kind == "nan":
            assert np.isnan(want)


@needs_numpy2
@pytest.mark.parametrize("q", [0.5, 1.0, 0.0, 0.25])
def test_abs_quantile_at_other_q(dev, q):
    for kind in ("gauss", "levels"):
        for n in (1, 2, 3, 64, 257, 1001, TILE + 1, 65537):
            x = make(kind, n)
            assert same_bits(ops.abs_quantile(dev.t(torch.from_numpy(x)), q).cpu().numpy(), np_quantile(x, q)), (kind, n)


@needs_numpy2
def test_quantile_plan_is_numpys_at_the_issue_lengths():
    """The weight shows itself where sorted |x| is 0 .. n - 1: the quantile IS the virtual index then, in numpy's own arithmetic."""
    for n in (1001, 160001):
        lo, hi, t = ops.quantile_plan(n, 0.999)
        assert hi == lo + 1 and float(t) == 0.0
    lo, hi, t = ops.quantile_plan((1 << 24) + 3, 0.999)
    assert float(lo) + float(t) == 16760441.0       # the float32 product of 2^24 + 2 and float32(0.999); the float64 product is 16760440.78
    for n in (1, 2, 1000, 1001, 65537):
        s = np.arange(n, dtype=np.float32)
        lo, hi, t = ops.quantile_plan(n, 0.999)
        d = s[hi] - s[lo]
        assert same_bits(s[hi] - d * (np.float32(1) - t) if t >= 0.5 else s[lo] + d * t, np.quantile(s, 0.999))


def test_out_of_range_lengths_are_refused(dev):
    with pytest.raises(ValueError):
        ops.abs_select(dev.t(torch.zeros(0)), 0, 0)
    with pytest.raises(ValueError):
        ops.abs_select(dev.t(torch.zeros(4)), 2, 4)
    lib = _lib.get()
    assert lib.aicg_abs_select_workspace_bytes(0) == -1 and lib.aicg_abs_select_workspace_bytes((1 << 27) + 1) == -1
    assert lib.aicg_abs_select_workspace_bytes(1) > 0 and lib.aicg_abs_select_workspace_bytes(1 << 27) > 0
    x = dev.t(torch.zeros(4))
    out = dev.t(torch.zeros(2))
    ws = dev.t(torch.zeros(lib.aicg_abs_select_workspace_bytes(4), dtype=torch.uint8))
    for n in (0, -5, (1 << 27) + 1):        # refused before anything is launched or read
        assert lib.aicg_abs_select_f32(x.data_ptr(), n, 0, 0, out.data_ptr(), ws.data_ptr(), None) == -1
    assert b"aicg_abs_select_f32" in lib.aicg_last_error()
    if dev.big:
        with pytest.raises(ValueError):
            ops.abs_select(torch.zeros((1 << 27) + 1, device=dev.device), 0, 0)


def test_largest_length(dev):
    if not dev.big:
        pytest.skip("2^27 elements run on the hardware only")
    n = 1 << 27
    x = torch.arange(n, device=dev.device, dtype=torch.int32).mul_(-1640531527).view(torch.float32)     # a bijection of the bit patterns
    x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    lo, hi, _ = ops.quantile_plan(n, 0.999)
    got = ops.abs_select(x, lo, hi).cpu().numpy()
    want = torch.sort(x.abs_()).values[[lo, hi]].cpu().numpy()
    assert same_bits(got, want)


def test_div_scalar_has_numpys_bits(dev):
    for n in (1, 257, 160001):
        x = make("gauss", n)
        for s in (np.float32(0.37), np.float32(3.0), np.float32(2.9360422e-3), np.float32(1e-39)):
            got = ops.div_scalar(dev.t(torch.from_numpy(x)), dev.t(torch.tensor(s))).cpu().numpy()
            with np.errstate(over="ignore"):
                assert same_bits(got, x / s), (n, s)
    mix = make("mix", 1001)
    with np.errstate(all="ignore"):
        assert same_bits(ops.div_scalar(dev.t(torch.from_numpy(mix)), dev.t(torch.tensor(np.float32(0.37)))).cpu().numpy(), mix / np.float32(0.37))


def median_stack(k, n):
    """Zeros, NaNs, ties, both infinities; column 0 all NaN, column 1 (where there is one) all -0.0: numpy's masked sum starts from
    +0, so it answers +0.  (Where +0 and -0 meet in one column their order after numpy's sort is the sort's own business; the values
    here are rounded to one decimal with the -0.0 that makes folded to +0.)"""
    rng = np.random.default_rng(100 * k + n)
    st = rng.standard_normal((k, n)).round(1) + 0.0
    for value, share in ((np.nan, 0.3), (np.inf, 0.1), (-np.inf, 0.1), (0.0, 0.1)):
        st[rng.random((k, n)) < share] = value
    st[:, 0] = np.nan
    if n > 1:
        st[:, 1] = -0.0
    return st


@pytest.mark.parametrize("k", range(1, 9))
def test_nanmedian_rows_equals_numpy(dev, k):
    for n in (1, 63, 64, 65, 1000):
        st = median_stack(k, n)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")     # All-NaN slice
            want = np.nanmedian(st, axis=0)
        got = ops.nanmedian_rows(dev.t(torch.from_numpy(st))).cpu().numpy()
        assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True), (k, n)
        assert np.array_equal(np.signbit(got) & ~np.isnan(got), np.signbit(want) & ~np.isnan(want))
        assert np.isnan(got[0])


def test_nanmedian_rows_refuses_nine_rows(dev):
    with pytest.raises(ValueError):
        ops.nanmedian_rows(dev.t(torch.zeros((9, 4), dtype=torch.float64)))
    with pytest.raises(ValueError):
        ops.nanmedian_rows(dev.t(torch.zeros((0, 4), dtype=torch.float64)))
    lib = _lib.get()
    assert lib.aicg_nanmedian_rows(None, 9, 4, None, None) == -1
