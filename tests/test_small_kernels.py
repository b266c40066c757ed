"""The small RMVPE / element-wise entry points (csrc/rmvpe.hip, csrc/elementwise.hip, dense_nt over csrc/gemm_nt.hip), each against a
float64 statement of the same operation on the same fp32 inputs.  Bar: 1e-6 relative RMS (test_gate_and_prior's) unless a test says
otherwise; every kernel at a size that is no multiple of its 256-thread workgroup and at size 1."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from aicovergen_amd import ops
from conftest import rel_rms


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("n", [1, 1000])
def test_complex_abs(dev, n):
    g = torch.Generator().manual_seed(n)
    re, im = torch.randn(3, n, generator=g) * 5, torch.randn(3, n, generator=g) * 5
    got = ops.complex_abs(dev.t(re), dev.t(im))
    assert got.shape == re.shape
    assert rel_rms(got, torch.sqrt(re.double() ** 2 + im.double() ** 2)) < 1e-6


def test_complex_abs_is_sqrt_of_the_fp32_sum_of_squares(dev):
    """The kernel is sqrtf(re * re + im * im) (reference rmvpe.py:314 `sqrt(real^2 + imag^2)` on fp32 tensors), NOT hypot: squares
    below fp32's range vanish (|1e-30 + 1e-30 i| = 0, not 1.4e-30) and squares above it overflow (|3e30 + 4e30 i| = inf, not 5e30).
    Magnitudes of audio spectra sit nowhere near either end; a change to hypot would be a decision, and this test would say so."""
    re = torch.tensor([1e-30, 3e30, 1e-30, 3e-20, 0.0, -3.0, 1e19, 1e-23])
    im = torch.tensor([1e-30, 4e30, 1.0, 4e-20, 0.0, 4.0, 1e19, 1e-23])
    got = ops.complex_abs(dev.t(re), dev.t(im)).cpu()
    assert got[0] == 0.0 and got[1] == float("inf")
    assert got[2] == 1.0 and got[4] == 0.0 and got[5] == 5.0
    exact = torch.sqrt(re.double() ** 2 + im.double() ** 2)
    assert abs(float(got[6]) / float(exact[6]) - 1) < 2e-7                  # 2e38 < FLT_MAX: the largest magnitudes still exact
    # squares in the subnormal range lose bits, or are flushed: 5e-20 comes back as 0 or within 1e-3, 1.4e-23 as 0 or within 10 %
    assert got[3] == 0.0 or abs(float(got[3]) / float(exact[3]) - 1) < 1e-3
    assert got[7] == 0.0 or abs(float(got[7]) / float(exact[7]) - 1) < 0.1


_ACTS = [ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LRELU, ops.ACT_GELU, ops.ACT_TANH, ops.ACT_SIGMOID, ops.ACT_LOGCLAMP]


def _act64(v, act):
    if act == ops.ACT_NONE:
        return v
    if act in (ops.ACT_RELU, ops.ACT_LRELU):                                  # channel_affine passes slope 0: leaky ReLU is ReLU
        return torch.relu(v)
    if act == ops.ACT_GELU:
        return 0.5 * v * (1.0 + torch.erf(v / 2.0 ** 0.5))
    if act == ops.ACT_TANH:
        return torch.tanh(v)
    if act == ops.ACT_SIGMOID:
        return torch.sigmoid(v)
    return torch.log(v.clamp_min(0.0))                                        # ACT_LOGCLAMP with the clamp channel_affine passes: 0


@pytest.mark.parametrize("act", _ACTS)
@pytest.mark.parametrize("shape", [(2, 5, 3, 7), (1, 1, 1, 1)])
def test_channel_affine(dev, shape, act):
    """act(x * scale[c] + shift[c]) per channel of (N, C, H, W): eval BatchNorm2d on RMVPE's input (rmvpe.py:92) with every activation
    code.  The entry point hands apply_act a slope / clamp of 0, so ACT_LRELU is ReLU and ACT_LOGCLAMP is log(max(v, 0)): -inf at
    v <= 0 -- asserted on one negative channel; the positive channels keep x * scale and shift of one sign, so no cancellation
    stands in front of the logarithm."""
    g = torch.Generator().manual_seed(act)
    x = torch.randn(shape, generator=g)
    c = shape[1]
    scale, shift = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    if act == ops.ACT_LOGCLAMP:
        x, shift = x.abs() + 0.1, shift.abs()
        if c > 1:
            scale[1], shift[1] = -scale[1], -shift[1]                         # channel 1: v < 0 everywhere
    got = ops.channel_affine(dev.t(x), dev.t(scale), dev.t(shift), act=act).cpu()
    v = x.double() * scale.double().view(1, c, 1, 1) + shift.double().view(1, c, 1, 1)
    ref = _act64(v, act)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin) and bool((got[~fin] == ref[~fin].float()).all())
    if act == ops.ACT_LOGCLAMP and c > 1:
        assert bool((~fin[:, 1]).all()) and bool(fin[:, 0].all())
    assert rel_rms(got[fin], ref[fin]) < 1e-6


@pytest.mark.parametrize("H,W", [(6, 10), (7, 10), (6, 11), (7, 11), (2, 2), (3, 3)])
def test_avgpool2x2_on_a_channel_slice(dev, H, W):
    """x = channels 2..4 of a (2, 7, H, W + 3) buffer cut to W columns: stride(0), stride(1) and stride(2) are not the packed ones,
    stride(3) == 1; odd H / W drop the last row / column as F.avg_pool2d does.  The rest of the buffer is NaN."""
    g = torch.Generator().manual_seed(H * 16 + W)
    buf = torch.full((2, 7, H, W + 3), float("nan"))
    x = torch.randn(2, 3, H, W, generator=g)
    buf[:, 2:5, :, :W] = x
    xd = dev.t(buf)[:, 2:5, :, :W]
    assert xd.stride(3) == 1 and xd.stride(1) != H * W and xd.stride(0) != 3 * H * W
    got = ops.avgpool2x2(xd)
    ref = F.avg_pool2d(x.double(), 2)
    assert got.shape == ref.shape
    assert rel_rms(got, ref) < 1e-6


@pytest.mark.parametrize("n", [1, 777])
def test_mul_and_axpbypcz(dev, n):
    """mul; alpha a + beta b + gamma c with every combination of absent b and c; out= aliasing a."""
    g = torch.Generator().manual_seed(n)
    a, b, c = (torch.randn(3, n, generator=g) for _ in range(3))
    al, be, ga = 0.75, -1.5, 0.3
    ad, bd, cd = dev.t(a), dev.t(b), dev.t(c)
    assert rel_rms(ops.mul(ad, bd), a.double() * b.double()) < 1e-6
    for hb, hc in itertools.product((False, True), repeat=2):
        ref = al * a.double() + (be * b.double() if hb else 0) + (ga * c.double() if hc else 0)
        got = ops.axpbypcz(ad, al, bd if hb else None, be, cd if hc else None, ga)
        assert rel_rms(got, ref) < 1e-6, (hb, hc)
        alias = dev.t(a.clone())
        out = ops.axpbypcz(alias, al, bd if hb else None, be, cd if hc else None, ga, out=alias)
        assert out.data_ptr() == alias.data_ptr() and torch.equal(bits(alias), bits(got)), (hb, hc)
    alias = dev.t(a.clone())
    ops.mul(alias, bd, out=alias)
    assert torch.equal(bits(alias), bits(ops.mul(ad, bd)))
    assert torch.equal(bits(ad), bits(a)) and torch.equal(bits(bd), bits(b)) and torch.equal(bits(cd), bits(c))   # inputs untouched


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("act", [ops.ACT_RELU, ops.ACT_SIGMOID])
@pytest.mark.parametrize("R,K,O", [(1, 4, 1), (131, 100, 37), (300, 36, 130), (77, 64, 40)])
def test_dense_nt(dev, R, K, O, act, with_bias):
    """act(x W^T + b) on aicg_gemm_nt with NULL row scale / shift (CREPE's Toeplitz layers: ReLU; its classifier: sigmoid) -- the
    epilogue test_linear_last_nt_gemm never takes; ragged rows (tile 128), K slabs (K a multiple of 4 only) and outputs (odd O: the
    scalar store; O = 40: the float4 store; O = 130: a second column tile).  Bar 1e-5, test_linear_last_nt_gemm's."""
    g = torch.Generator().manual_seed(R + K + O)
    x = torch.randn(R, K, generator=g)
    w, b = torch.randn(O, K, generator=g) * K ** -0.5, torch.randn(O, generator=g)
    got = ops.dense_nt(dev.t(x), dev.t(w), dev.t(b) if with_bias else None, act=act)
    assert got.shape == (R, O)
    z = x.double() @ w.double().t() + (b.double() if with_bias else 0)
    ref = torch.relu(z) if act == ops.ACT_RELU else torch.sigmoid(z)
    assert rel_rms(got, ref) < 1e-5
