"""The NT GEMM (csrc/gemm_nt.hip) at the forms production takes and the direct tests did not: the float4 ("wide") epilogue of an interior
128 x 128 tile with and without the per-channel affine (the TDF fallback at H = 48 / 32 / 24 / 12, CREPE's classifier), the
one-channel-per-MFMA-tile shortcut on both epilogues, a single partial K stage (K < 32), every activation, padded leading dimensions,
both tile orders, the refusals -- and the same forms on the split-precision twin.

Reference: `gemm_ref` in float64 on the fp32 operands --  act((A W^T + b) s[ch] + t[ch]) + res,  ch = (r / rows_per_ch) % n_ch.

Bar (fp32 kernel): the same expression evaluated by torch in float32 on the CPU has an error `e32` against float64; the kernel may
have 4 x that (an equally long fp32 summation in another order), in both measures:
  whole   relative RMS over the tensor;
  column  max over output columns o of (max over rows |got - ref|) / rms(ref[:, o]).
The split twin keeps the bar of tests/test_conv_split.py (its TOL, relative RMS).  Bit-equality takes no tolerance."""
import hashlib
import os
import subprocess
import sys

import pytest
import torch

from aicovergen_amd import _lib, ops
from conftest import rel_rms
from test_conv_split import TOL as SPLIT_TOL

FACTOR = 4.0
NAN = float("nan")

ACTS = {
    ops.ACT_NONE: lambda z: z,
    ops.ACT_RELU: torch.relu,
    ops.ACT_LRELU: torch.relu,                                        # the GEMM's ABI has no slope: apply_act(v, act, 0)
    ops.ACT_GELU: lambda z: 0.5 * z * (1 + torch.erf(z * 0.5 ** 0.5)),
    ops.ACT_TANH: torch.tanh,
    ops.ACT_SIGMOID: torch.sigmoid,
}   # AICG_ACT_LOGCLAMP is not listed: with the slope fixed at 0 it is log(max(v, 0)) = -inf on half the line, a form no caller can want


def make(R, K, O, n_ch, seed, bias=True, affine=True, res=True):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    p = dict(a=r(R, K), w=r(O, K) * K ** -0.5, b=r(O) * 0.5, s=torch.rand(n_ch, generator=g) + 0.5, t=r(n_ch) * 0.5, res=r(R, O))
    if not bias:
        p["b"] = None
    if not affine:
        p["s"] = p["t"] = None
    if not res:
        p["res"] = None
    return p


def gemm_ref(p, rows_per_ch, n_ch, act, dtype=torch.float64):
    c = lambda v: None if v is None else v.to(dtype)
    a, w, b, s, t, res = (c(p[k]) for k in ("a", "w", "b", "s", "t", "res"))
    z = a @ w.t()
    if b is not None:
        z = z + b
    if s is not None:
        ch = (torch.arange(a.shape[0]) // rows_per_ch) % n_ch
        z = z * s[ch, None] + t[ch, None]
    z = ACTS[act](z)
    return z if res is None else z + res


def padded(dev, m, pad):
    """(rows, n) -> the left n columns of a (rows, n + pad) buffer whose other columns are NaN"""
    buf = torch.full((m.shape[0], m.shape[1] + pad), NAN, dtype=torch.float32)
    buf[:, : m.shape[1]] = m
    return dev.t(buf)


def gemm(dev, p, rows_per_ch, n_ch, act, pads=(0, 0, 0, 0), fn="aicg_gemm_nt", rows=None):
    """The C ABI call; pads = extra columns of (a, w, c, res).  Returns the whole c buffer (R, O + pad), NaN where nothing was written.
    `rows`: only the first `rows` rows of a / res / c are handed over."""
    R, K = p["a"].shape if rows is None else (rows, p["a"].shape[1])
    O = p["w"].shape[0]
    a, w = padded(dev, p["a"][:R], pads[0]), padded(dev, p["w"], pads[1])
    res = None if p["res"] is None else padded(dev, p["res"][:R], pads[3])
    c = torch.full((R, O + pads[2]), NAN, dtype=torch.float32, device=dev.device)
    b, s, t = (None if p[k] is None else dev.t(p[k]) for k in ("b", "s", "t"))
    ptr = lambda v: 0 if v is None else v.data_ptr()
    st = torch.cuda.current_stream().cuda_stream if dev.kind == "hip" else 0
    _lib.call(fn, ptr(a), ptr(w), ptr(b), ptr(s), ptr(t), ptr(res), ptr(c), R, K, O, K + pads[0], K + pads[1], O + pads[2],
              O + pads[3], rows_per_ch, n_ch, act, st)
    dev.sync()
    return c.cpu()


def worst_column(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    return float(((got - ref).abs().amax(0) / ref.pow(2).mean(0).sqrt()).max())


def check(got, p, rows_per_ch, n_ch, act, what):
    ref, f32 = gemm_ref(p, rows_per_ch, n_ch, act), gemm_ref(p, rows_per_ch, n_ch, act, dtype=torch.float32)
    whole, col, e_whole, e_col = rel_rms(got, ref), worst_column(got, ref), rel_rms(f32, ref), worst_column(f32, ref)
    print("%s: whole %.3g (e32 %.3g), worst column %.3g (e32 %.3g)" % (what, whole, e_whole, col, e_col))
    assert not torch.isnan(got).any(), what
    assert whole <= FACTOR * e_whole, (what, whole, e_whole)
    assert col <= FACTOR * e_col, (what, col, e_col)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def head(p, R):
    return {k: (v[:R] if k in ("a", "res") and v is not None else v) for k, v in p.items()}


# ---- wide epilogue with affine and residual -------------------------------------------------------------------------------------
WIDE_AFFINE = [(256, 48, 384, 32, 3), (256, 24, 192, 32, 2), (384, 32, 256, 64, 4), (256, 12, 128, 32, 3)]


@pytest.mark.parametrize("R,K,O,rows_per_ch,n_ch", WIDE_AFFINE)
def test_wide_epilogue_with_affine_and_residual(dev, R, K, O, rows_per_ch, n_ch):
    """The TDF fallback's shapes (K = H, O = F, 32- / 64-row channels, K = 12 and 24: one partial K stage), bias + affine + ReLU +
    residual.  Three runs on the same rows: R rows (every tile interior: float4 epilogue), R + 32 rows (the last row tile is ragged and
    takes the scalar epilogue), and R rows with ldc = O + 1 (rows of c not 16-byte aligned: the scalar epilogue everywhere).  All
    against float64; the rows they share are bit-equal -- both epilogues apply the same fp32 operations in the same order to the same
    accumulator.  They are: bit-equal on the emulator and on the MI355X.
    Measured whole / worst column, emulator = MI355X to three digits; e32 in brackets: (256, 48, 384) 7.09e-8 (7.22e-8) / 1.13e-6 (1.13e-6);
    (256, 24, 192) 6.49e-8 (6.63e-8) / 8.34e-7 (9.42e-7); (384, 32, 256) 6.91e-8 (7.12e-8) / 1.05e-6 (1.07e-6); (256, 12, 128) 4.53e-8
    (4.84e-8) / 5.35e-7 (6.57e-7)."""
    p = make(R + 32, K, O, n_ch, R + K + O)
    short, long = gemm(dev, p, rows_per_ch, n_ch, ops.ACT_RELU, rows=R), gemm(dev, p, rows_per_ch, n_ch, ops.ACT_RELU)
    scalar = gemm(dev, p, rows_per_ch, n_ch, ops.ACT_RELU, pads=(0, 0, 1, 0), rows=R)
    check(short, head(p, R), rows_per_ch, n_ch, ops.ACT_RELU, "wide (%d, %d, %d)" % (R, K, O))
    check(long, p, rows_per_ch, n_ch, ops.ACT_RELU, "wide + ragged (%d, %d, %d)" % (R + 32, K, O))
    assert torch.equal(bits(long[:R]), bits(short))
    assert torch.equal(bits(scalar[:, :O]), bits(short)) and bool(torch.isnan(scalar[:, O]).all())


# ---- wide epilogue without affine (CREPE's classifier) --------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("act", [ops.ACT_RELU, ops.ACT_SIGMOID])
@pytest.mark.parametrize("R", [256, 131])
def test_wide_epilogue_without_affine(dev, R, act, with_bias):
    """ops.dense_nt at O = 360 (two interior column tiles and a ragged one), K = 64, R = 256 and 131 (three rows in a ragged tile).
    Measured, emulator = MI355X: ReLU 1.45e-7 / 5.72e-6 at worst, sigmoid 6.04e-8 / 7.58e-7; every figure within 1 % of its e32."""
    p = make(R, 64, 360, 1, R + act, bias=with_bias, affine=False, res=False)
    got = ops.dense_nt(dev.t(p["a"]), dev.t(p["w"]), None if p["b"] is None else dev.t(p["b"]), act=act)
    assert got.shape == (R, 360)
    check(got.cpu(), p, 1, 1, act, "dense_nt R %d act %d bias %d" % (R, act, with_bias))


# ---- one channel per MFMA tile on the scalar epilogue ---------------------------------------------------------------------------
def test_channel_per_tile_on_the_scalar_epilogue(dev):
    """O = 40 (no interior tile), 32-row channels: the scalar epilogue takes one (scale, shift) per 32-row MFMA tile.  16-row channels
    with every entry doubled are the same mathematics through the per-element branch: bit-equal.  Through ops.linear_last, too.
    Measured, emulator = MI355X: 6.41e-8 / 6.77e-7 (e32 6.66e-8 / 6.24e-7 on the emulator's host, 6.25e-8 / 6.24e-7 on the MI355X's)."""
    R, K, O, n_ch = 200, 36, 40, 3
    p = make(R, K, O, n_ch, 77)
    per_tile = gemm(dev, p, 32, n_ch, ops.ACT_RELU)
    check(per_tile, p, 32, n_ch, ops.ACT_RELU, "per tile")
    q = dict(p, s=p["s"].repeat_interleave(2), t=p["t"].repeat_interleave(2))
    assert torch.equal(bits(gemm(dev, q, 16, 2 * n_ch, ops.ACT_RELU)), bits(per_tile))
    # (B, C, T, F) = (2, 3, 32, K): 192 rows of the same problem through the wrapper the models call
    d = lambda v: dev.t(v.contiguous())
    via = ops.linear_last(d(p["a"][:192].view(2, 3, 32, K)), d(p["w"]), d(p["b"]), d(p["s"]), d(p["t"]), act=ops.ACT_RELU,
                          res=d(p["res"][:192].view(2, 3, 32, O)))
    assert torch.equal(bits(via.view(192, O)), bits(per_tile[:192]))


# ---- every activation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("R,K,O", [(256, 36, 128), (131, 36, 40)])
def test_every_activation(dev, R, K, O, act):
    """(256, 36, 128): the float4 epilogue; (131, 36, 40): the scalar one.  Bias, affine over 32-row channels, activation, residual.
    Measured (whole / worst column), emulator and MI355X: between 3.76e-8 / 1.93e-7 (sigmoid) and 8.62e-8 / 1.07e-6 (none, GELU); the
    worst ratio to e32 is 1.11 (GELU, column, wide: 1.07e-6 against 9.66e-7) on both."""
    p = make(R, K, O, 3, R + 10 * act)
    check(gemm(dev, p, 32, 3, act), p, 32, 3, act, "act %d (%d, %d, %d)" % (act, R, K, O))


# ---- padded leading dimensions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["aicg_gemm_nt", "aicg_gemm_nt_split"])
@pytest.mark.parametrize("R,K,O", [(256, 36, 128), (131, 36, 40)])
def test_padded_leading_dimensions(dev, R, K, O, fn):
    """lda = K + 4, ldw = K + 8, ldc = O + 4, ldr = O + 12, the pads of a, w and res NaN and c NaN beforehand: the result is the
    contiguous run's bit for bit and the pad columns of c are still NaN."""
    p = make(R, K, O, 3, R + K)
    plain = gemm(dev, p, 32, 3, ops.ACT_RELU, fn=fn)
    wide = gemm(dev, p, 32, 3, ops.ACT_RELU, pads=(4, 8, 4, 12), fn=fn)
    assert not torch.isnan(plain).any()
    assert torch.equal(bits(wide[:, :O]), bits(plain))
    assert bool(torch.isnan(wide[:, O:]).all())


# ---- tile order and epilogue switches --------------------------------------------------------------------------------------------
def _order_case_digest():
    """3 x 2 tiles (R = 300, O = 200), K = 36, 32-row channels: tile (0, 0) and (1, 0) are interior.  sha256 of the result's bytes."""
    import conftest
    conftest._bind("emu")
    dev = conftest.Dev("emu")
    p = make(300, 36, 200, 3, 300)
    got = gemm(dev, p, 32, 3, ops.ACT_RELU)
    check(got, p, 32, 3, ops.ACT_RELU, "order case")
    return hashlib.sha256(got.numpy().tobytes()).hexdigest()


def test_tile_order_and_epilogue_switches_on_the_emulator():
    """AICG_GEMM_ORDER = 0 / 1 (row-major tiles / column tiles dealt to the XCDs) x AICG_GEMM_WIDE = 0 / 1 give the same bits.  The
    switches are read once per process (AICG_SWITCH is a function-local static) and only by a library built with AICG_DEV_SWITCHES --
    the emulator; in the product library they are compile-time constants -- so this test has no hardware variant and runs one child
    per setting, all four at once."""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path.insert(0, %r); import conftest, test_gemm_nt_forms as m; print('digest', m._order_case_digest())" % tests
    kids = [(o, w, subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, AICG_GEMM_ORDER=str(o), AICG_GEMM_WIDE=str(w)),
                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)) for o in (0, 1) for w in (0, 1)]
    digests = {}
    for o, w, kid in kids:
        out, err = kid.communicate(timeout=600)
        assert kid.returncode == 0, out + err
        digests[(o, w)] = [ln.split()[1] for ln in out.splitlines() if ln.startswith("digest ")][0]
    assert len(set(digests.values())) == 1, digests


# ---- refusals --------------------------------------------------------------------------------------------------------------------
REFUSALS = {                         # K, lda, operands passed as NULL, rows_per_ch, error code
    "K_6": (6, 8, (), 32, -1),
    "lda_K_plus_2": (8, 10, (), 32, -1),
    "scale_without_shift": (8, 8, ("t",), 32, -2),
    "rows_per_ch_0": (8, 8, (), 0, -2),
}


@pytest.mark.parametrize("fn", ["aicg_gemm_nt", "aicg_gemm_nt_split"])
@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(dev, name, fn):
    """K or lda no multiple of 4 (float4 loads): AICG_E_SHAPE; half an affine, or an affine without rows_per_ch: AICG_E_ARG.  Nothing is
    launched: c keeps its contents."""
    K, lda, drop, rows_per_ch, code = REFUSALS[name]
    R, O = 40, 24
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev.device)
    d = dict(a=z(R, lda + 4), w=z(O, K + 4), b=z(O), s=z(3), t=z(3), res=z(R, O))
    c = torch.full((R, O), 7.0, dtype=torch.float32, device=dev.device)
    ptr = lambda k: 0 if k in drop else d[k].data_ptr()
    st = torch.cuda.current_stream().cuda_stream if dev.kind == "hip" else 0
    with pytest.raises(RuntimeError, match=r"%s failed \(%d\)" % (fn, code)):
        _lib.call(fn, ptr("a"), ptr("w"), ptr("b"), ptr("s"), ptr("t"), ptr("res"), c.data_ptr(), R, K, O, lda, K, O, O, rows_per_ch, 3,
                  ops.ACT_RELU, st)
    dev.sync()
    assert bool((c.cpu() == 7.0).all())


@pytest.mark.parametrize("fn", ["aicg_gemm_nt", "aicg_gemm_nt_split"])
def test_no_rows_is_no_error_and_no_write(dev, fn):
    p = make(8, 8, 24, 3, 1)
    c = torch.full((8, 24), 7.0, dtype=torch.float32, device=dev.device)
    a, w, b, s, t, res = (dev.t(p[k]) for k in ("a", "w", "b", "s", "t", "res"))
    st = torch.cuda.current_stream().cuda_stream if dev.kind == "hip" else 0
    _lib.call(fn, a.data_ptr(), w.data_ptr(), b.data_ptr(), s.data_ptr(), t.data_ptr(), res.data_ptr(), c.data_ptr(), 0, 8, 24, 8, 8, 24, 24,
              32, 3, ops.ACT_RELU, st)
    dev.sync()
    assert bool((c.cpu() == 7.0).all())


# ---- the split-precision twin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,K,O,rows_per_ch,n_ch", WIDE_AFFINE + [(131, 36, 40, 32, 3)])
def test_split_twin_at_the_same_forms(dev, R, K, O, rows_per_ch, n_ch):
    """aicg_gemm_nt_split at the wide-epilogue shapes (all K < 64: a single partial stage of its 64-wide K slab; K = 12 ends inside an
    8-k chunk) and at a scalar-epilogue shape, against float64 at test_conv_split's bar; the wide and the forced-scalar epilogue
    (ldc = O + 1) give the same bits.
    Measured relative RMS, emulator = MI355X: 2.43e-6, 2.53e-6, 2.45e-6, 2.67e-6, 2.15e-6 in the order of the cases."""
    p = make(R, K, O, n_ch, R + K + O + 1)
    got = gemm(dev, p, rows_per_ch, n_ch, ops.ACT_RELU, fn="aicg_gemm_nt_split")
    err = rel_rms(got, gemm_ref(p, rows_per_ch, n_ch, ops.ACT_RELU))
    print("split (%d, %d, %d): %.3g" % (R, K, O, err))
    assert not torch.isnan(got).any() and err < SPLIT_TOL, err
    scalar = gemm(dev, p, rows_per_ch, n_ch, ops.ACT_RELU, pads=(0, 0, 1, 0), fn="aicg_gemm_nt_split")
    assert torch.equal(bits(scalar[:, :O]), bits(got))
