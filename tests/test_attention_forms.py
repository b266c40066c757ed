"""The fused attention (csrc/attn.hip) at the forms the models reach and the direct tests did not: every forward and relative-value
instantiation, padded leading dimensions on row slices of one fused buffer (HuBERT), windows at least as long as the sequence, the
value kernel's 64-query block edges, key splits whose last part holds no tile, and the rescale branch under a window and a split.

Reference: `attention_f64`, tests/test_kernels_misc.py::test_attention's dense construction in float64 --
softmax(Q K^T scale + banded relative-key bias) V + banded P E^v.  The kernel sees fp32 inputs (the relative-key scores included:
they are formed in double and rounded once), the reference the same fp32 values in double.

Two measures per case, both 1e-5 (test_attention's bar; the kernel's documented error against a float64 softmax is < 1e-6):
  whole   relative RMS over the whole (C, T) output;
  column  max over queries i of |got[:, i] - ref[:, i]| / |ref[:, i]| -- one bad query column is not diluted by sqrt(T).
The docstrings record the worst column measured on the CPU emulator; the MI355X figures are still to be added (SUMMARY of the commit
that added this file)."""
import pytest
import torch

from aicovergen_amd import _lib, ops
from conftest import rel_rms

BAR = 1e-5


def attention_f64(q, k, v, H, scale, relk=None, ev=None, win=0):
    """q, k, v (C, T); relk (H, 2 win + 1, T) = scaled q_i . E^k_m; ev (2 win + 1, D) -> (C, T) float64."""
    C, T = q.shape
    D = C // H
    qh, kh, vh = (z.double().reshape(H, D, T).transpose(1, 2) for z in (q, k, v))
    sc = qh @ kh.transpose(1, 2) * scale
    i = torch.arange(T).view(T, 1)
    if relk is not None:
        m = torch.arange(T).view(1, T) - i + win
        band = (m >= 0) & (m <= 2 * win)
        rel = relk.double().transpose(1, 2)                                     # (H, T, 2 win + 1)
        sc = sc + torch.where(band, rel.gather(2, m.clamp(0, 2 * win).expand(H, T, T)), torch.zeros((), dtype=torch.float64))
    pa = torch.softmax(sc, -1)
    out = pa @ vh
    if ev is not None:
        jj = i + torch.arange(2 * win + 1).view(1, -1) - win                    # key of (query, offset)
        ok = (jj >= 0) & (jj < T)
        pb = pa.gather(2, jj.clamp(0, T - 1).expand(H, T, 2 * win + 1)) * ok
        out = out + pb @ ev.double()
    return out.transpose(1, 2).reshape(C, T)


def make(H, D, T, win, seed, relv=True):
    """fp32 operands of one case: q, k, v ~ N(0, 1), scale D^-0.5 (scores ~ N(0, 1)), E^k, E^v ~ N(0, 1 / D) as attentions.py draws them."""
    g = torch.Generator().manual_seed(seed)
    C, scale = H * D, D ** -0.5
    q, k, v = (torch.randn(C, T, generator=g) for _ in range(3))
    relk = ev = None
    if win:
        ek = torch.randn(2 * win + 1, D, generator=g, dtype=torch.float64) * D ** -0.5
        relk = ((q.double().reshape(H, D, T).transpose(1, 2) * scale) @ ek.t()).transpose(1, 2).float().contiguous()
        if relv:
            ev = torch.randn(2 * win + 1, D, generator=g) * D ** -0.5
    return dict(q=q, k=k, v=v, H=H, scale=scale, relk=relk, ev=ev, win=win)


def reference(c):
    return attention_f64(c["q"], c["k"], c["v"], c["H"], c["scale"], c["relk"], c["ev"], c["win"])


def run(dev, c, n_splits=None, q=None, k=None, v=None):
    t = lambda z: None if z is None else dev.t(z)
    return ops.attention(t(c["q"]) if q is None else q, t(c["k"]) if k is None else k, t(c["v"]) if v is None else v, c["H"],
                         relk=t(c["relk"]), relv_emb=t(c["ev"]), window=c["win"], scale=c["scale"], n_splits=n_splits)


def worst_column(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    return float(((got - ref).norm(dim=0) / ref.norm(dim=0)).max())


def check(got, ref, what):
    whole, col = rel_rms(got, ref), worst_column(got, ref)
    print("%s: whole %.3g, worst column %.3g" % (what, whole, col))
    assert whole < BAR, (what, whole)
    assert col < BAR, (what, col)
    return col


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def raw_attention(dev, q, k, v, c, n_splits, o):
    """ops.attention's sequence of C ABI calls with a caller-made output `o` (any row stride)."""
    H, win, T = c["H"], c["win"], q.shape[1]
    D = q.shape[0] // H
    relk = None if c["relk"] is None else dev.t(c["relk"])
    ev = None if c["ev"] is None else dev.t(c["ev"]).contiguous()
    lse = torch.empty((H, T), dtype=torch.float32, device=dev.device) if ev is not None else None
    st = torch.cuda.current_stream().cuda_stream if dev.kind == "hip" else 0
    p = lambda z: 0 if z is None else z.data_ptr()
    if n_splits > 1:
        scratch = torch.empty(n_splits * H * (D + 2) * T, dtype=torch.float32, device=dev.device)
        _lib.call("aicg_attention_split", p(q), p(k), p(v), p(relk), p(o), p(lse), T, H, D, win, q.stride(0), k.stride(0), v.stride(0),
                  o.stride(0), float(c["scale"]), n_splits, p(scratch), st)
    else:
        _lib.call("aicg_attention", p(q), p(k), p(v), p(relk), p(o), p(lse), T, H, D, win, q.stride(0), k.stride(0), v.stride(0),
                  o.stride(0), float(c["scale"]), st)
    if ev is not None:
        _lib.call("aicg_attention_relv", p(q), p(k), p(relk), p(ev), p(lse), p(o), T, H, D, win, q.stride(0), k.stride(0), o.stride(0),
                  float(c["scale"]), st)
    dev.sync()


# ---- 1. every instantiation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [97, 300])
@pytest.mark.parametrize("D,win,relv", [(32, 0, False), (64, 0, False), (96, 0, False), (128, 0, False),
                                        (96, 10, True), (64, 10, True), (32, 10, True), (32, 4, True), (128, 10, False)])
def test_every_instantiation(dev, D, win, relv, T):
    """attn_fwd_kernel<32 | 64 | 96 | 128> plain, and with the windows aicg_attention_relv instantiates -- (96, 10), (64, 10), (32, 10),
    (32, 4) -- with relative keys and values; D = 128 with relative keys only.  T = 97 / 300: 4 / 10 key tiles, 1 / 3 query blocks, a
    ragged last tile, the band crossing the query-block edges at 128 and 256.
    Worst column: emulator 1.12e-6 (D = 128, plain, T = 300); MI355X not measured yet."""
    c = make(2, D, T, win, 1000 * D + 10 * win + T, relv)
    check(run(dev, c), reference(c), "D %d w %d T %d" % (D, win, T))


@pytest.mark.parametrize("D,win", [(128, 10), (96, 4)])
def test_value_term_without_a_kernel_raises(dev, D, win):
    """A (D, window) pair aicg_attention_relv does not instantiate raises; it never returns an output that lacks the value term."""
    c = make(2, D, 97, win, 5)
    with pytest.raises(RuntimeError, match="not instantiated"):
        run(dev, c)
    dev.sync()


# ---- 2. padded leading dimensions, fused buffers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_splits", [1, 3])
@pytest.mark.parametrize("pad", [18, 1])
@pytest.mark.parametrize("D,win", [(64, 0), (96, 10)])
def test_padded_rows_of_one_fused_buffer(dev, D, win, pad, n_splits):
    """q, k, v = [:, :T] of row slices of one (3 C, T + pad) buffer whose padding is NaN (HuBERT: 13 198 -> 13 216), D = 64 plain and
    D = 96 with w = 10 (relk and lse keep stride T), single pass and 3 key splits (partials and merge see ldo): bit-equal to the
    contiguous call, both bars against float64, and -- through the C ABI with an output whose row stride is T + pad -- the output's own
    padding comes back untouched.  No key split here has an empty part: T = 200 is 7 tiles, 3 splits of 3, 3, 1.
    Worst column: emulator 8.3e-7 (D = 96, w = 10, single pass); MI355X not measured yet."""
    H, T = 2, 200
    C, ld = H * D, T + pad
    c = make(H, D, T, win, 77 + D)
    ref = reference(c)
    plain = run(dev, c, n_splits)
    buf = torch.full((3 * C, ld), float("nan"))
    buf[:, :T] = torch.cat([c["q"], c["k"], c["v"]])
    buf = dev.t(buf)
    q, k, v = (buf[r * C:(r + 1) * C, :T] for r in range(3))
    assert q.stride(0) == ld and not q.is_contiguous()
    got = run(dev, c, n_splits, q, k, v)
    assert torch.equal(bits(got), bits(plain))
    check(got, ref, "D %d w %d ld T + %d, %d splits" % (D, win, pad, n_splits))
    sentinel = -12345.678
    obuf = dev.t(torch.full((C, ld), sentinel))
    raw_attention(dev, q, k, v, c, n_splits, obuf[:, :T])
    assert torch.equal(bits(obuf[:, :T]), bits(plain))
    assert torch.equal(bits(obuf[:, T:]), bits(torch.full((C, pad), sentinel)))


# ---- 3. window >= T -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,win,T", [(32, 10, 1), (32, 10, 7), (32, 10, 21), (96, 10, 1), (96, 10, 7), (96, 10, 21), (32, 4, 5)])
def test_window_at_least_as_long_as_the_sequence(dev, D, win, T):
    """Every key lies inside every query's band (T <= w + 1), or the band is wider than the sequence (T = 21 at w = 10: 2 w + 1): the
    relative-key rows and the staged key columns i0 - w .. i0 + 63 + w reach past both ends.
    Worst column: emulator 4.7e-7 (D = 96, T = 21); MI355X not measured yet."""
    c = make(2, D, T, win, 31 * T + D)
    check(run(dev, c), reference(c), "D %d w %d T %d" % (D, win, T))


# ---- 4. block edges of the value kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [64, 65, 128, 129])
def test_value_kernel_block_edges(dev, T):
    """attn_relv_kernel<96, 21> owns 64 queries per workgroup: one full block, one query in a second block, and the same around the
    forward kernel's 128-query block.
    Worst column: emulator 9.1e-7 (T = 128); MI355X not measured yet."""
    c = make(2, 96, T, 10, 400 + T)
    check(run(dev, c), reference(c), "T %d" % T)


# ---- 5. empty trailing split ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,win", [(96, 10), (64, 0)])
@pytest.mark.parametrize("T,n_splits", [(150, 4), (205, 5)])
def test_key_split_whose_last_part_is_empty(dev, D, win, T, n_splits):
    """per = ceil(tiles / n_splits) leaves the last part without a tile: 5 tiles over 4 splits (2, 2, 1, 0), 7 over 5 (2, 2, 2, 1, 0).
    The empty part contributes (max -inf, sum 0, zeros); the merge must ignore it, also in the lse the relative-value pass reads.
    Worst column: emulator 6.7e-7 (D = 64, T = 150); MI355X not measured yet."""
    tiles = -(-T // 32)
    per = -(-tiles // n_splits)
    assert (n_splits - 1) * per >= tiles                 # the case is what it says: the last part starts past the last tile
    c = make(2, D, T, win, T + D)
    got = run(dev, c, n_splits)
    check(got, reference(c), "D %d w %d T %d, %d splits" % (D, win, T, n_splits))
    assert rel_rms(got, run(dev, c, 1).cpu()) < 2e-6    # test_attention_key_split_matches_single_pass's bar


def test_default_split_count_reaches_the_empty_part(dev):
    """ops.attention chooses 4 splits by itself at T = 150, H = 2 (5 key tiles): the default path runs the empty part.
    Worst column: emulator 8.5e-7; MI355X not measured yet."""
    H, T = 2, 150
    blocks = -(-T // 128) * H
    assert max(1, min(4, -(-T // 32), -(-1024 // blocks))) == 4          # ops.attention's arithmetic
    c = make(H, 96, T, 10, 150)
    got = run(dev, c, None)
    check(got, reference(c), "default splits")
    assert torch.equal(bits(got), bits(run(dev, c, 4)))


# ---- 6. rescale branch with a window and a split ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_splits", [1, 3])
def test_rescale_with_window_and_split(dev, n_splits):
    """test_attention_online_softmax_rescale's spike under a window: key 90 is 4 x query 85, a score of ~ 40 two tiles in -- the last
    tile of split 0 of 3 (7 tiles: 3, 3, 1) -- and inside query 85's band, so the relative-key bias lands on the spiked score; the
    merge then meets partial maxima tens apart.
    Worst column: emulator 1.66e-6 (3 splits; query 85's column, whose output is one value row); MI355X not measured yet."""
    H, D, T, win = 2, 96, 200, 10
    c = make(H, D, T, win, 9)
    c["k"][:, 90] = c["q"][:, 85] * 4.0
    ref = reference(c)
    assert float((c["q"][:D, 85] @ c["k"][:D, 90]) * c["scale"]) > 25.0     # the spike is one
    check(run(dev, c, n_splits), ref, "%d splits" % n_splits)
