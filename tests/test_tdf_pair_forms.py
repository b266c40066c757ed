"""The fused TDF block (csrc/tdf_pair.hip) at the forms the separator's models reach and the direct test did not: every instantiation
(H / 32 in {2, 3, 4, 6, 8, 12}: each has its own DMA piece schedule), F = 32 (one phase-1 stage: the W2 slab is handed over in stage 0),
the real level-1 shape of the dim_f = 3072 models, NULL optional operands, the refusals -- and the property the hand-over rests on:
an output row is a function of its input row and its channel alone, whichever lane, wave or workgroup computes it.

Reference: `tdf_ref` in float64 on the fp32 operands --  x + relu(bn2(relu(bn1(x W1^T + b1)) W2^T + b2)),  bn = per-channel scale / shift
with ch = (row / rows_per_ch) % n_ch.

Bar: the same expression evaluated by torch in float32 on the CPU has an error `e32` against float64; the kernel may have 4 x that (an
equally long fp32 summation in another order: MFMA k-pairs, not BLAS blocks), in both measures:
  whole   relative RMS over the tensor;
  column  max over output columns f of (max over rows |got - ref|) / rms(ref[:, f]) -- one bad column is not diluted by the others.
Every case is rows of t = 32 per channel, c = 3 channels, R = 192 rows (b = 2): a 128-row workgroup spans several channels (each wave its
own) and the second workgroup is half empty."""
import pytest
import torch

from aicovergen_amd import _lib, ops
from conftest import rel_rms

FACTOR = 4.0


def tdf_ref(x, w1, b1, s1, t1, w2, b2, s2, t2, rows_per_ch, n_ch, dtype=torch.float64):
    """x (R, F); any of b1, (s1, t1), b2, (s2, t2) may be None: that term is absent."""
    c = lambda v: None if v is None else v.to(dtype)
    x, w1, b1, s1, t1, w2, b2, s2, t2 = (c(v) for v in (x, w1, b1, s1, t1, w2, b2, s2, t2))
    ch = (torch.arange(x.shape[0]) // rows_per_ch) % n_ch
    h = x @ w1.t()
    if b1 is not None:
        h = h + b1
    if s1 is not None:
        h = h * s1[ch, None] + t1[ch, None]
    y = torch.relu(h) @ w2.t()
    if b2 is not None:
        y = y + b2
    if s2 is not None:
        y = y * s2[ch, None] + t2[ch, None]
    return x + torch.relu(y)


def make(F, H, R, n_ch, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(R, F), w1=r(H, F) / F ** 0.5, b1=r(H) * 0.1, s1=torch.rand(n_ch, generator=g) + 0.5, t1=r(n_ch) * 0.3,
                w2=r(F, H) / H ** 0.5, b2=r(F) * 0.1, s2=torch.rand(n_ch, generator=g) + 0.5, t2=r(n_ch) * 0.3)


def run(dev, p, rows_per_ch, n_ch, drop=(), x=None, s1=None, t1=None, s2=None, t2=None):
    """aicg_tdf_pair through the C ABI; operands named in `drop` are passed as NULL."""
    x = p["x"] if x is None else x
    R, F = x.shape
    H = p["w1"].shape[0]
    d = {k: dev.t(v.contiguous()) for k, v in dict(p, x=x, s1=p["s1"] if s1 is None else s1, t1=p["t1"] if t1 is None else t1,
                                                   s2=p["s2"] if s2 is None else s2, t2=p["t2"] if t2 is None else t2).items()}
    d["w1"], d["w2"] = dev.t(ops.pack_tdf_w1(p["w1"])), dev.t(ops.pack_tdf_w2(p["w2"]))
    out = torch.full((R, F), float("nan"), dtype=torch.float32, device=dev.device)
    ptr = lambda k: 0 if k in drop else d[k].data_ptr()
    st = torch.cuda.current_stream().cuda_stream if dev.kind == "hip" else 0
    _lib.call("aicg_tdf_pair", ptr("x"), ptr("w1"), ptr("b1"), ptr("s1"), ptr("t1"), ptr("w2"), ptr("b2"), ptr("s2"), ptr("t2"),
              out.data_ptr(), R, F, H, rows_per_ch, n_ch, st)
    dev.sync()
    return out.cpu()


def worst_column(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    return float(((got - ref).abs().amax(0) / ref.pow(2).mean(0).sqrt()).max())


def check(got, p, rows_per_ch, n_ch, what, drop=()):
    q = {k: (None if k in drop else v) for k, v in p.items()}
    args = (q["x"], q["w1"], q["b1"], q["s1"], q["t1"], q["w2"], q["b2"], q["s2"], q["t2"], rows_per_ch, n_ch)
    ref, f32 = tdf_ref(*args), tdf_ref(*args, dtype=torch.float32)
    whole, col, e_whole, e_col = rel_rms(got, ref), worst_column(got, ref), rel_rms(f32, ref), worst_column(f32, ref)
    print("%s: whole %.3g (e32 %.3g), worst column %.3g (e32 %.3g)" % (what, whole, e_whole, col, e_col))
    assert not torch.isnan(got).any(), what
    assert whole <= FACTOR * e_whole, (what, whole, e_whole)
    assert col <= FACTOR * e_col, (what, col, e_col)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# (F, H): NH 6 / NH 8 at the production ratio F = H; the others at the smallest F with more than one stage in either phase (F = 96: an odd
# number of stages, so phase 2 starts in the other LDS buffer)
FORMS = [(64, 64), (64, 96), (96, 128), (192, 192), (256, 256), (96, 384)]


@pytest.mark.parametrize("F,H", FORMS + [(32, h) for h in (64, 96, 128, 192, 256, 384)] + [(1536, 192)])
def test_every_instantiation(dev, F, H):
    """tdf_pair_kernel<2 | 3 | 4 | 6 | 8 | 12> with two or three stages per phase, with F = 32 (a single phase-1 stage, which also issues the
    first W2 slab), and <6> at F = 1536, level 1 of the dim_f = 3072 models.
    Measured whole / worst column.  The kernel's figures are the same on the CPU emulator and on the MI355X to the three digits printed
    (the same fp32 operations in the same order); e32 is the host's BLAS and differs between the two hosts:
      (192, 192)   1.26e-7 / 1.30e-6    e32 emulator host 1.27e-7 / 1.60e-6, MI355X host 1.27e-7 / 1.60e-6
      (256, 256)   1.86e-7 / 2.01e-6    e32 1.87e-7 / 2.01e-6, 1.37e-7 / 1.23e-6
      (96, 384)    1.59e-7 / 1.77e-6    e32 1.56e-7 / 1.54e-6, 1.28e-7 / 9.54e-7
      (32, 256)    8.95e-8 / 9.12e-7    e32 8.76e-8 / 8.73e-7, 7.06e-8 / 5.41e-7
      (1536, 192)  3.61e-7 / 4.11e-6    e32 2.07e-7 / 2.65e-6, 1.68e-7 / 2.36e-6
    (1536, 192) is the worst ratio of the thirteen: 1.75 / 1.55 on the emulator's host, 2.15 / 1.74 on the MI355X's -- 768 sequential
    MFMA k-pairs per accumulator against BLAS's blocked sums."""
    p = make(F, H, 192, 3, 100 * F + H)
    check(run(dev, p, 32, 3), p, 32, 3, "F %d H %d" % (F, H))


@pytest.mark.parametrize("drop", [("b1", "b2"), ("s1", "t1"), ("s2", "t2"), ("b1", "s1", "t1", "b2", "s2", "t2")], ids=lambda d: "no_" + "_".join(d))
@pytest.mark.parametrize("F,H", [(64, 96), (192, 192)])
def test_optional_operands(dev, F, H, drop):
    """NULL biases, NULL first affine, NULL second affine, all NULL (ops.tdf_pair always passes every operand): each against the float64
    expression without that term.  Worst ratio to e32, emulator and MI355X alike: 1.00 whole, 1.17 column ((192, 192) without biases:
    1.42e-6 against 1.21e-6)."""
    p = make(F, H, 192, 3, 7 * F + H)
    check(run(dev, p, 32, 3, drop=drop), p, 32, 3, "F %d H %d without %s" % (F, H, ", ".join(drop)), drop=drop)


@pytest.mark.parametrize("F,H", FORMS)
def test_output_is_a_function_of_the_row_and_its_channel(dev, F, H):
    """Rows of 64 per channel, 3 channels, 320 rows (two and a half workgroups; channel k owns the 64-row blocks k, k + 3).  Permuting
    the rows that belong to one channel -- across lanes, waves and workgroups -- permutes the output rows bit for bit: a row's
    arithmetic does not depend on who computes it, and every wave applies its own channel's scale and shift."""
    R, rpc, n_ch = 320, 64, 3
    p = make(F, H, R, n_ch, F + 3 * H)
    base = run(dev, p, rpc, n_ch)
    ch = (torch.arange(R) // rpc) % n_ch
    g = torch.Generator().manual_seed(5)
    perm = torch.arange(R)
    for k in range(n_ch):
        rows = torch.nonzero(ch == k).flatten()
        perm[rows] = rows[torch.randperm(len(rows), generator=g)]
    assert not torch.equal(perm, torch.arange(R)) and torch.equal(ch[perm], ch)
    got = run(dev, p, rpc, n_ch, x=p["x"][perm])
    assert torch.equal(bits(got), bits(base[perm]))


@pytest.mark.parametrize("F,H", FORMS)
def test_rows_in_another_workgroup_give_the_same_bits(dev, F, H):
    """32 rows of another channel in front: every row moves to the next wave, the last wave's rows to the next workgroup, and the
    channel table is rotated by one so that each row keeps its scale and shift.  Same bits."""
    R, rpc, n_ch = 192, 32, 3
    p = make(F, H, R, n_ch, 11 * F + H)
    base = run(dev, p, rpc, n_ch)
    g = torch.Generator().manual_seed(9)
    x2 = torch.cat([torch.randn(32, F, generator=g), p["x"]])
    roll = lambda v: torch.roll(v, 1)     # channel k of the first run is channel (k + 1) % n_ch of the second
    got = run(dev, p, rpc, n_ch, x=x2, s1=roll(p["s1"]), t1=roll(p["t1"]), s2=roll(p["s2"]), t2=roll(p["t2"]))
    assert torch.equal(bits(got[32:]), bits(base))


REFUSALS = {           # F, H, rows_per_ch, n_ch, operands passed as NULL, byte offset of x, of out, error code
    "H_160": (64, 160, 32, 3, (), 0, 0, -1),
    "F_48": (48, 64, 32, 3, (), 0, 0, -1),
    "rows_per_ch_48": (64, 64, 48, 3, (), 0, 0, -1),
    "rows_per_ch_0": (64, 64, 0, 3, (), 0, 0, -1),          # 0 and -32 are multiples of 32, too: the kernel would divide by them
    "rows_per_ch_minus_32": (64, 64, -32, 3, (), 0, 0, -1),
    "F_0": (0, 64, 32, 3, (), 0, 0, -1),
    "n_ch_0": (64, 64, 32, 0, (), 0, 0, -1),
    "scale_without_shift_1": (64, 64, 32, 3, ("t1",), 0, 0, -2),
    "shift_without_scale_2": (64, 64, 32, 3, ("s2",), 0, 0, -2),
    "x_off_4": (64, 64, 32, 3, (), 4, 0, -2),
    "out_off_4": (64, 64, 32, 3, (), 0, 4, -2),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(dev, name):
    """Unsupported shapes return AICG_E_SHAPE, half an affine and operands that are not 16-byte aligned AICG_E_ARG; nothing is launched: `out`
    keeps its contents.  Every buffer is large enough for the shape asked for, whatever the dispatcher decides."""
    F, H, rpc, n_ch, drop, x_off, out_off, code = REFUSALS[name]
    R = 192
    z = lambda n: torch.zeros(n, dtype=torch.float32, device=dev.device)
    w2_floats = (F + 31) // 32 * ((32 * (H + 4) + 255) // 256 * 256)
    d = dict(x=z(R * F + 4), w1=z(F * H + 4), b1=z(H), s1=z(3), t1=z(3), w2=z(w2_floats + 4), b2=z(F + 4), s2=z(3), t2=z(3))
    out = torch.full((R * F + 4,), 7.0, dtype=torch.float32, device=dev.device)
    ptr = lambda k: 0 if k in drop else d[k].data_ptr()
    st = torch.cuda.current_stream().cuda_stream if dev.kind == "hip" else 0
    with pytest.raises(RuntimeError, match=r"aicg_tdf_pair failed \(%d\)" % code):
        _lib.call("aicg_tdf_pair", ptr("x") + x_off, ptr("w1"), ptr("b1"), ptr("s1"), ptr("t1"), ptr("w2"), ptr("b2"), ptr("s2"), ptr("t2"),
                  out.data_ptr() + out_off, R, F, H, rpc, n_ch, st)
    dev.sync()
    assert bool((out.cpu() == 7.0).all())
    assert not ops.tdf_pair_supported(F, H, rpc) or code == -2 or n_ch == 0
