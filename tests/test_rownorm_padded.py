"""aicg_rownorm_act_ld (csrc/norm.hip) on rows padded to a common stride -- the form HuBERT's feature extractor hands over, reached so
far only through a whole-model test.  With ld != T a row's alignment class ((row * ld) & 3: the head scalars in front of the float4
body) and its segment boundaries no longer move together; the padding of x is NaN (nothing may read it), the padding of out holds a
sentinel (nothing may write it).  Reference: float64 group_norm (+ exact-erf GELU), bar 5e-6 as in test_rownorm_gelu."""
import pytest
import torch
import torch.nn.functional as F

from aicovergen_amd import ops
from conftest import rel_rms

ROWS = 7
SENTINEL = -4321.125


def _ld(T, kind):
    return {"T+1": T + 1, "T+3": T + 3, "up4+4": (T + 3) // 4 * 4 + 4}[kind]


_cache = {}


def _case(T):
    """x, gamma, beta and the float64 references (computed once per T, never modified)."""
    if T not in _cache:
        g = torch.Generator().manual_seed(4 + T)
        x = torch.randn(ROWS, T, generator=g) * 3 + 1
        x[3] = torch.randn(T, generator=g) * 0.5 + 8.0                        # a large mean over a small spread: the moment merge
        gam, bet = torch.rand(ROWS, generator=g) + 0.5, torch.randn(ROWS, generator=g)
        ref = F.group_norm(x.double().unsqueeze(0), ROWS, gam.double(), bet.double(), 1e-5)[0]
        _cache[T] = x, gam, bet, {ops.ACT_NONE: ref, ops.ACT_GELU: F.gelu(ref)}
    return _cache[T]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("kind", ["T+1", "T+3", "up4+4"])
@pytest.mark.parametrize("T", [1000, 4099, 16385, 16389])
def test_rownorm_padded_rows(dev, T, kind):
    """T = 1000: one workgroup per row; 4099: the split form, one segment; 16 385 / 16 389: two segments (16 384 elements each at
    most), tails of 1 and of every other length as the 7 rows' heads move.  ld = T + 1 and T + 3 walk the rows through every alignment
    class, round-up-to-4 + 4 keeps every row aligned (the DMA-staged convolution's form).
    Against float64 (bar 5e-6): worst case 3.0e-7 (T = 1000, no activation) on the emulator; not measured on the MI355X yet.
    Against the contiguous call: the one-workgroup form adds in an order that does not depend on the layout, so all of it is
    bit-equal.  The split form cuts a row into head scalars, float4 body and tail scalars by the row's ADDRESS, so a row whose
    alignment class differs between the two layouts has its moments merged in another order (ops.rownorm_act's docstring states
    this contract): measured on the emulator, such rows differ by up to 3.7e-7 relative RMS of the whole map (T = 16 389, ld = T + 1,
    the large-mean row), each layout inside the float64 bar on its own.  Rows of the same class -- rows 0 and 4 for every ld, all
    rows where ld - T is a multiple of 4 -- are bit-equal, and that is asserted."""
    x, gam, bet, refs = _case(T)
    ld = _ld(T, kind)
    buf = torch.full((ROWS, ld), float("nan"))
    buf[:, :T] = x
    xd = dev.t(buf)[:, :T]
    assert xd.stride(0) == ld
    gd, bd = dev.t(gam), dev.t(bet)
    same_class = torch.tensor([(r * ld) % 4 == (r * T) % 4 for r in range(ROWS)])
    assert bool(same_class[0]) and (kind == "up4+4" or not bool(same_class.all()))
    for act in (ops.ACT_GELU, ops.ACT_NONE):
        obuf = dev.t(torch.full((ROWS, ld), SENTINEL))
        y = ops.rownorm_act(xd, gd, bd, act=act, out=obuf[:, :T])
        dev.sync()
        err = rel_rms(y, refs[act])
        print("T %d ld %d act %d: %.3g" % (T, ld, act, err))
        assert err < 5e-6
        assert torch.equal(bits(obuf[:, T:]), bits(torch.full((ROWS, ld - T), SENTINEL)))
        plain = ops.rownorm_act(dev.t(x), gd, bd, act=act)
        exact = torch.ones(ROWS, dtype=torch.bool) if T < 4096 else same_class
        assert torch.equal(bits(y)[exact], bits(plain)[exact])
        # out=None: a view of a buffer laid out like x
        d = ops.rownorm_act(xd, gd, bd, act=act)
        assert d.shape == (ROWS, T) and d.stride(0) == ld and d.stride(1) == 1
        assert torch.equal(bits(d), bits(y))
