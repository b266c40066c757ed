"""Half storage for the vocoder's ResBlocks (AICG_HALF=1 + AICG_HALF_STORE=1 + .half()): csrc/conv1d_h.hip keeps x / res / out each in
fp16 or fp32 in memory, runs the products on the fp16 matrix pipe in the direct form and everything else in fp32.

Bounds (written where they are asserted):
  * a layer against float64 torch on operands rounded the same way, ref = out_scale (act(conv1d(h(pre_act(x)), h(w)) + b) + res) with
    h(t) = t.half().double(): elementwise |got - ref| <= 2 (K + 4) 2^-24 S, K = Cin k, S = out_scale (conv1d(|h(pre_act(x))|, |h(w)|) +
    |b| + |res|) -- the forward error bound of a K-term fp32 sum of exact products (fp16 x fp16 is exact in fp32) plus the epilogue's
    four operations; the factor 2 because the MFMA's internal summation is not documented as round-to-nearest.  An fp16 output adds its
    one store rounding, 2^-11 |ref| + 2^-25 (half an ulp of a normal / of a subnormal fp16);
  * a whole synthesizer against its fp32 self: the half mode's existing 2e-2 relative rms on the waveform (tests/test_half.py);
  * C1 through VC.pipeline: the half mode's existing 5e-3 relative rms of the int16 waveform, against the fp32 run and the reference's golden.

Reported, not gated: the distance to the AICG_HALF=1 run, and d_ref = the distance between oracle/synth.py run on .half()
tensors on the CPU and its own fp32 run.  torch's CPU half kernels do not carry the oracle's synthesizer as it stands (its harmonic
source is computed in float64 / fp32 and meets fp16 weights in the noise convolutions: a dtype error); where that is so the test
prints the error instead of a figure."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from aicovergen_amd import _lib, ops
from conftest import rel_rms

SLOPE = 0.1
F16, F32 = torch.float16, torch.float32
# (x, res, out) storage; "acc": accumulate with out_scale = 1 / 3 into a pre-filled fp32 out
COMBOS = [("f32_f32_f16", F32, F32, F16, False), ("f16_f16_f16", F16, F16, F16, False), ("f16_f16_f32acc", F16, F16, F32, True),
          ("f16_none_f16", F16, None, F16, False)]
ACTS = [(False, False), (True, False), (False, True), (True, True)]   # leaky ReLU in front of / behind the convolution


def _lrelu(t):
    return F.leaky_relu(t, SLOPE)


def _layer(dev, w, b, k, d):
    return ops.PackedConv(w, b, padding=(k - 1) // 2 * d, dilation=d, device=dev.device)


def _run(dev, pc, x, res, y0, out_dtype, pre, act, scale=1.0, accumulate=False):
    out = None if y0 is None else dev.t(y0.clone())
    got = ops.conv_h(dev.t(x), pc, res=None if res is None else dev.t(res), out=out, out_dtype=out_dtype,
                     pre_act=ops.ACT_LRELU if pre else ops.ACT_NONE, pre_slope=SLOPE, act=ops.ACT_LRELU if act else ops.ACT_NONE,
                     act_slope=SLOPE, out_scale=scale, accumulate=accumulate)
    dev.sync()
    return got.cpu()


def _reference(x, w, b, res, y0, k, d, pre, act, scale):
    """(ref, S, ref32): float64 on operands rounded as the kernel rounds them, the bound's magnitude sum, and the unrounded fp32-operand layer."""
    pad = (k - 1) // 2 * d
    xin = _lrelu(x.float()) if pre else x.float()                    # the pre-activation runs in fp32 on the stored value
    hx, hw = xin.half().double(), w.half().double()
    s = float(np.float32(scale))                                      # what the C ABI receives
    r = 0.0 if res is None else res.double()
    c = F.conv1d(hx, hw, b.double(), padding=pad, dilation=d)
    ref = s * ((_lrelu(c) if act else c) + r)
    S = s * (F.conv1d(hx.abs(), hw.abs(), b.double().abs(), padding=pad, dilation=d) + (0.0 if res is None else res.double().abs()))
    c32 = F.conv1d(xin.double(), w.double(), b.double(), padding=pad, dilation=d)
    ref32 = s * ((_lrelu(c32) if act else c32) + r)
    if y0 is not None:
        ref, ref32 = y0.double() + ref, y0.double() + ref32
    return ref, S, ref32


@pytest.mark.parametrize("n,ci,co", [(1, 16, 16), (1, 32, 32), (2, 48, 80), (1, 96, 64)])
@pytest.mark.parametrize("k,d", [(3, 1), (3, 5), (5, 1), (7, 3), (11, 5)])
def test_layer_exactness(dev, k, d, n, ci, co):
    """Every storage combination at T = 7 (shorter than every halo but (3, 1)'s), 63 (odd), 392 (two workgroups) and, on hardware, 1304,
    with the leaky ReLU in front, behind, on both sides and absent: the derived elementwise bound against float64 on equally rounded
    operands.  On hardware every (storage, placement) pair runs at every T; on the emulator, where a launch costs 0.2 s per tile, the
    placement rotates with the storage combination and T (every pair of the two still occurs but four of the sixteen): the
    activations act on fp32 values on either side of the storage conversions and share no code with them."""
    g = torch.Generator().manual_seed(1000 * k + 100 * d + ci + co)
    w, b = torch.randn(co, ci, k, generator=g) * 0.2, torch.randn(co, generator=g)
    pc = _layer(dev, w, b, k, d)
    assert pc.conv_h_supported()
    K = ci * k
    worst = 0.0
    for ti, T in enumerate((7, 63, 392) + ((1304,) if dev.big else ())):
        x32, r32, y0 = (torch.randn(n, c, T, generator=g) for c in (ci, co, co))
        for ci_, (name, xd, rd, od, accum) in enumerate(COMBOS):
            x, res = x32.to(xd), None if rd is None else r32.to(rd)
            for pre, act in (ACTS if dev.big else [ACTS[(ci_ + ti) % 4]]):
                scale = 1.0 / 3 if accum else 1.0
                got = _run(dev, pc, x, res, y0 if accum else None, od, pre, act, scale, accum)
                assert _lib.last_launch() == "conv1d_h_kernel"
                assert got.dtype == od and got.shape == (n, co, T)
                ref, S, ref32 = _reference(x, w, b, res, y0 if accum else None, k, d, pre, act, scale)
                bound = 2 * (K + 4) * 2.0 ** -24 * S
                if od == F16:
                    bound = bound + 2.0 ** -11 * ref.abs() + 2.0 ** -25
                err = (got.double() - ref).abs()
                ratio = float((err / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (name, T, pre, act, ratio)
                assert rel_rms(got, ref32) > 1e-5, (name, T, pre, act)         # (it IS fp16 arithmetic that ran)
    print("conv1d_h k%d d%d %d>%d: worst |err| / bound %.3f" % (k, d, ci, co, worst))


@pytest.mark.parametrize("xd,od", [(F16, F16), (F32, F16), (F16, F32)])
def test_strided_views_and_odd_offsets(dev, xd, od):
    """x, res and out as channel- and batch-sliced views of larger buffers whose rows start at odd element offsets (an fp16 row there
    is not dword-aligned) and have an odd pitch: the contiguous call's bits."""
    g = torch.Generator().manual_seed(7)
    n, ci, co, T, k, d = 2, 48, 80, 63, 7, 3
    w, b = torch.randn(co, ci, k, generator=g) * 0.2, torch.randn(co, generator=g)
    pc = _layer(dev, w, b, k, d)
    bx = torch.randn(n + 1, ci + 5, T + 4, generator=g).to(xd)
    br = torch.randn(n + 2, co + 3, T + 6, generator=g).to(F16)
    x, res = bx[1:, 2: 2 + ci, 2: 2 + T], br[2:, 1: 1 + co, 2: 2 + T]
    assert x.storage_offset() % 2 == 1 and res.storage_offset() % 2 == 1 and x.stride(1) % 2 == 1 and not x.is_contiguous()
    want = _run(dev, pc, x.contiguous(), res.contiguous(), None, od, True, False)
    xv = dev.t(bx)[1:, 2: 2 + ci, 2: 2 + T]
    rv = dev.t(br)[2:, 1: 1 + co, 2: 2 + T]
    bo = torch.full((n + 1, co + 2, T + 2), 7.0, dtype=od, device=dev.device)
    ov = bo[:n, 1: 1 + co, 1: 1 + T]
    ops.conv_h(xv, pc, res=rv, out=ov, pre_act=ops.ACT_LRELU, pre_slope=SLOPE)
    dev.sync()
    assert _lib.last_launch() == "conv1d_h_kernel"
    assert torch.equal(ov.cpu(), want)
    bo = bo.cpu()
    bo[:n, 1: 1 + co, 1: 1 + T] = 7.0
    assert bool((bo == 7.0).all())                 # nothing outside the view was written


@pytest.mark.parametrize("k,d", [(3, 1), (3, 5), (5, 1), (7, 3), (11, 5)])
def test_position_independence(dev, k, d):
    """A call on the slice [a, b) extended by the layer's halo computes, on [a, b), the full call's bits: an output's summation order does
    not depend on where it falls in a tile or in the row.  a = 77: odd, no multiple of 32, 64 or 256."""
    g = torch.Generator().manual_seed(50 + k + d)
    n, ci, co, T, a, e = 1, 32, 48, 392, 77, 301
    halo = (k - 1) // 2 * d
    w, b = torch.randn(co, ci, k, generator=g) * 0.2, torch.randn(co, generator=g)
    pc = _layer(dev, w, b, k, d)
    x, res = torch.randn(n, ci, T, generator=g).half(), torch.randn(n, co, T, generator=g).half()
    for od in (F16, F32):
        full = _run(dev, pc, x, res, None, od, True, True)
        part = _run(dev, pc, x[:, :, a - halo: e + halo].contiguous(), res[:, :, a - halo: e + halo].contiguous(), None, od, True, True)
        assert torch.equal(part[:, :, halo: halo + e - a], full[:, :, a:e])


def test_supported_shapes_and_errors(dev):
    lib = _lib.get()
    assert lib.aicg_conv1d_h_supported(16, 16, 3, 1) == 1 and lib.aicg_conv1d_h_supported(96, 80, 11, 5) == 1
    assert lib.aicg_conv1d_h_supported(32, 32, 9, 1) == 0          # k = 9
    assert lib.aicg_conv1d_h_supported(24, 32, 3, 1) == 0          # Cin = 24
    assert lib.aicg_conv1d_h_supported(32, 32, 3, 2) == 0          # dilation 2
    # a launch first, so that "unchanged" means something
    g = torch.Generator().manual_seed(3)
    ok = _layer(dev, torch.randn(16, 16, 3, generator=g), torch.randn(16, generator=g), 3, 1)
    ops.conv(dev.t(torch.randn(1, 16, 40, generator=g)), ok)
    dev.sync()
    before = _lib.last_launch()
    assert before and before != "conv1d_h_kernel"
    for ci, k, d in ((32, 9, 1), (24, 3, 1), (32, 3, 2)):
        pc = _layer(dev, torch.randn(32, ci, k, generator=g), torch.randn(32, generator=g), k, d)
        assert not pc.conv_h_supported()
        x = dev.t(torch.randn(1, ci, 40, generator=g).half())
        with pytest.raises(RuntimeError, match=r"aicg_conv1d_h failed \(-2\): \S"):
            ops.conv_h(x, pc)
        assert _lib.last_launch() == before
    # layers packed for the fp32-only models never get a half-storage image
    with ops.fp32_layers():
        f0_layer = _layer(dev, torch.randn(32, 32, 3, generator=g), torch.randn(32, generator=g), 3, 1)
    assert not f0_layer.conv_h_supported()


# ---- ResBlock chain and synthesizer ---------------------------------------------------------------------------------------------------

def _make(dev, cfg, seed):
    from aicovergen_amd.infer_pack.models import SynthesizerTrnMs768NSFsid
    from synthetic import weights
    net = SynthesizerTrnMs768NSFsid(*cfg, is_half=True)
    del net.enc_q
    net.load_state_dict(weights.synth_state_dict(cfg, seed), strict=False)
    return net.eval().to(dev.device)


def _infer(net, cfg, T, seed):
    from synthetic.inputs import synth_inputs
    phone, pitch, f0, nz, ns = synth_inputs(cfg, T, seed + 1)
    return net.infer(phone, torch.tensor([T]), pitch, f0, torch.tensor([1]), noise_z=nz, noise_src=ns)[0].cpu()


class _Spy:
    """Records (x dtype, res dtype, out dtype, kernel launched) of every ops.conv_h call."""

    def __init__(self, monkeypatch):
        self.calls = []
        orig = ops.conv_h

        def spy(x, pc, res=None, out=None, **kw):
            r = orig(x, pc, res=res, out=out, **kw)
            self.calls.append((x.dtype, None if res is None else res.dtype, r.dtype, _lib.last_launch()))
            return r
        monkeypatch.setattr(ops, "conv_h", spy)


def _d_ref(cfg, T, seed):
    """oracle/synth.py on .half() tensors against its own fp32 run (CPU), or the reason torch's CPU half kernels do not allow it."""
    from oracle import synth
    from synthetic import weights
    from synthetic.inputs import synth_inputs
    sd = weights.synth_state_dict(cfg, seed)
    phone, pitch, f0, nz, ns = synth_inputs(cfg, T, seed + 1)
    with torch.no_grad():
        o32 = synth.synth_infer(sd, cfg, phone, pitch, f0, torch.tensor([1]), nz, ns)[0]
        try:
            sdh = {k: v.half() if v.is_floating_point() else v for k, v in sd.items()}
            o16 = synth.synth_infer(sdh, cfg, phone.half(), pitch, f0.half(), torch.tensor([1]), nz.half(), ns.half())[0]
        except Exception as e:   # reported, not a gate
            return "not available (%s: %s)" % (type(e).__name__, str(e).splitlines()[0][:100])
    return "%.3e" % rel_rms(o16, o32)


_fp32_runs = {}


def _fp32_run(dev, net, cfg, T, seed):
    """The fp32 waveform of (cfg, T, seed): computed once per backend and shared."""
    key = (dev.kind, tuple(map(str, cfg)), T, seed)
    if key not in _fp32_runs:
        _fp32_runs[key] = _infer(net.float(), cfg, T, seed)
    return _fp32_runs[key]


def _synth_three_ways(dev, monkeypatch, cfg, T, seed=1234):
    monkeypatch.setenv("AICG_HALF", "1")
    monkeypatch.delenv("AICG_HALF_STORE", raising=False)
    net = _make(dev, cfg, seed)
    o32 = _fp32_run(dev, net, cfg, T, seed)
    o16 = _infer(net.half(), cfg, T, seed)
    monkeypatch.setenv("AICG_HALF_STORE", "1")
    spy = _Spy(monkeypatch)
    ohs = _infer(net.half(), cfg, T, seed)
    return o32, o16, ohs, spy.calls


def _check_synth(o32, o16, ohs, calls, nk=3):
    assert calls and all(c[3] == "conv1d_h_kernel" for c in calls)
    # per chain: the stage input (fp32) is read first, the stage sum (fp32) written last, every buffer between is fp16
    assert {c[2] for c in calls} == {F16, F32} and {c[0] for c in calls} == {F16, F32}
    assert sum(c[2] == F32 for c in calls) * 6 == len(calls)          # ResBlock1: six layers per chain, one fp32 store
    assert all(c[2] == F16 or c[0] == F16 for c in calls)               # no layer is fp32 -> fp32
    assert bool(torch.isfinite(ohs).all())
    e, e16 = rel_rms(ohs, o32), rel_rms(ohs, o16)
    assert 1e-5 < e < 2e-2, e
    assert not torch.equal(ohs, o16)
    return e, e16


def test_synth_tiny_half_store_against_fp32(dev, monkeypatch):
    from synthetic import weights
    cfg = weights.SYNTH_CFG_TINY          # stages of 64, 32, 16 and 8 channels: the 16-channel stage takes the new route, the 8-channel one cannot
    o32, o16, ohs, calls = _synth_three_ways(dev, monkeypatch, cfg, 12)
    e, e16 = _check_synth(o32, o16, ohs, calls)
    assert len(calls) == 18               # one stage: three chains of six layers
    print("tiny synthesizer, half storage: rel rms %.3e to fp32, %.3e to AICG_HALF=1 (that run: %.3e to fp32); oracle .half() on CPU to its fp32: %s"
          % (e, e16, rel_rms(o16, o32), _d_ref(cfg, 12, 1234)))


@pytest.mark.gpu
def test_synth_40k_half_store_against_fp32(monkeypatch):
    """Full-size v2 / 40 kHz synthesizer, 300 frames: the 64- and 32-channel stages on the half-storage kernel."""
    import conftest
    from synthetic import weights
    conftest._bind("hip")
    dev = conftest.Dev("hip")
    o32, o16, ohs, calls = _synth_three_ways(dev, monkeypatch, weights.SYNTH_CFG_40K_V2, 300)
    e, e16 = _check_synth(o32, o16, ohs, calls)
    assert len(calls) == 36               # two stages
    print("40k v2 synthesizer, half storage: rel rms %.3e to fp32, %.3e to AICG_HALF=1 (that run: %.3e to fp32)" % (e, e16, rel_rms(o16, o32)))


def test_windowed_decoder_equals_full_in_half_store_mode(dev, monkeypatch):
    """tests/test_synth_window.py's property in this mode: beyond decoder_reach() the window's samples are the full run's, bit for bit
    (rates 10, 2: stages of 32 and 16 channels, both on the half-storage kernel; reach 13 frames, granule 12)."""
    import test_synth_window as W
    monkeypatch.setattr(ops, "winograd1d_min_positions", 64)
    monkeypatch.setenv("AICG_HALF", "1")
    monkeypatch.setenv("AICG_HALF_STORE", "1")
    net = _make(dev, W.FAST, 4242).half()
    spy = _Spy(monkeypatch)
    T, upp = 131, net.upp
    inp = W._inputs(net, T, 11)
    full = W._back(dev, net, *inp)
    assert len(spy.calls) == 36 and full.shape == (1, 1, T * upp)
    for pad in (19, 40):
        keep = (pad * upp + 3, (T - pad) * upp - 5)
        assert net.decoder_window(T, keep) is not None
        assert torch.equal(W._back(dev, net, *inp, keep=keep), full[:, :, keep[0]:keep[1]])
    net.float()
    assert not torch.equal(W._back(dev, net, *inp), full)


def test_switch_hygiene(dev, monkeypatch):
    """AICG_HALF_STORE=1 without AICG_HALF=1: .half() marks nothing, the fp32 run's bits.  Both set: .half() selects the mode and .float()
    restores the fp32 bits (what the mode computes: test_synth_tiny_half_store_against_fp32)."""
    from synthetic import weights
    cfg, T, seed = weights.SYNTH_CFG_TINY, 12, 1234
    monkeypatch.delenv("AICG_HALF", raising=False)
    monkeypatch.delenv("AICG_HALF_STORE", raising=False)
    assert not ops.half_store_requested()
    net = _make(dev, cfg, seed)
    o32 = _fp32_run(dev, net, cfg, T, seed)
    monkeypatch.setenv("AICG_HALF_STORE", "1")
    assert not ops.half_store_requested()
    spy = _Spy(monkeypatch)
    net.half()
    assert not net._half and not net._half_store
    assert torch.equal(_infer(net, cfg, T, seed), o32) and not spy.calls
    monkeypatch.setenv("AICG_HALF", "1")
    assert ops.half_store_requested()
    net.half()
    assert net._half and net._half_store
    net.float()
    assert not net._half and not net._half_store
    assert torch.equal(_infer(net, cfg, T, seed), o32) and not spy.calls
    # AICG_HALF=1 alone: the fp16-operand mode without the half-storage route
    monkeypatch.delenv("AICG_HALF_STORE")
    net.half()
    assert net._half and not net._half_store
    net.float()


@pytest.mark.gpu
def test_c1_pipeline_half_store_against_fp32_and_the_reference(monkeypatch):
    """BASELINE C1 (30 s, full-size networks) through VC.pipeline in the half-storage mode: the coarse f0 bins of the fp32 run (the f0 models
    stay fp32), the int16 waveform within the half mode's 5e-3 relative rms of the fp32 run and of the reference's golden."""
    import conftest
    from synthetic import weights
    from synthetic.inputs import vocal_like
    from test_pipeline import build, noise_fn_for
    conftest._bind("hip")
    dev = conftest.Dev("hip")
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "pipeline_c1_30s.npz"))
    seed, x = int(gold["seed"][0]), tuple(int(v) for v in gold["x"])
    nets = weights.full_model_set(seed)
    audio = vocal_like(float(gold["seconds"][0]), 16000, seed + 5)
    monkeypatch.setenv("AICG_HALF", "1")
    monkeypatch.setenv("AICG_HALF_STORE", "1")
    spy = _Spy(monkeypatch)
    outs, bins = [], []
    for half in (False, True):
        vc, hub, net_g, tgt_sr = build(dev, nets, x)
        hub, net_g = (hub.half(), net_g.half()) if half else (hub.float(), net_g.float())
        seen, front = [], vc._vc_synth_front
        vc._vc_synth_front = lambda net, sid, n_samples, feats, feats0, pitch, *a, _f=front, _s=seen, **k: \
            _s.append(pitch.cpu().clone()) or _f(net, sid, n_samples, feats, feats0, pitch, *a, **k)
        outs.append(vc.pipeline(hub, net_g, 0, audio, "x.wav", [0, 0, 0], 0, "rmvpe", "", 0.5, 1, 3, tgt_sr, 0, 0.25, "v2", 0.33, 128,
                                noise_fn=noise_fn_for(nets)))
        bins.append(seen)
        assert bool(spy.calls) == half
    assert bins[0] and len(bins[0]) == len(bins[1]) and all(torch.equal(a, b) for a, b in zip(*bins))
    assert all(c[3] == "conv1d_h_kernel" for c in spy.calls)
    o32, ohs, ref = outs[0].astype(np.float64), outs[1].astype(np.float64), gold["audio"].astype(np.float64)
    e = float(np.sqrt(((ohs - o32) ** 2).sum() / (o32 ** 2).sum()))
    er = float(np.sqrt(((ohs - ref) ** 2).sum() / (ref ** 2).sum()))
    print("C1 half storage vs fp32: rel rms %.3e, <= 1 LSB on %.4f; vs the reference's fp32 output: %.3e" % (e, (np.abs(ohs - o32) <= 1).mean(), er))
    assert 1e-5 < e < 5e-3, e
    assert er < 5e-3, er
