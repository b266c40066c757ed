"""VC.front / VC.pipeline(front=): the voice-independent part of a conversion (plan, f0 estimate, HuBERT) computed once per track and
shared by every voice and every `f0_up_key`.  The bar is bit equality: a call with a front returns the int16 samples the same call
without one returns, under whichever schedule the front-less call takes (emulator: serial and progressive; hardware: the default).

Geometry: three chunks, so the bounds, the per-chunk pitch slices and the encoder-half stream are all exercised, on the seeded miniature
models -- on the hardware tests/test_pipeline.py's 8 s / x = (1, 1, 3, 4) track; on the emulator, which takes a minute for that one,
2.4 s cut at x = (1, 1, 1, 2)."""
import types

import numpy as np
import pytest
import torch

import test_pipeline as tp
from aicovergen_amd import crepe
from aicovergen_amd.vc_infer_pipeline import VoiceFront
from synthetic import weights
from synthetic.inputs import vocal_like

GEOMETRY = {"hip": ((1, 1, 3, 4), 8.0), "emu": ((1, 1, 1, 2), 2.4)}
SEED = 7
_ctx = {}


def ctx(dev, tmp_path_factory=None):
    """Per library (emulator / hardware): models, the track, an index file, and the front-less outputs already computed."""
    if dev.kind not in _ctx:
        nets = weights.small_model_set(1234)
        x, seconds = GEOMETRY[dev.kind]
        vc, hub, net_g, tgt_sr = tp.build(dev, nets, x)
        audio = vocal_like(seconds, 16000, seed=21)
        assert len(vc.chunk_bounds(*vc.plan(audio)[1:3])) == 3
        _ctx[dev.kind] = types.SimpleNamespace(nets=nets, vc=vc, hub=hub, net_g=net_g, tgt_sr=tgt_sr, audio=audio, index=None, refs={},
                                               fronts={})
    return _ctx[dev.kind]


def index_file(c, tmp_path_factory):
    """A flat index (a .npy of vectors, which retrieval.load_index reads) scattered around the track's own HuBERT features."""
    if c.index is None:
        feats = c.vc._hubert_many(c.hub, [c.audio[:16000]], "v2")[0][0].cpu().numpy()
        rng = np.random.default_rng(8)
        train = (feats[rng.integers(0, feats.shape[0], 300)] + 0.2 * rng.standard_normal((300, feats.shape[1]))).astype(np.float32)
        c.index = str(tmp_path_factory.mktemp("front_index") / "total_fea.npy")
        np.save(c.index, train)
    return c.index


def convert(c, front=None, key=0, protect=0.33, index="", f0_method="rmvpe", if_f0=1, version="v2", net_g=None, vc=None, audio=None,
            **kw):
    vc = vc or c.vc
    out = vc.pipeline(c.hub, net_g or c.net_g, 0, c.audio if audio is None else audio, "x.wav", [0, 0, 0], key, f0_method, index, 0.75,
                      if_f0, 3, c.tgt_sr, 0, 0.25, version, protect, 128, noise_seed=SEED, front=front, **kw)
    return out


def make_front(c, f0_method="rmvpe", if_f0=1, version="v2", vc=None, audio=None):
    return (vc or c.vc).front(c.hub, c.audio if audio is None else audio, "x.wav", f0_method, if_f0, version, 3, 128)


def schedules(dev):
    """AICG_F0_SEGMENTS values the front-less reference runs under: the emulator's serial and progressive schedules, the hardware's default."""
    return ("0", "3") if dev.kind == "emu" else (None,)


def with_segments(monkeypatch, seg):
    if seg is None:
        monkeypatch.delenv("AICG_F0_SEGMENTS", raising=False)
    else:
        monkeypatch.setenv("AICG_F0_SEGMENTS", seg)


def same(a, b):
    return a.dtype == np.int16 and torch.equal(torch.from_numpy(a), torch.from_numpy(b))


@pytest.mark.parametrize("with_index", [False, True], ids=["noindex", "index"])
@pytest.mark.parametrize("protect", [0.33, 0.5])
@pytest.mark.parametrize("key", [0, 12, -5])
def test_1_front_call_equals_frontless_call_bit_for_bit(dev, monkeypatch, tmp_path_factory, key, protect, with_index):
    c = ctx(dev)
    index = index_file(c, tmp_path_factory) if with_index else ""
    for seg in schedules(dev):
        with_segments(monkeypatch, seg)
        if seg not in c.fronts:           # one front per schedule, shared by all twelve cases: it is read-only
            c.fronts[seg] = make_front(c)
        front = c.fronts[seg]
        assert front.schedule == {"0": "serial", "3": "progressive", None: "progressive"}[seg]
        want = convert(c, None, key, protect, index)
        assert c.vc.last_profile["f0_progressive"] == (0.0 if seg == "0" else 1.0) and "front_reused" not in c.vc.last_profile
        times = [0, 0, 0]
        got = c.vc.pipeline(c.hub, c.net_g, 0, c.audio, "x.wav", times, key, "rmvpe", index, 0.75, 1, 3, c.tgt_sr, 0, 0.25, "v2", protect,
                            128, noise_seed=SEED, front=front)
        prof = c.vc.last_profile
        assert prof["front_reused"] == 1.0 and prof["f0_progressive"] == 0.0 and prof["f0_s"] > 0 and prof["chunks_s"] > 0
        assert all(t > 0 for t in times)
        assert np.abs(want).max() > 100 and same(got, want), (seg, int(np.abs(got.astype(np.int32) - want).max()))
        c.refs[(seg, key, protect, with_index)] = want
    # the parameters really reach the output: another key or the index change it (protect alone does not: without retrieval the
    # protected features are the features)
    base = c.refs.get((schedules(dev)[0], 0, protect, False))
    if base is not None and (key, with_index) != (0, False):
        assert not np.array_equal(want, base)


def test_1b_front_holds_what_plan_and_the_estimator_return(dev, monkeypatch):
    """The front's fields: plan / chunk_bounds' results as they are, the contour UNTRANSPOSED (get_f0 at key 0 returns it), HuBERT's
    output per chunk before the voice touches it; all on the device, untouched by the calls that used it."""
    c = ctx(dev)
    with_segments(monkeypatch, schedules(dev)[0])
    front = make_front(c)
    assert isinstance(front, VoiceFront)
    audio_hp, audio_pad, opt_ts, p_len = c.vc.plan(c.audio)
    assert torch.equal(front.audio, audio_hp) and torch.equal(front.audio_pad, audio_pad)
    assert front.opt_ts == opt_ts and front.p_len == p_len and front.bounds == c.vc.chunk_bounds(audio_pad, opt_ts)
    assert front.f0.dtype == torch.float64 and front.f0.shape == (p_len,) and front.f0.device.type == dev.device.type
    assert len(front.feats) == 3 and all(f.dim() == 3 and f.device.type == dev.device.type for f in front.feats)
    assert front.key["audio_len"] == len(c.audio) and front.key["version"] == "v2" and front.key["x_max"] == GEOMETRY[dev.kind][0][3]
    assert front.nbytes() > 0
    if dev.kind == "emu":           # (hardware: the default schedule estimates in segments, get_f0 in one launch -- other GEMM tiles)
        _, f0 = c.vc.get_f0("x.wav", audio_pad, p_len, 0, "rmvpe", 3, 128)
        assert np.array_equal(front.f0.cpu().numpy(), f0[:p_len])
    before = [front.f0.clone()] + [f.clone() for f in front.feats]
    convert(c, front, 12, 0.33)
    assert all(torch.equal(a, b) for a, b in zip(before, [front.f0] + list(front.feats)))


def test_2_front_for_something_else_is_refused(dev, monkeypatch):
    c = ctx(dev)
    with_segments(monkeypatch, schedules(dev)[0])
    f2 = make_front(c)
    f1 = make_front(c, version="v1")
    assert f1.feats[0].shape[-1] != f2.feats[0].shape[-1]          # final_proj was applied for v1
    with pytest.raises(ValueError, match="version"):
        convert(c, f2, version="v1")
    with pytest.raises(ValueError, match="version"):
        convert(c, f1, version="v2")
    with pytest.raises(ValueError, match="audio_len"):
        convert(c, f2, audio=c.audio[:-160])
    other = c.audio.copy()
    other[5000] += np.float32(0.01)
    with pytest.raises(ValueError, match="audio_sum"):
        convert(c, f2, audio=other)
    with pytest.raises(ValueError, match="f0_method"):
        convert(c, f2, f0_method="mangio-crepe")
    with pytest.raises(ValueError, match="if_f0"):
        convert(c, f2, if_f0=0)
    vc_other, _, _, _ = tp.build(dev, c.nets, (1, 1, 2, 3))
    vc_other.model_rmvpe = c.vc.model_rmvpe
    with pytest.raises(ValueError, match="x_query|x_center|x_max"):
        convert(c, f2, vc=vc_other)
    with pytest.raises(ValueError, match="f0_file"):
        convert(c, f2, f0_file=types.SimpleNamespace(name="curve.csv"))
    with pytest.raises(ValueError, match="process group"):
        convert(c, f2, group=object())
    # a device-resident copy of the same audio is the same audio
    assert same(convert(c, f2, audio=torch.from_numpy(c.audio).to(dev.device)), convert(c, f2))


def test_3_work_is_shared(dev, monkeypatch):
    """One front() and three calls with it run HuBERT and RMVPE once; three calls without run them three times."""
    c = ctx(dev)
    with_segments(monkeypatch, "3" if dev.kind == "emu" else None)      # the schedule with one HuBERT pass over all chunks
    n = {"hubert": 0, "rmvpe": 0}

    def counted(obj, name, what):
        real = getattr(obj, name)

        def spy(*a, **k):
            n[what] += 1
            return real(*a, **k)
        monkeypatch.setattr(obj, name, spy)
    counted(c.hub, "extract_features_many", "hubert")
    counted(c.hub, "extract_features", "hubert")
    for entry in ("infer_from_audio", "infer_progressive"):
        counted(c.vc.model_rmvpe, entry, "rmvpe")
    front = make_front(c)
    outs = [convert(c, front, key) for key in (0, 12, -5)]
    assert n == {"hubert": 1, "rmvpe": 1}
    n.update(hubert=0, rmvpe=0)
    refs = [convert(c, None, key) for key in (0, 12, -5)]
    assert n == {"hubert": 3, "rmvpe": 3}
    assert all(same(a, b) for a, b in zip(outs, refs))


def test_4_mangio_crepe_and_models_without_f0(dev, monkeypatch):
    c = ctx(dev)
    with_segments(monkeypatch, schedules(dev)[0])
    monkeypatch.setattr(crepe, "DITHER", lambda n: (torch.arange(n) % 7 - 3).float())      # torchcrepe's dither is random: pinned
    c.vc.model_crepe = {"full": crepe.Crepe(weights.crepe_state_dict(weights.CREPE_MICRO, 5), dev.device)}
    try:
        front = make_front(c, f0_method="mangio-crepe")
        assert front.schedule == "serial" and front.f0.shape == (front.p_len,) and float(front.f0.max()) > 0
        for key in (0, -5):
            assert same(convert(c, front, key, f0_method="mangio-crepe"), convert(c, None, key, f0_method="mangio-crepe"))
    finally:
        del c.vc.model_crepe
    # `_nono` models (if_f0 == 0): no contour, no protect blend
    from aicovergen_amd.infer_pack.models import SynthesizerTrnMs768NSFsid_nono
    cfg = list(c.nets["synth_cfg"])
    nono = SynthesizerTrnMs768NSFsid_nono(*cfg)
    del nono.enc_q
    nono.load_state_dict(weights.synth_state_dict(cfg, 41, f0=False), strict=False)
    nono.eval().to(dev.device)
    front = make_front(c, if_f0=0)
    assert front.f0 is None and len(front.feats) == 3
    got, want = convert(c, front, if_f0=0, net_g=nono), convert(c, None, if_f0=0, net_g=nono)
    assert np.abs(want).max() > 50 and same(got, want)


def test_4b_v1_model(dev, monkeypatch):
    """v1 voices: layer 9 + final_proj in the front, the 256-channel synthesizer behind it."""
    from aicovergen_amd.infer_pack.models import SynthesizerTrnMs256NSFsid
    c = ctx(dev)
    with_segments(monkeypatch, schedules(dev)[-1])
    cfg = list(c.nets["synth_cfg"])
    net = SynthesizerTrnMs256NSFsid(*cfg, is_half=False)
    del net.enc_q
    net.load_state_dict(weights.synth_state_dict(cfg, 31, phone_dim=256), strict=False)
    net.eval().to(dev.device)
    front = make_front(c, version="v1")
    assert same(convert(c, front, 12, version="v1", net_g=net), convert(c, None, 12, version="v1", net_g=net))


def test_5_device_output(dev, monkeypatch):
    c = ctx(dev)
    with_segments(monkeypatch, schedules(dev)[-1])
    front = make_front(c)
    host = convert(c, front, -5)
    on_dev = convert(c, front, -5, device_out=True)
    assert torch.is_tensor(on_dev) and on_dev.dtype == torch.int16 and on_dev.device.type == dev.device.type
    assert torch.equal(on_dev.cpu(), torch.from_numpy(host))
