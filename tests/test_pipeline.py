"""VC.pipeline end to end on the HIP kernels vs (a) the golden int16 output of the REFERENCE's own VC.pipeline
(tests/golden/pipeline_small_2p6s.npz) and (b) the oracle pipeline.  Bar: |diff| <= 1 LSB on >= 99.9 % of the int16
samples, identical cut points, coarse-pitch bin agreement reported as a rate."""
import contextlib
import os

import numpy as np
import pytest
import torch

from aicovergen_amd.hubert import HubertModel
from aicovergen_amd.infer_pack.models import SynthesizerTrnMs768NSFsid
from aicovergen_amd.rmvpe import RMVPE
from aicovergen_amd.vc_infer_pipeline import VC, Pipeline, change_rms
from conftest import rel_rms
from oracle import pipeline as opipe
from synthetic import weights
from synthetic.inputs import vocal_like

GOLD = os.path.join(os.path.dirname(__file__), "golden")


class _Cfg:
    def __init__(self, device, x=(1, 1, 1, 2)):
        self.x_pad, self.x_query, self.x_center, self.x_max = x
        self.is_half, self.device = False, device


def build(dev, nets, x=(1, 1, 1, 2)):
    tgt_sr = nets["synth_cfg"][-1]
    vc = VC(tgt_sr, _Cfg(dev.device, x))
    hub = HubertModel(nets["hubert_sd"], nets["hubert_cfg"]).to(dev.device)
    vc.model_rmvpe = RMVPE(None, False, dev.device, state_dict=nets["rmvpe_sd"])
    net_g = SynthesizerTrnMs768NSFsid(*nets["synth_cfg"], is_half=False)
    del net_g.enc_q
    net_g.load_state_dict(nets["synth_sd"], strict=False)
    net_g.eval().to(dev.device)
    return vc, hub, net_g, tgt_sr


def noise_fn_for(nets, seed=7):
    cfg = nets["synth_cfg"]
    upp = int(np.prod(cfg[12]))

    def fn(ci, s, e):
        nz, ns = opipe.chunk_noise(ci, opipe.chunk_frames(e - s), cfg[2], upp, seed)
        return nz, ns[0]
    return fn


def run(dev, nets, audio, x=(1, 1, 1, 2), group=None):
    vc, hub, net_g, tgt_sr = build(dev, nets, x)
    times = [0, 0, 0]
    out = vc.pipeline(hub, net_g, 0, audio, "x.wav", times, 0, "rmvpe", "", 0.5, 1, 3, tgt_sr, 0, 0.25, "v2", 0.33, 128,
                      noise_fn=noise_fn_for(nets), group=group)
    return out, times, vc


def test_pipeline_alias():
    assert Pipeline is VC


def test_pipeline_small_vs_reference_golden(dev):
    gold = np.load(os.path.join(GOLD, "pipeline_small_2p6s.npz"))
    nets = weights.small_model_set(int(gold["seed"][0]))
    audio = vocal_like(float(gold["seconds"][0]), 16000, int(gold["seed"][0]) + 5)
    out, times, vc = run(dev, nets, audio)
    assert out.dtype == np.int16 and out.shape == gold["audio"].shape
    diff = np.abs(out.astype(np.int32) - gold["audio"].astype(np.int32))
    # fp32 synthesizer differences (~1e-5 absolute) are amplified ~4x by the RMS mix before the truncating int16
    # cast: <= 1 LSB on >= 99.9 % of the samples (SURVEY 8d bar), never more than 3 LSB
    assert diff.max() <= 3, "max int16 difference %d" % diff.max()
    assert (diff <= 1).mean() >= 0.999
    assert (diff == 0).mean() > 0.5
    assert all(t > 0 for t in times)          # times = [hubert, f0, synth] are accumulated like the reference
    # formula for the un-chunked output length is covered by the chunked case summing up
    geo = opipe.Geometry(vc.t_pad_tgt // vc.x_pad, 1, 1, 1, 2)
    ref_audio, info = opipe.vc_pipeline(nets, geo, audio, tgt_sr=nets["synth_cfg"][-1])
    _, audio_pad, opt_ts, p_len = vc.plan(audio)
    assert [int(t) for t in opt_ts] == [int(t) for t in info["opt_ts"]]     # cut points: bit-exact
    coarse, f0 = vc.get_f0("x.wav", audio_pad, p_len, 0, "rmvpe", 3, 128)
    assert_bins_agree(coarse[:p_len], f0[:p_len], info["coarse"][:p_len], info["f0"][:p_len], info["hidden"])


def test_f0_file_branch_vs_reference_golden(dev, tmp_path):
    """The f0 curve file argument (reference src/vc_infer_pipeline.py:511-519 reads it, :349-358 splices it over the estimate from
    x_pad seconds on): tests/golden/pipeline_small_f0file.npz is the REFERENCE's own VC.pipeline run with such a file
    (make_golden.py branches).  rvc_infer never passes one (src/rvc.py:150), the web UI's upstream does."""
    import types
    gold = np.load(os.path.join(GOLD, "pipeline_small_f0file.npz"))
    nets = weights.small_model_set(int(gold["seed"][0]))
    audio = vocal_like(float(gold["seconds"][0]), 16000, int(gold["seed"][0]) + 5)
    f = tmp_path / "curve.csv"
    f.write_text("\n".join("%.6f,%.6f" % (t, v) for t, v in gold["f0_rows"]) + "\n")
    vc, hub, net_g, tgt_sr = build(dev, nets)
    seen = {}
    orig = vc.get_f0

    def spy(*a, **k):
        seen["coarse"], seen["f0"] = orig(*a, **k)
        return seen["coarse"], seen["f0"]
    vc.get_f0 = spy
    out = vc.pipeline(hub, net_g, 0, audio, "x.wav", [0, 0, 0], 0, "rmvpe", "", 0.5, 1, 3, tgt_sr, 0, 0.25, "v2", 0.33, 128,
                      f0_file=types.SimpleNamespace(name=str(f)), noise_fn=noise_fn_for(nets))
    # the spliced span is the file's curve exactly (np.interp on the same float32 rows), the rest the estimator's track
    tf0 = vc.sr // vc.window
    n_rep = int(np.round((gold["f0_rows"][:, 0].max() - gold["f0_rows"][:, 0].min()) * tf0 + 1))
    lo = vc.x_pad * tf0
    n = min(len(seen["f0"]), len(gold["f0"]))
    assert np.allclose(seen["f0"][lo:lo + n_rep], gold["f0"][lo:lo + n_rep], rtol=1e-6, atol=1e-6)
    assert not np.allclose(seen["f0"][lo:lo + n_rep], 0)                 # the curve really landed there
    assert np.array_equal(seen["coarse"][lo:lo + n_rep], gold["coarse"][lo:lo + n_rep])
    assert (np.asarray(seen["coarse"][:n]) != gold["coarse"][:n]).mean() <= 0.002
    diff = np.abs(out.astype(np.int32) - gold["audio"].astype(np.int32))
    assert out.shape == gold["audio"].shape and diff.max() <= 3 and (diff <= 1).mean() >= 0.999


def test_resample_sr_branch_vs_reference_golden(dev):
    """resample_sr != 0 (reference src/vc_infer_pipeline.py:639-644: change_rms at tgt_sr FIRST, then librosa.resample, then the
    peak normalisation and the int16 cast).  The golden is the reference's own run with librosa.resample served by scipy's
    polyphase resampler (librosa / resampy are not installable here; stated in make_golden.py): it pins the branch's order of
    operations and output length, not resampy's filter."""
    gold = np.load(os.path.join(GOLD, "pipeline_small_resample32k.npz"))
    nets = weights.small_model_set(int(gold["seed"][0]))
    audio = vocal_like(float(gold["seconds"][0]), 16000, int(gold["seed"][0]) + 5)
    vc, hub, net_g, tgt_sr = build(dev, nets)
    out = vc.pipeline(hub, net_g, 0, audio, "x.wav", [0, 0, 0], 0, "rmvpe", "", 0.5, 1, 3, tgt_sr, int(gold["resample_sr"][0]), 0.25,
                      "v2", 0.33, 128, noise_fn=noise_fn_for(nets))
    assert out.dtype == np.int16 and out.shape == gold["audio"].shape
    diff = np.abs(out.astype(np.int32) - gold["audio"].astype(np.int32))
    assert diff.max() <= 3 and (diff <= 1).mean() >= 0.999


def test_progressive_f0_schedule_matches_one_launch(dev, monkeypatch):
    """Multi-GPU schedule: the BiGRU recurrence in segments (AICG_F0_SEGMENTS; the default for world > 1 and, since r4, for one
    rank on a GPU; "1" = one launch), the pitch of
    a frame range published as soon as both directions have passed it, the chunks taken middle-out with a per-chunk wait.  On a
    6-chunk track the int16 output must equal the one-launch schedule's -- BIT FOR BIT on the emulator (one tile path per layer);
    on the hardware to <= 1 LSB on 99.9 % of the samples and never more than 3 LSB: the recurrence itself is bit-identical in segments
    (tests/test_hubert_rmvpe.py), but the classifier GEMM over a frame RANGE may be routed to other tiles than over the whole track,
    i.e. another fp32 summation order of the salience -- and the chunk order must really differ."""
    nets = weights.small_model_set(1234)
    audio = vocal_like(6.3, 16000, 1239)
    monkeypatch.setenv("AICG_F0_SEGMENTS", "1")
    ref, _, vc0 = run(dev, nets, audio)
    assert vc0.last_profile["f0_progressive"] == 0.0
    monkeypatch.setenv("AICG_F0_SEGMENTS", "6")
    vc, hub, net_g, tgt_sr = build(dev, nets, (1, 1, 1, 2))
    seen = []
    orig = vc._vc_synth_front

    def spy(net, sid, n_samples, *a, **k):
        seen.append(n_samples)
        return orig(net, sid, n_samples, *a, **k)
    vc._vc_synth_front = spy
    out = vc.pipeline(hub, net_g, 0, audio, "x.wav", [0, 0, 0], 0, "rmvpe", "", 0.5, 1, 3, tgt_sr, 0, 0.25, "v2", 0.33, 128,
                      noise_fn=noise_fn_for(nets))
    assert vc.last_profile["f0_progressive"] == 1.0
    if dev.kind == "emu":
        assert np.array_equal(out, ref)
    else:   # on the hardware the classifier GEMM over a frame range may take other tiles than over the whole track (fp32 summation order)
        diff = np.abs(out.astype(np.int32) - ref.astype(np.int32))
        assert diff.max() <= 3 and (diff <= 1).mean() >= 0.999
    _, audio_pad, opt_ts, _ = vc.plan(audio)
    bounds = vc.chunk_bounds(audio_pad, opt_ts)
    assert len(bounds) >= 5 and seen != [e - s for s, e in bounds] and sorted(seen) == sorted(e - s for s, e in bounds)


def test_every_f0_estimate_passes_the_seam_under_both_schedules(dev, monkeypatch):
    """VC._estimated_f0 (the seam tests/test_bench_sizes.py injects the reference's f0 through): called once with the whole track under the
    one-launch schedule, range by range -- middle first, disjoint, covering every pitch frame -- under the progressive one; replacing
    the estimate there changes the output under either schedule, and a constant track gives the same output under both."""
    nets = weights.small_model_set(1234)
    audio = vocal_like(6.3, 16000, 1239)
    outs = {}
    for nseg in ("1", "6"):
        monkeypatch.setenv("AICG_F0_SEGMENTS", nseg)
        vc, hub, net_g, tgt_sr = build(dev, nets, (1, 1, 1, 2))
        seen = []

        def flat(lo, hi, f0, _seen=seen):
            _seen.append((lo, hi, len(f0)))
            return (torch.full_like(f0, 220.0) if torch.is_tensor(f0) else np.full_like(f0, 220.0))
        vc._estimated_f0 = flat
        outs[nseg] = vc.pipeline(hub, net_g, 0, audio, "x.wav", [0, 0, 0], 0, "rmvpe", "", 0.5, 1, 3, tgt_sr, 0, 0.25, "v2", 0.33, 128,
                                 noise_fn=noise_fn_for(nets))
        _, audio_pad, _, p_len = vc.plan(audio)
        if nseg == "1":
            assert len(seen) == 1 and seen[0][0] == 0 and seen[0][2] >= p_len
        else:
            assert len(seen) > 2 and seen[0][0] > 0 and all(hi - lo == n for lo, hi, n in seen)
            cov = np.zeros(max(hi for _, hi, _ in seen), dtype=int)
            for lo, hi, _ in seen:
                cov[lo:hi] += 1
            assert np.all(cov[:p_len] == 1)
    assert np.array_equal(outs["1"], outs["6"])          # same (constant) pitch in -> same waveform out, whatever the schedule
    ref, _, _ = run(dev, nets, audio)
    assert not np.array_equal(outs["1"], ref)


# ---- exchange-timeout recovery -------------------------------------------------------------------------------------------
# The multi-workgroup BiGRU reports a partner timeout only on a busy shared GPU.  These tests never make a kernel time out: they make the
# two poll functions (ops.gru_timed_out, ops.GruSegments.timed_out) SAY so, and check what pipeline() does then -- f0 again on the
# single-workgroup kernel through get_f0's tail, this rank's chunks again.

def _gru_timeout_on_next_poll(monkeypatch):
    """ops.gru_timed_out reports a timeout on its next poll and only there (the real poll still runs: it drains the pending flags)."""
    from aicovergen_amd import ops
    real, state = ops.gru_timed_out, {"polls": 0}

    def poll():
        state["polls"] += 1
        return bool(real()) or state["polls"] == 1
    monkeypatch.setattr(ops, "gru_timed_out", poll)
    return state


@contextlib.contextmanager
def _single_workgroup_gru(monkeypatch):
    """For the run a recovery is compared with: recovery re-estimates f0 on the single-workgroup recurrence, and the multi-workgroup kernels
    (the small models have RMVPE's hidden size, 256: the emulator runs them too) sum in another fp32 order -- 1.5e-7 apart, which moves an
    int16 sample now and then.  Pinned to the same form (AICG_GRU_2WG=0), the comparison is bit for bit."""
    from aicovergen_amd import ops
    with monkeypatch.context() as m:
        m.setattr(ops, "GRU_TWO_WORKGROUPS", False)
        yield


def _assert_same_track(dev, out, ref):
    """Bit for bit on the emulator; on the hardware the bar of test_progressive_f0_schedule_matches_one_launch, for its reason: the
    classifier GEMM may be routed to other tiles from one run to the other (fp32 summation order of the salience)."""
    assert out.dtype == np.int16 and out.shape == ref.shape
    diff = np.abs(out.astype(np.int32) - ref.astype(np.int32))
    print("recovery vs reference run: max diff %d LSB, <= 1 LSB on %.5f, equal on %.5f" % (diff.max(), (diff <= 1).mean(), (diff == 0).mean()))
    if dev.kind == "emu":
        assert np.array_equal(out, ref)
    else:
        assert diff.max() <= 3 and (diff <= 1).mean() >= 0.999


def test_progressive_recovery_after_a_late_exchange_timeout(dev, monkeypatch):
    """The timeout shows at the end-of-loop poll only: every chunk has been synthesised from the (declared invalid) progressive pitch, the
    call warns, and its output is the one-launch schedule's -- recovery is a whole-track f0 through get_f0's tail."""
    nets = weights.small_model_set(1234)
    audio = vocal_like(6.3, 16000, 1239)
    monkeypatch.setenv("AICG_F0_SEGMENTS", "1")
    with _single_workgroup_gru(monkeypatch):
        ref, _, _ = run(dev, nets, audio)
    monkeypatch.setenv("AICG_F0_SEGMENTS", "6")
    state = _gru_timeout_on_next_poll(monkeypatch)
    with pytest.warns(RuntimeWarning, match="BiGRU timed out"):
        out, times, vc = run(dev, nets, audio)
    assert vc.last_profile["f0_progressive"] == 1.0 and state["polls"] == 1
    assert len(vc.chunk_bounds(*vc.plan(audio)[1:3])) >= 5 and all(t > 0 for t in times)
    _assert_same_track(dev, out, ref)


def test_progressive_recovery_after_an_early_exchange_timeout(dev, monkeypatch):
    """The recurrence's error word is set from the first poll on (settle): the chunk loop synthesises NOTHING from the invalid pitch, every
    chunk comes from recovery -- in chunk order, once each -- and the output is the same as after a late timeout."""
    from aicovergen_amd import ops
    nets = weights.small_model_set(1234)
    audio = vocal_like(6.3, 16000, 1239)
    monkeypatch.setenv("AICG_F0_SEGMENTS", "1")
    with _single_workgroup_gru(monkeypatch):
        ref, _, _ = run(dev, nets, audio)
    monkeypatch.setenv("AICG_F0_SEGMENTS", "6")
    vc, hub, net_g, tgt_sr = build(dev, nets, (1, 1, 1, 2))
    events = []
    monkeypatch.setattr(ops.GruSegments, "timed_out", lambda self: events.append("poll") or True)
    front, back = vc._vc_synth_front, vc._vc_synth_back

    def spy_front(net, sid, n_samples, *a, **k):
        events.append(n_samples)
        return front(net, sid, n_samples, *a, **k)

    def spy_back(*a, **k):
        events.append("back")
        return back(*a, **k)
    vc._vc_synth_front, vc._vc_synth_back = spy_front, spy_back
    with pytest.warns(RuntimeWarning, match="BiGRU timed out"):
        out = vc.pipeline(hub, net_g, 0, audio, "x.wav", [0, 0, 0], 0, "rmvpe", "", 0.5, 1, 3, tgt_sr, 0, 0.25, "v2", 0.33, 128,
                          noise_fn=noise_fn_for(nets))
    assert vc.last_profile["f0_progressive"] == 1.0
    _, audio_pad, opt_ts, _ = vc.plan(audio)
    bounds = vc.chunk_bounds(audio_pad, opt_ts)
    assert len(bounds) >= 5 and events.count("poll") == 1          # settle's poll; the loop ends before its own
    settle = events.index("poll")
    # before settle: nothing -- except, with the encoder halves on their own stream (hardware), the first chunk's, which the progressive
    # schedule queues ahead of settle by design; its vocoder half never runs
    ahead = events[:settle]
    assert len(ahead) <= (1 if dev.kind == "hip" else 0) and "back" not in ahead
    assert [n for n in events[settle + 1:] if n != "back"] == [e - s for s, e in bounds]     # exactly len(bounds) fronts, all from recovery
    assert events.count("back") == len(bounds)
    _assert_same_track(dev, out, ref)


def test_one_launch_recovery_after_an_exchange_timeout(dev, monkeypatch, tmp_path):
    """One-launch overlapped schedule (f0 on the side stream, the recurrence as one launch; an f0 curve file keeps it whatever
    AICG_F0_SEGMENTS says, which makes it reachable on the emulator): a timeout at its poll re-estimates f0 with two_workgroups=False,
    and the output is the uninjected run's -- within the reference golden's bar."""
    import types
    gold = np.load(os.path.join(GOLD, "pipeline_small_f0file.npz"))
    nets = weights.small_model_set(int(gold["seed"][0]))
    audio = vocal_like(float(gold["seconds"][0]), 16000, int(gold["seed"][0]) + 5)
    f = tmp_path / "curve.csv"
    f.write_text("\n".join("%.6f,%.6f" % (t, v) for t, v in gold["f0_rows"]) + "\n")
    monkeypatch.setenv("AICG_F0_SEGMENTS", "6")

    def convert(calls):
        vc, hub, net_g, tgt_sr = build(dev, nets)
        orig = vc.model_rmvpe.infer_from_audio_device

        def spy(audio, thred=0.03, two_workgroups=None, group=None):
            calls.append(two_workgroups)
            return orig(audio, thred, two_workgroups, group)
        vc.model_rmvpe.infer_from_audio_device = spy
        out = vc.pipeline(hub, net_g, 0, audio, "x.wav", [0, 0, 0], 0, "rmvpe", "", 0.5, 1, 3, tgt_sr, 0, 0.25, "v2", 0.33, 128,
                          f0_file=types.SimpleNamespace(name=str(f)), noise_fn=noise_fn_for(nets))
        assert vc.last_profile["overlap_f0"] == 1.0 and vc.last_profile["f0_progressive"] == 0.0
        return out
    plain, injected = [], []
    with _single_workgroup_gru(monkeypatch):
        ref = convert(plain)
    state = _gru_timeout_on_next_poll(monkeypatch)
    out = convert(injected)
    assert plain[0] is None and injected == [None, False] and state["polls"] == 1
    _assert_same_track(dev, out, ref)
    diff = np.abs(out.astype(np.int32) - gold["audio"].astype(np.int32))
    assert out.shape == gold["audio"].shape and diff.max() <= 3 and (diff <= 1).mean() >= 0.999


def assert_bins_agree(coarse, f0, want_coarse, want_f0, want_salience, max_rate=0.002):
    """The C1 test's criterion: coarse-pitch bins equal to the oracle's on >= 99.8 % of the frames; every other frame
    is listed with its f0 distance and the oracle's top-1 - top-2 salience margin and must be a neighbouring bin (a cents value
    that rounds across a bin edge) or a near-tie of the salience argmax."""
    n = min(len(coarse), len(want_coarse))
    bad = np.nonzero(np.asarray(coarse[:n]) != np.asarray(want_coarse[:n]))[0]
    top2 = np.sort(np.asarray(want_salience)[bad], axis=1)[:, -2:] if len(bad) else np.zeros((0, 2))
    for t, m in zip(bad, top2[:, 1] - top2[:, 0]):
        print("  frame %d: bin %d vs %d, f0 %.4f vs %.4f Hz, salience top1-top2 %.3e" % (t, coarse[t], want_coarse[t], f0[t], want_f0[t], m))
    print("coarse-bin agreement %.5f (%d of %d frames differ)" % (1 - len(bad) / max(n, 1), len(bad), n))
    assert len(bad) <= max_rate * n, "%d of %d coarse bins differ" % (len(bad), n)
    for t, m in zip(bad, top2[:, 1] - top2[:, 0]):
        assert abs(int(coarse[t]) - int(want_coarse[t])) <= 1 or m < 1e-3


def test_cut_points_do_not_depend_on_the_filter_implementation(dev, monkeypatch):
    """plan() high-passes on the device (block-parallel filtfilt, ~5e-8 of the peak from scipy's sequential one) and then searches
    the quietest sample bit-exactly: the cut points -- and with them every chunk boundary -- must equal the ones the host filter
    gives.  CPU: 9 s with 1 s windows; GPU: the bench's 240 s track with main.py's preset."""
    nets = weights.small_model_set(3)
    x = (3, 10, 60, 65) if dev.big else (1, 1, 1, 2)
    vc, _, _, _ = build(dev, nets, x)
    audio = vocal_like(240.0 if dev.big else 9.0, 16000, 1234)
    _, pad_dev, ts_dev, p_dev = vc.plan(audio)
    monkeypatch.setenv("AICG_FILTFILT", "host")
    _, pad_host, ts_host, p_host = vc.plan(audio)
    assert len(ts_dev) >= 3 and [int(t) for t in ts_dev] == [int(t) for t in ts_host] and p_dev == p_host
    assert float((pad_dev - pad_host).abs().max()) < 1e-6 * float(pad_host.abs().max())


def test_change_rms_matches_oracle():
    rng = np.random.default_rng(0)
    a = rng.standard_normal(16000 * 2).astype(np.float64) * 0.1
    b = rng.standard_normal(40000 * 2).astype(np.float32) * 0.2
    want = opipe.change_rms(a, 16000, b.copy(), 40000, 0.25)
    got = change_rms(a, 16000, b.copy(), 40000, 0.25)
    assert np.allclose(got, want, rtol=1e-6, atol=1e-7)


def test_unsupported_f0_method_raises(dev):
    nets = weights.small_model_set(1)
    vc, _, _, _ = build(dev, nets)
    with pytest.raises(NotImplementedError):
        vc.get_f0("x", np.zeros(16000), 100, 0, "harvest", 3, 128)


@pytest.mark.gpu
def test_pipeline_full_models_vs_oracle():
    """Full-size HuBERT-base + RMVPE + 40 kHz v2 synthesizer on 8 s of audio with chunking forced
    (x = 1,1,3,4 -> 3 chunks) vs the oracle pipeline on the host CPU."""
    import conftest
    conftest._bind("hip")
    dev = conftest.Dev("hip")
    nets = weights.full_model_set(1234)
    audio = vocal_like(8.0, 16000, seed=21)
    x = (1, 1, 3, 4)
    out, times, vc = run(dev, nets, audio, x)
    geo = opipe.Geometry(40000, *x)
    ref, info = opipe.vc_pipeline(nets, geo, audio, tgt_sr=40000)
    assert out.shape == ref.shape and len(info["opt_ts"]) == 2
    diff = np.abs(out.astype(np.int32) - ref.astype(np.int32))
    scale = np.abs(ref).max()
    # fp32 kernels vs fp32 CPU through ~150 layers: relative RMS <= 1e-3 on the waveform; after the
    # truncating int16 cast that is a few LSB at full scale, so the LSB agreement is reported, not gated at 99.9 %
    rel = np.sqrt(np.sum(diff.astype(np.float64) ** 2) / np.sum(ref.astype(np.float64) ** 2))
    print("pipeline full: rel rms %.3e, max diff %d of peak %d, <=1 LSB on %.4f" % (rel, diff.max(), scale, (diff <= 1).mean()))
    assert rel < 1e-3
    assert diff.max() <= max(3, 1e-3 * scale), "max diff %d of peak %d" % (diff.max(), scale)
    assert (diff <= 1).mean() > 0.85
    _, audio_pad, opt_ts, p_len = vc.plan(audio)
    assert [int(t) for t in opt_ts] == [int(t) for t in info["opt_ts"]]     # cut points: bit-exact
    coarse, f0 = vc.get_f0("x.wav", audio_pad, p_len, 0, "rmvpe", 3, 128)
    assert_bins_agree(coarse[:p_len], f0[:p_len], info["coarse"][:p_len], info["f0"][:p_len], info["hidden"])


def test_device_post_processing_matches_oracle(dev):
    """Cut search (box sum + argmin, bit-exact), change_rms, peak and int16 conversion kernels vs numpy/oracle."""
    from aicovergen_amd import ops
    rng = np.random.default_rng(0)
    a = rng.standard_normal(16000 * 3 + 37) * 0.1
    ap = np.pad(a, (80, 80), mode="reflect")
    s = np.zeros_like(a)
    for i in range(160):
        s += ap[i: i - 160]
    got = ops.box_sum_f64(dev.t(torch.from_numpy(ap)), len(a), 160)
    assert np.array_equal(got.cpu().numpy(), s)
    st, ln = [1000, 20000, 0], [5000, 7000, len(a)]
    want = [int(np.where(np.abs(s[x:x + l]) == np.abs(s[x:x + l]).min())[0][0]) for x, l in zip(st, ln)]
    assert ops.argmin_abs_f64(got, st, ln).cpu().tolist() == want
    b = (rng.standard_normal(40000 * 3 + 11) * 0.2).astype(np.float32)
    r1 = ops.frame_rms(dev.t(torch.from_numpy(a)), 16000, 8000)
    r2 = ops.frame_rms(dev.t(torch.from_numpy(b)), 40000, 20000)
    assert np.allclose(r1.cpu().numpy(), opipe.rms_frames(a, 16000, 8000)[0], rtol=1e-12)
    assert np.allclose(r2.cpu().numpy(), opipe.rms_frames(b, 40000, 20000)[0], rtol=1e-6)
    # clips of <= 0.5 s: the reflect padding is longer than the signal (numpy reflects repeatedly, librosa.feature.rms accepts it)
    for n in (1, 2, 37, 3000, 8000, 8001):
        c = rng.standard_normal(n)
        assert np.allclose(ops.frame_rms(dev.t(torch.from_numpy(c)), 16000, 8000).cpu().numpy(),
                           opipe.rms_frames(c, 16000, 8000)[0], rtol=1e-12), n
    want = opipe.change_rms(a, 16000, b.copy(), 40000, 0.25)
    d = dev.t(torch.from_numpy(b.copy()))
    ops.rms_mix_(d, r1, r2, 0.25)
    assert np.abs(d.cpu().numpy() - want).max() < 1e-6 * np.abs(want).max()
    assert abs(ops.absmax(d).item() - np.abs(d.cpu().numpy()).max()) == 0
    sc = 32768 / (np.abs(want).max() / 0.99)
    assert np.array_equal(ops.to_int16(d, sc).cpu().numpy(), (d.cpu().numpy() * np.float32(sc)).astype(np.int16))


def test_vc_chunk_v1_model_matches_oracle(dev):
    """v1 voice models: HuBERT layer 9 + final_proj (768 -> 256) feeding SynthesizerTrnMs256NSFsid
    (vc_infer_pipeline.py:398-406, models.py:532-640) -- the chunk-level path against the oracle's pieces."""
    import torch.nn.functional as F
    from aicovergen_amd.infer_pack.models import SynthesizerTrnMs256NSFsid
    from oracle import hubert as ohub
    from oracle import synth as osynth
    nets = weights.small_model_set()
    cfg = list(nets["synth_cfg"])
    sd = weights.synth_state_dict(cfg, 31, phone_dim=256)
    vc = VC(cfg[-1], _Cfg(dev.device))
    hub = HubertModel(nets["hubert_sd"], nets["hubert_cfg"]).to(dev.device)
    net_g = SynthesizerTrnMs256NSFsid(*cfg, is_half=False)
    del net_g.enc_q
    net_g.load_state_dict(sd, strict=False)
    net_g.eval().to(dev.device)
    audio0 = vocal_like(0.9, 16000, 3).astype(np.float64)
    p_len = audio0.shape[0] // 160
    torch.manual_seed(2)
    pitchf = torch.where(torch.rand(1, p_len) > 0.3, 110 + 200 * torch.rand(1, p_len), torch.zeros(1, p_len))
    pitch = (pitchf / 4).long().clamp(1, 255)
    T = opipe.chunk_frames(audio0.shape[0])
    upp = int(np.prod(cfg[12]))
    nz, ns = opipe.chunk_noise(0, T, cfg[2], upp, 5)
    sid = torch.tensor([0])
    got = vc.vc(hub, net_g, sid.to(dev.device), audio0, pitch.to(dev.device), pitchf.to(dev.device), [0, 0, 0], None, None, 0,
                "v1", 0.33, noise=(nz, ns[0]))
    # oracle: the same steps with the reference's formulas
    wav = torch.from_numpy(audio0).float().view(1, -1)
    with torch.no_grad():
        feats = ohub.final_proj(nets["hubert_sd"], ohub.extract_features(nets["hubert_sd"], nets["hubert_cfg"], wav, 9))
    feats0 = feats.clone()
    feats = F.interpolate(feats.permute(0, 2, 1), scale_factor=2).permute(0, 2, 1)
    feats0 = F.interpolate(feats0.permute(0, 2, 1), scale_factor=2).permute(0, 2, 1)
    n = min(p_len, feats.shape[1])
    pf = pitchf[:, :n]
    w = pf.clone()
    w[pf > 0] = 1
    w[pf < 1] = 0.33
    w = w.unsqueeze(-1)
    feats = feats[:, :n] * w + feats0[:, :n] * (1 - w)
    with torch.no_grad():
        ro, _ = osynth.synth_infer(sd, cfg, feats, pitch[:, :n], pf, sid, nz[:, :, :n], ns[:, :n * upp])
    assert got.shape == (n * upp,)
    assert rel_rms(torch.from_numpy(got), ro[0, 0]) < 1e-4


def test_pipeline_without_f0_model(dev):
    """`_nono` voice models (if_f0 = 0, plain HiFi-GAN generator: models.py:754-955): no f0 branch, no protect blend."""
    from aicovergen_amd.infer_pack.models import SynthesizerTrnMs768NSFsid_nono
    nets = weights.small_model_set()
    cfg = list(nets["synth_cfg"])
    sd = weights.synth_state_dict(cfg, 41, f0=False)
    vc = VC(cfg[-1], _Cfg(dev.device))
    hub = HubertModel(nets["hubert_sd"], nets["hubert_cfg"]).to(dev.device)
    net_g = SynthesizerTrnMs768NSFsid_nono(*cfg)
    del net_g.enc_q
    net_g.load_state_dict(sd, strict=False)
    net_g.eval().to(dev.device)
    audio = vocal_like(1.0, 16000, 8)
    upp = int(np.prod(cfg[12]))

    def noise_fn(ci, s, e):
        nz, _ = opipe.chunk_noise(ci, opipe.chunk_frames(e - s), cfg[2], upp, 3)
        return nz, None

    outs = [vc.pipeline(hub, net_g, 0, audio, "x.wav", [0, 0, 0], 0, "rmvpe", "", 0.5, 0, 3, cfg[-1], 0, 1, "v2", 0.5, 128,
                        noise_fn=noise_fn) for _ in range(2)]
    assert outs[0].dtype == np.int16 and np.array_equal(outs[0], outs[1])
    assert abs(len(outs[0]) / cfg[-1] - 1.0) < 0.06 and np.abs(outs[0]).max() > 50
    assert not hasattr(vc, "model_rmvpe")     # the f0 estimator is never built for these models
