"""f0_method "pm": Praat's autocorrelation pitch on the device (csrc/pitch_ac.hip) against its float64 restatement
(tests/praat_ac_ref.py), from the geometry call up to VC.pipeline.  Tolerances are measured here, on the restatement alone: its float32
run against its float64 run (same operands, another rounding), with the margin 4 of tests/test_resample_mc.py."""
import ctypes

import numpy as np
import pytest
import torch

import praat_ac_ref as R
from aicovergen_amd import _lib, ops

SR = 16000
TONES = (55.0, 110.0, 220.0, 441.3, 880.0, 1050.0)
# |f_ref64 - f0| / f0 the restatement reaches on the clean tones: 2.6e-4 at 55 Hz (three periods of the floor in the window), below
# 2e-6 from 110 Hz up.  The parabola alone stands at 1.9e-3.
REF_REL_BOUND = 3.0e-4
_cache = {}


def tone(f0, n=8000):
    t = np.arange(n) / SR
    return (0.3 * sum(np.sin(2 * np.pi * f0 * h * t + h) / h for h in range(1, 6) if f0 * h < 7000)).astype(np.float32)


def tone_refs():
    """{f0: (x, f_ref64, f_ref32)} and d32, the largest distance between the two runs over the six signals"""
    if "tones" not in _cache:
        refs = {f0: (tone(f0), R.pitch_ac(tone(f0)), R.pitch_ac(tone(f0), dtype=np.float32)) for f0 in TONES}
        _cache["tones"] = refs, max(float(np.abs(a - b).max()) for _, a, b in refs.values())
    return _cache["tones"]


def vocal(seed=3, seconds=3.0):
    """A glide 110 -> 330 Hz with vibrato, a noise burst at 1.2 .. 1.4 s and a near-silent gap at 2.0 .. 2.3 s."""
    rng = np.random.default_rng(seed)
    n = int(seconds * SR)
    t = np.arange(n) / SR
    f = 110.0 * 3.0 ** (t / seconds) * (1.0 + 0.02 * np.sin(2 * np.pi * 5.5 * t))
    ph = 2 * np.pi * np.cumsum(f) / SR
    x = sum(np.sin(h * ph + h) / h for h in range(1, 7)) * 0.25 + 0.003 * rng.standard_normal(n)
    b0, b1 = int(1.2 * SR), int(1.4 * SR)
    x[b0:b1] = 0.2 * rng.standard_normal(b1 - b0)
    x[int(2.0 * SR):int(2.3 * SR)] *= 0.001
    return x.astype(np.float32)


def vocal_refs():
    if "vocal" not in _cache:
        x = vocal()
        _cache["vocal"] = x, R.pitch_ac(x, full=True), R.pitch_ac(x, dtype=np.float32, full=True)
    return _cache["vocal"]


# ---- 1. geometry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [960, 961, 1119, 1120, 8000, 3840000])
def test_geometry(dev, n):
    g = R.geometry(n)
    got = ops.pitch_ac_geometry(SR, n)
    assert got[:6] == (g["nw"], g["nfft"], g["maxlag"], g["brent"], g["n_frames"], int(np.floor(g["t1s"])))
    assert got[:4] == (958, 2048, 321, 479)
    assert got[4] == {960: 1, 961: 1, 1119: 1, 1120: 2, 8000: 45, 3840000: 23995}[n]
    if n == 8000:
        assert got[5] == 480 and R.frame_start(g, 0) == 1
    assert R.frame_start(g, 0) >= 0 and R.frame_start(g, g["n_frames"] - 1) + g["nw"] <= n
    assert got[7] >= got[4] * 16


@pytest.mark.parametrize("n", [960, 8000, 8001, 12345])
def test_frame_times(dev, n):
    g = R.geometry(n)
    t = ops.pitch_ac_frame_times(SR, n)
    assert np.array_equal(t, R.frame_times(g))
    assert t[0] * SR == n / 2 - (len(t) - 1) * 80 and (len(t) == 1 or np.allclose(np.diff(t), 0.01, rtol=0, atol=1e-12))


def test_geometry_short_signal_is_an_error(dev):
    with pytest.raises(ValueError):
        R.geometry(959)
    with pytest.raises(ValueError):
        ops.pitch_ac_geometry(SR, 959)
    with pytest.raises(ValueError):
        ops.pitch_ac(dev.t(torch.zeros(959)))
    g = (ctypes.c_int64 * 8)()
    assert _lib.get().aicg_pitch_ac_geometry(SR, 959, 0.01, 50.0, 1100.0, ctypes.addressof(g)) == -1   # AICG_E_SHAPE


# ---- 2. known pitch ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f0", TONES)
def test_known_pitch(dev, f0):
    refs, d32 = tone_refs()
    x, r64, _ = refs[f0]
    got = ops.pitch_ac(dev.t(torch.from_numpy(x))).cpu().numpy()
    dist = float(np.abs(got - r64).max())
    print("f0 %g: |dev - ref64| %.3g Hz, d32 %.3g Hz, |ref64 - f0| / f0 %.3g" % (f0, dist, d32, np.abs(r64 - f0).max() / f0))
    assert got.shape == (45,) and got.dtype == np.float64
    assert (got > 0).all()
    assert dist <= 4 * d32


@pytest.mark.parametrize("f0", TONES)
def test_restatement_finds_the_known_pitch(f0):
    r64 = tone_refs()[0][f0][1]
    assert (r64 > 0).all()
    assert np.abs(r64 - f0).max() / f0 < REF_REL_BOUND


# ---- 3. unvoiced and silence -------------------------------------------------------------------------------------------------------
def test_noise_is_unvoiced(dev):
    x = (0.1 * np.random.default_rng(0).standard_normal(8000)).astype(np.float32)
    got = ops.pitch_ac(dev.t(torch.from_numpy(x))).cpu().numpy()
    assert got.shape == (45,) and (got == 0).all()
    assert (R.pitch_ac(x) == 0).all()


def test_silent_half_is_unvoiced(dev):
    x = (0.3 * np.sin(2 * np.pi * 220 * np.arange(8000) / SR)).astype(np.float32)
    x[4000:] *= 0.001
    got = ops.pitch_ac(dev.t(torch.from_numpy(x))).cpu().numpy()
    ref = R.pitch_ac(x)
    assert (got[:18] > 0).all() and (got[30:] == 0).all()
    assert (ref[:18] > 0).all() and (ref[30:] == 0).all()
    assert np.abs(got[:18] - 220).max() < 0.5


# ---- 4. the path finder alone ------------------------------------------------------------------------------------------------------
def random_table(n_frames, per_frame, seed):
    rng = np.random.default_rng(seed)
    cand = np.zeros((n_frames, 15, 2), np.float32)
    cand[:, :, 0] = rng.uniform(40.0, 1300.0, (n_frames, 15))
    cand[:, :, 1] = rng.uniform(0.0, 1.0, (n_frames, 15))
    cand[:, 0, 0] = 0.0                        # candidate 0 is the unvoiced one
    count = rng.integers(1, 16, n_frames).astype(np.int32) if per_frame == "mixed" else np.full(n_frames, per_frame, np.int32)
    return cand, count


@pytest.mark.parametrize("per_frame", [1, 2, 15, "mixed"])
@pytest.mark.parametrize("n_frames", [1, 2, 63, 64, 65, 1000])
def test_path_equals_the_restatement(dev, n_frames, per_frame):
    for seed in range(20):                      # redraw until no decision of the restatement is closer than 1e-9
        cand, count = random_table(n_frames, per_frame, 1000 * seed + n_frames)
        f0, states, pmargin, _ = R.path(cand, count, want_margins=True)
        if pmargin > 1e-9:
            break
    assert pmargin > 1e-9
    got, st = ops.pitch_ac_path(dev.t(torch.from_numpy(cand)), dev.t(torch.from_numpy(count)), return_states=True)
    assert np.array_equal(st.cpu().numpy(), states)
    assert np.array_equal(got.cpu().numpy(), f0)
    if per_frame == 15 and n_frames >= 63:
        assert (f0 >= 1100).any() or (f0 == 0).any()


def test_path_ties_go_to_the_lowest_index(dev):
    cand = np.zeros((40, 15, 2), np.float32)
    cand[:, 0] = (0.0, 0.1)
    cand[:, 1] = (200.0, 0.9)
    cand[:, 2] = (200.0, 0.9)
    count = np.full(40, 3, np.int32)
    _, st = ops.pitch_ac_path(dev.t(torch.from_numpy(cand)), dev.t(torch.from_numpy(count)), return_states=True)
    assert (st.cpu().numpy() == 1).all()
    assert (R.path(cand, count)[1] == 1).all()


def test_path_stays_on_the_octave(dev):
    """Frames 20 .. 24 of 64 prefer the octave below by 0.05 per frame; going there and back costs 2 x 0.35 octave-jump cost, more than
    the 5 x 0.05 to be gained: the path stays on 220 Hz, frame-wise argmax would not."""
    cand = np.zeros((64, 15, 2), np.float32)
    cand[:, 0] = (0.0, 0.3)
    cand[:, 1] = (220.0, 0.90)
    cand[:, 2] = (110.0, 0.80)
    cand[20:25, 2, 1] = 0.95 + 0.01    # octave cost: log2(1100 / 110) - log2(1100 / 220) = 1 -> 0.01 less for the lower octave
    count = np.full(64, 3, np.int32)
    node = cand[:, 1:3, 1] - 0.01 * np.log2(1100.0 / cand[:, 1:3, 0])
    assert (np.argmax(node[20:25], axis=1) == 1).all() and 5 * (node[20:25, 1] - node[20:25, 0]).max() < 2 * 0.35
    got = ops.pitch_ac_path(dev.t(torch.from_numpy(cand)), dev.t(torch.from_numpy(count))).cpu().numpy()
    assert (got == 220.0).all()
    assert (R.path(cand, count)[0] == 220.0).all()


# ---- 5. candidates end to end ------------------------------------------------------------------------------------------------------
def _decisions(f):
    return f > 0


def vocal_margins():
    """(excluded frames, d32 on the rest): frames whose margin in the float64 run is below m = 4 x the largest change of the margin
    between the float32 and the float64 run."""
    x, (c64, n64, f64, s64, _, fm64), (c32, n32, f32, s32, _, fm32) = vocal_refs()
    both = np.isfinite(fm64) & np.isfinite(fm32)
    m = 4 * float(np.abs(fm64[both] - fm32[both]).max())
    excluded = fm64 < m
    keep = ~excluded & (f64 > 0) & (f32 > 0)
    return excluded, float(np.abs(f64 - f32)[keep].max()), m


def test_restatement_float32_run_stays_inside_the_cap():
    x, r64, r32 = vocal_refs()
    excluded, d32, m = vocal_margins()
    f64, f32 = r64[2], r32[2]
    print("vocal: %d frames, margin bar m %.3g, excluded %d, d32 %.3g Hz, voiced %d" % (len(f64), m, excluded.sum(), d32, (f64 > 0).sum()))
    assert excluded.mean() <= 0.02
    ok = ~excluded
    assert np.array_equal(_decisions(f64)[ok], _decisions(f32)[ok])
    assert 100 < (f64 > 0).sum() < len(f64) - 30          # voiced stretches, the burst and the gap


def test_candidates_end_to_end(dev):
    x, r64, _ = vocal_refs()
    excluded, d32, m = vocal_margins()
    f64 = r64[2]
    xd = dev.t(torch.from_numpy(x))
    got, cand, count = ops.pitch_ac(xd, return_candidates=True)
    again, cand2, count2 = ops.pitch_ac(xd, return_candidates=True)
    assert torch.equal(got, again) and torch.equal(cand, cand2) and torch.equal(count, count2)     # bit-identical
    got = got.cpu().numpy()
    ok = ~excluded
    assert np.array_equal(_decisions(got)[ok], _decisions(f64)[ok])
    v = ok & (f64 > 0)
    print("vocal: |dev - ref64| %.3g Hz on %d voiced frames, d32 %.3g Hz, %d excluded" % (np.abs(got - f64)[v].max(), v.sum(), d32, excluded.sum()))
    assert (np.abs(np.log2(got[v] / f64[v])) < 0.5).all()
    assert np.abs(got - f64)[v].max() <= 4 * d32
    cnt = count.cpu().numpy()
    assert cand.shape == (len(f64), 15, 2) and (cnt >= 1).all() and (cnt <= 15).all()
    assert (cand.cpu().numpy()[:, 0, 0] == 0).all()


# ---- 6. get_f0 and the pipeline ------------------------------------------------------------------------------------------------------
def _vc_without_f0_models(dev, nets, x):
    """tests/test_pipeline.py's VC without the seeded RMVPE it injects, and with nowhere to load one from."""
    import test_pipeline as tp
    vc = tp.build(dev, nets, x)[0]
    del vc.model_rmvpe
    vc.rmvpe_path = "/nonexistent/rmvpe.pt"
    return vc


def test_get_f0_pads_like_the_reference(dev):
    from synthetic import weights
    vc = _vc_without_f0_models(dev, weights.small_model_set(1234), (1, 1, 1, 2))
    x = tone(220.0)
    coarse, f0 = vc.get_f0("x", x, 50, 2, "pm", 3, 128)
    assert coarse.shape == (50,) and f0.shape == (50,)
    assert (f0[:3] == 0).all() and (f0[-2:] == 0).all() and (f0[3:-2] > 0).all()
    raw = ops.pitch_ac(dev.t(torch.from_numpy(x))).cpu().numpy()
    assert np.allclose(f0[3:-2], raw * 2 ** (2 / 12), rtol=1e-12, atol=0)
    assert not hasattr(vc, "model_rmvpe") and not hasattr(vc, "model_crepe")


def test_pipeline_pm_runs_without_f0_weights_and_shares_its_front(dev):
    import test_voice_front as tvf
    c = tvf.ctx(dev)
    vc = _vc_without_f0_models(dev, c.nets, tvf.GEOMETRY[dev.kind][0])
    plain = tvf.convert(c, f0_method="pm", vc=vc)
    assert plain.dtype == np.int16 and len(plain) > 0 and np.abs(plain.astype(np.int64)).max() > 0
    assert not hasattr(vc, "model_rmvpe") and not hasattr(vc, "model_crepe")
    front = tvf.make_front(c, f0_method="pm", vc=vc)
    assert front.f0 is not None and front.schedule == "serial"
    shared = tvf.convert(c, front=front, f0_method="pm", vc=vc)
    assert np.array_equal(plain, shared)
    with pytest.raises(ValueError):
        tvf.convert(c, front=front, f0_method="rmvpe", vc=vc)
    assert not hasattr(vc, "model_rmvpe") and not hasattr(vc, "model_crepe")


# ---- 7. a whole cover ------------------------------------------------------------------------------------------------------------------
def test_cover_with_pm_needs_no_rmvpe_file(dev, tmp_path, monkeypatch):
    """tests/test_cover_pipeline.py's miniature models and 3 s song, in a models directory WITHOUT rmvpe.pt."""
    import glob
    import json
    import os
    import shutil
    import types
    from scipy.io import wavfile
    import test_cover_pipeline as tcp
    from aicovergen_amd import audio_io, cover, mdx, rvc
    from aicovergen_amd.vc_infer_pipeline import VC
    from synthetic import weights
    from synthetic.inputs import song_like
    from test_onnx_weights import CFG
    monkeypatch.setattr(rvc, "_PRESET_HALF", (1, 1, 1, 2))
    if dev.kind == "emu":
        monkeypatch.setattr(torch.cuda, "get_device_properties", lambda d=None: types.SimpleNamespace(total_memory=64 << 30, name="emulated"))

    def no_rmvpe():
        raise AssertionError("f0_method pm resolved rmvpe.pt")
    monkeypatch.setattr(VC, "_default_rmvpe_path", staticmethod(no_rmvpe))
    tmp = str(tmp_path)
    mdx_dir, rvc_dir, out_dir = (os.path.join(tmp, d) for d in ("mdxnet_models", "rvc_models", "song_output"))
    for d in (mdx_dir, os.path.join(rvc_dir, "Voice"), out_dir):
        os.makedirs(d)
    entry = {"mdx_dim_f_set": CFG["dim_f"], "mdx_dim_t_set": 4, "mdx_n_fft_scale_set": 2048, "primary_stem": "Vocals"}
    params = {}
    for i, name in enumerate(cover.MDX_MODEL_FILES):
        path = os.path.join(mdx_dir, name)
        shutil.copy(os.path.join(tcp.ROOT, "tests", "golden", "mdx_tiny.onnx"), path)
        with open(path, "ab") as f:
            f.write(b"\x32" + bytes([i + 1]) + b"m" * (i + 1))
        params[mdx.MDX.get_hash(path)] = dict(entry, compensate=(1.021, 1.035, 1.0)[i])
    json.dump(params, open(os.path.join(mdx_dir, "model_data.json"), "w"))
    nets = weights.small_model_set()
    torch.save({"model": nets["hubert_sd"], "cfg": {}, "args": None}, os.path.join(rvc_dir, "hubert_base.pt"))
    cfg = list(nets["synth_cfg"])
    cfg[12], cfg[14], cfg[-1] = [10, 2, 2, 2], [20, 4, 4, 4], 8000
    synth_sd = weights.synth_state_dict(cfg, 1236)
    cfg[-3] = 109
    torch.save({"config": cfg, "weight": synth_sd, "f0": 1, "version": "v2", "info": "seeded"}, os.path.join(rvc_dir, "Voice", "voice.pth"))
    assert not os.path.exists(os.path.join(rvc_dir, "rmvpe.pt"))
    song = os.path.join(tmp, "song.wav")
    audio_io.write_wav_pcm16(song, (song_like(3.0, 44100, seed=9).astype(np.float32) * 0.6).T, 44100)
    session = cover.CoverSession(mdx_dir, rvc_dir, out_dir)
    out = session.song_cover_pipeline(song, "Voice", 0, True, f0_method="pm", output_format="wav", noise_seed=tcp.SEED)
    assert os.path.exists(out)
    d = os.path.dirname(out)
    vocals = [f for f in glob.glob(os.path.join(d, "song_Voice_*.wav")) if not f.endswith("_mixed.wav")]     # (the effects chain's file)
    assert len(vocals) == 1 and vocals[0].endswith("_pro0.33_pm.wav"), vocals
    cpt, version, net_g, tgt_sr, vc, index = session.voice("Voice")
    assert not hasattr(vc, "model_rmvpe") and not hasattr(vc, "model_crepe")
    dereverb = os.path.join(d, tcp.STEMS[4])
    _, stem = wavfile.read(dereverb)
    x = torch.from_numpy(np.ascontiguousarray(stem.T.astype(np.float32) / 32768.0)).to(dev.device)
    alone = vc.pipeline(session.hubert, net_g, 0, ops.resample_poly_mono(x, 44100, 16000), dereverb, [0, 0, 0], 0, "pm", index, 0.5,
                        cpt.get("f0", 1), 3, tgt_sr, 0, 0.25, version, 0.33, 128, noise_seed=tcp.SEED)
    sr_out, got = wavfile.read(vocals[0])
    assert sr_out == tgt_sr and got.dtype == np.int16 and np.abs(got).max() > 100
    assert np.array_equal(got, alone)


# ---- 8. two ranks --------------------------------------------------------------------------------------------------------------------
def _pm_pipeline(group=None, spy=None):
    import conftest
    import test_pipeline as tp
    from synthetic import weights
    from synthetic.inputs import vocal_like
    nets = weights.small_model_set(1234)
    vc, hub, net_g, tgt_sr = tp.build(conftest.Dev("emu"), nets)
    del vc.model_rmvpe
    if spy is not None:
        spy(vc)
    return vc.pipeline(hub, net_g, 0, vocal_like(2.6, 16000, 1239), "x.wav", [0, 0, 0], 0, "pm", "", 0.5, 1, 3, tgt_sr, 0, 0.25, "v2", 0.33,
                       128, noise_fn=tp.noise_fn_for(nets), group=group)


def _pm_worker(rank, world, port, q):
    import os
    import torch.distributed as td
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), AICG_EMU_THREADS="2")
    torch.set_num_threads(2)
    import conftest
    conftest._bind("emu")
    td.init_process_group("gloo", rank=rank, world_size=world)
    try:
        inside, calls, total = [False], [], [0]
        names = [n for n in ("all_gather", "all_gather_into_tensor", "all_reduce", "broadcast", "barrier", "send", "recv", "isend", "irecv",
                             "all_to_all", "gather", "scatter", "reduce", "all_gather_object", "broadcast_object_list") if hasattr(td, n)]
        for n in names:
            def wrap(fn, n=n):
                def f(*a, **k):
                    total[0] += 1
                    if inside[0]:
                        calls.append(n)
                    return fn(*a, **k)
                return f
            setattr(td, n, wrap(getattr(td, n)))

        def spy(vc):
            est = vc._estimate_f0

            def estimate(*a, **k):
                inside[0] = True
                try:
                    return est(*a, **k)
                finally:
                    inside[0] = False
            vc._estimate_f0 = estimate
        out = _pm_pipeline(spy=spy)
        q.put((rank, out, calls, total[0]))
    finally:
        td.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_give_the_one_rank_bytes_without_f0_collectives():
    import os
    import conftest
    import torch.multiprocessing as mp
    conftest._bind("emu")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + ((os.getpid() + 137) % 500)
    procs = [ctx.Process(target=_pm_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    ref = _pm_pipeline()
    got = [q.get(timeout=500) for _ in range(2)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, out, calls, total in got:
        assert calls == [], (rank, calls)
        assert total > 0                       # the chunks were shared out and joined: the spy sees the job's collectives
    assert np.array_equal(dict((g[0], g[1]) for g in got)[0], ref)


# ---- 9. the pin against Praat itself -------------------------------------------------------------------------------------------------
def test_parselmouth_pin(dev):
    parselmouth = pytest.importorskip("parselmouth")

    def praat(x):
        return parselmouth.Sound(x.astype(np.float64), SR).to_pitch_ac(time_step=0.01, voicing_threshold=0.6, pitch_floor=50, pitch_ceiling=1100)

    for f0 in TONES:
        x = tone(f0)
        p = praat(x)
        g = R.geometry(len(x))
        assert p.get_number_of_frames() == g["n_frames"]
        assert np.allclose(p.xs(), ops.pitch_ac_frame_times(SR, len(x)), rtol=0, atol=1e-12)
        got = ops.pitch_ac(dev.t(torch.from_numpy(x))).cpu().numpy()
        assert np.array_equal(got > 0, p.selected_array["frequency"] > 0)
        nf = p.get_number_of_frames()           # the padded length get_f0 builds from Praat's own frame count (reference :290-294)
        pad = (50 - nf + 1) // 2
        assert len(got) + pad + (50 - nf - pad) == 50 and (pad, 50 - nf - pad) == (3, 2)
    x = vocal()
    got = ops.pitch_ac(dev.t(torch.from_numpy(x))).cpu().numpy()
    ref = praat(x).selected_array["frequency"]
    assert len(got) == len(ref)
    both = (got > 0) & (ref > 0)
    print("vocal against Praat: largest distance %.4g Hz on %d frames voiced in both, %d voicing differences"
          % (np.abs(got - ref)[both].max(), both.sum(), ((got > 0) != (ref > 0)).sum()))
