"""A whole cover in one call (aicovergen_amd.cover.CoverSession.song_cover_pipeline) against the file-by-file route it replaces, on
the miniature seeded models and directory layout of tests/test_reference_main.py: every file it leaves is compared byte for byte
with what mdx.run_mdx x3 / VC.pipeline / cover.add_audio_effects / cover.pitch_shift / cover.combine_audio write.

AI vocals: the stand-alone VC.pipeline call (same models, same noise_seed, input = ops.resample_poly_mono of the kept DeReverb file) is
first run twice.  Seen on the host emulator: the two runs are bit-identical, and so is the pipeline's file.  Should the stand-alone
call differ from itself (a device run whose reductions are not ordered), the test bounds the file by that measured self-distance
instead; the assertion message prints it."""
import filecmp
import json
import os
import shutil
import types

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import conftest
from aicovergen_amd import audio_io, cover, mdx, ops, rvc
from aicovergen_amd import hubert as hubert_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7
KW = dict(pitch_change_all=2, output_format="wav", noise_seed=SEED)
VOCALS = "song_Voice_p2_i0.5_fr3_rms0.25_pro0.33_rmvpe.wav"          # main.py:286 for pitch_change 0, -pall 2
STEMS = ["song_Instrumental.wav", "song_Vocals.wav", "song_Vocals_Backup.wav", "song_Vocals_Main.wav", "song_Vocals_Main_DeReverb.wav"]


@pytest.fixture(scope="module", params=[pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)])
def world(request, tmp_path_factory):
    """Model directories, a 3 s song, one session, and the keep_files=True run every comparison starts from."""
    from synthetic import weights
    from synthetic.inputs import song_like
    from test_onnx_weights import CFG
    conftest._bind(request.param)
    tmp = str(tmp_path_factory.mktemp("cover_" + request.param))
    saved = rvc._PRESET_HALF, torch.cuda.get_device_properties
    rvc._PRESET_HALF = (1, 1, 1, 2)             # several chunks in 3 s (the preset main.py's Config(device, True) selects)
    if request.param == "emu":                  # run_mdx asks for the card's memory, like the reference; the emulator host has no card
        torch.cuda.get_device_properties = lambda d=None: types.SimpleNamespace(total_memory=64 << 30, name="emulated")
    mdx_dir, rvc_dir, out_dir = (os.path.join(tmp, d) for d in ("mdxnet_models", "rvc_models", "song_output"))
    for d in (mdx_dir, os.path.join(rvc_dir, "Voice"), out_dir):
        os.makedirs(d)
    fixture = os.path.join(ROOT, "tests", "golden", "mdx_tiny.onnx")
    entry = {"mdx_dim_f_set": CFG["dim_f"], "mdx_dim_t_set": 4, "mdx_n_fft_scale_set": 2048, "primary_stem": "Vocals"}
    params = {}
    for i, name in enumerate(cover.MDX_MODEL_FILES):            # three files with distinct hashes: a doc_string field (ModelProto field 6) appended to the fixture
        path = os.path.join(mdx_dir, name)
        shutil.copy(fixture, path)
        with open(path, "ab") as f:
            f.write(b"\x32" + bytes([i + 1]) + b"m" * (i + 1))
        params[mdx.MDX.get_hash(path)] = dict(entry, compensate=(1.021, 1.035, 1.0)[i])
    assert len(params) == 3
    json.dump(params, open(os.path.join(mdx_dir, "model_data.json"), "w"))
    nets = weights.small_model_set()
    torch.save({"model": nets["hubert_sd"], "cfg": {}, "args": None}, os.path.join(rvc_dir, "hubert_base.pt"))
    # the miniature synthesizer with upsampling x80 instead of x16: 8 kHz output, the lowest rate the reverb's delay lines take
    cfg = list(nets["synth_cfg"])
    cfg[12], cfg[14], cfg[-1] = [10, 2, 2, 2], [20, 4, 4, 4], 8000
    synth_sd = weights.synth_state_dict(cfg, 1236)
    cfg[-3] = 109
    torch.save({"config": cfg, "weight": synth_sd, "f0": 1, "version": "v2", "info": "seeded"}, os.path.join(rvc_dir, "Voice", "voice.pth"))
    torch.save(nets["rmvpe_sd"], os.path.join(rvc_dir, "rmvpe.pt"))
    song = os.path.join(tmp, "song.wav")
    audio_io.write_wav_pcm16(song, (song_like(3.0, 44100, seed=9).astype(np.float32) * 0.6).T, 44100)
    session = cover.CoverSession(mdx_dir, rvc_dir, out_dir)
    w = types.SimpleNamespace(kind=request.param, tmp=tmp, mdx_dir=mdx_dir, rvc_dir=rvc_dir, out_dir=out_dir, params=params, song=song,
                              session=session, device=torch.device("cuda:0" if request.param == "hip" else "cpu"))
    w.cover = session.song_cover_pipeline(song, "Voice", 0, True, **KW)
    w.dir = os.path.dirname(w.cover)
    yield w
    rvc._PRESET_HALF, torch.cuda.get_device_properties = saved


def _chain(w, song, out):
    """main.py's preprocess_song through mdx.run_mdx: the five stem files."""
    os.makedirs(out, exist_ok=True)
    p = lambda name: os.path.join(w.mdx_dir, name)
    v, i = mdx.run_mdx(w.params, out, p(cover.MDX_MODEL_FILES[0]), song, denoise=True, keep_orig=True)
    b, m = mdx.run_mdx(w.params, out, p(cover.MDX_MODEL_FILES[1]), v, suffix="Backup", invert_suffix="Main", denoise=True)
    _, d = mdx.run_mdx(w.params, out, p(cover.MDX_MODEL_FILES[2]), m, invert_suffix="DeReverb", exclude_main=True, denoise=True)
    return v, i, b, m, d


def test_1_separation_stems_equal_three_chained_run_mdx(world):
    w = world
    assert os.path.basename(w.dir) == cover.get_hash(w.song) and w.cover == os.path.join(w.dir, "song (Voice Ver).wav")
    files = _chain(w, w.song, os.path.join(w.tmp, "direct"))
    assert sorted(os.path.basename(f) for f in files) == STEMS
    for f in files:
        assert filecmp.cmp(f, os.path.join(w.dir, os.path.basename(f)), shallow=False), f
    assert np.abs(wavfile.read(os.path.join(w.dir, STEMS[4]))[1]).max() > 30


def test_2_ai_vocals_equal_a_separate_pipeline_call(world):
    w = world
    cpt, version, net_g, tgt_sr, vc, index = w.session.voice("Voice")
    dereverb = os.path.join(w.dir, STEMS[4])
    sr, d = wavfile.read(dereverb)

    def separate():
        x = torch.from_numpy(np.ascontiguousarray(d.T.astype(np.float32) / 32768.0)).to(w.device)
        audio = ops.resample_poly_mono(x, 44100, 16000)
        return vc.pipeline(w.session.hubert, net_g, 0, audio, dereverb, [0, 0, 0], 2, "rmvpe", index, 0.5, cpt.get("f0", 1), 3, tgt_sr, 0,
                           0.25, version, 0.33, 128, noise_seed=SEED)
    a, b = separate(), separate()
    self_distance = int(np.abs(a.astype(np.int32) - b).max())
    path = os.path.join(w.dir, VOCALS)
    sr_out, got = wavfile.read(path)
    assert sr_out == tgt_sr and got.dtype == np.int16 and got.ndim == 1 and np.abs(got).max() > 100
    if self_distance == 0:
        direct = os.path.join(w.tmp, "direct_vocals.wav")
        wavfile.write(direct, tgt_sr, a)
        assert filecmp.cmp(path, direct, shallow=False)
    else:
        assert got.shape == a.shape and int(np.abs(got.astype(np.int32) - a).max()) <= self_distance, self_distance


def test_3_effects_pitch_shift_and_mix_equal_the_file_functions(world):
    w = world
    d2 = os.path.join(w.tmp, "post")
    os.makedirs(d2)
    names = [VOCALS, "song_Instrumental.wav", "song_Vocals_Backup.wav"]
    for n in names:
        shutil.copy(os.path.join(w.dir, n), d2)
    mixed = cover.add_audio_effects(os.path.join(d2, VOCALS), 0.15, 0.2, 0.8, 0.7)
    inst = cover.pitch_shift(os.path.join(d2, names[1]), 2)
    backup = cover.pitch_shift(os.path.join(d2, names[2]), 2)
    out = os.path.join(d2, "cover.wav")
    cover.combine_audio([mixed, backup, inst], out, 0, 0, 0, "wav")
    for f in (mixed, inst, backup):
        assert filecmp.cmp(f, os.path.join(w.dir, os.path.basename(f)), shallow=False), f
    assert os.path.basename(inst) == "song_Instrumental_p2.wav" and os.path.basename(mixed) == VOCALS[:-4] + "_mixed.wav"
    assert filecmp.cmp(out, w.cover, shallow=False)
    assert sorted(os.listdir(w.dir)) == sorted(STEMS + [VOCALS, VOCALS[:-4] + "_mixed.wav", "song_Instrumental_p2.wav",
                                                        "song_Vocals_Backup_p2.wav", "song (Voice Ver).wav"])


@pytest.fixture(scope="module")
def lean(world):
    """keep_files=False into a fresh output directory, through the same session."""
    w = world
    s = w.session
    s.output_dir = os.path.join(w.tmp, "lean_output")
    os.makedirs(s.output_dir)
    try:
        path = s.song_cover_pipeline(w.song, "Voice", 0, False, **KW)
        yield types.SimpleNamespace(cover=path, dir=os.path.dirname(path), output_dir=s.output_dir)
    finally:
        s.output_dir = w.out_dir


def test_4_files_left_behind(world, lean):
    left = ["song (Voice Ver).wav", "song_Instrumental.wav", VOCALS, "song_Vocals_Backup.wav", "song_Vocals_Main_DeReverb.wav"]
    assert sorted(os.listdir(lean.dir)) == sorted(left)
    for n in left:
        assert filecmp.cmp(os.path.join(lean.dir, n), os.path.join(world.dir, n), shallow=False), n


def test_5_cached_stems_are_reused(world, lean, monkeypatch):
    calls = []
    real = mdx.run_mdx_device
    monkeypatch.setattr(mdx, "run_mdx_device", lambda *a, **k: calls.append(a) or real(*a, **k))
    before = open(lean.cover, "rb").read()
    os.remove(lean.cover)
    os.remove(os.path.join(lean.dir, VOCALS))            # the conversion runs again, from the cached DeReverb file
    world.session.output_dir = lean.output_dir
    try:
        again = world.session.song_cover_pipeline(world.song, "Voice", 0, False, **KW)
    finally:
        world.session.output_dir = world.out_dir
    assert calls == [] and again == lean.cover and open(again, "rb").read() == before
    assert filecmp.cmp(os.path.join(lean.dir, VOCALS), os.path.join(world.dir, VOCALS), shallow=False)


def test_6_session_reuse_and_7_mono_input(world, monkeypatch):
    """A second song through the same session constructs no model; it is a mono file, whose stems equal run_mdx's on that file."""
    from synthetic.inputs import song_like
    w = world
    made = []
    for mod, name in ((mdx, "MDX"), (hubert_mod, "HubertModel"), (rvc, "get_vc"), (rvc, "load_hubert")):
        real = getattr(mod, name)
        monkeypatch.setattr(mod, name, lambda *a, _r=real, _n=name, **k: made.append(_n) or _r(*a, **k))
    mono = os.path.join(w.tmp, "mono.wav")
    wavfile.write(mono, 44100, np.rint(song_like(1.0, 44100, seed=4)[0] * 0.5 * 32767).astype(np.int16))
    path = w.session.song_cover_pipeline(mono, "Voice", 0, True, output_format="wav", noise_seed=SEED)
    assert made == []
    monkeypatch.undo()
    assert os.path.basename(path) == "mono (Voice Ver).wav" and wavfile.read(path)[1].shape[1] == 2
    for f in _chain(w, mono, os.path.join(w.tmp, "direct_mono")):
        assert filecmp.cmp(f, os.path.join(os.path.dirname(path), os.path.basename(f)), shallow=False), f


def test_7_naming_and_inputs(world, lean, monkeypatch):
    w = world
    # mangio-crepe carries its hop length in the AI-vocals name (main.py:286): a file of that name is found and used as it is
    crepe = os.path.join(lean.dir, "song_Voice_p2_i0.5_fr3_rms0.25_pro0.33_mangio-crepe_64.wav")
    shutil.copy(os.path.join(lean.dir, VOCALS), crepe)
    monkeypatch.setattr(w.session, "_convert", lambda *a, **k: pytest.fail("looked for another AI-vocals name"))
    w.session.output_dir = lean.output_dir
    try:
        out = w.session.song_cover_pipeline(w.song, "Voice", 0, False, f0_method="mangio-crepe", crepe_hop_length=64, **KW)
        os.rename(crepe, os.path.join(lean.dir, "song_Voice_p14_i0.5_fr3_rms0.25_pro0.33_rmvpe.wav"))       # 1 * 12 + 2, no suffix
        w.session.song_cover_pipeline(w.song, "Voice", 1, False, **KW)
    finally:
        w.session.output_dir = w.out_dir
    assert filecmp.cmp(out, w.cover, shallow=False)
    with pytest.raises(ValueError, match="download"):
        w.session.song_cover_pipeline("https://www.youtube.com/watch?v=abc", "Voice", 0, False)
    with pytest.raises(FileNotFoundError, match="nowhere.wav does not exist."):
        w.session.song_cover_pipeline(os.path.join(w.tmp, "nowhere.wav"), "Voice", 0, False)
    with pytest.raises(ValueError, match="Ensure that the song input field and voice model field is filled."):
        w.session.song_cover_pipeline("", "Voice", 0, False)
    os.makedirs(os.path.join(w.rvc_dir, "Empty"), exist_ok=True)
    with pytest.raises(FileNotFoundError, match="No model file exists in"):
        cover.get_rvc_model(w.rvc_dir, "Empty")


def test_8_command_line_has_main_pys_flags_and_defaults():
    import argparse
    p = argparse.ArgumentParser()                  # the flag list of src/main.py:321-339
    p.add_argument('-i', '--song-input', type=str, required=True)
    p.add_argument('-dir', '--rvc-dirname', type=str, required=True)
    p.add_argument('-p', '--pitch-change', type=int, required=True)
    p.add_argument('-k', '--keep-files', action=argparse.BooleanOptionalAction)
    p.add_argument('-ir', '--index-rate', type=float, default=0.5)
    p.add_argument('-fr', '--filter-radius', type=int, default=3)
    p.add_argument('-rms', '--rms-mix-rate', type=float, default=0.25)
    p.add_argument('-palgo', '--pitch-detection-algo', type=str, default='rmvpe')
    p.add_argument('-hop', '--crepe-hop-length', type=int, default=128)
    p.add_argument('-pro', '--protect', type=float, default=0.33)
    p.add_argument('-mv', '--main-vol', type=int, default=0)
    p.add_argument('-bv', '--backup-vol', type=int, default=0)
    p.add_argument('-iv', '--inst-vol', type=int, default=0)
    p.add_argument('-pall', '--pitch-change-all', type=int, default=0)
    p.add_argument('-rsize', '--reverb-size', type=float, default=0.15)
    p.add_argument('-rwet', '--reverb-wetness', type=float, default=0.2)
    p.add_argument('-rdry', '--reverb-dryness', type=float, default=0.8)
    p.add_argument('-rdamp', '--reverb-damping', type=float, default=0.7)
    p.add_argument('-oformat', '--output-format', type=str, default='mp3')
    ours = cover.build_parser()
    for argv in (["-i", "a.wav", "-dir", "Voice", "-p", "1"],
                 ["-i", "a.wav", "-dir", "V", "-p", "-1", "-k", "-ir", "0.7", "-fr", "5", "-rms", "0.5", "-palgo", "mangio-crepe", "-hop", "64",
                  "-pro", "0.5", "-mv", "1", "-bv", "-2", "-iv", "3", "-pall", "2", "-rsize", "0.3", "-rwet", "0.1", "-rdry", "0.9", "-rdamp",
                  "0.2", "-oformat", "wav"],
                 ["--song-input", "b.wav", "--rvc-dirname", "V", "--pitch-change", "0", "--no-keep-files", "--output-format", "wav"]):
        want, got = vars(p.parse_args(argv)), vars(ours.parse_args(argv))
        extra = {k: got.pop(k) for k in ("mdx_models_dir", "rvc_models_dir", "output_dir")}
        assert got == want and all(extra.values())
    got = ours.parse_args(["-i", "a", "-dir", "V", "-p", "0", "--mdx-models-dir", "/m", "--rvc-models-dir", "/r", "--output-dir", "/o"])
    assert (got.mdx_models_dir, got.rvc_models_dir, got.output_dir) == ("/m", "/r", "/o")
    with pytest.raises(SystemExit):
        ours.parse_args(["-i", "a.wav"])
