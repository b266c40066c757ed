"""One song, many voices (CoverSession's song cache, CoverSession.song_covers, the repeated `-dir` flag), on the miniature models and the
models-on-disk layout of tests/test_cover_pipeline.py.  The reference of every comparison is what this session type wrote before it
kept anything between calls: one song_cover_pipeline call per cover with the song cache switched off (AICG_SONG_CACHE=0), byte for byte.

Three voice directories: Voice, Other (another seeded synthesizer) and Again -- a copy of Voice's model, which stands for "the first
voice again at another pitch": the first directory itself cannot appear twice, both entries would write 'song (Voice Ver).wav'
(that is test_10)."""
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
from aicovergen_amd.vc_infer_pipeline import VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(pitch_change_all=2, output_format="wav")
VOICES = [dict(voice_model="Voice", pitch_change=0, noise_seed=7), dict(voice_model="Other", pitch_change=0, noise_seed=8),
          dict(voice_model="Again", pitch_change=-1, noise_seed=9, protect=0.5, index_rate=0.25)]


class Counters:
    """Call counts of what a cache hit must not do again."""

    def __init__(self, monkeypatch):
        self.n = {}
        for obj, name in ((mdx, "run_mdx_device"), (cover, "read_pcm16"), (ops, "resample_poly_mono"), (VC, "front"),
                          (cover, "pitch_shift_signal")):
            real = getattr(obj, name)
            self.n[name] = 0
            monkeypatch.setattr(obj, name, lambda *a, _r=real, _n=name, **k: self._count(_n) or _r(*a, **k))

    def _count(self, name):
        self.n[name] += 1

    def reset(self):
        for k in self.n:
            self.n[k] = 0


@pytest.fixture(scope="module", params=[pytest.param("emu"), pytest.param("hip", marks=pytest.mark.gpu)])
def world(request, tmp_path_factory):
    from synthetic import weights
    from synthetic.inputs import song_like
    from test_onnx_weights import CFG
    conftest._bind(request.param)
    tmp = str(tmp_path_factory.mktemp("voices_" + request.param))
    saved = rvc._PRESET_HALF, torch.cuda.get_device_properties, os.environ.get("AICG_SONG_CACHE")
    rvc._PRESET_HALF = (1, 1, 1, 2)
    if request.param == "emu":
        torch.cuda.get_device_properties = lambda d=None: types.SimpleNamespace(total_memory=64 << 30, name="emulated")
    mdx_dir, rvc_dir = os.path.join(tmp, "mdxnet_models"), os.path.join(tmp, "rvc_models")
    for d in (mdx_dir, os.path.join(rvc_dir, "Voice"), os.path.join(rvc_dir, "Other")):
        os.makedirs(d)
    fixture = os.path.join(ROOT, "tests", "golden", "mdx_tiny.onnx")
    entry = {"mdx_dim_f_set": CFG["dim_f"], "mdx_dim_t_set": 4, "mdx_n_fft_scale_set": 2048, "primary_stem": "Vocals"}
    params = {}
    for i, name in enumerate(cover.MDX_MODEL_FILES):
        path = os.path.join(mdx_dir, name)
        shutil.copy(fixture, path)
        with open(path, "ab") as f:
            f.write(b"\x32" + bytes([i + 1]) + b"m" * (i + 1))
        params[mdx.MDX.get_hash(path)] = dict(entry, compensate=(1.021, 1.035, 1.0)[i])
    json.dump(params, open(os.path.join(mdx_dir, "model_data.json"), "w"))
    nets = weights.small_model_set()
    torch.save({"model": nets["hubert_sd"], "cfg": {}, "args": None}, os.path.join(rvc_dir, "hubert_base.pt"))
    cfg = list(nets["synth_cfg"])
    cfg[12], cfg[14], cfg[-1] = [10, 2, 2, 2], [20, 4, 4, 4], 8000           # 8 kHz output: the lowest rate the reverb's delay lines take
    for name, seed in (("Voice", 1236), ("Other", 1301)):
        sd = weights.synth_state_dict(cfg, seed)
        torch.save({"config": cfg[:-3] + [109] + cfg[-2:], "weight": sd, "f0": 1, "version": "v2", "info": "seeded"},
                   os.path.join(rvc_dir, name, name.lower() + ".pth"))
    shutil.copytree(os.path.join(rvc_dir, "Voice"), os.path.join(rvc_dir, "Again"))
    torch.save(nets["rmvpe_sd"], os.path.join(rvc_dir, "rmvpe.pt"))
    song = os.path.join(tmp, "song.wav")
    audio_io.write_wav_pcm16(song, (song_like(2.4, 44100, seed=9).astype(np.float32) * 0.6).T, 44100)
    other_song = os.path.join(tmp, "other.wav")
    audio_io.write_wav_pcm16(other_song, (song_like(1.0, 44100, seed=4).astype(np.float32) * 0.5).T, 44100)

    def fresh(name):
        out = os.path.join(tmp, name)
        os.makedirs(out)
        return cover.CoverSession(mdx_dir, rvc_dir, out)
    w = types.SimpleNamespace(kind=request.param, tmp=tmp, mdx_dir=mdx_dir, rvc_dir=rvc_dir, song=song, other_song=other_song, fresh=fresh)
    # the reference: one call per cover, nothing kept between them
    os.environ["AICG_SONG_CACHE"] = "0"
    ref = fresh("ref_output")
    w.ref = [ref.song_cover_pipeline(song, v["voice_model"], v["pitch_change"], False,
                                     **dict(KW, **{k: x for k, x in v.items() if k not in ("voice_model", "pitch_change")})) for v in VOICES]
    assert ref.song is None
    os.environ.pop("AICG_SONG_CACHE")
    w.ref_dir = os.path.dirname(w.ref[0])
    yield w
    rvc._PRESET_HALF, torch.cuda.get_device_properties = saved[:2]
    if saved[2] is not None:
        os.environ["AICG_SONG_CACHE"] = saved[2]


def same_files(a_dir, b_dir):
    names = sorted(os.listdir(a_dir))
    assert names == sorted(os.listdir(b_dir))
    for n in names:
        assert filecmp.cmp(os.path.join(a_dir, n), os.path.join(b_dir, n), shallow=False), n
    return names


def test_06_song_covers_leaves_the_files_of_one_call_per_cover(world, monkeypatch):
    w = world
    count = Counters(monkeypatch)
    s = w.fresh("multi_output")
    covers = s.song_covers(w.song, VOICES, keep_files=False, **KW)
    assert [os.path.basename(p) for p in covers] == ["song (Voice Ver).wav", "song (Other Ver).wav", "song (Again Ver).wav"]
    assert [os.path.basename(p) for p in covers] == [os.path.basename(p) for p in w.ref]
    names = same_files(os.path.dirname(covers[0]), w.ref_dir)
    assert len(names) == 3 + 3 + 3 and np.abs(wavfile.read(covers[2])[1]).max() > 100
    assert not filecmp.cmp(covers[0], covers[1], shallow=False) and not filecmp.cmp(covers[0], covers[2], shallow=False)
    # queued once: three separation passes, one hand-over, one front, one shift of the two backing stems
    assert count.n == {"run_mdx_device": 3, "read_pcm16": 0, "resample_poly_mono": 1, "front": 1, "pitch_shift_signal": 2}
    assert s.song is not None and s.song.id == cover.get_hash(w.song) and list(s.song.shifted) == [2] and len(s.song.fronts) == 1
    assert s.song.nbytes() > 0


def test_07_cache_hit_and_08_keep_files_and_09_eviction(world, monkeypatch):
    w = world
    s = w.fresh("hit_output")
    v0, v1 = VOICES[0], VOICES[1]
    first = s.song_cover_pipeline(w.song, "Voice", 0, False, noise_seed=v0["noise_seed"], **KW)
    assert filecmp.cmp(first, w.ref[0], shallow=False)
    count = Counters(monkeypatch)
    second = s.song_cover_pipeline(w.song, "Other", 0, False, noise_seed=v1["noise_seed"], **KW)
    assert all(v == 0 for v in count.n.values()), count.n                      # 7: nothing voice-independent runs or is read again
    assert filecmp.cmp(second, w.ref[1], shallow=False)
    vocals = [n for n in os.listdir(w.ref_dir) if "_Other_p2_" in n]
    assert len(vocals) == 1 and filecmp.cmp(os.path.join(os.path.dirname(second), vocals[0]), os.path.join(w.ref_dir, vocals[0]), shallow=False)
    assert list(s.song.fronts) == [("rmvpe", 128, 3, 1, "v2")]
    # 8: keep_files separates again, as main.py does
    count.reset()
    kept = s.song_cover_pipeline(w.song, "Other", 0, True, noise_seed=v1["noise_seed"], **KW)
    assert count.n["run_mdx_device"] == 3 and kept == second and filecmp.cmp(kept, w.ref[1], shallow=False)
    # 9: another song evicts; drop_song() empties
    count.reset()
    song_id = s.song.id
    s.song_cover_pipeline(w.other_song, "Voice", 0, False, noise_seed=1, output_format="wav")
    assert s.song.id == cover.get_hash(w.other_song) != song_id and count.n["run_mdx_device"] == 3 and count.n["front"] == 1
    count.reset()
    again = s.song_cover_pipeline(w.song, "Voice", 0, False, noise_seed=v0["noise_seed"], **KW)     # stems and AI vocals are files by now
    assert count.n["run_mdx_device"] == 0 and count.n["read_pcm16"] >= 3 and s.song.id == song_id
    assert filecmp.cmp(again, w.ref[0], shallow=False)
    s.drop_song()
    assert s.song is None
    count.reset()
    s.song_cover_pipeline(w.song, "Voice", 0, False, noise_seed=v0["noise_seed"], **KW)
    assert count.n["read_pcm16"] >= 3 and s.song is not None


def test_10_two_entries_with_one_cover_path_are_refused_before_any_work(world, monkeypatch):
    w = world
    s = w.fresh("dup_output")
    count = Counters(monkeypatch)
    with pytest.raises(ValueError, match=r"\(Voice Ver\)\.wav"):
        s.song_covers(w.song, [dict(voice_model="Voice", pitch_change=0), dict(voice_model="Other", pitch_change=0),
                               dict(voice_model="Voice", pitch_change=1)], **KW)
    assert os.listdir(s.output_dir) == [] and all(v == 0 for v in count.n.values()) and s.song is None
    with pytest.raises(ValueError, match="pitch_change"):
        s.song_covers(w.song, [dict(voice_model="Voice")], **KW)
    with pytest.raises(FileNotFoundError):
        s.song_covers(os.path.join(w.tmp, "nowhere.wav"), [dict(voice_model="Voice", pitch_change=0)], **KW)
    assert os.listdir(s.output_dir) == []


def test_11_command_line_takes_dir_more_than_once(world, capsys):
    w = world

    def cli(out, *dirs):
        argv = ["-i", w.song, "-p", "0", "-pall", "2", "-oformat", "wav", "--mdx-models-dir", w.mdx_dir, "--rvc-models-dir", w.rvc_dir,
                "--output-dir", os.path.join(w.tmp, out)]
        for d in dirs:
            argv += ["-dir", d]
        os.makedirs(os.path.join(w.tmp, out))
        torch.manual_seed(5)                       # the command line has no noise_seed: the synthesizer draws from torch's generator
        capsys.readouterr()
        got = cover.main(argv)
        return got, [l for l in capsys.readouterr().out.splitlines() if l.startswith("[+]")]
    got, lines = cli("cli2_output", "Voice", "Other")
    assert [os.path.basename(p) for p in got] == ["song (Voice Ver).wav", "song (Other Ver).wav"] and all(os.path.exists(p) for p in got)
    assert lines == ["[+] Cover generated at %s" % p for p in got]
    one, lines = cli("cli1_output", "Voice")
    assert isinstance(one, str) and lines == ["[+] Cover generated at %s" % one]
    torch.manual_seed(5)                           # (before the session, as in main(): building the models draws from it too)
    s = w.fresh("cli_ref_output")
    want = s.song_cover_pipeline(w.song, "Voice", 0, None, **KW)
    same_files(os.path.dirname(one), os.path.dirname(want))
    assert filecmp.cmp(got[0], want, shallow=False)         # the first of several covers is that cover too
