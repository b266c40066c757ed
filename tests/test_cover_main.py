"""The reference's own add_audio_effects and combine_audio (src/main.py:206-233) run through the opt-in stand-ins under src/compat
(pedalboard, pedalboard.io, pydub) on the host emulator, against aicovergen_amd.cover's file-level functions; and src/run_main.py
routes `import pedalboard` to the stand-in only when AICG_DEVICE_POST=1.  The main.py test needs the reference checkout and is
skipped where it is absent; the launcher test writes its own main.py."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_MAIN = "/root/reference/src/main.py"

CHILD = r'''
import filecmp, os, sys, types
ROOT, REF_SRC, TMP = %r, %r, %r
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import conftest
conftest._bind("emu")
from scipy.io import wavfile
from aicovergen_amd import audio_io, cover


class _Absent:
    def __init__(self, *a, **k): pass
    def __call__(self, *a, **k): raise AssertionError("out-of-scope dependency reached")


def stub(name, **attrs):
    m = types.ModuleType(name); m.__dict__.update(attrs); sys.modules[name] = m

stub("gradio", Progress=_Absent, Error=Exception)
stub("sox", Transformer=_Absent)
stub("yt_dlp", YoutubeDL=_Absent)
stub("soundfile", read=_Absent(), write=_Absent())
stub("librosa", load=_Absent())

# main.py's imports: the stand-ins first, then the shadows, then the reference's own src/
sys.path[:0] = [os.path.join(ROOT, "src", "compat"), os.path.join(ROOT, "src"), REF_SRC]
import main
import pedalboard, pydub
assert os.path.samefile(main.__file__, os.path.join(REF_SRC, "main.py"))
assert pedalboard.__file__.startswith(os.path.join(ROOT, "src", "compat")) and main.Pedalboard is pedalboard.Pedalboard
assert main.AudioSegment is pydub.AudioSegment

rng = np.random.default_rng(5)
def pcm(seconds, sr, ch, amp):
    n = int(seconds * sr); t = np.arange(n) / sr
    x = np.stack([amp * np.sin(2 * np.pi * (200 + 90 * c) * t) * (0.4 + 0.6 * np.sin(2 * np.pi * 0.8 * t) ** 2)
                  + 0.05 * rng.standard_normal(n) for c in range(ch)], 1)
    x = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    return x[:, 0] if ch == 1 else x

vocals = os.path.join(TMP, "song_Voice_p0_i0.5_fr3_rms0.25_pro0.33_rmvpe.wav")
backup = os.path.join(TMP, "song_Vocals_Backup.wav")
inst = os.path.join(TMP, "song_Instrumental.wav")
wavfile.write(vocals, 40000, pcm(2.6, 40000, 1, 0.7))
wavfile.write(backup, 44100, pcm(2.5, 44100, 2, 0.3))
wavfile.write(inst, 44100, pcm(2.7, 44100, 2, 0.4))

# ---- add_audio_effects: main.py's own loop (1-second chunks, reset=False) vs one cover call
mixed = main.add_audio_effects(vocals, 0.15, 0.2, 0.8, 0.7)
assert mixed == os.path.join(TMP, "song_Voice_p0_i0.5_fr3_rms0.25_pro0.33_rmvpe_mixed.wav")
sr_m, got = wavfile.read(mixed)
os.rename(mixed, mixed + ".main")
direct = cover.add_audio_effects(vocals, 0.15, 0.2, 0.8, 0.7)
assert direct == mixed
sr_d, want = wavfile.read(direct)
assert sr_m == sr_d == 40000 and got.dtype == want.dtype == np.int16 and got.shape == want.shape == (104000,)
assert np.abs(got.astype(np.int32) - want).max() <= 1
assert np.abs(got.astype(np.int32) - wavfile.read(vocals)[1]).max() > 100      # the effects did something

# ---- combine_audio: main.py's own pydub expression vs cover.combine_audio
out_main = os.path.join(TMP, "song (Voice Ver).wav")
main.combine_audio([direct, backup, inst], out_main, 2, -1, 0.5, "wav")
out_direct = os.path.join(TMP, "direct.wav")
cover.combine_audio([direct, backup, inst], out_direct, 2, -1, 0.5, "wav")
assert filecmp.cmp(out_main, out_direct, shallow=False)
sr_c, c = wavfile.read(out_main)
assert sr_c == 44100 and c.shape[1] == 2 and c.shape[0] == cover.pydub_slice_frames(cover.ratecv_frames(104000, 40000, 44100), 44100)
print("main.py effects + mix through the stand-ins ok")
'''


@pytest.mark.skipif(not os.path.exists(REF_MAIN), reason="the reference checkout exists in the build container only")
def test_reference_main_effects_and_mix_through_the_stand_ins(tmp_path):
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.dirname(REF_MAIN), str(tmp_path))], capture_output=True, text=True,
                       cwd="/", timeout=900)
    assert r.returncode == 0 and "through the stand-ins ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]


@pytest.mark.parametrize("post", [None, "0", "1"])
def test_launcher_routes_pedalboard_only_with_device_post(tmp_path, post):
    (tmp_path / "main.py").write_text(
        "try:\n    import pedalboard, pedalboard.io, pydub\n    print('pedalboard', pedalboard.__file__, pydub.__file__)\n"
        "except ImportError:\n    print('pedalboard absent')\n")
    env = {k: v for k, v in os.environ.items() if k != "AICG_DEVICE_POST"}
    if post is not None:
        env["AICG_DEVICE_POST"] = post
    r = subprocess.run([sys.executable, os.path.join(ROOT, "src", "run_main.py"), str(tmp_path / "main.py")], capture_output=True,
                       text=True, cwd="/", env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    compat = os.path.join(ROOT, "src", "compat") + os.sep
    if post == "1":
        assert r.stdout.startswith("pedalboard " + compat) and (" " + compat + "pydub") in r.stdout, r.stdout
    else:
        assert compat not in r.stdout, r.stdout


def test_stand_ins_name_what_they_support():
    sys.path.insert(0, os.path.join(ROOT, "src", "compat"))
    try:
        import pedalboard
        import pydub
        with pytest.raises(NotImplementedError, match="HighpassFilter"):
            pedalboard.Chorus
        with pytest.raises(NotImplementedError, match="overlay"):
            pydub.AudioSegment(None, 44100).append
        with pytest.raises(NotImplementedError, match="freeze_mode"):
            pedalboard.Reverb(freeze_mode=1.0)
    finally:
        sys.path.remove(os.path.join(ROOT, "src", "compat"))
        for m in ("pedalboard", "pedalboard.io", "pydub"):
            sys.modules.pop(m, None)
