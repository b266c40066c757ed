"""The reference's own pitch_shift (src/main.py:138-147) run through the opt-in sox stand-in under src/compat on the host emulator,
against aicovergen_amd.cover.pitch_shift; src/run_main.py routes `import sox` to the stand-in only when AICG_DEVICE_POST=1; and the
stand-in names what it supports.  soundfile stays the user's own: here it is a test-local stub over scipy.io.wavfile with
libsndfile's scalings (16-bit PCM read as int16 / 32768, written as round(clip(x) * 32767)).  The main.py test needs the reference
checkout and is skipped where it is absent; the launcher test writes its own main.py."""
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
from aicovergen_amd import cover


class _Absent:
    def __init__(self, *a, **k): pass
    def __call__(self, *a, **k): raise AssertionError("out-of-scope dependency reached")


def stub(name, **attrs):
    m = types.ModuleType(name); m.__dict__.update(attrs); sys.modules[name] = m


def sf_read(path):
    sr, data = wavfile.read(path)
    assert data.dtype == np.int16
    return data.astype(np.float64) / 32768.0, sr


def sf_write(path, data, sr):
    wavfile.write(path, sr, np.rint(np.clip(np.asarray(data, np.float64), -1.0, 1.0) * 32767.0).astype(np.int16))

stub("gradio", Progress=_Absent, Error=Exception)
stub("yt_dlp", YoutubeDL=_Absent)
stub("soundfile", read=sf_read, write=sf_write)
stub("librosa", load=_Absent())

# main.py's imports: the stand-ins first, then the shadows, then the reference's own src/
sys.path[:0] = [os.path.join(ROOT, "src", "compat"), os.path.join(ROOT, "src"), REF_SRC]
import main
import sox
assert os.path.samefile(main.__file__, os.path.join(REF_SRC, "main.py"))
assert sox.__file__.startswith(os.path.join(ROOT, "src", "compat")) and main.sox is sox

rng = np.random.default_rng(7)
def pcm(seconds, sr, ch, amp):
    n = int(seconds * sr); t = np.arange(n) / sr
    x = np.stack([amp * np.sin(2 * np.pi * (200 + 90 * c) * t) * (0.4 + 0.6 * np.sin(2 * np.pi * 0.8 * t) ** 2)
                  + 0.05 * rng.standard_normal(n) for c in range(ch)], 1)
    x = np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    return x[:, 0] if ch == 1 else x

for name, ch, rate in (("song_Instrumental.wav", 2, 11025), ("song_Vocals_Backup.wav", 1, 8000)):
    src = os.path.join(TMP, name)
    wavfile.write(src, rate, pcm(1.3, rate, ch, 0.5))
    out = main.pitch_shift(src, 2)
    assert out == os.path.splitext(src)[0] + "_p2.wav" and os.path.exists(out)
    sr_o, got = wavfile.read(out)
    assert sr_o == rate and got.dtype == np.int16 and got.shape == wavfile.read(src)[1].shape
    assert np.abs(got.astype(np.int32) - wavfile.read(src)[1]).max() > 100            # the shift did something
    # a second call returns without rewriting the file
    with open(out, "ab") as f: f.write(b"mark")
    assert main.pitch_shift(src, 2) == out and open(out, "rb").read().endswith(b"mark")
    os.rename(out, out + ".main")
    with open(out + ".main", "r+b") as f: f.truncate(os.path.getsize(out + ".main") - 4)
    direct = cover.pitch_shift(src, 2)
    assert direct == out and filecmp.cmp(out, out + ".main", shallow=False)
    assert cover.pitch_shift(src, 2) == out
print("main.py pitch_shift through the stand-in ok")
'''


@pytest.mark.skipif(not os.path.exists(REF_MAIN), reason="the reference checkout exists in the build container only")
def test_reference_main_pitch_shift_through_the_stand_in(tmp_path):
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.dirname(REF_MAIN), str(tmp_path))], capture_output=True, text=True,
                       cwd="/", timeout=900)
    assert r.returncode == 0 and "through the stand-in ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]


@pytest.mark.parametrize("post", [None, "0", "1"])
def test_launcher_routes_sox_only_with_device_post(tmp_path, post):
    (tmp_path / "main.py").write_text(
        "try:\n    import sox\n    print('sox', sox.__file__)\nexcept ImportError:\n    print('sox absent')\n")
    env = {k: v for k, v in os.environ.items() if k != "AICG_DEVICE_POST"}
    if post is not None:
        env["AICG_DEVICE_POST"] = post
    r = subprocess.run([sys.executable, os.path.join(ROOT, "src", "run_main.py"), str(tmp_path / "main.py")], capture_output=True,
                       text=True, cwd="/", env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    compat = os.path.join(ROOT, "src", "compat") + os.sep
    if post == "1":
        assert r.stdout.startswith("sox " + compat + "sox"), r.stdout
    else:
        assert compat not in r.stdout, r.stdout


def test_sox_stand_in_names_what_it_supports():
    sys.path.insert(0, os.path.join(ROOT, "src", "compat"))
    try:
        import sox
        with pytest.raises(NotImplementedError, match="pitch"):
            sox.Transformer().tempo
        with pytest.raises(NotImplementedError, match="pitch"):
            sox.Combiner
        with pytest.raises(NotImplementedError, match="quick"):
            sox.Transformer().pitch(2, quick=True)
        with pytest.raises(NotImplementedError, match="channels"):
            sox.Transformer().pitch(2).build_array(input_array=__import__("numpy").zeros((100, 3)), sample_rate_in=8000)
    finally:
        sys.path.remove(os.path.join(ROOT, "src", "compat"))
        sys.modules.pop("sox", None)
