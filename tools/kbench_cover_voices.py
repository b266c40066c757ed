"""One song, four covers: what the session's song cache and CoverSession.song_covers save.  A 240 s 44.1 kHz stereo `song_like` input,
full-size seeded stand-in models in main.py's directory layout (tools/kbench_cover_e2e.py builds them), two v2 voice directories x
two values of `-p`, `wav` output, `-pall 2`.  Each route starts from an empty output directory and a session whose models are loaded
and warm; wall clock with a final device synchronise, median of --iters after --warmup:

  (a) sequential   four song_cover_pipeline calls with the song cache switched off (AICG_SONG_CACHE=0 through _env.dev): every call
                   reads and uploads the stems again, resamples, estimates f0, runs HuBERT and shifts the backing stems;
  (b) song_covers  one song_covers call: separation, front and shift queued once, the files of cover k written while k + 1 runs;
  (c) single       one song_cover_pipeline call, cache off and on -- the cost of a single cover must not move (compare it with the same
                   number measured at the parent commit, runs alternating; --single-only prints just this).

The same voice directory cannot appear twice in one song_covers call (both covers would have one file name), so the two `-p` values
of a voice go to two directories holding the same model.

    python tools/kbench_cover_voices.py [--seconds 240] [--iters 3] [--warmup 1] [--json profiles/r07_cover_voices.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("AICG_DEV", "1")
from aicovergen_amd import _lib, audio_io, cover  # noqa: E402
from synthetic import weights  # noqa: E402
from synthetic.inputs import song_like  # noqa: E402
import kbench_cover_e2e as e2e  # noqa: E402

KW = dict(pitch_change_all=2, output_format="wav")
VOICES = [dict(voice_model="Voice", pitch_change=0, noise_seed=1), dict(voice_model="Voice_b", pitch_change=1, noise_seed=2),
          dict(voice_model="Other", pitch_change=0, noise_seed=3), dict(voice_model="Other_b", pitch_change=-1, noise_seed=4)]


def timed(fn, session, iters, warmup, tmp, cache):
    ts = []
    os.environ["AICG_SONG_CACHE"] = "1" if cache else "0"
    for k in range(warmup + iters):
        out = os.path.join(tmp, "out")
        shutil.rmtree(out, ignore_errors=True)
        os.makedirs(out)
        session.output_dir = out
        session.drop_song()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append(time.perf_counter() - t0)
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "iters": iters, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "r07_cover_voices.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available() and _lib.backend() == "hip", "kbench_cover_voices times the device: it needs a GPU"
    tmp = tempfile.mkdtemp(prefix="cover_voices_")
    try:
        mdx_dir, rvc_dir, _ = e2e.make_dirs(tmp)
        os.makedirs(os.path.join(rvc_dir, "Other"))
        torch.save({"config": list(weights.SYNTH_CFG_40K_V2), "weight": weights.synth_state_dict(weights.SYNTH_CFG_40K_V2, 1301), "f0": 1,
                    "version": "v2"}, os.path.join(rvc_dir, "Other", "other.pth"))
        for name in ("Voice", "Other"):
            shutil.copytree(os.path.join(rvc_dir, name), os.path.join(rvc_dir, name + "_b"))
        song = os.path.join(tmp, "song.wav")
        audio_io.write_wav_pcm16(song, (song_like(a.seconds, 44100, 1).astype(np.float32) * 0.6).T, 44100)
        session = cover.CoverSession(mdx_dir, rvc_dir, tmp)
        for v in VOICES:
            session.voice(v["voice_model"])
        has_cache = hasattr(session, "drop_song")
        if not has_cache:                       # the same file runs at the parent commit for the single-cover comparison
            session.drop_song = lambda: None

        def one(v):
            return session.song_cover_pipeline(song, v["voice_model"], v["pitch_change"], False, noise_seed=v["noise_seed"], **KW)
        res = {"seconds": a.seconds, "voices": len(VOICES), "pitch_change_all": 2, "models": "full-size seeded (bench.py's)",
               "device": torch.cuda.get_device_name(0)}
        res["single_cache_off"] = timed(lambda: one(VOICES[0]), session, a.iters, a.warmup, tmp, False)
        if has_cache:
            res["single_cache_on"] = timed(lambda: one(VOICES[0]), session, a.iters, a.warmup, tmp, True)
        if has_cache and not a.single_only:
            res["sequential_cache_off"] = timed(lambda: [one(v) for v in VOICES], session, a.iters, a.warmup, tmp, False)
            before = torch.cuda.memory_allocated()
            res["song_covers"] = timed(lambda: session.song_covers(song, VOICES, False, **KW), session, a.iters, a.warmup, tmp, True)
            res["song_cache_bytes"] = int(session.song.nbytes())
            res["memory_allocated_delta_bytes"] = int(torch.cuda.memory_allocated() - before)
            res["front_bytes"] = int(sum(f.nbytes() for f in session.song.fronts.values()))
            res["song_covers_over_sequential"] = res["song_covers"]["median_s"] / res["sequential_cache_off"]["median_s"]
        print(json.dumps(res), flush=True)
        if not a.single_only:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
