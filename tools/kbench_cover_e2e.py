"""Wall time of a whole cover: a 240 s 44.1 kHz stereo `song_like` input, full-size seeded models (the ones bench.py builds), `wav`
output, `-pall 0` and `-pall 2`.  Three routes, each wall-clock with a final device synchronise, median of --iters after --warmup:

  (a) file_route   the functions main.py strings together, as they were before the one-call route existed: mdx.run_mdx x3,
                   rvc.Config / load_hubert / get_vc / rvc_infer (voice_change), cover.add_audio_effects, cover.pitch_shift x2,
                   cover.combine_audio -- every stage through WAV files, every model reloaded;
  (b) first_song   CoverSession(...) + song_cover_pipeline: what a single cover costs, models loaded once;
  (c) second_song  another song through the same session, with its per-stage split (CoverSession.profile_stages: the device is
                   drained after every stage for the split, in runs of their own that do not enter the median).

The model directories are written to a scratch directory in main.py's layout (hubert_base.pt, rmvpe.pt, <voice>/voice.pth,
model_data.json).  The three .onnx files are placeholders with distinct hashes: mdx.load_network_state is pointed at the seeded
full-size state dicts for both routes, so decoding an .onnx file is in neither time (it would add to (a) three times a song, to
(b) three times a session); packing the weight images is in both.

    python tools/kbench_cover_e2e.py [--seconds 240] [--iters 5] [--warmup 2] [--json profiles/cover_e2e.json]
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
from aicovergen_amd import _lib, audio_io, cover, mdx, rvc  # noqa: E402
from synthetic import weights  # noqa: E402
from synthetic.inputs import song_like  # noqa: E402

MDX_CFGS = (weights.MDX_VOC_FT, weights.MDX_KARA2, weights.MDX_REVERB_HQ)
FX = (0.15, 0.2, 0.8, 0.7)


def make_dirs(tmp):
    mdx_dir, rvc_dir = os.path.join(tmp, "mdxnet_models"), os.path.join(tmp, "rvc_models")
    os.makedirs(os.path.join(rvc_dir, "Voice"))
    os.makedirs(mdx_dir)
    params, states = {}, {}
    for i, (name, cfg) in enumerate(zip(cover.MDX_MODEL_FILES, MDX_CFGS)):
        path = os.path.join(mdx_dir, name)
        with open(path, "wb") as f:
            f.write(b"placeholder %d" % i)
        params[mdx.MDX.get_hash(path)] = {"mdx_dim_f_set": cfg["dim_f"], "mdx_dim_t_set": int(np.log2(cfg["dim_t"])),
                                          "mdx_n_fft_scale_set": cfg["n_fft"], "primary_stem": "Vocals", "compensate": 1.021}
        states[path] = weights.mdx_state_dict(cfg, 1234 + i)
    mdx.load_network_state = lambda p: states[p]
    with open(os.path.join(mdx_dir, "model_data.json"), "w") as f:
        json.dump(params, f)
    torch.save({"model": weights.hubert_state_dict(weights.HUBERT_BASE, 1234)}, os.path.join(rvc_dir, "hubert_base.pt"))
    torch.save(weights.rmvpe_state_dict(weights.RMVPE_FULL, 1235), os.path.join(rvc_dir, "rmvpe.pt"))
    torch.save({"config": list(weights.SYNTH_CFG_40K_V2), "weight": weights.synth_state_dict(weights.SYNTH_CFG_40K_V2, 1236), "f0": 1,
                "version": "v2"}, os.path.join(rvc_dir, "Voice", "voice.pth"))
    return mdx_dir, rvc_dir, params


def file_route(song, out, mdx_dir, rvc_dir, params, pall):
    """main.py:241-313 for a local file, through the file-level functions."""
    p = lambda n: os.path.join(mdx_dir, n)
    v, inst = mdx.run_mdx(params, out, p(cover.MDX_MODEL_FILES[0]), song, denoise=True, keep_orig=True)
    backup, main = mdx.run_mdx(params, out, p(cover.MDX_MODEL_FILES[1]), v, suffix="Backup", invert_suffix="Main", denoise=True)
    _, dereverb = mdx.run_mdx(params, out, p(cover.MDX_MODEL_FILES[2]), main, invert_suffix="DeReverb", exclude_main=True, denoise=True)
    ai = os.path.join(out, "ai.wav")
    config = rvc.Config("cuda:0", True)
    hub = rvc.load_hubert("cuda:0", config.is_half, os.path.join(rvc_dir, "hubert_base.pt"))
    cpt, version, net_g, tgt_sr, vc = rvc.get_vc("cuda:0", config.is_half, config, os.path.join(rvc_dir, "Voice", "voice.pth"))
    vc.rmvpe_path = os.path.join(rvc_dir, "rmvpe.pt")
    rvc.rvc_infer("", 0.5, dereverb, ai, pall, "rmvpe", cpt, version, net_g, 3, tgt_sr, 0.25, 0.33, 128, vc, hub)
    mixed = cover.add_audio_effects(ai, *FX)
    if pall != 0:
        inst, backup = cover.pitch_shift(inst, pall), cover.pitch_shift(backup, pall)
    cover.combine_audio([mixed, backup, inst], os.path.join(out, "cover.wav"), 0, 0, 0, "wav")


def timed(fn, iters, warmup, tmp):
    ts = []
    for k in range(warmup + iters):
        out = os.path.join(tmp, "out")
        shutil.rmtree(out, ignore_errors=True)
        os.makedirs(out)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(out)
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append(time.perf_counter() - t0)
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "iters": iters, "warmup": warmup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "cover_e2e.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available() and _lib.backend() == "hip", "kbench_cover_e2e times the device: it needs a GPU"
    tmp = tempfile.mkdtemp(prefix="cover_e2e_")
    try:
        mdx_dir, rvc_dir, params = make_dirs(tmp)
        songs = []
        for seed in (1, 2):
            path = os.path.join(tmp, "song%d.wav" % seed)
            audio_io.write_wav_pcm16(path, (song_like(a.seconds, 44100, seed).astype(np.float32) * 0.6).T, 44100)
            songs.append(path)
        res = {"seconds": a.seconds, "input": "44.1 kHz stereo song_like, 16-bit PCM WAV", "models": "full-size seeded (bench.py's)",
               "output_format": "wav", "device": torch.cuda.get_device_name(0)}
        for pall in (0, 2):
            kw = dict(pitch_change_all=pall, output_format="wav", noise_seed=1234)
            r = {"file_route": timed(lambda out: file_route(songs[0], out, mdx_dir, rvc_dir, params, pall), a.iters, a.warmup, tmp)}
            r["first_song"] = timed(lambda out: cover.CoverSession(mdx_dir, rvc_dir, out).song_cover_pipeline(songs[0], "Voice", 0, False, **kw),
                                    a.iters, a.warmup, tmp)
            session = cover.CoverSession(mdx_dir, rvc_dir, tmp)
            session.song_cover_pipeline(songs[0], "Voice", 0, False, **kw)

            def second(out):
                session.output_dir = out
                session.song_cover_pipeline(songs[1], "Voice", 0, False, **kw)
            r["second_song"] = timed(second, a.iters, a.warmup, tmp)
            session.profile_stages = True
            splits = []
            for _ in range(3):
                timed(second, 1, 0, tmp)
                splits.append(dict(session.last_profile))
            r["second_song_stages_s"] = {k: float(np.median([s[k] for s in splits])) for k in splits[0]}
            r["first_song_le_file_route"] = r["first_song"]["median_s"] <= r["file_route"]["median_s"]
            res["pall_%d" % pall] = r
            print(json.dumps({"pall": pall, **r}), flush=True)
            with open(a.json, "w") as f:         # after every setting: a run cut short keeps what it measured
                json.dump(res, f, indent=1)
                f.write("\n")
        print("wrote", a.json)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
