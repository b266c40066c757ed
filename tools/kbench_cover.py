"""Times the tail of song_cover_pipeline at a 240 s track on the device (aicovergen_amd.cover): the vocal effects chain at main.py's
defaults (40 kHz mono, the RVC output), the same chain as one sequential segment, the opt-in pedalboard stand-in fed 1-second chunks
the way main.py's add_audio_effects feeds it, and the three-stem mix (40 kHz mono vocals, 44.1 kHz stereo backup + instrumental).
For scale it also times, on the host, the stdlib audioop calls pydub makes for the same mix.

    python tools/kbench_cover.py [--seconds 240] [--iters 5] [--json out.json]
"""
import argparse
import audioop
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aicovergen_amd import _lib, cover  # noqa: E402


def timeit(fn, iters, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "iters": iters}


def host_time(fn, iters):
    ts = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_cover times the device: it needs a GPU"
    assert _lib.backend() == "hip"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    sr_v, sr_s = 40000, 44100
    n = int(a.seconds * sr_v)
    t = np.arange(n) / sr_v
    v = (0.5 * np.sin(2 * np.pi * 180 * t) * (0.3 + 0.7 * np.sin(2 * np.pi * 0.4 * t) ** 2) + 0.05 * rng.standard_normal(n))
    x = torch.from_numpy(np.clip(v, -1, 1).astype(np.float32)).to(dev)
    res = {"seconds": a.seconds, "vocals": "40 kHz mono", "stems": "44.1 kHz stereo"}

    fx = lambda **k: cover.vocal_effects(x, sr_v, 0.15, 0.2, 0.8, 0.7, **k)
    res["effects_segmented"] = timeit(lambda: fx(), a.iters)
    res["effects_single_segment"] = timeit(lambda: fx(segment=0), max(1, a.iters // 2))
    y_seg, _ = fx()
    y_one, _ = fx(segment=0)
    res["effects_segmented_vs_single_max_abs"] = float((y_seg - y_one).abs().max())

    # the opt-in stand-in as main.py drives it: Pedalboard(...)(chunk, sr, reset=False) per second of audio (host in / out)
    sys.path.insert(0, os.path.join(ROOT, "src", "compat"))
    import pedalboard
    xh = x.cpu().numpy().reshape(1, -1)

    def chunked():
        board = pedalboard.Pedalboard([pedalboard.HighpassFilter(), pedalboard.Compressor(ratio=4, threshold_db=-15),
                                       pedalboard.Reverb(room_size=0.15, dry_level=0.8, wet_level=0.2, damping=0.7)])
        for i in range(0, n, sr_v):
            board(xh[:, i:i + sr_v], sr_v, reset=False)
    res["effects_compat_1s_chunks"] = timeit(chunked, 1)

    def pcm(seconds, rate, ch, amp, seed):
        r = np.random.default_rng(seed)
        m = int(seconds * rate)
        tt = np.arange(m) / rate
        z = np.stack([amp * np.sin(2 * np.pi * (300 + 50 * c) * tt) + 0.1 * amp * r.standard_normal(m) for c in range(ch)], 1)
        return np.clip(np.round(z * 32767), -32768, 32767).astype(np.int16)
    mv, mb, mi = pcm(a.seconds, sr_v, 1, 0.8, 1), pcm(a.seconds, sr_s, 2, 0.5, 2), pcm(a.seconds, sr_s, 2, 0.5, 3)
    dv, db, di = (torch.from_numpy(q).to(dev) for q in (mv, mb, mi))
    res["mix"] = timeit(lambda: cover.mix_stems(dv, sr_v, db, sr_s, di, sr_s, 0, 0, 0), a.iters)

    def audioop_mix():  # the calls pydub makes: 3 x 2 mul, tostereo, ratecv 40 -> 44.1 kHz, 2 x add
        g = lambda d, db_: audioop.mul(d, 2, 10 ** (db_ / 20))
        m = audioop.tostereo(g(g(mv.tobytes(), -4), 0), 2, 1, 1)
        m = audioop.ratecv(m, 2, 2, sr_v, sr_s, None)[0]
        b = g(g(mb.tobytes(), -6), 0)
        i = g(g(mi.tobytes(), -7), 0)
        k = min(len(m), len(b))
        m = audioop.add(m[:k], b[:k], 2) + m[k:]
        k = min(len(m), len(i))
        return audioop.add(m[:k], i[:k], 2) + m[k:]
    res["mix_host_audioop"] = host_time(audioop_mix, 2)
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
