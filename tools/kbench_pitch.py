"""Times pitch_shift (main.py `-pall N`) on the device for the two backing stems of a 240 s track (44.1 kHz stereo instrumental and
backup vocals) at N = +2 and N = -3: the WSOLA time-stretch with both stems in one launch (one workgroup each) and one stem alone,
the resampling by 2^(N/12), and cover.pitch_shift_signal called per stem the way main.py calls pitch_shift.  Reports the share of
WSOLA steps on which the two stems' offsets sit at the search range's ends, as a sanity figure.

    python tools/kbench_pitch.py [--seconds 240] [--iters 5] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aicovergen_amd import _lib, cover, ops  # noqa: E402


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


def stem(seconds, sr, seed):
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    t = np.arange(n) / sr
    ch = []
    for c in range(2):
        s = 0.02 * rng.standard_normal(n)
        for f0, a in ((220.0 + 30 * c, 0.25), (331.0, 0.15), (523.0 + 11 * c, 0.1)):
            s += a * np.sin(2 * np.pi * f0 * t + 2.0 * np.sin(2 * np.pi * (4.0 + c) * t) + rng.uniform(0, 6))
        ch.append(s * (0.4 + 0.6 * np.sin(2 * np.pi * 0.7 * t + c) ** 2))
    return np.stack(ch).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_pitch times the device: it needs a GPU"
    assert _lib.backend() == "hip"
    dev = torch.device("cuda:0")
    sr = 44100
    x = torch.from_numpy(np.stack([stem(a.seconds, sr, 1), stem(a.seconds, sr, 2)])).to(dev)      # (2 stems, 2 channels, n)
    n = x.shape[2]
    res = {"seconds": a.seconds, "stems": "2 x 44.1 kHz stereo", "frames": n}
    for semis in (2, -3):
        d = 2.0 ** (semis / 12.0)
        seg, search, ovl, skip, steps, n_out = ops.tempo_wsola_geometry(sr, 1.0 / d, n)
        r = {"ratio": d, "wsola_steps": steps, "stretched_frames": n_out, "resample_half_taps": ops.resample_ratio_design(d)[2]}
        r["wsola_two_stems_one_launch"] = timeit(lambda: ops.tempo_wsola(x, sr, 1.0 / d), a.iters)
        r["wsola_one_stem"] = timeit(lambda: ops.tempo_wsola(x[0], sr, 1.0 / d), a.iters)
        z, offs = ops.tempo_wsola(x, sr, 1.0 / d)
        r["wsola_us_per_step"] = 1e6 * r["wsola_two_stems_one_launch"]["median_s"] / steps
        r["wsola_multiply_adds_per_step"] = search * ovl * 2
        r["resample_two_stems_one_launch"] = timeit(lambda: ops.resample_ratio(z, d, n), a.iters)
        taps = 2 * r["resample_half_taps"] + 1
        r["resample_gflops_float64"] = 2 * 2.0 * taps * 2 * n * 2 / r["resample_two_stems_one_launch"]["median_s"] * 1e-9
        r["pitch_shift_signal_two_calls"] = timeit(lambda: [cover.pitch_shift_signal(x[s], sr, semis) for s in range(2)], a.iters)
        r["offsets_at_range_end_share"] = float(((offs[:, 1:] == 0) | (offs[:, 1:] == search - 1)).float().mean())
        res["N%+d" % semis] = r
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
