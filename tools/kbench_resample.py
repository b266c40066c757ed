"""Times ops.resample_poly (aicg_resample_poly_mc) at the two places it serves, on a 240 s track: the song input (stereo 48 kHz ->
44.1 kHz, from the file's 16-bit PCM and from float32) and the conversion output (mono 40 kHz -> 48 kHz).  For each: milliseconds
per call (device events around the call, output allocation and launch included; warm-up first, median of the iterations), the
bytes the kernel must move (input once, output once) per second, that as a share of the 8 TB/s HBM figure, and as a share of what a
plain device copy of the same bytes reaches here.  For scale it times, on the host, the pass this replaces: audio_io.load_wav's
scipy.signal.resample_poly of the same array (scipy runs it on one thread; at most 16 are allowed).

One call's input and output (177 MB for the stereo song) would fit in the 256 MB last-level cache if every iteration reused them, and
the figures would then say more than HBM streaming gives.  Every iteration therefore takes the next of several copies of the input
and leaves its output alive in a ring of the same depth, at least 1 GB in all between two uses of one buffer; the copy baseline rotates
in the same way.

    python tools/kbench_resample.py [--seconds 240] [--iters 50] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = str(min(16, int(os.environ.get(_v, "16"))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy.signal import resample_poly  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aicovergen_amd import _lib, ops  # noqa: E402

HBM_BYTES_PER_S = 8e12
ROTATE_BYTES = 1e9       # bytes touched between two uses of one buffer: four times the last-level cache


def timeit(fn, iters, warm=3):
    """fn(i) is iteration i: it picks its buffers by i."""
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    ts = []
    for i in range(warm, warm + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_resample times the device: it needs a GPU"
    assert _lib.backend() == "hip"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    res = {"seconds": a.seconds, "hbm_bytes_per_s": HBM_BYTES_PER_S}
    for name, ch, sr_in, sr_out, pcm in (("song_48k_stereo_pcm16_to_44k1", 2, 48000, 44100, True),
                                         ("song_48k_stereo_f32_to_44k1", 2, 48000, 44100, False),
                                         ("vocals_40k_mono_f32_to_48k", 1, 40000, 48000, False)):
        n = int(a.seconds * sr_in)
        t = np.arange(n) / sr_in
        xh = np.stack([0.5 * np.sin(2 * np.pi * (180 + 40 * c) * t) * (0.3 + 0.7 * np.sin(2 * np.pi * 0.4 * t) ** 2)
                       + 0.05 * rng.standard_normal(n) for c in range(ch)]).astype(np.float32)
        if pcm:
            x = torch.from_numpy(np.ascontiguousarray(np.clip(np.rint(xh * 32768.0), -32768, 32767).astype(np.int16).T)).to(dev)
        else:
            x = torch.from_numpy(xh).to(dev)
        y = ops.resample_poly(x, sr_in, sr_out)
        moved = x.numel() * x.element_size() + y.numel() * y.element_size()
        sets = max(2, int(np.ceil(ROTATE_BYTES / moved)))
        xs, ring = [x] + [x.clone() for _ in range(sets - 1)], [None] * sets

        def call(i):
            ring[i % sets] = None                                       # its block returns to the allocator: the oldest output's
            ring[i % sets] = ops.resample_poly(xs[i % sets], sr_in, sr_out)
        r = timeit(call, a.iters)
        del xs, ring
        # a plain copy that reads and writes the same number of bytes: what a pure stream reaches on this device
        bufs = [torch.zeros(moved // 2 // 4, dtype=torch.float32, device=dev) for _ in range(sets)]
        outs = [torch.empty_like(b) for b in bufs]
        c = timeit(lambda i: outs[i % sets].copy_(bufs[i % sets]), a.iters)
        r["buffer_sets"] = sets
        r.update(ms=r["median_s"] * 1e3, bytes_moved=moved, gb_per_s=moved / r["median_s"] * 1e-9,
                 share_of_hbm=moved / r["median_s"] / HBM_BYTES_PER_S, copy_ms=c["median_s"] * 1e3,
                 copy_gb_per_s=moved / c["median_s"] * 1e-9, share_of_copy=c["median_s"] / r["median_s"])
        g = np.gcd(sr_in, sr_out)
        h = host_time(lambda: resample_poly(xh, sr_out // g, sr_in // g, axis=1).astype(np.float32), a.host_iters)
        r.update(host_scipy_s=h["median_s"], host_over_device=h["median_s"] / r["median_s"])
        if not pcm:
            ref = resample_poly(xh.astype(np.float64), sr_out // g, sr_in // g, axis=1)
            r["max_abs_vs_scipy_float64"] = float(np.abs(y.cpu().numpy() - ref).max())
        res[name] = r
        print("%-32s %8.3f ms  %7.1f GB/s  %5.1f %% of 8 TB/s  (copy of the same bytes %7.3f ms: %4.0f %% of it)   host scipy %7.3f s = %6.0f x"
              % (name, r["ms"], r["gb_per_s"], 100 * r["share_of_hbm"], r["copy_ms"], 100 * r["share_of_copy"], r["host_scipy_s"],
                 r["host_over_device"]), flush=True)
        del x, y, bufs, outs
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
