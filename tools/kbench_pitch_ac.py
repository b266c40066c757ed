"""Time f0_method "pm" (ops.pitch_ac, csrc/pitch_ac.hip) on a 240 s, 16 kHz vocal-like track: the frame stage, the path finder and the
whole call, and RMVPE's infer_from_audio (full-size network, seeded weights) on the same track in the same process; median of 20 after
warm-up, one JSON line.  usage: python tools/kbench_pitch_ac.py [seconds]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aicovergen_amd import ops  # noqa: E402
from synthetic.inputs import vocal_like  # noqa: E402


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def wall(fn, reps=20, warm=3):
    """host wall time (infer_from_audio ends on the host, as VC.get_f0 uses it)"""
    import time
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 240.0
    x = torch.from_numpy(vocal_like(seconds, 16000, seed=21)).float().cuda()
    cand, count = ops.pitch_ac_candidates(x)
    f0 = ops.pitch_ac(x)
    res = {"seconds": seconds, "frames": int(f0.numel()), "voiced": int((f0 > 0).sum()),
           "candidates_ms": timed(lambda: ops.pitch_ac_candidates(x)),
           "path_ms": timed(lambda: ops.pitch_ac_path(cand, count)),
           "pitch_ac_ms": timed(lambda: ops.pitch_ac(x)),
           "pitch_ac_to_host_ms": wall(lambda: ops.pitch_ac(x).cpu())}
    from aicovergen_amd.rmvpe import RMVPE
    from synthetic import weights
    rmvpe = RMVPE(None, False, x.device, state_dict=weights.rmvpe_state_dict(weights.RMVPE_FULL, 1235))
    res["rmvpe_infer_from_audio_ms"] = wall(lambda: rmvpe.infer_from_audio(x, thred=0.03))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
