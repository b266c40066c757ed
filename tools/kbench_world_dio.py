"""Time f0_method "dio" (ops.world_dio / stonemask / medfilt3, csrc/world_dio.hip) on a 240 s, 16 kHz vocal-like track: the count call
(mean, low-cut, band bank, crossing counts, scan), the second call (band bank again with emission, candidates, repair), the repair
alone, StoneMask, the median and the whole get_f0_dio_computation chain, beside ops.pitch_ac and RMVPE's infer_from_audio (full-size
network, seeded weights) on the same track in the same process; median of 20 after warm-up.  Writes profiles/world_dio_kbench.json and
prints the same JSON line.  usage: python tools/kbench_world_dio.py [seconds]"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from aicovergen_amd import ops  # noqa: E402
from kbench_pitch_ac import timed, wall  # noqa: E402
from synthetic.inputs import vocal_like  # noqa: E402


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 240.0
    x = torch.from_numpy(vocal_like(seconds, 16000, seed=21)).float().cuda()
    n = x.numel()
    g = ops.world_dio_geometry(16000, n)
    taps = ops._world_dio_plan(g, x.device)
    scratch = torch.empty(g["count_scratch"], dtype=torch.uint8, device=x.device)
    index = torch.empty(g["index_ints"], dtype=torch.int32, device=x.device)
    args = (16000, 10.0, 50.0, 1100.0, 2.0)
    st = ops._stream(x)
    ops._check(x, taps)

    def count():
        ops._call("aicg_world_dio_count", ops._ptr(x), n, *args, ops._ptr(taps), ops._ptr(scratch), ops._ptr(index), None, st)
    count()
    total = int(index[-1].item())
    ev_ip = torch.empty(max(total, 1), dtype=torch.int32, device=x.device)
    ev_fr = torch.empty(max(total, 1), dtype=torch.float32, device=x.device)
    nb, nf = g["n_bands"], g["n_frames"]
    cand, score = (torch.empty((nb, nf), dtype=torch.float32, device=x.device) for _ in range(2))
    f0 = torch.empty((nf,), dtype=torch.float64, device=x.device)
    rs = torch.empty(g["repair_scratch"], dtype=torch.uint8, device=x.device)

    def second():
        ops._call("aicg_world_dio", n, *args, 0.1, ops._ptr(taps), ops._ptr(scratch), ops._ptr(index), total, ops._ptr(ev_ip), ops._ptr(ev_fr),
                  ops._ptr(rs), ops._ptr(cand), ops._ptr(score), ops._ptr(f0), st)
    second()

    def chain():
        f = ops.world_dio(x)
        return ops.medfilt3(ops.stonemask(x, f, 16000, 10.0))
    out = chain()
    res = {"seconds": seconds, "frames": nf, "voiced": int((out > 0).sum()), "crossings": total,
           "count_call_ms": timed(count), "emit_candidates_repair_ms": timed(second),
           "repair_ms": timed(lambda: ops.world_dio_repair(cand, score)),
           "stonemask_ms": timed(lambda: ops.stonemask(x, f0, 16000, 10.0)),
           "medfilt3_ms": timed(lambda: ops.medfilt3(f0)),
           "world_dio_ms": wall(lambda: ops.world_dio(x)),
           "dio_chain_to_host_ms": wall(lambda: chain().cpu()),
           "pitch_ac_ms": timed(lambda: ops.pitch_ac(x))}
    from aicovergen_amd.rmvpe import RMVPE
    from synthetic import weights
    rmvpe = RMVPE(None, False, x.device, state_dict=weights.rmvpe_state_dict(weights.RMVPE_FULL, 1235))
    res["rmvpe_infer_from_audio_ms"] = wall(lambda: rmvpe.infer_from_audio(x, thred=0.03))
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "world_dio_kbench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
