"""Time the quantile normalisation in front of mangio-crepe and hybrid[...] (x / np.quantile(np.abs(x), 0.999)) on a 240 s, 16 kHz
vocal-like track that lives on the device, two ways in one process: the host route (device -> host copy, np.quantile, the division,
the upload the estimators need) and the device route (ops.abs_quantile: radix select and numpy's interpolation, then ops.div_scalar;
csrc/select.hip), with the device route's pieces and the nan-median of three 24 000-frame tracks beside np.nanmedian; median of 20
after warm-up.  Checks that both routes give the same bits.  Writes profiles/quantile_kbench.json and prints the same JSON line.
usage: python tools/kbench_quantile.py [seconds]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from aicovergen_amd import ops  # noqa: E402
from kbench_pitch_ac import timed, wall  # noqa: E402
from synthetic.inputs import vocal_like  # noqa: E402


def host_route(x):
    h = x.cpu().numpy().astype(np.float32)
    return torch.from_numpy(h / np.quantile(np.abs(h), 0.999)).to(x.device)


def device_route(x):
    return ops.div_scalar(x, ops.abs_quantile(x, 0.999))


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 240.0
    x = torch.from_numpy(vocal_like(seconds, 16000, seed=21)).float().cuda()
    n = x.numel()
    same = bool(torch.equal(host_route(x).view(torch.int32), device_route(x).view(torch.int32)))
    lo, hi, _ = ops.quantile_plan(n, 0.999)
    s = ops.abs_quantile(x, 0.999)
    h = x.cpu().numpy()
    rows = torch.rand(3, int(seconds * 100), dtype=torch.float64, device=x.device)
    rows[rows < 0.2] = float("nan")
    rows_h = rows.cpu().numpy()

    def np_quantile_only():
        np.quantile(np.abs(h), 0.999)

    import time

    def host_ms(fn, reps=20):
        fn()
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            out.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(out))

    res = {"seconds": seconds, "samples": n, "numpy": np.__version__, "same_bits": same,
           "host_route_ms": wall(lambda: host_route(x)),
           "device_route_ms": wall(lambda: device_route(x)),
           "device_route_gpu_ms": timed(lambda: device_route(x)),
           "abs_select_gpu_ms": timed(lambda: ops.abs_select(x, lo, hi)),
           "div_scalar_gpu_ms": timed(lambda: ops.div_scalar(x, s)),
           "host_np_quantile_ms": host_ms(np_quantile_only),
           "host_download_ms": wall(lambda: x.cpu()),
           "nanmedian_rows_3_to_host_ms": wall(lambda: ops.nanmedian_rows(rows).cpu()),
           "np_nanmedian_3_from_device_ms": wall(lambda: np.nanmedian(rows.cpu().numpy(), axis=0)),
           "np_nanmedian_3_ms": host_ms(lambda: np.nanmedian(rows_h, axis=0))}
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "quantile_kbench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
