"""The vocoder's ResBlock layers (C, k, d) at one 66 s chunk's lengths (40 kHz v2: 6600 frames -> 66 000 x 256, 660 000 x 128,
1 320 000 x 64, 2 640 000 x 32): the half-storage kernel (csrc/conv1d_h.hip, fp16 x / res / out) against the Winograd kernel with fp16
operands and fp32 storage (conv_g1w, what AICG_HALF=1 runs), both as the mid-chain step  out = res + conv(lrelu(x)).
The two are timed in turn, round-robin, one event pair per launch; the median of the rounds is reported with the effective HBM rate
(x + res + out once each, at each kernel's own storage width) and the algorithmic TFLOP/s (2 C^2 k L).
    python tools/kbench_conv1d_h.py [--frames 6600] [--rounds 9]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from aicovergen_amd import _lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=6600)
ap.add_argument("--rounds", type=int, default=9)
args = ap.parse_args()
dev = torch.device("cuda:0")
SLOPE = 0.1


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


print("%-22s | %-34s | %-34s | %s" % ("layer", "conv_g1w fp16 operands, fp32 store", "conv1d_h fp16 store", "g1w / h"))
for C, rate in ((256, 10), (128, 100), (64, 200), (32, 400)):
    L = args.frames * rate
    g = torch.Generator().manual_seed(C)
    x32 = torch.randn(1, C, L, generator=g).to(dev)
    o32 = torch.empty_like(x32)
    x16, o16 = x32.half(), torch.empty(1, C, L, dtype=torch.float16, device=dev)
    for k in (3, 7, 11):
        for d in (1, 3, 5):
            w, b = torch.randn(C, C, k, generator=g) * (0.5 / (C * k) ** 0.5), torch.randn(C, generator=g) * 0.1
            pc = ops.PackedConv(w, b, padding=(k - 1) // 2 * d, dilation=d, device=dev)
            ops.mark_half(pc)
            f_w = lambda: ops.conv(x32, pc, res=x32, out=o32, pre_act=ops.ACT_LRELU, pre_slope=SLOPE)
            f_h = lambda: ops.conv_h(x16, pc, res=x16, out=o16, pre_act=ops.ACT_LRELU, pre_slope=SLOPE)
            f_w()
            name_w = _lib.last_launch()
            f_h()
            assert _lib.last_launch() == "conv1d_h_kernel"
            torch.cuda.synchronize()
            diff = float(((o16.float() - o32).pow(2).sum() / o32.pow(2).sum()).sqrt())
            ev = {"w": [], "h": []}
            for _ in range(args.rounds):
                ev["w"].append(once(f_w))
                ev["h"].append(once(f_h))
            torch.cuda.synchronize()
            t = {key: statistics.median(a.elapsed_time(b) for a, b in v) * 1e-3 for key, v in ev.items()}
            fl = 2.0 * C * C * k * L
            cell = lambda s, width: "%8.1f us %5.2f TB/s %6.1f TF/s" % (s * 1e6, 3.0 * C * L * width / s / 1e12, fl / s / 1e12)
            print("C%-3d L%-8d k%-2d d%d | %s | %s | %.2fx  (%s; rel diff %.1e)"
                  % (C, L, k, d, cell(t["w"], 4), cell(t["h"], 2), t["w"] / t["h"], name_w, diff), flush=True)
