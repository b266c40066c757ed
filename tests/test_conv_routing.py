"""Which kernel aicg_conv_forward routes a layer to, pinned shape by shape.

The dispatcher (csrc/conv.hip) is a chain of kernel families, each with a measured tile policy; nothing below compares numbers (the
parity tests do), every row only fingerprints the ROUTE: the family name from _lib.last_launch() and, on the emulator, the launch's
grid and block from emu::g_grid / emu::g_block (tests/emu/emu_rt.cpp) -- grid.y is the row tile, grid.x the position tile and patch
shape, block the wave count.  (Two instantiations that share all of these -- the fp32 and fp16 forms of one conv_g1 / conv_g1w tile --
are told apart by their rows' position in the policy only.)  On hardware the family name alone is asserted.

The expected values are literals recorded from the dispatcher as it stood BEFORE it was split into per-family functions
(`python tests/test_conv_routing.py SETTING` prints a setting's rows as JSON, with a hash of each output for one-off bit comparisons):
a change to this table is a change of routing and needs a measurement, not a re-recording.

The development switches are read once per process, so every setting but the default runs in a child process on the emulator,
the way test_conv.py reaches the large tiles (AICG_CONV_WANT=1 lowers the fill target, AICG_CONV_WS=0 skips the wave-specialised forms).
Forced tile codes (gemm_tile) appear where the code is the route's only way in (conv_g1s 128 x 256) or where the policy threshold needs
a problem too large for the emulator (conv_g1 192 x 256: 6 GFLOP; the fp16 128 x 256 tile: > 768 workgroups)."""
import contextlib
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conftest  # noqa: E402,F401  (first: it puts the repository on sys.path and the development switches on, also in the recording mode below)

from aicovergen_amd import _lib, ops  # noqa: E402

SETTINGS = {
    "default": {},
    "want1": {"AICG_CONV_WANT": "1"},
    "ws0": {"AICG_CONV_WS": "0"},
    "ws0_want1": {"AICG_CONV_WS": "0", "AICG_CONV_WANT": "1"},
    "wino_split": {"AICG_WINO_SPLIT_TILES": "1"},
}


def row(name, family, grid, block, **spec):
    return name, spec, family, grid, block


# spec: n, ci, co, k (int: 1-D over `hw` positions; pair: 2-D over the `hw` map), stride, pad, dil, groups; res / act / pre_act: the fused
# epilogue; split / f16: the layer's precision; tile: aicg_conv_desc.gemm_tile; wino: "rows" or the conv_w2d code; wino1d; up: the
# kernel = stride = 2 transposed convolution whose GEMM this is ("mul": with the multiplicative skip)
TABLE = {
    "default": [
        row("pointwise_few_in", "conv_pointwise_kernel", (1, 2, 1), (256, 1, 1), n=2, ci=4, co=48, k=(1, 1), hw=(4, 64)),
        row("pointwise_few_out", "conv_pointwise_kernel", (1, 2, 1), (256, 1, 1), n=2, ci=48, co=4, k=(1, 1), hw=(4, 64)),
        row("g1w_32x512", "conv_g1w_kernel", (4, 1, 1), (256, 1, 1), ci=16, co=64, k=3, pad=1, hw=1024, wino1d=True),
        row("g1w_32x512_k7_d3", "conv_g1w_kernel", (2, 1, 1), (256, 1, 1), ci=16, co=32, k=7, pad=9, dil=3, hw=512, wino1d=True, res=True, pre_act=ops.ACT_LRELU),
        row("g1w_32x512_f16", "conv_g1w_kernel", (4, 1, 1), (256, 1, 1), ci=16, co=64, k=3, pad=1, hw=1024, wino1d=True, f16=True),
        row("w2d_8_pairs", "conv_w2d_kernel", (8, 1, 1), (512, 1, 1), ci=8, co=48, k=(3, 3), pad=1, hw=(8, 64), wino=12),
        row("w2d_8_dword", "conv_w2d_kernel", (8, 1, 1), (512, 1, 1), ci=8, co=48, k=(3, 3), pad=1, hw=(8, 64), wino=2),
        row("w2d_4_dword", "conv_w2d_kernel", (8, 1, 1), (256, 1, 1), ci=8, co=96, k=(3, 3), pad=1, hw=(8, 64), wino=3),
        row("w2d_8_quads", "conv_w2d_kernel", (8, 1, 1), (512, 1, 1), ci=8, co=48, k=(3, 3), pad=1, hw=(8, 64), wino=4),
        row("w2d_4_quads", "conv_w2d_kernel", (8, 1, 1), (256, 1, 1), ci=8, co=48, k=(3, 3), pad=1, hw=(8, 64), wino=5),
        row("wino_rows_96", "conv_ws3w_kernel", (8, 2, 1), (512, 1, 1), ci=8, co=192, k=(3, 3), pad=1, hw=(4, 64), wino="rows"),
        row("wino_rows_64", "conv_ws3w_kernel", (8, 4, 1), (512, 1, 1), ci=8, co=256, k=(3, 3), pad=1, hw=(4, 64), wino="rows"),
        row("wino_rows_48", "conv_ws3w_kernel", (8, 1, 1), (768, 1, 1), ci=8, co=48, k=(3, 3), pad=1, hw=(8, 64), wino="rows"),
        row("wino_rows_32", "conv_ws3w_kernel", (8, 5, 1), (512, 1, 1), ci=8, co=160, k=(3, 3), pad=1, hw=(4, 64), wino="rows"),
        row("wino_rows_144_small_map", "conv_ws3w_kernel", (8, 3, 1), (768, 1, 1), ci=8, co=144, k=(3, 3), pad=1, hw=(8, 64), wino="rows"),
        row("g1_forced_128x256", "conv_g1_kernel", (6, 1, 1), (256, 1, 1), ci=16, co=384, k=1, hw=512, tile=2),
        row("g1_forced_64x256", "conv_g1_kernel", (12, 1, 1), (256, 1, 1), ci=16, co=384, k=1, hw=512, tile=3),
        row("g1_forced_192x256", "conv_g1_kernel", (4, 1, 1), (256, 1, 1), ci=16, co=384, k=1, hw=512, tile=4),
        row("g1_policy_64x256", "conv_g1_kernel", (513, 1, 1), (256, 1, 1), ci=16, co=192, k=1, hw=43776),
        row("g1_policy_128x256", "conv_g1_kernel", (172, 1, 1), (256, 1, 1), ci=16, co=192, k=1, hw=22016),
        row("g1_policy_192x256", "conv_g1_kernel", (171, 1, 1), (256, 1, 1), ci=256, co=192, k=1, hw=43776),
        row("g1_below_256_workgroups", "conv_ws3_kernel", (1020, 1, 1), (512, 1, 1), ci=16, co=64, k=1, hw=65280),
        row("g1_off_by_code", "conv_ws3_kernel", (512, 1, 1), (512, 1, 1), ci=16, co=64, k=1, hw=65536, tile=1),
        row("g1_f16_policy_64x256", "conv_g1_kernel", (12, 1, 1), (256, 1, 1), ci=16, co=384, k=1, hw=512, f16=True),
        row("g1_f16_forced_128x256", "conv_g1_kernel", (6, 1, 1), (256, 1, 1), ci=16, co=384, k=1, hw=512, f16=True, tile=2),
        row("g1_f16_policy_128x256", "conv_g1_kernel", (400, 1, 1), (256, 1, 1), ci=16, co=128, k=1, hw=102400, f16=True),
        row("g1_shuffle_forced_64x256", "conv_g1_kernel", (1, 1, 1), (256, 1, 1), ci=16, co=16, hw=(4, 64), up="mul", tile=3),
        row("g1s_forced_128x256", "conv_g1s_kernel", (4, 1, 1), (256, 1, 1), ci=16, co=256, k=2, stride=2, hw=1024, tile=2),
        row("g1s_forced_64x256", "conv_g1s_kernel", (8, 1, 1), (256, 1, 1), ci=16, co=256, k=2, stride=2, hw=1024, tile=3, res=True),
        row("g1s_policy_64x256", "conv_g1s_kernel", (160, 1, 1), (256, 1, 1), ci=16, co=512, k=2, stride=2, hw=9736),
        row("g1s_below_160_workgroups", "conv_ws3_kernel", (76, 8, 1), (512, 1, 1), ci=16, co=512, k=2, stride=2, hw=9728),
        row("ws3s_64_rows_small_fall_to_single_role", "conv_mfma_kernel", (3, 2, 1), (256, 1, 1), ci=16, co=64, k=3, pad=1, hw=300, split=True),
        row("ws3s_64x64", "conv_ws3s_kernel", (625, 1, 1), (512, 1, 1), ci=16, co=64, k=3, pad=1, hw=40000, split=True),
        row("ws3s_64x64_wide_m", "conv_ws3s_kernel", (5, 2, 1), (512, 1, 1), ci=16, co=96, k=3, pad=1, hw=300, split=True),
        row("ws3s_32x128", "conv_ws3s_kernel", (3, 1, 1), (512, 1, 1), ci=16, co=32, k=3, pad=1, hw=300, split=True),
        row("ws3m16h_16", "conv_ws3m16h_kernel", (256, 1, 1), (512, 1, 1), ci=8, co=16, k=3, pad=1, hw=65536),
        row("ws3m16h_48", "conv_ws3m16h_kernel", (256, 1, 1), (512, 1, 1), ci=8, co=48, k=(3, 3), pad=1, hw=(64, 1024), act=ops.ACT_RELU),
        row("m16_16", "conv_ws16_kernel", (256, 1, 1), (512, 1, 1), ci=4, co=16, k=3, pad=1, hw=65536),
        row("m16_48", "conv_ws16_kernel", (256, 1, 1), (512, 1, 1), ci=4, co=48, k=(3, 3), pad=1, hw=(64, 1024)),
        row("g1_policy_shuffle_64x256", "conv_g1_kernel", (256, 1, 1), (256, 1, 1), ci=8, co=12, hw=(128, 512), up="mul"),
        row("ws3m16h_48_shuffle", "conv_ws3m16h_kernel", (260, 1, 1), (512, 1, 1), ci=8, co=12, hw=(130, 510), up="mul"),
        row("ws3_64_rows_small_fall_to_single_role", "conv_mfma_kernel", (3, 2, 1), (256, 1, 1), ci=32, co=64, k=3, pad=1, hw=300, res=True),
        row("ws3_64x64", "conv_ws3_kernel", (625, 1, 1), (512, 1, 1), ci=16, co=64, k=3, pad=1, hw=40000),
        row("ws3_64x64_wide_m", "conv_ws3_kernel", (2, 4, 1), (512, 1, 1), ci=16, co=200, k=3, pad=1, hw=70),
        row("ws3_32x128", "conv_ws3_kernel", (3, 1, 1), (512, 1, 1), ci=32, co=32, k=3, pad=1, hw=300),
        row("ws3_32x128_grouped", "conv_ws3_kernel", (2, 1, 4), (512, 1, 1), ci=96, co=96, k=16, pad=8, groups=4, hw=130),
        row("shuffle_48_rows_small_fall_to_single_role", "conv_mfma_kernel", (1, 2, 1), (256, 1, 1), ci=24, co=12, hw=(5, 9), up="mul"),
        row("ws_64x64", "conv_ws_kernel", (625, 1, 1), (512, 1, 1), ci=4, co=64, k=3, pad=1, hw=40000),
        row("ws_64x64_wide_m", "conv_ws_kernel", (5, 2, 1), (512, 1, 1), ci=4, co=96, k=3, pad=1, hw=300),
        row("ws_32x128", "conv_ws_kernel", (2, 1, 1), (512, 1, 1), ci=4, co=24, k=(3, 3), pad=1, hw=(5, 20)),
        row("ws_160_rows_stay_classic_small", "conv_ws_kernel", (2, 3, 1), (512, 1, 1), ci=16, co=150, k=3, pad=1, hw=70),
    ],
    "want1": [
        row("ws3s_128x128", "conv_ws3s_kernel", (3, 2, 1), (512, 1, 1), ci=16, co=250, k=3, pad=1, hw=300, split=True),
        row("ws3s_96x128", "conv_ws3s_kernel", (2, 2, 1), (512, 1, 1), ci=16, co=192, k=3, pad=1, hw=200, split=True),
        row("ws3s_64x256", "conv_ws3s_kernel", (3, 1, 1), (512, 1, 1), ci=16, co=64, k=3, pad=1, hw=600, split=True),
        row("ws3s_64x128_patch_too_wide_for_256", "conv_ws3s_kernel", (3, 1, 1), (512, 1, 1), ci=16, co=64, k=3, stride=2, hw=601, split=True),
        row("ws3s_32x256", "conv_ws3s_kernel", (3, 1, 1), (512, 1, 1), ci=16, co=32, k=3, pad=1, hw=520, split=True),
        row("ws3s_32x128_patch_too_wide_for_256", "conv_ws3s_kernel", (3, 1, 1), (512, 1, 1), ci=16, co=32, k=3, stride=2, hw=601, split=True),
        row("ws3s_144_rows", "conv_ws3s_kernel", (1, 3, 1), (512, 1, 1), ci=16, co=144, k=3, pad=1, hw=150, split=True),
        row("ws3_160x128", "conv_ws3_kernel", (3, 2, 1), (512, 1, 1), ci=16, co=300, k=3, pad=1, hw=300),
        row("ws3_128x128", "conv_ws3_kernel", (3, 2, 1), (512, 1, 1), ci=16, co=250, k=3, pad=1, hw=300, res=True),
        row("ws3_96x128", "conv_ws3_kernel", (6, 2, 1), (512, 1, 1), ci=16, co=192, k=(3, 3), pad=1, hw=(12, 40)),
        row("ws3_64x128", "conv_ws3_kernel", (3, 1, 1), (512, 1, 1), ci=16, co=64, k=3, pad=1, hw=300),
        row("ws3_32x256", "conv_ws3_kernel", (3, 1, 1), (512, 1, 1), ci=16, co=32, k=3, pad=1, hw=520),
        row("ws_160x128_shuffle", "conv_ws_kernel", (3, 1, 1), (512, 1, 1), ci=16, co=40, hw=(8, 40), up="mul"),
        row("ws_160x128_res_mul_add", "conv_ws_kernel", (3, 1, 1), (512, 1, 1), ci=16, co=40, hw=(8, 40), up="add"),
        row("ws_128x128", "conv_ws_kernel", (3, 2, 1), (768, 1, 1), ci=4, co=250, k=3, pad=1, hw=300),
        row("ws_64x128_for_256_rows", "conv_ws_kernel", (3, 4, 1), (512, 1, 1), ci=4, co=256, k=3, pad=1, hw=300),
        row("ws_96x128", "conv_ws_kernel", (3, 2, 1), (512, 1, 1), ci=4, co=192, k=3, pad=1, hw=300),
        row("ws_64x128", "conv_ws_kernel", (3, 1, 1), (512, 1, 1), ci=4, co=64, k=3, pad=1, hw=300),
        row("ws_32x256", "conv_ws_kernel", (3, 1, 1), (512, 1, 1), ci=4, co=32, k=3, pad=1, hw=520),
        row("single_role_lds_retry_on_64x64", "conv_mfma_kernel", (5, 1, 1), (256, 1, 1), ci=4, co=64, k=13, stride=13, hw=4000),
    ],
    "ws0": [
        row("sr_64x64", "conv_mfma_kernel", (3, 2, 1), (256, 1, 1), ci=16, co=64, k=3, pad=1, hw=300),
        row("sr_32x128", "conv_mfma_kernel", (3, 1, 1), (256, 1, 1), ci=16, co=32, k=3, pad=1, hw=300),
        row("sr_m16_16", "conv_mfma16_kernel", (256, 1, 1), (256, 1, 1), ci=4, co=16, k=3, pad=1, hw=65536),
        row("sr_m16_48", "conv_mfma16_kernel", (256, 1, 1), (256, 1, 1), ci=4, co=48, k=(3, 3), pad=1, hw=(64, 1024)),
    ],
    "ws0_want1": [
        row("sr_160x128", "conv_mfma_kernel", (3, 2, 1), (256, 1, 1), ci=16, co=300, k=3, pad=1, hw=300),
        row("sr_128x128_8w", "conv_mfma_kernel", (3, 2, 1), (512, 1, 1), ci=16, co=250, k=3, pad=1, hw=300),
        row("sr_96x128", "conv_mfma_kernel", (3, 2, 1), (256, 1, 1), ci=16, co=192, k=3, pad=1, hw=300),
        row("sr_64x128", "conv_mfma_kernel", (6, 1, 1), (256, 1, 1), ci=16, co=64, k=(3, 3), pad=1, hw=(9, 40)),
        row("sr_32x256", "conv_mfma_kernel", (3, 1, 1), (256, 1, 1), ci=16, co=32, k=3, pad=1, hw=520),
        row("sr_lds_retry_on_64x64", "conv_mfma_kernel", (10, 1, 1), (256, 1, 1), ci=4, co=32, k=13, stride=13, hw=8000),
    ],
    "wino_split": [
        row("wino_rows_144_split_96_48", "conv_ws3w_kernel", (8, 1, 1), (768, 1, 1), ci=8, co=144, k=(3, 3), pad=1, hw=(8, 64), wino="rows"),
        row("wino_rows_240_split_96_48", "conv_ws3w_kernel", (8, 1, 1), (768, 1, 1), n=2, ci=8, co=240, k=(3, 3), pad=1, hw=(5, 66), wino="rows"),
        row("wino_rows_96_not_split", "conv_ws3w_kernel", (8, 1, 1), (512, 1, 1), ci=8, co=96, k=(3, 3), pad=1, hw=(4, 64), wino="rows"),
    ],
}

_OPS_GLOBALS = ("split_precision", "gemm_tile", "winograd_min_positions", "winograd2d", "winograd2d_waves", "winograd2d_quads",
                "winograd2d_pairs", "winograd2d_code", "winograd1d_min_positions")
_W2D = {12: (8, False, True), 2: (8, False, False), 3: (4, False, False), 4: (8, True, False), 5: (4, True, False)}   # code: waves, quads, pairs


@contextlib.contextmanager
def _ops_settings(spec):
    old = {k: getattr(ops, k) for k in _OPS_GLOBALS}
    try:
        ops.split_precision = bool(spec.get("split"))
        ops.gemm_tile = spec.get("tile", 0)
        ops.winograd2d_code = 0
        wino = spec.get("wino")
        ops.winograd_min_positions = 1 if wino else 1 << 60
        ops.winograd2d = wino not in (None, "rows")
        if ops.winograd2d:
            ops.winograd2d_waves, ops.winograd2d_quads, ops.winograd2d_pairs = _W2D[wino]
            assert ops._w2d_code()[0] == wino
        ops.winograd1d_min_positions = 1 if spec.get("wino1d") else 1 << 60
        yield
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


def launch(spec, device):
    """One table row through ops.conv / ops.conv_transpose on seeded data; returns the output."""
    torch.manual_seed(0)
    n, ci, co, hw = spec.get("n", 1), spec["ci"], spec["co"], spec["hw"]
    with _ops_settings(spec):
        if spec.get("up"):
            x = torch.randn(n, ci, *hw)
            pt = ops.PackedConvTranspose(torch.randn(ci, co, 2, 2) * 0.2, torch.randn(co), stride=2, device=device)
            skip = torch.randn(n, co, 2 * hw[0], 2 * hw[1]).to(device)
            return ops.conv_transpose(x.to(device), pt, act=ops.ACT_RELU, **{spec["up"]: skip})
        k, groups = spec["k"], spec.get("groups", 1)
        one_d = isinstance(k, int)
        x = torch.randn(n, ci, hw) if one_d else torch.randn(n, ci, *hw)
        w = (torch.randn(co, ci // groups, k) if one_d else torch.randn(co, ci // groups, *k)) * 0.1
        pc = ops.PackedConv(w, torch.randn(co), stride=spec.get("stride", 1), padding=spec.get("pad", 0), dilation=spec.get("dil", 1),
                            groups=groups, device=device)
        pc.f16 = bool(spec.get("f16"))
        ho, wo = pc.out_hw(1 if one_d else hw[0], hw if one_d else hw[1])
        res = (torch.randn(n, co, wo) if one_d else torch.randn(n, co, ho, wo)).to(device) if spec.get("res") else None
        return ops.conv(x.to(device), pc, res=res, act=spec.get("act", ops.ACT_NONE), pre_act=spec.get("pre_act", ops.ACT_NONE), pre_slope=0.1)


def record(setting, device, geometry):
    """[(name, family, grid, block, sha256 of the output)] of a setting's rows; grid / block (emulator only) are None without `geometry`."""
    out = []
    for name, spec, _, _, _ in TABLE[setting]:
        y = launch(spec, device)
        family, grid, block = _lib.last_launch(), None, None
        if geometry:
            lib = _lib.get()
            grid = tuple((ctypes.c_uint * 3).in_dll(lib, "_ZN3emu6g_gridE"))      # emu::g_grid, emu::g_block: dim3 = three unsigned
            block = tuple((ctypes.c_uint * 3).in_dll(lib, "_ZN3emu7g_blockE"))
        out.append((name, family, grid, block, hashlib.sha256(y.detach().cpu().contiguous().numpy().tobytes()).hexdigest()))
    return out


def _expected(setting, geometry):
    return [(name, family, grid if geometry else None, block if geometry else None) for name, _, family, grid, block in TABLE[setting]]


def _record_in_child(setting):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), setting], env=dict(os.environ, **SETTINGS[setting]), cwd=root,
                         capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    return [(r["name"], r["family"], tuple(r["grid"]), tuple(r["block"])) for r in rows]


def test_default_routing(dev):
    """The product's routing (no switch set): every family's small-problem tiles, the forced codes, the policy gates of conv_g1 /
    conv_g1s from both sides, the fp16 and shuffle / res_mul routes, the 16 x 16 x 4 forms."""
    got = [r[:4] for r in record("default", dev.device, dev.kind == "emu")]
    assert got == _expected("default", dev.kind == "emu")


@pytest.mark.parametrize("setting", [s for s in SETTINGS if s != "default"])
def test_switched_routing_on_the_emulator(setting):
    """The large tiles (fill target lowered), the single-role fallbacks incl. their AICG_E_LDS retry on 64 x 64, the two-launch
    96 + 48 split of the row-Winograd form: one child process per setting."""
    assert _record_in_child(setting) == _expected(setting, True)


if __name__ == "__main__":
    conftest._bind("emu")
    for name, family, grid, block, sha in record(sys.argv[1], torch.device("cpu"), True):
        print(json.dumps({"name": name, "family": family, "grid": grid, "block": block, "sha": sha}), flush=True)
