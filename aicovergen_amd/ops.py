"""Thin torch-tensor wrappers over the C ABI (include/aicg.h).  No arithmetic happens here: these
functions validate shapes, allocate outputs with torch, and hand raw device pointers + the current HIP
stream to libaicg_hip.so."""
import contextlib
import ctypes
import functools
import math
import os
import threading
from collections import namedtuple

import numpy as np
import torch
from . import _env, _lib


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream(t):
    if t.is_cuda:
        return torch.cuda.current_stream(t.device).cuda_stream
    return 0


_tls = threading.local()


def _check(*tensors):
    """All tensors must be fp32/int, contiguous where required by the caller, and live where the bound
    library executes: HIP device memory of ONE device for the product library, host memory for the test emulator.
    Remembers that device for the launch that follows (`_call`)."""
    be = _lib.backend()
    dev = None
    for t in tensors:
        if t is None:
            continue
        if be == "hip" and not t.is_cuda:
            raise RuntimeError("aicovergen_amd: tensor on %s, but the HIP kernels need device memory" % t.device)
        if be == "emu" and t.is_cuda:
            raise RuntimeError("emulator backend needs host tensors")
        if t.is_cuda:
            if dev is None:
                dev = t.device.index
            elif dev != t.device.index:
                raise RuntimeError("aicovergen_amd: operands on different devices (cuda:%d and cuda:%d)" % (dev, t.device.index))
    _tls.dev = dev


def _call(name, *args):
    """_lib.call with the operands' device made current: the C ABI launches on the calling thread's current HIP device, and
    the stream / pointers handed over belong to the tensors' device (MDX(processor=1), Config('cuda:1') never call
    torch.cuda.set_device)."""
    dev = getattr(_tls, "dev", None)
    if dev is not None and dev != torch.cuda.current_device():
        with torch.cuda.device(dev):
            return _lib.call(name, *args)
    return _lib.call(name, *args)


# ---------------------------------------------------------------------------------------------------
# Optional per-stage accounting for bench.py's `stages` list (HIP events on the launch stream around the wrapped ops)
# ---------------------------------------------------------------------------------------------------
class StageProfile:
    """name -> launches, algorithmic flops / bytes, HIP-event time.  Enabled with `ops.stage_profile = StageProfile()`."""

    def __init__(self):
        self.rec = {}

    def add(self, name, e0, e1, flops, nbytes):
        r = self.rec.setdefault(name, {"events": [], "flops": 0.0, "bytes": 0.0, "launches": 0})
        r["events"].append((e0, e1))
        r["flops"] += flops
        r["bytes"] += nbytes
        r["launches"] += 1

    def summary(self):
        torch.cuda.synchronize()
        return {name: {"launches": r["launches"], "ms": sum(a.elapsed_time(b) for a, b in r["events"]), "flops": r["flops"], "bytes": r["bytes"]}
                for name, r in self.rec.items()}


stage_profile = None


def _staged(name, work):
    """Decorator: a call is one launch of stage `name`, timed only while a profile is set and the first argument is a CUDA tensor.  work(args, kwargs, result) -> (flops, HBM bytes)."""
    def decorate(fn):
        @functools.wraps(fn)
        def wrapped(*a, **k):
            prof = stage_profile
            if prof is None or not (a and torch.is_tensor(a[0]) and a[0].is_cuda):
                return fn(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            prof.add(name, e0, e1, *work(a, k, r))
            return r
        return wrapped
    return decorate


def _numel(*ts):
    return float(sum(t.numel() for t in ts if t is not None))


# ---------------------------------------------------------------------------------------------------
# STFT / iSTFT
# ---------------------------------------------------------------------------------------------------
_fft_tables = {}


def fft_tables(n_fft, device, window=None):
    """(window, tw_half, tw_full) on `device`; twiddles are evaluated in float64 and rounded once."""
    key = (n_fft, str(device))
    if key not in _fft_tables:
        m = n_fft // 2
        k = np.arange(m, dtype=np.float64)
        th = np.exp(-2j * np.pi * k / m)
        k2 = np.arange(m + 1, dtype=np.float64)
        tf = np.exp(-2j * np.pi * k2 / n_fft)
        tw_half = torch.from_numpy(np.stack([th.real, th.imag], -1).astype(np.float32)).contiguous().to(device)
        tw_full = torch.from_numpy(np.stack([tf.real, tf.imag], -1).astype(np.float32)).contiguous().to(device)
        hann = torch.hann_window(n_fft, periodic=True, dtype=torch.float32).to(device)
        _fft_tables[key] = (hann, tw_half, tw_full)
    hann, tw_half, tw_full = _fft_tables[key]
    if window is None:
        window = hann
    return window, tw_half, tw_full


@_staged("stft", lambda a, k, r: (0.0, 4.0 * _numel(a[0], r)))
def stft(x, n_fft, hop, n_bins_out=None, frame_major=False, window=None):
    """x: (n_sig, L) fp32.  Returns the complex spectrogram split into planes:
    frame_major=False -> (n_sig, 2, n_bins_out, n_frames)  [torch.stft + view_as_real + permute layout]
    frame_major=True  -> (n_sig, 2, n_frames, n_bins_out)  [bins contiguous: coalesced stores]"""
    assert x.dim() == 2 and x.dtype == torch.float32
    x = x.contiguous()
    n_sig, L = x.shape
    n_frames = 1 + L // hop
    nb = n_fft // 2 + 1 if n_bins_out is None else n_bins_out
    window, tw_half, tw_full = fft_tables(n_fft, x.device, window)
    _check(x, window)
    if frame_major:
        out = torch.empty((n_sig, 2, n_frames, nb), dtype=torch.float32, device=x.device)
        o_bin, o_frame = 1, nb
    else:
        out = torch.empty((n_sig, 2, nb, n_frames), dtype=torch.float32, device=x.device)
        o_bin, o_frame = n_frames, 1
    _call("aicg_stft", _ptr(x), _ptr(out), _ptr(window), _ptr(tw_half), _ptr(tw_full), n_sig, L, n_fft, hop,
              n_frames, nb, 2 * nb * n_frames, nb * n_frames, o_bin, o_frame, _stream(x))
    return out


@_staged("istft", lambda a, k, r: (0.0, 4.0 * _numel(a[0], r)))
def istft(spec, n_fft, hop, length, frame_major=False, window=None):
    """spec: (n_sig, 2, n_bins_in, n_frames) (or (n_sig, 2, n_frames, n_bins_in) if frame_major);
    bins above n_bins_in are zero.  Returns (n_sig, length)."""
    assert spec.dim() == 4 and spec.shape[1] == 2 and spec.dtype == torch.float32
    spec = spec.contiguous()
    n_sig = spec.shape[0]
    if frame_major:
        n_frames, nb = spec.shape[2], spec.shape[3]
        i_bin, i_frame = 1, nb
    else:
        nb, n_frames = spec.shape[2], spec.shape[3]
        i_bin, i_frame = n_frames, 1
    window, tw_half, tw_full = fft_tables(n_fft, spec.device, window)
    _check(spec, window)
    frames = torch.empty((n_sig, n_frames, n_fft), dtype=torch.float32, device=spec.device)
    out = torch.empty((n_sig, length), dtype=torch.float32, device=spec.device)
    st = _stream(spec)
    _call("aicg_istft_frames", _ptr(spec), _ptr(frames), _ptr(window), _ptr(tw_half), _ptr(tw_full), n_sig,
              n_fft, n_frames, nb, 2 * nb * n_frames, nb * n_frames, i_bin, i_frame, st)
    _call("aicg_istft_ola", _ptr(frames), _ptr(window), _ptr(out), n_sig, length, n_fft, hop, n_frames, st)
    return out


# ---------------------------------------------------------------------------------------------------
# Convolution (implicit GEMM on fp32 MFMA)
# ---------------------------------------------------------------------------------------------------
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_GELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4, 5


class ConvDesc(ctypes.Structure):
    """Mirror of aicg_conv_desc (include/aicg.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in "N Cin H W Cout Ho Wo KH KW stride_h stride_w pad_h pad_w dil_h dil_w groups".split()] + \
               [(n, ctypes.c_int64) for n in "x_sn x_sc x_sh y_sn y_sc y_sh r_sn r_sc r_sh".split()] + \
               [(n, ctypes.c_float if n in ("pre_slope", "act_slope", "out_scale") else ctypes.c_int32) for n in
                "pre_act pre_slope act act_slope out_scale accumulate res_before_act pad_h_end pad_w_end shuffle res_mul packed_v3 split wino gemm_tile".split()]


def conv_bkc(taps):
    return _lib.get().aicg_conv_bkc(int(taps))


# Opt-in split precision for the convolution family (AICG_PRECISION=bf16x3; default fp32 on the fp32 MFMA): layers packed while
# this is set carry a third weight image and run csrc/conv_ws3s.h.  Read once at import; tests flip the module attribute.
split_precision = os.environ.get("AICG_PRECISION", "fp32").lower() in ("bf16x3", "split")


# Opt-in fp16 matrix arithmetic for the RVC half (AICG_HALF=1 AND the caller's is_half=True, i.e. what src/main.py:196 asks for and the
# reference runs in fp16 on a GPU, src/rvc.py:103-104,137-138): HubertModel.half() / Synthesizer.half() mark their layers (mark_half), and a
# marked layer that takes one of the LDS-DMA staged kernels (csrc/conv_g1.h, csrc/conv_g1w.h) rounds its operands to fp16 in registers in
# front of the MFMA -- fp32 activations in HBM, fp32 accumulation, fp32 epilogue.  The f0 models, SineGen and every layer on another
# kernel stay fp32.  Default (and the headline bench): off -- .half() is then the no-op it was.
def half_requested():
    return os.environ.get("AICG_HALF", "0") == "1"


def half_store_requested():
    """AICG_HALF=1 AND AICG_HALF_STORE=1: the vocoder's ResBlocks additionally keep their activations in fp16 in HBM on the stages routed
    to csrc/conv1d_h.hip (conv_h).  A variable of its own: a run that only asks for fp16 operands (AICG_HALF=1) stays as it is."""
    return half_requested() and os.environ.get("AICG_HALF_STORE", "0") == "1"


def mark_half(tree, on=True):
    """Set / clear the fp16-operand flag on every PackedConv reachable from `tree` (dicts, lists, tuples, PackedConvTranspose)."""
    if isinstance(tree, PackedConv):
        tree.f16 = bool(on) and not tree.fp32_only and not tree.split
    elif isinstance(tree, PackedConvTranspose):
        mark_half(tree.gemm, on)
    elif isinstance(tree, dict):
        for v in tree.values():
            mark_half(v, on)
    elif isinstance(tree, (list, tuple)):
        for v in tree:
            mark_half(v, on)


_fp32_depth = 0


@contextlib.contextmanager
def fp32_layers():
    """Layers packed inside this block stay on the fp32 MFMA whatever AICG_PRECISION says: the f0 estimators and the retrieval
    search select INDICES (pitch bins, neighbour ids), which are kept bit-exact (BASELINE north_star)."""
    global split_precision, _fp32_depth
    old, split_precision = split_precision, False
    _fp32_depth += 1
    try:
        yield
    finally:
        split_precision = old
        _fp32_depth -= 1


def fp32_only(fn):
    """Decorator form of fp32_layers for constructors."""
    @functools.wraps(fn)
    def wrapped(*a, **k):
        with fp32_layers():
            return fn(*a, **k)
    return wrapped


def _split_image(out):
    """(groups, taps, Cin_pad, Mpad) fp32 -> the bf16 hi / lo image [tap][Cin_pad/16][hi|lo][h][Mpad][8], as fp32 words."""
    g, taps, cpad, mpad = out.shape
    hi = out.to(torch.bfloat16)                       # round to nearest even
    lo = (out - hi.to(torch.float32)).to(torch.bfloat16)
    both = torch.stack([hi, lo], 0)                   # (part, g, taps, cpad, mpad)
    both = both.reshape(2, g, taps, cpad // 16, 2, 8, mpad).permute(1, 2, 3, 0, 4, 6, 5).contiguous()
    return both.view(torch.int16).reshape(-1).view(torch.float32)


def pack_conv_weight(w, groups=1, split=False):
    """(Cout, Cin/groups, KH, KW) -> two images back to back (pure re-layout + zero pad; Cin_pad and Mpad are multiples of
    32): per group [tap][Cin_pad][Mpad], then per group [tap][Cin_pad/8][2][Mpad][4] (aicg_conv_desc.packed_v3); with `split` a
    third one of the same size, the bf16 hi / lo pairs of aicg_conv_desc.split."""
    w = w.detach().to(torch.float32)
    cout, cin_g, kh, kw = w.shape
    taps = kh * kw
    cpad = (cin_g + 31) // 32 * 32
    cout_g = cout // groups
    mpad = (cout_g + 31) // 32 * 32
    out = torch.zeros((groups, taps, cpad, mpad), dtype=torch.float32, device=w.device)
    out[:, :, :cin_g, :cout_g] = w.reshape(groups, cout_g, cin_g, taps).permute(0, 3, 2, 1)
    # second image for the 16-byte-fragment kernels (csrc/conv_ws3.h): input channel ci = 8 q + 2 j + parity is element j of the
    # quad at [tap][q][parity][m]
    v3 = out.reshape(groups, taps, cpad // 8, 4, 2, mpad).permute(0, 1, 2, 4, 5, 3)
    parts = [out.reshape(-1), v3.reshape(-1)]
    if split:
        parts.append(_split_image(out))
    return torch.cat(parts).contiguous()


# Winograd F(2, 3) along rows for plain 3 x 3 layers (csrc/conv_ws3w.h): 12 instead of 18 MFMA contractions per output pair.  Layers
# packed while this is set carry the transformed kernel next to the direct one; conv() takes it where _winograd_applies.
# The f0 models (packed under fp32_layers()) never do: their goldens pin the direct summation order's bins.
winograd = _env.dev("AICG_WINOGRAD", "1") != "0"
winograd_min_positions = 32768   # below this the 64-column tiles (4 or 8 rows) do not fill the chip (tests lower it)


def winograd_kernel(w):
    """(Cout, Cin, 3, 3) -> (Cout, Cin, 3, 4): G g along the last axis, G = [[1, 0, 0], [1/2, 1/2, 1/2], [1/2, -1/2, 1/2], [0, 0, 1]]."""
    g0, g1, g2 = w[..., 0], w[..., 1], w[..., 2]
    return torch.stack([g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2], -1).contiguous()


def _aligned16(t4):   # 16-byte base address, batch and channel strides multiples of four floats
    sn, sc = t4.stride()[:2]
    return t4.data_ptr() % 16 == 0 and sn % 4 == 0 and sc % 4 == 0


def _winograd_applies(pc, r4, wo, positions, is1d, pre_act, act, out_scale, accumulate, shuffle, out_len):   # bias + none / ReLU epilogue, even rows, enough output
    return (pc.w_wino is not None and not is1d and r4 is None and not accumulate and pre_act == ACT_NONE and out_scale == 1.0
            and act in (ACT_NONE, ACT_RELU) and not shuffle and out_len is None and wo % 2 == 0 and positions >= winograd_min_positions)


# The two-dimensional form F(2 x 2, 3 x 3) (csrc/conv_w2d.h): 16 instead of 36 contractions per 2 x 2 output block, for layers whose
# output channels come in units of 48 (every MDX-Net level).  AICG_WINOGRAD=1 keeps the row-only form everywhere.
winograd2d = _env.dev("AICG_WINOGRAD", "2") == "2"
winograd2d_waves = int(_env.dev("AICG_W2D_WAVES", "8"))   # 8: two waves per SIMD on an 8 x 64 tile; 4: one per SIMD on 4 x 64
winograd2d_code = int(_env.dev("AICG_W2D_CODE", "0"))       # tools: a schedule variant under test (aicg_conv_desc.wino 6 ..)
winograd2d_quads = _env.dev("AICG_W2D_QUADS", "0") == "1"   # fragment image: [s][p / 4][ks][m][p % 4] (16-byte fragments)
# the eight-wave form reads PAIR fragments ([s][p / 2][ks][m][p % 2], one ds_read_b64 per two MFMAs: aicg_conv_desc.wino 12) unless
# AICG_W2D_PAIRS=0 (dword fragments, wino 2): 1-6 % faster on the five MDX-Net levels (profiles/r06_kbench_w2d_pairs.txt)
winograd2d_pairs = _env.dev("AICG_W2D_PAIRS", "1") != "0"


def _w2d_code():
    """aicg_conv_desc.wino of a layer on the two-dimensional form, and which image it reads ("dword" / "pairs" / "quads")."""
    code = winograd2d_code or ((4 if winograd2d_quads else 12 if winograd2d_pairs else 2) if winograd2d_waves == 8
                               else (5 if winograd2d_quads else 3))
    return code, ("pairs" if code in (12, 13, 14, 15, 16) else "quads" if code in (4, 5) else "dword")


def winograd2d_image(w, quads=False, pairs=False):
    """(Cout, Cin, 3, 3), Cout % 48 == 0 -> the image aicg_conv_desc.wino == 2 reads (include/aicg.h): U = G g G^T per (co, ci), laid out
    [Cout / 48][ceil(Cin / 8)][s][point 4 i + q][ks][m] with input channel 8 chunk + 4 s + ks (zero beyond Cin); `quads`:
    [Cout / 48][ceil(Cin / 8)][s][point / 4][ks][m][point % 4] (wino == 4 / 5)."""
    co, ci = w.shape[:2]
    assert co % 48 == 0 and tuple(w.shape[2:]) == (3, 3)
    G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device=w.device)
    U = torch.einsum("ia,ocab,jb->ocij", G, w.double(), G).to(torch.float32)          # exact: every factor is a power of two
    cpad = (ci + 7) // 8 * 8
    Up = torch.zeros((co, cpad, 16), dtype=torch.float32, device=w.device)
    Up[:, :ci] = U.reshape(co, ci, 16)
    if quads:
        return Up.view(co // 48, 48, cpad // 8, 2, 4, 4, 4).permute(0, 2, 3, 5, 4, 1, 6).contiguous().view(-1)
    if pairs:   # [Cout / 48][ceil(Cin / 8)][s][point / 2][ks][m][point % 2] (wino == 12)
        return Up.view(co // 48, 48, cpad // 8, 2, 4, 8, 2).permute(0, 2, 3, 5, 4, 1, 6).contiguous().view(-1)
    return Up.view(co // 48, 48, cpad // 8, 2, 4, 16).permute(0, 2, 3, 5, 4, 1).contiguous().view(-1)


def _winograd2d_applies(pc, x4, w):   # a call on the row form takes the two-dimensional one: the layer has it, the map is float4-aligned
    return winograd2d and pc.w_wino2 is not None and w % 4 == 0 and _aligned16(x4) and x4.stride(2) % 4 == 0


# One-dimensional Winograd F(2, 3) for the vocoder's k = 3 / 7 / 11 ResBlock layers, dilation 1 / 3 / 5 (csrc/conv_g1w.h): 4 / 10 / 15 products
# per output pair and input channel instead of 6 / 14 / 22.  Layers packed while this is set carry the slot image next to the direct one;
# conv() takes it where _winograd1d_applies.  The f0 models never do (fp32_layers()).
winograd1d = _env.dev("AICG_WINOGRAD1D", "1") != "0"
winograd1d_min_positions = int(_env.dev("AICG_WINOGRAD1D_MIN", "16384"))


def winograd1d_kernel(w):
    """(Cout, Cin, K), K in {3, 7, 11} -> (Cout, Cin, S) slot weights of csrc/conv_g1w.h, S = 4 / 10 / 15: per 3-tap group (g0, g1, g2)
    the four F(2, 3) weights (g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2); a remainder of two taps (a, b): (a, a + b, b); one tap a:
    (a, -a).  Sums in float64, rounded once."""
    k = w.shape[-1]
    assert k in (3, 5, 7, 11)
    wd = w.detach().double()
    slots = []
    for g in range(k // 3):
        g0, g1, g2 = wd[..., 3 * g], wd[..., 3 * g + 1], wd[..., 3 * g + 2]
        slots += [g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2]
    if k % 3 == 2:
        a, b = wd[..., k - 2], wd[..., k - 1]
        slots += [a, a + b, b]
    elif k % 3 == 1:
        a = wd[..., k - 1]
        slots += [a, -a]
    return torch.stack(slots, -1).to(torch.float32).contiguous()


def _winograd1d_applies(pc, x4, o4, r4, w, positions, is1d, pre_act, pre_slope, shuffle, res_mul, out_len):
    """The first line is ours alone: the switch, 16 output channels and more (fewer -- the vocoder's conv_post, 32 -> 1 -- are one HBM pass: the
    streaming kernels keep them), enough positions.  The rest is the other half of a contract with conv_g1w_applicable() (csrc/conv_g1w.h), in the
    order of its clauses (its layer clauses are what packs w_wino1): a call sent there that the library rejects is an error, not a fall-through."""
    return (winograd1d and pc.w_wino1 is not None and pc.cout >= 16 and positions >= winograd1d_min_positions
            and is1d and out_len is None and w % 4 == 0
            and pre_act in (ACT_NONE, ACT_LRELU) and 0.0 <= pre_slope <= 1.0
            and not shuffle and not res_mul and w < (1 << 24) and x4.stride(1) < (1 << 24) and x4.stride(1) >= w
            and _aligned16(x4) and _aligned16(o4) and (r4 is None or _aligned16(r4))
            and 15 * (-(-(pc.cin // pc.groups) // 32) * 32) * (-(-pc.cout // 32) * 32) * 4 < (1 << 31))


class PackedConv:
    """A convolution layer ready for aicg_conv_forward: packed weights + geometry.  1-D layers use KH=1."""

    def __init__(self, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, device=None, padding_end=None):
        self.padding_end = None if padding_end is None else (0, _one(padding_end)) if weight.dim() == 3 else _pair(padding_end)
        if weight.dim() == 3:  # Conv1d (Cout, Cin_g, K)
            weight = weight.unsqueeze(2)
            stride, padding, dilation = (1, _one(stride)), (0, _one(padding)), (1, _one(dilation))
        elif weight.dim() == 2:  # Linear (out, in)
            weight = weight[:, :, None, None]
            stride, padding, dilation = (1, 1), (0, 0), (1, 1)
        else:
            stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
        self.cout, cin_g, self.kh, self.kw = weight.shape
        self.cin, self.groups = cin_g * groups, groups
        self.stride, self.padding, self.dilation = stride, padding, dilation
        device = weight.device if device is None else device
        self.split = bool(split_precision)
        self.fp32_only = _fp32_depth > 0                    # packed inside fp32_layers(): never marked for fp16 operands
        self.f16 = False                                    # mark_half()
        w32 = weight.detach().to(device=device, dtype=torch.float32)    # the one fp32 device copy the packers share
        self.w = pack_conv_weight(w32, groups, self.split)
        self.bias = None if bias is None else bias.detach().to(device=device, dtype=torch.float32).contiguous()
        self.w_wino = self.w_wino2 = self.w_wino1 = None
        same_1d = (self.kh == 1 and self.kw in (3, 5, 7, 11) and stride == (1, 1) and padding == (0, (self.kw - 1) // 2 * dilation[1])
                   and self.padding_end is None and groups == 1)     # odd-k same-padded stride-1 one-group 1-D: the 1-D Winograd form, conv_h
        self._half = same_1d and not self.split and not self.fp32_only
        # images built on first use, by kind ("dword" / "pairs" / "quads": wino2_image, "half": conv_h_image), from the caller's own tensor (a reference, normally host memory)
        self._lazy_src, self._lazy_dev, self._lazy = weight.detach() if self._half else None, device, {}
        routed = not self.split and not _fp32_depth   # the Winograd forms: never for split-precision or fp32_layers() layers
        if winograd1d and routed and same_1d and dilation[1] in ((1, 3, 5) if self.kw != 5 else (1,)) and cin_g >= 16:
            # slot image of the 1-D Winograd form, packed like any k-tap kernel (slots in the taps' place): the matrix pipe is given 4 / 7 / 10 / 15
            # slots per output PAIR, not 2 k -- times 32 / 30 for the dilated layers' two idle lanes per tile
            self.w_wino1 = pack_conv_weight(winograd1d_kernel(w32[:, :, 0]).unsqueeze(2), 1, False)
            self._wino1_executed = {3: 4, 5: 7, 7: 10, 11: 15}[self.kw] / (2.0 * self.kw) * (1.0 if dilation[1] == 1 else 32.0 / 30.0)
        if (winograd and routed and (self.kh, self.kw) == (3, 3) and stride == (1, 1) and dilation == (1, 1)
                and padding == (1, 1) and self.padding_end is None and groups == 1 and cin_g >= 8):
            self.w_wino = pack_conv_weight(winograd_kernel(w32), 1, False)
            if winograd2d and self.cout % 48 == 0:
                # ONE image on the device, the one the routed kernel reads (_w2d_code()); the other layouts (16/9 of the weights each) are for the dev switches / A-B tools
                self._lazy_src = weight.detach()
                self.w_wino2 = self.wino2_image(_w2d_code()[1])

    def conv_h_supported(self):
        """This layer has a half-storage form (aicg_conv1d_h_supported; never for fp32_only or split-precision layers)."""
        return self._half and bool(_lib.get().aicg_conv1d_h_supported(self.cin, self.cout, self.kw, self.dilation[1]))

    def conv_h_image(self):
        """aicg_conv1d_h's w_packed: fp16 (round to nearest even) [Cout_pad / 32][Cin / 8][k][2][32][4], built on first use."""
        if "half" not in self._lazy:
            assert self.conv_h_supported(), "conv_h: layer has no half-storage form"
            w = self._lazy_src.to(device=self._lazy_dev, dtype=torch.float32)[:, :, 0]
            cout, cin, k = w.shape
            cpad = 32 if cout <= 32 else -(-cout // 64) * 64
            wp = torch.zeros(cpad, cin, k, dtype=torch.float32, device=w.device)
            wp[:cout] = w
            # (m, i, g, h, e, tap) -> (m, g, tap, h, i, e)
            self._lazy["half"] = wp.reshape(cpad // 32, 32, cin // 8, 2, 4, k).permute(0, 2, 5, 3, 1, 4).contiguous().half()
        return self._lazy["half"]

    def wino2_image(self, kind):
        """The F(2 x 2, 3 x 3) weight image with "dword" / "pairs" / "quads" fragments (winograd2d_image)."""
        if kind not in self._lazy:
            self._lazy[kind] = winograd2d_image(self._lazy_src.to(device=self._lazy_dev, dtype=torch.float32), quads=kind == "quads", pairs=kind == "pairs")
        return self._lazy[kind]

    def out_hw(self, h, w):
        pe = self.padding if self.padding_end is None else self.padding_end
        ho = (h + self.padding[0] + pe[0] - self.dilation[0] * (self.kh - 1) - 1) // self.stride[0] + 1
        wo = (w + self.padding[1] + pe[1] - self.dilation[1] * (self.kw - 1) - 1) // self.stride[1] + 1
        return ho, wo


def _one(v):
    return int(v[0]) if isinstance(v, (tuple, list)) else int(v)


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _as4d(t):
    return t.unsqueeze(2) if t.dim() == 3 else t


class ConvProfile:
    """Optional per-launch accounting of the conv kernel (bench.py roofline): algorithmic FLOPs and HIP-event time of
    every aicg_conv_forward launch on the current stream.  Enabled with `ops.conv_profile = ConvProfile()`."""

    def __init__(self):
        self.events = []
        self.flops = 0.0
        self.flops_executed = 0.0  # what the matrix pipe was given (the Winograd forms execute fewer multiply-adds than the direct form)
        self.bytes = 0.0  # algorithmic HBM bytes: input + packed weights + output (+ residual / accumulate reads), each once
        self.launches = 0
        self.shapes = []  # per launch: (shape key, flops) -- by_shape() groups them

    def record(self, e0, e1, pc, x4, ho, wo, residual, accumulate, shuffle, form):
        """One launch of conv(): its event pair, the layer, the input view, the map computed, the epilogue's reads, the form taken."""
        n, c, h, w = x4.shape
        weights = pc.cout * (pc.cin // pc.groups) * pc.kh * pc.kw
        flops = 2.0 * n * weights * ho * wo
        self.events.append((e0, e1))
        self.flops += flops
        self.flops_executed += flops * form.executed
        self.bytes += 4.0 * (n * c * h * w + weights + n * pc.cout * ho * wo * (1 + bool(residual) + bool(accumulate)))
        self.launches += 1
        self.shapes.append(("N%d C%d>%d %dx%d k%dx%d s%d,%d d%d,%d g%d%s%s%s" % (
            n, c, pc.cout, h, w, pc.kh, pc.kw, pc.stride[0], pc.stride[1], pc.dilation[0], pc.dilation[1], pc.groups,
            " res" if residual else "", " acc" if accumulate else "", (" shuf" if shuffle else "") + form.label), flops))

    def by_shape(self):
        """[{shape, launches, ms, tflops, gflop}] sorted by time: where the family's time goes (bench.py --conv-shapes)."""
        torch.cuda.synchronize()
        agg = {}
        for (key, fl), (a, b) in zip(self.shapes, self.events):
            r = agg.setdefault(key, [0, 0.0, 0.0])
            r[0] += 1
            r[1] += a.elapsed_time(b)
            r[2] += fl
        rows = [{"shape": k, "launches": v[0], "ms": v[1], "gflop": v[2] / 1e9, "tflops": v[2] / (v[1] * 1e-3) / 1e12 if v[1] > 0 else 0.0}
                for k, v in agg.items()]
        return sorted(rows, key=lambda r: -r["ms"])

    def summary(self):
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for a, b in self.events)
        return {"launches": self.launches, "flops": self.flops, "flops_executed": self.flops_executed, "ms": ms, "bytes": self.bytes,
                "tflops": (self.flops / (ms * 1e-3) / 1e12) if ms > 0 else 0.0,
                "tflops_executed": (self.flops_executed / (ms * 1e-3) / 1e12) if ms > 0 else 0.0}


conv_profile = None
gemm_tile = 0   # tools: aicg_conv_desc.gemm_tile of every launch (0 = the library's policy; 1 keeps 1 x 1 layers off csrc/conv_g1.h; 2 / 3 / 4 force a tile)
# the form of one conv() call: aicg_conv_desc.wino, the image that code reads, the share of the direct form's multiply-adds executed, the shape key's suffix
_ConvForm = namedtuple("_ConvForm", "wino image executed label")


def _conv_form(pc, x4, o4, r4, w, wo, positions, gate_positions, is1d, pre_act, pre_slope, act, out_scale, accumulate, shuffle, res_mul, out_len):
    if _winograd_applies(pc, r4, wo, positions, is1d, pre_act, act, out_scale, accumulate, shuffle, out_len):
        if _winograd2d_applies(pc, x4, w):
            code, kind = _w2d_code()
            return _ConvForm(code, pc.wino2_image(kind), 4.0 / 9.0, " wino2")    # F(2 x 2, 3 x 3): 16 of 36 multiply-adds
        return _ConvForm(1, pc.w_wino, 2.0 / 3.0, " wino")                       # the row form: 12 of 18
    if _winograd1d_applies(pc, x4, o4, r4, w, gate_positions, is1d, pre_act, pre_slope, shuffle, res_mul, out_len):
        return _ConvForm(8, pc.w_wino1, pc._wino1_executed, " wino1d")
    return _ConvForm(0, pc.w, 1.0, "")


def _conv_desc(pc, x4, o4, r4, ho, wo, pre_act, pre_slope, act, act_slope, out_scale, accumulate, res_before_act, shuffle, res_mul, wino):
    d = ConvDesc()
    d.N, d.Cin, d.H, d.W = x4.shape
    d.Cout, d.Ho, d.Wo, d.KH, d.KW, d.groups = pc.cout, ho, wo, pc.kh, pc.kw, pc.groups
    (d.stride_h, d.stride_w), (d.pad_h, d.pad_w), (d.dil_h, d.dil_w) = pc.stride, pc.padding, pc.dilation
    d.x_sn, d.x_sc, d.x_sh, _ = x4.stride()
    d.y_sn, d.y_sc, d.y_sh, _ = o4.stride()
    if r4 is not None:
        d.r_sn, d.r_sc, d.r_sh, _ = r4.stride()
    d.pre_act, d.pre_slope, d.act, d.act_slope, d.out_scale = pre_act, pre_slope, act, act_slope, out_scale
    d.accumulate, d.res_before_act, d.res_mul = 1 if accumulate else 0, 1 if res_before_act else 0, 1 if res_mul else 0
    d.pad_h_end, d.pad_w_end = (-1, -1) if pc.padding_end is None else pc.padding_end
    d.shuffle, d.packed_v3, d.split, d.wino, d.gemm_tile = int(shuffle), 1, 1 if pc.split else 2 if pc.f16 else 0, wino, gemm_tile
    return d


def conv(x, pc, res=None, out=None, pre_act=ACT_NONE, pre_slope=0.0, act=ACT_NONE, act_slope=0.0, out_scale=1.0,
         accumulate=False, bias=None, res_before_act=False, out_len=None, shuffle=0, res_mul=False, plan_w=None):
    """y = [y +] out_scale * (act(conv(pre_act(x)) + bias) + res).  x: (N,C,T) or (N,C,H,W), last dim contiguous;
    views with arbitrary batch/channel/row strides are accepted for x, res and out.
    `plan_w`: x is a window of a row of plan_w columns (the windowed vocoder) -- every size gate here and every tile policy of the
    library counts with plan_w (aicg_conv_forward_planned), so that the window runs the kernel and tile of the uncropped layer."""
    is1d = x.dim() == 3
    x4 = _as4d(x)
    n, c, h, w = x4.shape
    assert c == pc.cin, "conv: input has %d channels, layer expects %d" % (c, pc.cin)
    assert x4.stride(3) == 1 or w == 1
    # the kernels' range-checked buffer loads bound a channel chunk by its channel stride: a channel's rows must lie inside it
    assert h == 1 or c == 1 or x4.stride(1) >= x4.stride(2) * (h - 1) + w, "conv: input rows must lie inside the channel stride"
    assert plan_w is None or plan_w >= w
    gate_w = w if plan_w is None else int(plan_w)
    ho, wo = pc.out_hw(h, w)
    if out_len is not None:  # compute only the first out_len columns (e.g. SamePad of an even kernel)
        assert out_len <= wo
        wo = out_len
    # shuffle = 2: this is the GEMM of a kernel = stride = 2 ConvTranspose2d and the epilogue scatters row m of position
    # (ho, wo) to out[m >> 2][2 ho + ((m >> 1) & 1)][2 wo + (m & 1)] (see conv_transpose)
    oshape = (n, pc.cout // 4, 2 * ho, 2 * wo) if shuffle else (n, pc.cout, ho, wo)
    if out is None:
        out = torch.empty((n, pc.cout, wo) if is1d else oshape, dtype=torch.float32, device=x.device)
        assert not accumulate
    o4 = _as4d(out)
    assert o4.shape == oshape, (o4.shape, oshape)
    assert o4.stride(3) == 1 or wo == 1
    r4 = None if res is None else _as4d(res)
    assert r4 is None or (r4.shape == o4.shape and (r4.stride(3) == 1 or wo == 1))
    b = pc.bias if bias is None else bias
    if o4.numel() == 0:  # empty batch / no output positions: nothing to launch (empty tensors have no storage to point at)
        return out
    _check(x, out, res, pc.w, b)
    form = _conv_form(pc, x4, o4, r4, w, wo, n * ho * wo, n * gate_w, is1d, pre_act, pre_slope, act, out_scale, accumulate, shuffle, res_mul, out_len)
    d = _conv_desc(pc, x4, o4, r4, ho, wo, pre_act, pre_slope, act, act_slope, out_scale, accumulate, res_before_act, shuffle, res_mul, form.wino)
    prof = conv_profile
    timed = prof is not None and x.is_cuda
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    if plan_w is None:
        _call("aicg_conv_forward", ctypes.addressof(d), _ptr(x4), _ptr(form.image), _ptr(b), _ptr(r4), _ptr(o4), _stream(x))
    else:
        _call("aicg_conv_forward_planned", ctypes.addressof(d), _ptr(x4), _ptr(form.image), _ptr(b), _ptr(r4), _ptr(o4), gate_w, _stream(x))
    if timed:
        e1.record()
        prof.record(e0, e1, pc, x4, ho, wo, r4 is not None, accumulate, shuffle, form)
    return out


def conv_h(x, pc, res=None, out=None, out_dtype=torch.float16, pre_act=ACT_NONE, pre_slope=0.0, act=ACT_NONE, act_slope=0.0,
           out_scale=1.0, accumulate=False):
    """conv's formula, y = [y +] out_scale * (act(conv(pre_act(x)) + bias) + res), on the half-storage kernel (csrc/conv1d_h.hip):
    x, res and out (N, C, T), last dim contiguous, are each fp16 or fp32; a new output is allocated as `out_dtype`.  Products on the
    fp16 matrix pipe, everything else fp32, one rounding at an fp16 store."""
    assert x.dim() == 3 and x.shape[1] == pc.cin, "conv_h: input (N, %d, T) expected, got %s" % (pc.cin, tuple(x.shape))
    n, c, t = x.shape
    for name, a in (("x", x), ("res", res), ("out", out)):
        assert a is None or a.dtype in (torch.float16, torch.float32), "conv_h: %s is %s" % (name, a.dtype)
        assert a is None or a.stride(2) == 1 or t == 1, "conv_h: %s rows must be contiguous" % name
    if out is None:
        assert not accumulate
        out = torch.empty((n, pc.cout, t), dtype=out_dtype, device=x.device)
    assert tuple(out.shape) == (n, pc.cout, t), (tuple(out.shape), (n, pc.cout, t))
    assert res is None or res.shape == out.shape
    if out.numel() == 0:
        return out
    if not pc.conv_h_supported():    # the library's message, without a launch
        _check(x, out, res, pc.bias)
        _call("aicg_conv1d_h", _ptr(x), 0, _ptr(pc.bias), _ptr(res), _ptr(out), n, c, pc.cout, t, pc.kw, pc.dilation[1], 0, 0, 0,
              0, 0, 0, 0, 0, 0, pre_act, pre_slope, act, act_slope, out_scale, 0, _stream(x))
    w = pc.conv_h_image()
    _check(x, out, res, w, pc.bias)
    h = lambda a: int(a is not None and a.dtype == torch.float16)
    _call("aicg_conv1d_h", _ptr(x), _ptr(w), _ptr(pc.bias), _ptr(res), _ptr(out), n, c, pc.cout, t, pc.kw, pc.dilation[1],
          h(x), h(res), h(out), x.stride(0), x.stride(1), 0 if res is None else res.stride(0), 0 if res is None else res.stride(1),
          out.stride(0), out.stride(1), pre_act, pre_slope, act, act_slope, out_scale, 1 if accumulate else 0, _stream(x))
    return out


# ---------------------------------------------------------------------------------------------------
# Transposed convolution = 1x1 GEMM (aicg_conv_forward) + gather (aicg_col2im)
# ---------------------------------------------------------------------------------------------------
class PackedConvTranspose:
    """ConvTranspose1d/2d weights (Cin, Cout, K) / (Cin, Cout, KH, KW) re-laid-out as the (Cout*KH*KW, Cin)
    matrix of the 1x1 GEMM; `bias` is applied by col2im."""

    def __init__(self, weight, bias=None, stride=1, padding=0, output_padding=0, device=None):
        if weight.dim() == 3:
            weight = weight.unsqueeze(2)
            stride, padding, output_padding = (1, _one(stride)), (0, _one(padding)), (0, _one(output_padding))
        else:
            stride, padding, output_padding = _pair(stride), _pair(padding), _pair(output_padding)
        self.cin, self.cout, self.kh, self.kw = weight.shape
        self.stride, self.padding, self.output_padding = stride, padding, output_padding
        device = weight.device if device is None else device
        gemm_w = weight.detach().permute(1, 2, 3, 0).reshape(self.cout * self.kh * self.kw, self.cin)
        self.gemm = PackedConv(gemm_w.contiguous(), None, device=device)
        self.bias = None if bias is None else bias.detach().to(device=device, dtype=torch.float32).contiguous()
        # per-GEMM-row bias for the fused kernel = stride = 2 form (row = co * 4 + tap)
        self.bias4 = None if self.bias is None else self.bias.repeat_interleave(self.kh * self.kw).contiguous()

    def out_hw(self, h, w):
        ho = (h - 1) * self.stride[0] - 2 * self.padding[0] + self.kh + self.output_padding[0]
        wo = (w - 1) * self.stride[1] - 2 * self.padding[1] + self.kw + self.output_padding[1]
        return ho, wo


def mul(a, b, out=None):
    assert a.is_contiguous() and b.is_contiguous() and a.shape == b.shape
    if out is None:
        out = torch.empty_like(a)
    _check(a, b, out)
    _call("aicg_mul", _ptr(a), _ptr(b), _ptr(out), a.numel(), _stream(a))
    return out


_mul = mul   # conv_transpose's `mul` parameter shadows the function


def conv_transpose(x, pt, out=None, add=None, pre_act=ACT_NONE, pre_slope=0.0, act=ACT_NONE, act_slope=0.0, mul=None, plan_w=None):
    """y = act(conv_transpose(pre_act(x)) + bias) + add   (or ... * mul: the MDX U-Net's multiplicative skip).
    `plan_w`: as in conv() -- the row length x was cut from (1-D layers)."""
    is1d = x.dim() == 3
    x4 = _as4d(x)
    n, c, h, w = x4.shape
    assert add is None or mul is None
    if (not is1d and (pt.kh, pt.kw) == (2, 2) and pt.stride == (2, 2) and pt.padding == (0, 0)
            and pt.output_padding == (0, 0)):
        # non-overlapping taps: every output element is one GEMM element -> scatter + bias + act + skip in the GEMM epilogue
        return conv(x4, pt.gemm, res=add if mul is None else mul, out=out, pre_act=pre_act, pre_slope=pre_slope, act=act,
                    act_slope=act_slope, bias=pt.bias4, shuffle=2, res_mul=mul is not None)
    cols = conv(x4, pt.gemm, pre_act=pre_act, pre_slope=pre_slope, plan_w=plan_w)  # (N, Cout*KH*KW, H, W)
    ho, wo = pt.out_hw(h, w)
    if out is None:
        out = torch.empty((n, pt.cout, wo) if is1d else (n, pt.cout, ho, wo), dtype=torch.float32, device=x.device)
    o4 = _as4d(out)
    assert o4.shape == (n, pt.cout, ho, wo) and (o4.stride(3) == 1 or wo == 1)
    a4 = None if add is None else _as4d(add)
    if a4 is not None:
        assert a4.shape == o4.shape and (a4.stride(3) == 1 or wo == 1)
    _check(cols, out, add, pt.bias)
    asn, asc, ash = (a4.stride(0), a4.stride(1), a4.stride(2)) if a4 is not None else (0, 0, 0)
    _call("aicg_col2im", _ptr(cols), _ptr(pt.bias), _ptr(a4), _ptr(o4), n, pt.cout, h, w, ho, wo, pt.kh, pt.kw,
              pt.stride[0], pt.stride[1], pt.padding[0], pt.padding[1], act, act_slope,
              o4.stride(0), o4.stride(1), o4.stride(2), asn, asc, ash, _stream(x))
    if mul is not None:
        _mul(out, mul, out=out)
    return out


# ---------------------------------------------------------------------------------------------------
# Synthesizer helpers
# ---------------------------------------------------------------------------------------------------
@_staged("sine_source", lambda a, k, r: (0.0, 4.0 * _numel(a[0], a[1], r)))
def sine_source(f0, noise, upp, sr, lin_w, lin_b, sine_amp=0.1, noise_std=0.003):
    """f0: (T,) Hz; noise: (T*upp,) N(0,1) draws -> harmonic source (T*upp,) after l_linear + tanh."""
    f0 = f0.contiguous().float()
    noise = noise.contiguous().float()
    t = f0.numel()
    assert noise.numel() == t * upp
    _check(f0, noise)
    prefix = torch.empty(t, dtype=torch.float64, device=f0.device)
    out = torch.empty(t * upp, dtype=torch.float32, device=f0.device)
    _call("aicg_sine_source", _ptr(f0), _ptr(noise), _ptr(prefix), _ptr(out), t, int(upp), float(sr), sine_amp,
              noise_std, float(lin_w), float(lin_b), _stream(f0))
    return out


@_staged("sine_source", lambda a, k, r: (0.0, 4.0 * _numel(a[0], r, r)))
def sine_source_window(f0, noise, upp, sr, lin_w, lin_b, first, count, sine_amp=0.1, noise_std=0.003):
    """Samples first .. first + count - 1 of sine_source(f0, noise, ...) -- the same bits: the phase is integrated from frame 0 and sample
    n reads noise[n] of the full-length draw --, zero where that index lies outside the signal (first may be negative: the zero
    padding of the vocoder's noise convolutions).  Only the window is written."""
    f0 = f0.contiguous().float()
    noise = noise.contiguous().float()
    t = f0.numel()
    first, count = int(first), int(count)
    assert noise.numel() == t * upp and count >= 0
    _check(f0, noise)
    # the library cuts a source it generates in quads (upp % 4 == 0) on quads: ask for the enclosing quads, return the slice
    lead = first % 4 if upp % 4 == 0 else 0
    n = -(-(lead + count) // 4) * 4 if upp % 4 == 0 else count
    prefix = torch.empty(max(t, 1), dtype=torch.float64, device=f0.device)
    out = torch.empty(n, dtype=torch.float32, device=f0.device)
    _call("aicg_sine_source_window", _ptr(f0), _ptr(noise), _ptr(prefix), _ptr(out), t, int(upp), float(sr), sine_amp,
              noise_std, float(lin_w), float(lin_b), first - lead, n, _stream(f0))
    return out[lead: lead + count]


def gate_tanh_sigmoid(a, out=None):
    """a: (N, 2C, T) contiguous -> tanh(a[:, :C]) * sigmoid(a[:, C:])."""
    assert a.is_contiguous() and a.dim() == 3 and a.shape[1] % 2 == 0
    n, c2, t = a.shape
    if out is None:
        out = torch.empty((n, c2 // 2, t), dtype=torch.float32, device=a.device)
    assert out.is_contiguous()
    _check(a, out)
    _call("aicg_gate_tanh_sigmoid", _ptr(a), _ptr(out), n, c2 // 2, t, _stream(a))
    return out


def prior_sample(stats, noise, scale):
    """stats: (1, 2C, T) = [m; logs]; noise (1, C, T) -> m + exp(logs) * noise * scale."""
    assert stats.is_contiguous() and noise.is_contiguous() and stats.shape[0] == 1
    c, t = noise.shape[1], noise.shape[2]
    assert stats.shape[1] == 2 * c and stats.shape[2] == t
    out = torch.empty_like(noise)
    _check(stats, noise)
    _call("aicg_prior_sample", _ptr(stats), _ptr(noise), _ptr(out), c, t, float(scale), _stream(stats))
    return out


def feats_prepare(feats, t_out, feats0=None, pitchf=None, protect=0.5):
    """(Th, C) token-major features -> (1, C, t_out) channel-major, nearest x2 upsampled, protect-blended."""
    feats = feats.contiguous()
    th, c = feats.shape
    out = torch.empty((1, c, t_out), dtype=torch.float32, device=feats.device)
    if feats0 is not None:
        feats0 = feats0.contiguous()
        pitchf = pitchf.contiguous().float()
        assert pitchf.numel() >= t_out
    _check(feats, feats0, pitchf)
    _call("aicg_feats_prepare", _ptr(feats), _ptr(feats0), _ptr(pitchf), _ptr(out), th, c, int(t_out), float(protect),
              _stream(feats))
    return out


@_staged("layernorm", lambda a, k, r: (0.0, 4.0 * _numel(a[0], k.get("res"), r)))
def layernorm_ct(x, gamma, beta, res=None, out=None, eps=1e-5):
    """LayerNorm over channels of contiguous (N, C, T); out = LN(x + res)."""
    assert x.is_contiguous() and x.dim() == 3
    n, c, t = x.shape
    if out is None:
        out = torch.empty_like(x)
    if res is not None:
        assert res.is_contiguous() and res.shape == x.shape
    _check(x, res, gamma, beta, out)
    _call("aicg_layernorm_ct", _ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(out), n, c, t, float(eps), c * t, c * t,
              c * t, _stream(x))
    return out


@_staged("groupnorm_gelu", lambda a, k, r: (0.0, 4.0 * _numel(a[0], r)))
def rownorm_act(x, gamma, beta, act=ACT_NONE, eps=1e-5, out=None):
    """x: (rows, T), unit stride along T: per-row (x - mean)/sqrt(var + eps) * gamma + beta, then act.  x (and out) may be views of rows
    padded to a common stride (x.stride(0) >= T); `out` defaults to a buffer laid out like x.  The padding is neither read nor written.
    Layout and bits: rows shorter than 4096 give the same bits for every stride.  Longer rows take the split form, which cuts a row into
    head scalars, a 16-byte-aligned float4 body and tail scalars by the row's address and merges the parts' moments in that order, so
    a row gives the same bits under two strides only where (row * stride) % 4 agrees; otherwise the two results differ by the fp32
    rounding of the moment merge (each within the kernel's error against float64; tests/test_rownorm_padded.py)."""
    assert x.dim() == 2 and (x.stride(1) == 1 or x.shape[1] == 1)
    rows, t = x.shape
    ld = x.stride(0) if rows > 1 else max(x.stride(0), t)
    if out is None:
        out = torch.empty((rows, ld), dtype=torch.float32, device=x.device)[:, :t] if ld != t else torch.empty_like(x)
    assert out.shape == x.shape and (out.stride(1) == 1 or t == 1) and (rows <= 1 or out.stride(0) == ld)
    _check(x, gamma, beta, out)
    need = ctypes.c_int64(0)
    _call("aicg_rownorm_act_workspace_floats", rows, t, ctypes.addressof(need))
    ws = torch.empty(need.value, dtype=torch.float32, device=x.device) if need.value else None
    _call("aicg_rownorm_act_ld", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), rows, t, ld, float(eps), act, _ptr(ws), _stream(x))
    return out


@_staged("attention", lambda a, k, r: (4.0 * a[0].numel() * a[0].shape[1], 4.0 * _numel(a[0], a[1], a[2], r)))      # 4 T^2 D per head
def attention(q, k, v, n_heads, relk=None, relv_emb=None, window=0, scale=1.0, n_splits=None):
    """q, k, v: (C, T) channel-major (rows may be slices of a fused QKV buffer; stride(1) == 1).
    relk: (H, 2w+1, T) precomputed q.E^k (or None); relv_emb: (2w+1, D) for the relative value term."""
    c, t = q.shape
    d = c // n_heads
    assert q.stride(1) == 1 and k.stride(1) == 1 and v.stride(1) == 1
    o = torch.empty((c, t), dtype=torch.float32, device=q.device)
    lse = torch.empty((n_heads, t), dtype=torch.float32, device=q.device) if relv_emb is not None else None
    if relk is not None:
        assert relk.is_contiguous() and relk.shape == (n_heads, 2 * window + 1, t)
    _check(q, k, v, relk, relv_emb)
    st = _stream(q)
    # (query block, head) pairs alone do not fill 256 CUs for a few heads: split the keys until ~1024 workgroups exist
    blocks = -(-t // 128) * n_heads
    # (> 4: the merge pass costs more than it fills; HuBERT's 312 blocks, round-5 kernel: 4 splits 0.353 ms, 3 0.361, 2 0.398, 8 0.377)
    splits = max(1, min(4, -(-t // 32), -(-1024 // blocks))) if n_splits is None else n_splits
    if splits > 1:
        scratch = torch.empty(splits * n_heads * (d + 2) * t, dtype=torch.float32, device=q.device)
        _call("aicg_attention_split", _ptr(q), _ptr(k), _ptr(v), _ptr(relk), _ptr(o), _ptr(lse), t, n_heads, d, window,
                  q.stride(0), k.stride(0), v.stride(0), o.stride(0), float(scale), splits, _ptr(scratch), st)
    else:
        _call("aicg_attention", _ptr(q), _ptr(k), _ptr(v), _ptr(relk), _ptr(o), _ptr(lse), t, n_heads, d, window,
                  q.stride(0), k.stride(0), v.stride(0), o.stride(0), float(scale), st)
    if relv_emb is not None:
        relv_emb = relv_emb.contiguous()
        _call("aicg_attention_relv", _ptr(q), _ptr(k), _ptr(relk), _ptr(relv_emb), _ptr(lse), _ptr(o), t, n_heads, d,
                  window, q.stride(0), k.stride(0), o.stride(0), float(scale), st)
    return o


# ---------------------------------------------------------------------------------------------------
# RMVPE helpers
# ---------------------------------------------------------------------------------------------------
ACT_LOGCLAMP = 6


def complex_abs(re, im):
    assert re.is_contiguous() and im.is_contiguous() and re.shape == im.shape
    out = torch.empty_like(re)
    _check(re, im)
    _call("aicg_complex_abs", _ptr(re), _ptr(im), _ptr(out), re.numel(), _stream(re))
    return out


def channel_affine(x, scale, shift, act=ACT_NONE):
    assert x.is_contiguous() and x.dim() >= 2
    n, c = x.shape[0], x.shape[1]
    hw = x.numel() // (n * c)
    out = torch.empty_like(x)
    _check(x, scale, shift)
    _call("aicg_channel_affine", _ptr(x), _ptr(scale), _ptr(shift), _ptr(out), n, c, hw, act, _stream(x))
    return out


def avgpool2x2(x):
    n, c, h, w = x.shape
    assert x.stride(3) == 1
    out = torch.empty((n, c, h // 2, w // 2), dtype=torch.float32, device=x.device)
    _check(x)
    _call("aicg_avgpool2x2", _ptr(x), _ptr(out), n, c, h, w, x.stride(0), x.stride(1), x.stride(2), _stream(x))
    return out


GRU_TWO_WORKGROUPS = _env.dev("AICG_GRU_2WG", "1") != "0"     # "0": the single-workgroup kernel (no co-residency needed)
GRU_WORKGROUPS = int(_env.dev("AICG_GRU_WG", "4"))             # workgroups per direction of the multi-workgroup form: 4 or 2


_gru_pending = []


def gru_timed_out():
    """True if any multi-workgroup GRU launch since the last call reported a partner-exchange timeout (the partner workgroup
    was not co-resident in time: a busy or shared GPU).  Call after the stream that ran them has been drained.  The result
    of such a launch is invalid; callers recompute with the single-workgroup kernel (`gru_bidir(two_workgroups=False)`)."""
    pend, _gru_pending[:] = list(_gru_pending), []     # (the tensor references of the launches go with the list)
    bad = False
    for f, _ in pend:
        bad = bad or int(f.item()) != 0
    return bad


def gru_check_pending():
    """Raise if a multi-workgroup GRU launch timed out (for callers that cannot recompute)."""
    if gru_timed_out():
        raise RuntimeError("aicg_gru_bidir_2wg: partner workgroup exchange timed out")


def _gru_repair_backlog():
    """A caller that never polls gru_timed_out(): bound the backlog (this synchronises) and REPAIR instead of failing -- every pending
    launch whose flag is set is recomputed by the single-workgroup kernel into the same output tensor, on the stream that is current
    NOW.  The repair fixes `out` for LATER readers only: anything already derived from a flagged output (classifier, decode) stays
    wrong and is not re-run -- which is why a flagged launch is also reported (warning), and why callers that can recompute their
    dependants should poll gru_timed_out() themselves, as pipeline() and RMVPE.infer_from_audio do."""
    import warnings
    pend, _gru_pending[:] = list(_gru_pending), []
    for f, (gi, whh_t, bhh, out, hidden) in pend:
        if int(f.item()) != 0:
            warnings.warn("aicg_gru_bidir: a multi-workgroup launch timed out %d launches ago and nobody polled gru_timed_out(); its "
                          "output is recomputed in place now -- results already derived from it are stale" % len(pend))
            _call("aicg_gru_bidir", _ptr(gi), _ptr(whh_t), _ptr(bhh), _ptr(out), hidden, gi.shape[1], _stream(gi))


def gru_bidir(gi, whh_t, bhh, hidden, two_workgroups=None):
    """gi: (6*hidden, T) channel-major input projections -> (2*hidden, T).  Default: the multi-workgroup-per-direction
    kernel (all of W_hh on chip); `two_workgroups=False` (or AICG_GRU_2WG=0) selects the single-workgroup kernel.
    The multi-workgroup kernels need their workgroups co-resident; a launch that timed out waiting for a partner sets a flag that
    pipeline() polls with gru_timed_out() (and recomputes).  Callers that never poll are covered too: once 16 launches are
    pending, the flagged ones are recomputed in place by the single-workgroup kernel (_gru_repair_backlog)."""
    assert gi.is_contiguous() and gi.shape[0] == 6 * hidden
    t = gi.shape[1]
    out = torch.empty((2 * hidden, t), dtype=torch.float32, device=gi.device)
    _check(gi, whh_t, bhh)
    if GRU_TWO_WORKGROUPS if two_workgroups is None else two_workgroups:
        scratch = torch.empty(32 * hidden + 64, dtype=torch.uint8, device=gi.device)
        # hidden 256 (every RMVPE): four workgroups per direction, all of W_hh in registers; other sizes: two (part of it in LDS)
        _call("aicg_gru_bidir_4wg" if hidden == 256 and GRU_WORKGROUPS == 4 else "aicg_gru_bidir_2wg", _ptr(gi), _ptr(whh_t), _ptr(bhh),
              _ptr(out), hidden, t, _ptr(scratch), _stream(gi))
        # the kernel's exchange-timeout flag is read back lazily (gru_timed_out): an .item() here would park the host
        # until the recurrence ends, which is exactly the time pipeline() wants to spend queueing HuBERT work
        _gru_pending.append((scratch[32 * hidden: 32 * hidden + 4].view(torch.int32), (gi, whh_t, bhh, out, hidden)))
        if len(_gru_pending) > 16:
            _gru_repair_backlog()
        return out
    _call("aicg_gru_bidir", _ptr(gi), _ptr(whh_t), _ptr(bhh), _ptr(out), hidden, t, _stream(gi))
    return out


class GruSegments:
    """The BiGRU recurrence of gru_bidir cut into segments of steps (aicg_gru_bidir*_seg): `run(s0, s1)` queues steps s0 .. s1 - 1 of
    both directions -- forward frames s0 .. s1 - 1, backward frames T - s1 .. T - s0 - 1 -- on the current stream.  Bit-identical to the
    one-launch form (the hidden state is carried in fp32); what it buys is that the frames BOTH directions have passed,
    `ready(s1)` = [T - s1, s1), grow from the middle of the track while the recurrence is still on its way to the ends."""

    def __init__(self, gi, whh_t, bhh, hidden, two_workgroups=None):
        assert gi.is_contiguous() and gi.shape[0] == 6 * hidden
        _check(gi, whh_t, bhh)
        self.gi, self.whh_t, self.bhh, self.hidden, self.T = gi, whh_t, bhh, hidden, gi.shape[1]
        self.out = torch.empty((2 * hidden, self.T), dtype=torch.float32, device=gi.device)
        self.state = torch.zeros((2, hidden), dtype=torch.float32, device=gi.device)
        multi = GRU_TWO_WORKGROUPS if two_workgroups is None else two_workgroups
        self.multi = bool(multi) and hidden == 256 and GRU_WORKGROUPS == 4     # the four-workgroup kernel; otherwise the single-workgroup one
        self.scratch = torch.empty(32 * hidden + 64, dtype=torch.uint8, device=gi.device) if self.multi else None
        self.done = 0
        # the error word inside `scratch` is zeroed by the FIRST segment's launch (on the stream that launch runs on): until that launch
        # has completed the word is uninitialised allocator memory, and timed_out() -- polled from another stream -- must not read it
        self._first_done = None

    def run(self, s1):
        """Queue steps self.done .. s1 - 1."""
        s0, s1 = self.done, min(int(s1), self.T)
        if s1 <= s0:
            return
        if self.multi:
            _call("aicg_gru_bidir_4wg_seg", _ptr(self.gi), _ptr(self.whh_t), _ptr(self.bhh), _ptr(self.out), self.hidden, self.T, s0, s1,
                  _ptr(self.state), _ptr(self.scratch), _stream(self.gi))
            if s0 == 0 and self.gi.is_cuda:
                self._first_done = torch.cuda.Event()
                self._first_done.record(torch.cuda.current_stream(self.gi.device))
            if s1 == self.T:   # one flag for the whole recurrence (the error word accumulates over the segments)
                _gru_pending.append((self.scratch[32 * self.hidden: 32 * self.hidden + 4].view(torch.int32),
                                     (self.gi, self.whh_t, self.bhh, self.out, self.hidden)))
        else:
            _call("aicg_gru_bidir_seg", _ptr(self.gi), _ptr(self.whh_t), _ptr(self.bhh), _ptr(self.out), self.hidden, self.T, s0, s1,
                  _ptr(self.state), _stream(self.gi))
        self.done = s1

    def timed_out(self):
        """The recurrence's error word as of NOW (a 4-byte read on the current stream; the segments may still be running on another):
        nonzero = a partner exchange of the multi-workgroup kernel timed out, the output of that and every later segment is invalid
        (later segments bail out early).  pipeline() polls it between chunks instead of synthesising a whole track from bad pitch.
        False while the first segment -- whose launch zeroes the word -- has not run to completion (nothing can have timed out yet, and
        the word is not initialised before it: ADVICE r5)."""
        if not self.multi or self.done == 0:
            return False
        if self._first_done is not None and not self._first_done.query():
            return False
        return int(self.scratch[32 * self.hidden: 32 * self.hidden + 4].view(torch.int32).item()) != 0

    def ready(self):
        """[lo, hi): frames whose forward AND backward state exist after the steps queued so far (empty: lo >= hi)."""
        return max(0, self.T - self.done), min(self.T, self.done)


def salience_decode(salience, thred=0.03, want_center=False):
    """salience (T, 360) fp32 row-major -> (cents float64 (T,), f0 float64 (T,)[, argmax int32 (T,)])."""
    salience = salience.contiguous().float()
    t, nb = salience.shape
    cents = torch.empty(t, dtype=torch.float64, device=salience.device)
    f0 = torch.empty(t, dtype=torch.float64, device=salience.device)
    center = torch.empty(t, dtype=torch.int32, device=salience.device) if want_center else None
    _check(salience)
    _call("aicg_salience_decode", _ptr(salience), _ptr(cents), _ptr(f0), _ptr(center), t, nb, float(thred), _stream(salience))
    return (cents, f0, center) if want_center else (cents, f0)


def f0_coarse(f0, factor, mel_min, mel_max):
    """f0 float64 (n,) -> (f0 * factor float64, coarse int64 in [1, 255])."""
    f0 = f0.contiguous().double()
    out = torch.empty_like(f0)
    coarse = torch.empty(f0.shape, dtype=torch.int64, device=f0.device)
    _check(f0)
    _call("aicg_f0_coarse", _ptr(f0), float(factor), _ptr(out), _ptr(coarse), f0.numel(), float(mel_min), float(mel_max),
              _stream(f0))
    return out, coarse


# ---------------------------------------------------------------------------------------------------
# MDX-Net helpers
# ---------------------------------------------------------------------------------------------------
_gemm_work = lambda a, k, r: (2.0 * r.numel() * a[1].shape[1], 4.0 * _numel(a[0], a[1], r, k.get("res")))


@_staged("tdf_gemm_nt", _gemm_work)
def linear_last(x, weight, bias=None, ch_scale=None, ch_shift=None, act=ACT_NONE, res=None, out=None, fp32=False):
    """nn.Linear over the last axis of a contiguous (B, C, T, F) map (+ per-channel affine, act, residual).  `fp32`: never the
    split-precision kernel (layers that select indices: CREPE)."""
    assert x.is_contiguous() and x.dim() == 4 and weight.is_contiguous()
    b, c, t, f = x.shape
    o = weight.shape[0]
    assert weight.shape[1] == f
    if out is None:
        out = torch.empty((b, c, t, o), dtype=torch.float32, device=x.device)
    if res is not None:
        assert res.is_contiguous() and res.shape == out.shape
    _check(x, weight, bias, ch_scale, ch_shift, res, out)
    _call("aicg_gemm_nt_split" if split_precision and not fp32 else "aicg_gemm_nt", _ptr(x), _ptr(weight), _ptr(bias), _ptr(ch_scale),
          _ptr(ch_shift), _ptr(res), _ptr(out), b * c * t, f, o, f, f, o, o, t, c, act, _stream(x))
    return out


_linear_last = linear_last.__wrapped__   # the undecorated function, for dense_nt: a stage of its own, never also a tdf_gemm_nt


@_staged("dense_gemm_nt", _gemm_work)
def dense_nt(x, weight, bias=None, act=ACT_NONE):
    """act(x @ weight.T + bias) for a contiguous (rows, K) matrix on the fp32 NT GEMM (CREPE's Toeplitz layers and classifier)."""
    return _linear_last(x.view(1, 1, x.shape[0], x.shape[1]), weight, bias, act=act, fp32=True).view(x.shape[0], weight.shape[0])


def pack_tdf_w1(w1):
    """(H, F) -> [F / 8][2][H][4]: element e of quad (g, par, h) = W1[h][8 g + 2 e + par] (aicg_tdf_pair's w1_packed)."""
    h, f = w1.shape
    assert f % 8 == 0
    return w1.detach().float().t().reshape(f // 8, 4, 2, h).permute(0, 2, 3, 1).contiguous()


def pack_tdf_w2(w2):
    """(F, H) -> [F / 32] slabs of 32 rows x (H + 4) floats, each slab zero-padded to a multiple of 256 floats (aicg_tdf_pair's
    w2_packed: the LDS image of a stage, row padding included, so that a stage is one contiguous HBM -> LDS DMA)."""
    f, h = w2.shape
    assert f % 32 == 0
    slab = (32 * (h + 4) + 255) // 256 * 256
    out = torch.zeros((f // 32, slab), dtype=torch.float32, device=w2.device)
    rows = torch.zeros((f // 32, 32, h + 4), dtype=torch.float32, device=w2.device)
    rows[:, :, :h] = w2.detach().float().reshape(f // 32, 32, h)
    out[:, : 32 * (h + 4)] = rows.reshape(f // 32, -1)
    return out.contiguous()


def tdf_pair_supported(f, h, rows_per_ch):
    return bool(_lib.get().aicg_tdf_pair_supported(int(f), int(h), int(rows_per_ch)))


# 2 GEMMs of R x F x H; x once (re-read for the residual from L2), out, weights
@_staged("tdf_pair", lambda a, k, r: (4.0 * a[0].numel() * (a[1].numel() // a[0].shape[3]), 4.0 * _numel(a[0], r, a[1], a[1])))
def tdf_pair(x, w1p, b1, s1, t1, w2p, b2, s2, t2, out=None):
    """x + relu(bn2(relu(bn1(x W1^T + b1)) W2^T + b2)) over the last axis of a contiguous (B, C, T, F) map, one launch.
    w1p = pack_tdf_w1(W1), w2p = pack_tdf_w2(W2)."""
    assert x.is_contiguous() and x.dim() == 4 and w2p.is_contiguous() and w1p.is_contiguous()
    b, c, t, f = x.shape
    h = w1p.numel() // f
    assert w1p.numel() == f * h and w2p.shape[0] == f // 32
    if out is None:
        out = torch.empty_like(x)
    _check(x, w1p, b1, s1, t1, w2p, b2, s2, t2, out)
    _call("aicg_tdf_pair", _ptr(x), _ptr(w1p), _ptr(b1), _ptr(s1), _ptr(t1), _ptr(w2p), _ptr(b2), _ptr(s2), _ptr(t2), _ptr(out),
          b * c * t, f, h, t, c, _stream(x))
    return out


def axpbypcz(a, alpha, b=None, beta=0.0, c=None, gamma=0.0, out=None):
    """out = alpha*a + beta*b + gamma*c over contiguous fp32 tensors of one shape."""
    assert a.is_contiguous() and (b is None or b.is_contiguous()) and (c is None or c.is_contiguous())
    if out is None:
        out = torch.empty_like(a)
    _check(a, b, c, out)
    _call("aicg_axpbypcz", _ptr(a), float(alpha), _ptr(b), float(beta), _ptr(c), float(gamma), _ptr(out), a.numel(),
              _stream(a))
    return out


# ---------------------------------------------------------------------------------------------------
# VC.pipeline pre/post on the device
# ---------------------------------------------------------------------------------------------------
def box_sum_f64(x, n, window):
    """x: float64 (n + window - 1,) -> out[j] = sum_{i<window} x[j+i] (reference summation order)."""
    x = x.contiguous()
    assert x.dtype == torch.float64 and x.numel() >= n + window - 1
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    _check(x)
    _call("aicg_box_sum_f64", _ptr(x), _ptr(out), n, window, _stream(x))
    return out


def argmin_abs_f64(x, starts, lens):
    """first index of min |x[s : s+l]| for each (s, l)."""
    assert x.dtype == torch.float64
    st = torch.tensor(list(starts), dtype=torch.int64, device=x.device)
    ln = torch.tensor(list(lens), dtype=torch.int64, device=x.device)
    out = torch.empty(len(st), dtype=torch.int64, device=x.device)
    _check(x)
    _call("aicg_argmin_abs_f64", _ptr(x), _ptr(st), _ptr(ln), _ptr(out), len(st), _stream(x))
    return out


def frame_rms(x, frame_length, hop_length):
    """librosa.feature.rms (center, reflect) of a 1-D float32 / float64 device tensor -> float64 (n_frames,)."""
    x = x.contiguous()
    assert x.dim() == 1 and x.dtype in (torch.float32, torch.float64)
    n = x.numel()
    out = torch.empty(1 + n // hop_length, dtype=torch.float64, device=x.device)
    _check(x)
    _call("aicg_frame_rms", _ptr(x), 1 if x.dtype == torch.float64 else 0, _ptr(out), n, frame_length, hop_length, _stream(x))
    return out


def rms_mix_(data, rms1, rms2, rate):
    assert data.is_contiguous() and data.dtype == torch.float32
    _check(data, rms1, rms2)
    _call("aicg_rms_mix", _ptr(data), data.numel(), _ptr(rms1), rms1.numel(), _ptr(rms2), rms2.numel(), float(rate),
              _stream(data))
    return data


def absmax(x):
    assert x.is_contiguous() and x.dtype == torch.float32
    out = torch.zeros(1, dtype=torch.float32, device=x.device)
    _check(x)
    _call("aicg_absmax", _ptr(x), x.numel(), _ptr(out), _stream(x))
    return out


def to_int16(x, scale):
    assert x.is_contiguous() and x.dtype == torch.float32
    out = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    _check(x)
    _call("aicg_to_int16", _ptr(x), _ptr(out), x.numel(), float(scale), _stream(x))
    return out


# ---------------------------------------------------------------------------------------------------
# Vocal effects chain and stem mix (csrc/fx.hip); parameters are derived in cover.py
# ---------------------------------------------------------------------------------------------------
FX_HPF, FX_COMP = 1, 2


def fx_reverb_state_size(sr):
    n = ctypes.c_int64(0)
    _lib.call("aicg_fx_reverb_state_size", int(sr), ctypes.addressof(n))
    return n.value


def fx_dynamics(x, state_in, seg_len, warm, coefs, flags):
    """x: (C, n) fp32.  coefs: (b0, b1, a1, cte_attack, cte_release, threshold, threshold_inv, ratio_inv).
    Returns (y, state_out (C, 2))."""
    assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.float32
    C, n = x.shape
    y = torch.empty_like(x)
    st = torch.empty((C, 2), dtype=torch.float32, device=x.device)
    assert state_in is None or (state_in.shape == st.shape and state_in.is_contiguous() and state_in.dtype == torch.float32)
    _check(x, state_in)
    _call("aicg_fx_dynamics", _ptr(x), _ptr(y), _ptr(state_in), _ptr(st), C, n, int(seg_len), int(warm),
          *[float(v) for v in coefs], int(flags), _stream(x))
    return y, st


def fx_reverb(x, sr, state_in, seg_len, warm, coefs):
    """x: (C, n) fp32.  coefs: (gain, damp, feedback, wet1, wet2, dry).  Returns (y, state_out (C, fx_reverb_state_size(sr)))."""
    assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.float32
    C, n = x.shape
    y = torch.empty_like(x)
    st = torch.empty((C, fx_reverb_state_size(sr)), dtype=torch.float32, device=x.device)
    assert state_in is None or (state_in.shape == st.shape and state_in.is_contiguous() and state_in.dtype == torch.float32)
    _check(x, state_in)
    _call("aicg_fx_reverb", _ptr(x), _ptr(y), _ptr(state_in), _ptr(st), C, n, int(sr), int(seg_len), int(warm),
          *[float(v) for v in coefs], _stream(x))
    return y, st


def fx_to_pcm16(x):
    """(C, n) fp32 -> (n, C) int16, round to nearest of clamp(x, -1, 1) * 32767."""
    assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.float32
    C, n = x.shape
    out = torch.empty((n, C), dtype=torch.int16, device=x.device)
    _check(x)
    _call("aicg_fx_to_pcm16", _ptr(x), _ptr(out), C, n, _stream(x))
    return out


def pcm16_mix(a, a_rate, a_gains, b, b_rate, b_gains, out_frames):
    """a.overlay(b) in pydub's arithmetic.  a, b: (frames, channels) int16; *_gains: the two audioop.mul factors applied in order.
    Returns (out_frames, max(channels)) int16 at max(a_rate, b_rate)."""
    for t in (a, b):
        assert t.dim() == 2 and t.is_contiguous() and t.dtype == torch.int16
    ch = max(a.shape[1], b.shape[1])
    out = torch.empty((int(out_frames), ch), dtype=torch.int16, device=a.device)
    _check(a, b, out)
    _call("aicg_pcm16_mix", _ptr(a), a.shape[1], int(a_rate), a.shape[0], float(a_gains[0]), float(a_gains[1]),
          _ptr(b), b.shape[1], int(b_rate), b.shape[0], float(b_gains[0]), float(b_gains[1]), _ptr(out), int(out_frames), _stream(a))
    return out


# ---------------------------------------------------------------------------------------------------
# Stems handed from one stage of a cover to the next (csrc/handover.hip): the head and the tail of run_mdx on the device
# ---------------------------------------------------------------------------------------------------
STEM_PCM16, STEM_F32 = 0, 1


def stem_normalise(x):
    """x: (frames, C) int16 PCM (read as x / 32768) or (C, n) float32, C = 1 or 2 (mono serves both rows).
    Returns (wave (2, n) float32 = x / peak, peak (1,) float32 = max(max(x), |min(x)|)), both on x's device: nothing waits for the
    peak."""
    if x.dim() != 2:
        raise ValueError("stem_normalise takes (frames, channels) int16 or (channels, n) float32, got %s" % (tuple(x.shape),))
    if not x.is_contiguous():
        raise ValueError("stem_normalise takes a contiguous tensor (strides %s of shape %s)" % (x.stride(), tuple(x.shape)))
    fmt = {torch.int16: STEM_PCM16, torch.float32: STEM_F32}.get(x.dtype, -1)   # any other dtype: the library names what it reads
    n, C = (x.shape[1], x.shape[0]) if fmt == STEM_F32 else (x.shape[0], x.shape[1])
    out = torch.empty((2, n), dtype=torch.float32, device=x.device)
    peak = torch.empty(1, dtype=torch.float32, device=x.device)
    _check(x)
    _call("aicg_stem_normalise", _ptr(x), fmt, C, n, _ptr(out), _ptr(peak), _stream(x))
    return out, peak


def mdx_stems_pcm16(wave, separated, peak, compensation, want_main=True, want_inverted=True):
    """wave (the normalised input), separated: (2, n) float32; peak: (1,) float32 on the device.  Returns (main, inverted): (n, 2)
    int16 of separated * peak and of wave - (separated * peak) * compensation, None for a stem that is not wanted."""
    for t in (wave, separated):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != 2:
            raise TypeError("mdx_stems_pcm16 takes (2, n) float32 signals, got %s %s" % (t.dtype, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("mdx_stems_pcm16 takes contiguous tensors (strides %s of shape %s)" % (t.stride(), tuple(t.shape)))
    if wave.shape != separated.shape:
        raise ValueError("mdx_stems_pcm16: wave %s and separated %s differ in shape" % (tuple(wave.shape), tuple(separated.shape)))
    if peak.dtype != torch.float32 or peak.numel() != 1:
        raise TypeError("mdx_stems_pcm16: peak is one float32 on the device, got %s %s" % (peak.dtype, tuple(peak.shape)))
    n = wave.shape[1]
    main = torch.empty((n, 2), dtype=torch.int16, device=wave.device) if want_main else None
    inv = torch.empty((n, 2), dtype=torch.int16, device=wave.device) if want_inverted else None
    _check(wave, separated, peak)
    _call("aicg_mdx_stems_pcm16", _ptr(wave), _ptr(separated), _ptr(peak), float(compensation), n, _ptr(main), _ptr(inv), _stream(wave))
    return main, inv


# ---------------------------------------------------------------------------------------------------
# Pitch shift of the backing stems (csrc/pitch.hip): WSOLA time-stretch, then resampling by an irrational ratio
# ---------------------------------------------------------------------------------------------------
def tempo_wsola_geometry(sr, tempo, n):
    """(seg, search, ovl, skip, steps, n_out) in frames: sox's `tempo` music defaults at `sr` for the tempo factor `tempo`."""
    g = (ctypes.c_int64 * 6)()
    _lib.call("aicg_tempo_wsola_geometry", int(sr), float(tempo), int(n), ctypes.addressof(g))
    return tuple(int(v) for v in g)


def tempo_wsola(x, sr, tempo, offsets=None):
    """x: (C, n) or (S, C, n) fp32 (S signals of one length, one workgroup each).  Duration is multiplied by 1 / tempo, pitch kept.
    offsets: int32 (steps,) / (S, steps) to use instead of searching, or None.  Returns (y (.., C, n_out), offsets int32)."""
    assert x.dim() in (2, 3) and x.is_contiguous() and x.dtype == torch.float32
    S = 1 if x.dim() == 2 else x.shape[0]
    C, n = x.shape[-2:]
    steps, n_out = tempo_wsola_geometry(sr, tempo, n)[4:]
    y = torch.empty(x.shape[:-1] + (n_out,), dtype=torch.float32, device=x.device)
    offs = torch.zeros(x.shape[:-2] + (steps,), dtype=torch.int32, device=x.device)
    if offsets is not None:
        assert offsets.shape == offs.shape and offsets.dtype == torch.int32 and offsets.is_contiguous()
    _check(x, offsets)
    _call("aicg_tempo_wsola", _ptr(x), _ptr(y), _ptr(offs), _ptr(offsets), S, C, n, int(sr), float(tempo), _stream(x))
    return y, offs


# The resampling filter.  The output is stored as 16-bit PCM, so the response may deviate from the ideal one by at most
# half a step of full scale, 2^-16 = -96.3 dB, in both bands; a Kaiser window has equal ripple in both, and A = 100 dB leaves the
# window formulas' approximation some room (the achieved response is asserted in tests/test_cover_pitch.py).
RESAMPLE_ATT_DB = 100.0
RESAMPLE_PASS = 0.90       # passband edge as a share of the narrower Nyquist frequency; the stopband begins at that Nyquist
RESAMPLE_PHASES = 1024     # table rows per input sample: linear interpolation between rows stays below 2^-18


def resample_ratio_design(ratio):
    """(fc, beta, half): cutoff in cycles per input sample (the middle of the transition band), Kaiser beta, and the filter's
    half length in input samples, for y[m] = sum_t h(m ratio - t) x[t]."""
    nu = min(1.0, 1.0 / float(ratio))
    beta = 0.1102 * (RESAMPLE_ATT_DB - 8.7)
    width = (1.0 - RESAMPLE_PASS) * nu / 2.0
    half = int(math.ceil((RESAMPLE_ATT_DB - 7.95) / (2.285 * 2.0 * math.pi * width) / 2.0))
    return (1.0 + RESAMPLE_PASS) / 2.0 * nu / 2.0, beta, half


def resample_ratio_filter(tau, ratio):
    """h(tau) in float64: 2 fc sinc(2 fc tau) I0(beta sqrt(1 - (tau / half)^2)) / I0(beta) inside (-half, half), 0 outside."""
    fc, beta, half = resample_ratio_design(ratio)
    tau = np.asarray(tau, np.float64)
    u = 1.0 - (tau / half) ** 2
    w = np.where(u > 0.0, np.i0(beta * np.sqrt(np.maximum(u, 0.0))) / np.i0(beta), 0.0)
    return 2.0 * fc * np.sinc(2.0 * fc * tau) * w


_ratio_tables = {}


def resample_ratio_table(ratio):
    """(table float32 (PHASES + 1, 2 half + 1), half): table[r][j + half] = h(r / PHASES + j), computed in float64."""
    half = resample_ratio_design(ratio)[2]
    r = np.arange(RESAMPLE_PHASES + 1, dtype=np.float64)[:, None] / RESAMPLE_PHASES
    j = np.arange(-half, half + 1, dtype=np.float64)[None, :]
    return resample_ratio_filter(r + j, ratio).astype(np.float32), half


def resample_ratio(x, ratio, n_out):
    """x: (C, n_in) or (S, C, n_in) fp32 -> (.., C, n_out): y[m] = sum_t h(m ratio - t) x[t], band-limited to the narrower Nyquist."""
    assert x.dim() in (2, 3) and x.is_contiguous() and x.dtype == torch.float32
    S = 1 if x.dim() == 2 else x.shape[0]
    C, n_in = x.shape[-2:]
    key = (float(ratio), str(x.device))
    if key not in _ratio_tables:
        t, half = resample_ratio_table(ratio)
        _ratio_tables[key] = (torch.from_numpy(t).to(x.device), half)
    table, half = _ratio_tables[key]
    y = torch.empty(x.shape[:-1] + (int(n_out),), dtype=torch.float32, device=x.device)
    _check(x, table)
    _call("aicg_resample_ratio", _ptr(x), _ptr(y), S, C, n_in, int(n_out), float(ratio), _ptr(table), RESAMPLE_PHASES, half, _stream(x))
    return y


# ---------------------------------------------------------------------------------------------------
# f0_method "pm" (csrc/pitch_ac.hip): Praat's autocorrelation pitch
# ---------------------------------------------------------------------------------------------------
PITCH_AC_CANDIDATES = 15        # Praat's defaults behind parselmouth's to_pitch_ac
PITCH_AC_SILENCE = 0.03
PITCH_AC_OCTAVE_COST = 0.01
PITCH_AC_OCTAVE_JUMP_COST = 0.35
PITCH_AC_VOICED_UNVOICED_COST = 0.14


def pitch_ac_geometry(sr, n, time_step=0.01, pitch_floor=50.0, pitch_ceiling=1100.0):
    """(nsamp_window, nsampFFT, maximumLag, brent_ixmax, n_frames, floor(t1 in samples), candidate scratch bytes, path scratch bytes).
    ValueError for a signal shorter than one window."""
    g = (ctypes.c_int64 * 8)()
    try:
        _lib.call("aicg_pitch_ac_geometry", int(sr), int(n), float(time_step), float(pitch_floor), float(pitch_ceiling), ctypes.addressof(g))
    except RuntimeError as e:
        raise ValueError(str(e))
    return tuple(int(v) for v in g)


def pitch_ac_frame_times(sr, n, time_step=0.01, pitch_floor=50.0, pitch_ceiling=1100.0):
    """Centre of every frame in seconds, float64 (n_frames,): (t1 + i time_step sr) / sr with t1 = n / 2 - (n_frames - 1) time_step sr / 2
    in samples, exactly as the kernels place the frames (the geometry call returns floor(t1) only)."""
    n_frames = pitch_ac_geometry(sr, n, time_step, pitch_floor, pitch_ceiling)[4]
    step = float(time_step) * float(sr)
    return (0.5 * n - 0.5 * (n_frames - 1) * step + np.arange(n_frames, dtype=np.float64) * step) / float(sr)


def pitch_ac_tables(nw, nfft, brent):
    """(window, window_ac, twiddle) float32, computed in float64: the Hanning window 0.5 - 0.5 cos(2 pi i / (nw + 1)), i = 1 .. nw, its
    autocorrelation over lags 0 .. brent normalised to 1 at lag 0, and exp(-2 pi i k / nfft) as (cos, -sin) pairs."""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, nw + 1, dtype=np.float64) / (nw + 1))
    wr = np.fft.irfft(np.abs(np.fft.rfft(w, nfft)) ** 2, nfft)
    wr = wr[:brent + 1] / wr[0]
    a = 2.0 * np.pi * np.arange(nfft, dtype=np.float64) / nfft
    tw = np.stack([np.cos(a), -np.sin(a)], axis=1)
    return w.astype(np.float32), wr.astype(np.float32), tw.astype(np.float32)


_pitch_ac_plans = {}


def _pitch_ac_plan(nw, nfft, brent, device):
    key = (nw, nfft, brent, str(device))
    if key not in _pitch_ac_plans:
        _pitch_ac_plans[key] = tuple(torch.from_numpy(t).to(device) for t in pitch_ac_tables(nw, nfft, brent))
    return _pitch_ac_plans[key]


def pitch_ac_candidates(x, sr=16000, time_step=0.01, pitch_floor=50.0, pitch_ceiling=1100.0, voicing_threshold=0.6,
                        max_candidates=PITCH_AC_CANDIDATES, silence_threshold=PITCH_AC_SILENCE, octave_cost=PITCH_AC_OCTAVE_COST):
    """x: 1-D fp32 -> (cand fp32 (n_frames, max_candidates, 2) = (frequency, strength), count int32 (n_frames,))."""
    assert x.dim() == 1 and x.dtype == torch.float32 and x.is_contiguous()
    nw, nfft, _, brent, n_frames, _, cs, _ = pitch_ac_geometry(sr, x.numel(), time_step, pitch_floor, pitch_ceiling)
    window, wac, tw = _pitch_ac_plan(nw, nfft, brent, x.device)
    scratch = torch.empty(cs, dtype=torch.uint8, device=x.device)
    cand = torch.empty((n_frames, int(max_candidates), 2), dtype=torch.float32, device=x.device)
    count = torch.empty((n_frames,), dtype=torch.int32, device=x.device)
    _check(x, window, wac, tw)
    _call("aicg_pitch_ac_candidates", _ptr(x), x.numel(), int(sr), float(time_step), float(pitch_floor), float(pitch_ceiling),
          int(max_candidates), float(voicing_threshold), float(silence_threshold), float(octave_cost), _ptr(window), _ptr(wac), _ptr(tw),
          _ptr(scratch), _ptr(cand), _ptr(count), _stream(x))
    return cand, count


def pitch_ac_path(cand, count, time_step=0.01, pitch_ceiling=1100.0, octave_cost=PITCH_AC_OCTAVE_COST,
                  octave_jump_cost=PITCH_AC_OCTAVE_JUMP_COST, voiced_unvoiced_cost=PITCH_AC_VOICED_UNVOICED_COST, return_states=False):
    """The best path through a candidate table (float64 accumulation) -> f0 float64 (n_frames,) [, chosen indices int32]."""
    assert cand.dim() == 3 and cand.shape[2] == 2 and cand.dtype == torch.float32 and cand.is_contiguous()
    assert count.shape == (cand.shape[0],) and count.dtype == torch.int32 and count.is_contiguous()
    n_frames, K = cand.shape[:2]
    scratch = torch.empty(n_frames * (16 * 2 * 8 + 16), dtype=torch.uint8, device=cand.device)
    f0 = torch.empty((n_frames,), dtype=torch.float64, device=cand.device)
    states = torch.empty((n_frames,), dtype=torch.int32, device=cand.device)
    _check(cand, count)
    _call("aicg_pitch_ac_path", _ptr(cand), _ptr(count), n_frames, K, float(time_step), float(pitch_ceiling), float(octave_cost),
          float(octave_jump_cost), float(voiced_unvoiced_cost), _ptr(scratch), _ptr(f0), _ptr(states), _stream(cand))
    return (f0, states) if return_states else f0


def pitch_ac(x, sr=16000, time_step=0.01, pitch_floor=50.0, pitch_ceiling=1100.0, voicing_threshold=0.6,
             max_candidates=PITCH_AC_CANDIDATES, silence_threshold=PITCH_AC_SILENCE, octave_cost=PITCH_AC_OCTAVE_COST,
             octave_jump_cost=PITCH_AC_OCTAVE_JUMP_COST, voiced_unvoiced_cost=PITCH_AC_VOICED_UNVOICED_COST, return_candidates=False):
    """Praat's `Sound: To Pitch (ac)...` (parselmouth's to_pitch_ac, src/vc_infer_pipeline.py:279-289) on the device.  x: 1-D float32 or
    float64 (cast on the device) -> f0 in Hz float64 (n_frames,), 0 = unvoiced [, cand, count].  ValueError for a signal shorter than
    one window (3 / pitch_floor seconds)."""
    assert x.dim() == 1
    x = x.contiguous().float()
    cand, count = pitch_ac_candidates(x, sr, time_step, pitch_floor, pitch_ceiling, voicing_threshold, max_candidates, silence_threshold,
                                      octave_cost)
    f0 = pitch_ac_path(cand, count, time_step, pitch_ceiling, octave_cost, octave_jump_cost, voiced_unvoiced_cost)
    return (f0, cand, count) if return_candidates else f0


# ---------------------------------------------------------------------------------------------------
# f0_method "dio" (csrc/world_dio.hip): WORLD's DIO, StoneMask, the 3-point median
# ---------------------------------------------------------------------------------------------------
WORLD_DIO_NUTTALL = (0.355768, -0.487396, 0.144232, -0.012604)


def world_dio_geometry(sr, n, frame_period=10.0, f0_floor=50.0, f0_ceil=1100.0, channels_in_octave=2.0):
    """dict: n_frames, n_bands, n_tiles, lowcut (taps), pad, vrm, count_scratch / repair_scratch (bytes), index_ints, tile, half (per
    band), boundary (per band, float64).  ValueError for a shape the kernels cannot serve."""
    g = (ctypes.c_int64 * 26)()
    b = (ctypes.c_double * 16)()
    try:
        _lib.call("aicg_world_dio_geometry", int(sr), int(n), float(frame_period), float(f0_floor), float(f0_ceil), float(channels_in_octave),
                  ctypes.addressof(g), ctypes.addressof(b))
    except RuntimeError as e:
        raise ValueError(str(e))
    nb = int(g[1])
    names = ("n_frames", "n_bands", "n_tiles", "lowcut", "pad", "vrm", "count_scratch", "repair_scratch", "index_ints", "tile")
    out = {k: int(g[i]) for i, k in enumerate(names)}
    out["half"] = [int(g[10 + i]) for i in range(nb)]
    out["boundary"] = np.array([b[i] for i in range(nb)], dtype=np.float64)
    return out


def world_dio_tables(lowcut, half):
    """float64 taps, the low-cut's then every band's: 1 at the centre minus the Hanning low-pass 0.5 - 0.5 cos(2 pi i / (N + 1)), i = 1 ..
    N, normalised to sum 1; per band the Nuttall window of 4 h points sampled at i / (4 h - 1)."""
    h = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, lowcut + 1, dtype=np.float64) / (lowcut + 1))
    h = -h / h.sum()
    h[(lowcut - 1) // 2] += 1.0
    taps = [h]
    for hb in half:
        t = np.arange(4 * hb, dtype=np.float64) / (4 * hb - 1.0)
        taps.append(sum(c * np.cos(2.0 * np.pi * k * t) for k, c in enumerate(WORLD_DIO_NUTTALL)))
    return np.concatenate(taps)


_world_dio_plans = {}


def _world_dio_plan(g, device):
    key = (g["lowcut"], tuple(g["half"]), str(device))
    if key not in _world_dio_plans:
        _world_dio_plans[key] = torch.from_numpy(world_dio_tables(g["lowcut"], g["half"])).to(device)
    return _world_dio_plans[key]


def world_dio_repair(cand, score, frame_period=10.0, f0_floor=50.0, allowed_range=0.1):
    """Best band per frame and WORLD's four repair steps on (n_bands, n_frames) fp32 tables -> f0 float64 (n_frames,)."""
    assert cand.dim() == 2 and cand.shape == score.shape and cand.dtype == score.dtype == torch.float32
    assert cand.is_contiguous() and score.is_contiguous()
    nb, nf = cand.shape
    f0 = torch.empty((nf,), dtype=torch.float64, device=cand.device)
    scratch = torch.empty(nf * 16 + 64, dtype=torch.uint8, device=cand.device)
    _check(cand, score)
    _call("aicg_world_dio_repair", _ptr(cand), _ptr(score), nb, nf, float(frame_period), float(f0_floor), float(allowed_range), _ptr(scratch),
          _ptr(f0), _stream(cand))
    return f0


def world_dio(x, sr=16000, frame_period=10.0, f0_floor=50.0, f0_ceil=1100.0, channels_in_octave=2.0, allowed_range=0.1,
              return_candidates=False, return_bands=False):
    """pyworld.dio(x, fs, f0_floor, f0_ceil, channels_in_octave, frame_period, speed=1, allowed_range)[0] on the device.  x: 1-D float32
    or float64 (cast on the device) -> f0 in Hz float64 (n_frames,), 0 = unvoiced [, cand, score (n_bands, n_frames) fp32, crossing
    counts (n_bands, 4) int64 (host), the crossings themselves (integer parts int32, fractions fp32, row starts per band and kind)]
    [, the band signals (n_bands, n) fp32: a development return].  The crossing workspace is sized from the counts, which come to the
    host between the two calls (one small copy)."""
    assert x.dim() == 1
    x = x.contiguous().float()
    n = x.numel()
    g = world_dio_geometry(sr, n, frame_period, f0_floor, f0_ceil, channels_in_octave)
    nb, nf, rows = g["n_bands"], g["n_frames"], 4 * g["n_bands"]
    taps = _world_dio_plan(g, x.device)
    scratch = torch.empty(g["count_scratch"], dtype=torch.uint8, device=x.device)
    index = torch.empty(g["index_ints"], dtype=torch.int32, device=x.device)
    bands = torch.zeros((nb, n), dtype=torch.float32, device=x.device) if return_bands else None
    _check(x, taps)
    args = (int(sr), float(frame_period), float(f0_floor), float(f0_ceil), float(channels_in_octave))
    _call("aicg_world_dio_count", _ptr(x), n, *args, _ptr(taps), _ptr(scratch), _ptr(index), _ptr(bands) if return_bands else None, _stream(x))
    row_start = index[2 * rows * g["n_tiles"]:].cpu().numpy().astype(np.int64)
    total = int(row_start[-1])
    ev_ip = torch.empty(max(total, 1), dtype=torch.int32, device=x.device)
    ev_fr = torch.empty(max(total, 1), dtype=torch.float32, device=x.device)
    cand = torch.empty((nb, nf), dtype=torch.float32, device=x.device)
    score = torch.empty((nb, nf), dtype=torch.float32, device=x.device)
    f0 = torch.empty((nf,), dtype=torch.float64, device=x.device)
    rs = torch.empty(g["repair_scratch"], dtype=torch.uint8, device=x.device)
    _call("aicg_world_dio", n, *args, float(allowed_range), _ptr(taps), _ptr(scratch), _ptr(index), total, _ptr(ev_ip), _ptr(ev_fr), _ptr(rs),
          _ptr(cand), _ptr(score), _ptr(f0), _stream(x))
    out = (f0,)
    if return_candidates:
        out += (cand, score, np.diff(row_start).reshape(nb, 4), (ev_ip[:total], ev_fr[:total], row_start))
    if return_bands:
        out += (bands,)
    return out if len(out) > 1 else f0


def stonemask(x, f0, sr=16000, frame_period=10.0):
    """pyworld.stonemask(x, f0, t, fs) with t[i] = i frame_period / 1000 on the device.  x 1-D float32 / float64, f0 float64 (n_frames,) ->
    refined f0 float64."""
    assert x.dim() == 1 and f0.dim() == 1 and x.numel() >= 1
    x = x.contiguous().float()
    f0 = f0.contiguous().double()
    out = torch.empty_like(f0)
    _check(x, f0)
    _call("aicg_stonemask", _ptr(x), x.numel(), int(sr), float(frame_period), _ptr(f0), f0.numel(), _ptr(out), _stream(x))
    return out


def medfilt3(f0):
    """scipy.signal.medfilt(f0, 3) on a float64 track: zeros beyond both ends."""
    assert f0.dim() == 1 and f0.dtype == torch.float64
    f0 = f0.contiguous()
    out = torch.empty_like(f0)
    if f0.numel():
        _check(f0)
        _call("aicg_medfilt3", _ptr(f0), f0.numel(), _ptr(out), _stream(f0))
    return out


# ---------------------------------------------------------------------------------------------------
# Around the estimators of hybrid[...] / mangio-crepe (csrc/select.hip): the quantile of |x|, the division by it, the nan-median
# ---------------------------------------------------------------------------------------------------
NANMEDIAN_MAX_ROWS = 8


def numpy_quantile_mirrored():
    """Whether abs_quantile restates the installed numpy: the index and weight arithmetic below is numpy 2.x's (a Python-float q is
    cast to the data's float32 before the virtual index is formed; 1.x forms it in float64)."""
    return np.__version__.split(".")[0] == "2"


def abs_select(x, rank_lo, rank_hi):
    """Elements rank_lo and rank_hi (= rank_lo or rank_lo + 1) of sorted(|x|) -> (2,) float32 on x's device; both NaN when x holds
    a NaN.  x: 1-D float32, 1 to 2^27 elements (ValueError beyond).  Exact (radix select on the bit patterns), no synchronisation."""
    assert x.dim() == 1 and x.dtype == torch.float32
    x = x.contiguous()
    n = x.numel()
    _check(x)
    nbytes = _lib.get().aicg_abs_select_workspace_bytes(n)
    if nbytes <= 0:
        raise ValueError("abs_select: %d elements (1 to 2^27 are served)" % n)
    if not (0 <= rank_lo <= rank_hi < n and rank_hi - rank_lo <= 1):
        raise ValueError("abs_select: ranks %d, %d of %d elements" % (rank_lo, rank_hi, n))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    _call("aicg_abs_select_f32", _ptr(x), n, int(rank_lo), int(rank_hi), _ptr(out), _ptr(ws), _stream(x))
    return out


def quantile_plan(n, q):
    """(rank_lo, rank_hi, weight) of np.quantile(a, q) (method 'linear') for n float32 values and a Python-float q, from n alone, in
    numpy 2.x's own arithmetic (numpy/lib/_function_base_impl.py: _quantile, _get_indexes, _get_gamma): q and n - 1 become float32,
    the virtual index is their float32 product, the lower rank its floor and the weight what is left; at or past the last element
    both ranks are n - 1 and the weight is index + 1 (harmless: the two values are one)."""
    if not 0.0 <= q <= 1.0:
        raise ValueError("Quantiles must be in the range [0, 1]")
    virtual = np.asanyarray((n - 1) * np.asanyarray(q, dtype=np.float32))
    previous = np.asanyarray(np.floor(virtual))
    nxt = np.asanyarray(previous + 1)
    if virtual >= n - 1:
        previous, nxt = np.asanyarray(np.float32(-1)), np.asanyarray(np.float32(-1))
    gamma = np.asanyarray(virtual - previous, dtype=virtual.dtype)
    return int(previous.astype(np.intp)) % n, int(nxt.astype(np.intp)) % n, np.float32(gamma)


def abs_quantile(x, q):
    """np.quantile(np.abs(x), q) of a 1-D float32 device tensor -> 0-dim float32 tensor on the same device, bit for bit what numpy
    2.x returns (NaN where numpy gives NaN: a NaN in x, or an infinite neighbour).  The two ranks and the weight come from len(x) on
    the host (quantile_plan), the two order statistics from abs_select and the interpolation from a kernel that rounds like numpy's
    _lerp; nothing is synchronised.  Under another major version of numpy the arithmetic of the index may differ: callers that
    promise numpy's bits ask numpy_quantile_mirrored() and keep the host route otherwise."""
    lo, hi, t = quantile_plan(x.numel(), float(q))
    ab = abs_select(x, lo, hi)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    _call("aicg_quantile_lerp", _ptr(ab), float(t), _ptr(out), _stream(x))
    return out


def div_scalar(x, s):
    """x / s for float32 x and a 0-dim float32 tensor s on the same device: IEEE division, numpy's bits (torch.div by a host scalar
    multiplies by the reciprocal on the device)."""
    assert x.dtype == torch.float32 and s.dtype == torch.float32 and s.numel() == 1 and s.device == x.device
    x = x.contiguous()
    y = torch.empty_like(x)
    if x.numel():
        _check(x, s)
        _call("aicg_div_scalar", _ptr(x), _ptr(s), _ptr(y), x.numel(), _stream(x))
    return y


def nanmedian_rows(stack):
    """np.nanmedian(stack, axis=0) of a (k, n) float64 tensor, 1 <= k <= 8 (ValueError beyond: the caller joins on the host) ->
    (n,) float64, the same bits: NaNs ignored, NaN for a column of NaNs, (a + b) / 2 for an even count."""
    assert stack.dim() == 2 and stack.dtype == torch.float64
    k, n = stack.shape
    if not 1 <= k <= NANMEDIAN_MAX_ROWS:
        raise ValueError("nanmedian_rows: %d rows (1 to %d are served)" % (k, NANMEDIAN_MAX_ROWS))
    stack = stack.contiguous()
    out = torch.empty(n, dtype=torch.float64, device=stack.device)
    if n:
        _check(stack)
        _call("aicg_nanmedian_rows", _ptr(stack), k, n, _ptr(out), _stream(stack))
    return out


# ---------------------------------------------------------------------------------------------------
# The cover's file, encoded where the mix lives (csrc/flac.hip)
# ---------------------------------------------------------------------------------------------------
FLAC_BLOCKS = (256, 512, 1024, 2048, 4096)


def flac_encode(pcm, sr, block=4096):
    """(frames, channels) int16 PCM, 1 or 2 channels, on the device -> 1-D uint8 tensor on the same device: exactly the bytes of a FLAC
    file (RFC 9639) that decodes to `pcm`.  "fLaC", one STREAMINFO block and the frames of a fixed-blocksize stream of `block` samples
    (256, 512, 1024, 2048 or 4096); no seek table and no tags, and STREAMINFO's MD5 field is all zero, which the RFC allows as "not
    computed".  Subframes: the cheapest by exact bit count of CONSTANT, VERBATIM, FIXED 0-4 and LPC 1-8 with partitioned Rice coding,
    stereo decorrelation per frame; CRCs on the device.  Zero frames give the 42 header bytes.  The file's size is read back from
    the device (one 8-byte copy: the call waits for the encoder).  TypeError for another dtype, ValueError for another channel count,
    block size or sample rate."""
    if not isinstance(pcm, torch.Tensor) or pcm.dtype != torch.int16:
        raise TypeError("flac_encode: (frames, channels) int16 PCM expected, found %s" % (getattr(pcm, "dtype", type(pcm)),))
    if pcm.dim() == 1:
        pcm = pcm.view(-1, 1)
    if pcm.dim() != 2 or pcm.shape[1] not in (1, 2):
        raise ValueError("flac_encode: 1 or 2 channels are encoded, found shape %s" % (tuple(pcm.shape),))
    if int(block) not in FLAC_BLOCKS:
        raise ValueError("flac_encode: block size %r (one of %s)" % (block, ", ".join(map(str, FLAC_BLOCKS))))
    if not 1 <= int(sr) < (1 << 20):
        raise ValueError("flac_encode: sample rate %r" % (sr,))
    pcm = pcm.contiguous()
    n, ch = pcm.shape
    _check(pcm)
    geom = torch.zeros(4, dtype=torch.int64)
    _call("aicg_flac_geometry", n, ch, int(sr), int(block), _ptr(geom))
    _, ws_bytes, capacity, _ = geom.tolist()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pcm.device)
    out = torch.empty(capacity, dtype=torch.uint8, device=pcm.device)
    size = torch.zeros(1, dtype=torch.int64, device=pcm.device)
    _call("aicg_flac_encode", _ptr(pcm), n, ch, int(sr), int(block), _ptr(ws), _ptr(out), capacity, _ptr(size), _stream(pcm))
    return out[:int(size.item())]



# ---------------------------------------------------------------------------------------------------
# CREPE helpers
# ---------------------------------------------------------------------------------------------------
def frame_normalize(frames):
    assert frames.is_contiguous() and frames.dim() == 2
    out = torch.empty_like(frames)
    _check(frames)
    _call("aicg_frame_normalize", _ptr(frames), _ptr(out), frames.shape[0], frames.shape[1], _stream(frames))
    return out


def affine_maxpool2(x, scale, shift):
    """x (N, C, W) contiguous -> max over pairs of (x * scale[c] + shift[c]) -> (N, C, W/2)."""
    assert x.is_contiguous() and x.dim() == 3
    n, c, w = x.shape
    out = torch.empty((n, c, w // 2), dtype=torch.float32, device=x.device)
    _check(x, scale, shift)
    _call("aicg_affine_maxpool2", _ptr(x), _ptr(scale), _ptr(shift), _ptr(out), n, c, w, _stream(x))
    return out


def crepe_viterbi(probs, seq_len, bin_lo, bin_hi):
    """probs (n_seq, 360, max_steps) fp32, seq_len list -> bins int64 (n_seq, max_steps)."""
    probs = probs.contiguous()
    n_seq, nb, ms = probs.shape
    sl = torch.tensor(list(seq_len), dtype=torch.int32, device=probs.device)
    logp = torch.empty((n_seq, ms, nb), dtype=torch.float32, device=probs.device)
    ptr = torch.empty((n_seq, ms, nb), dtype=torch.int16, device=probs.device)
    bins = torch.zeros((n_seq, ms), dtype=torch.int64, device=probs.device)
    _check(probs)
    _call("aicg_crepe_viterbi", _ptr(probs), _ptr(sl), _ptr(logp), _ptr(ptr), _ptr(bins), n_seq, nb, ms, int(bin_lo),
              int(bin_hi), _stream(probs))
    return bins


# ---------------------------------------------------------------------------------------------------
# Signal processing either side of the networks (csrc/dsp.hip)
# ---------------------------------------------------------------------------------------------------
def filter3(x, mode):
    """3-tap NaN-aware filter of a float32 frame sequence: mode 'median' (lower median) or 'mean'
    (torchcrepe.filter.median / .mean with win_length 3)."""
    x = x.contiguous().float()
    out = torch.empty_like(x)
    _check(x)
    _call("aicg_filter3", _ptr(x), _ptr(out), x.numel(), {"median": 0, "mean": 1}[mode], _stream(x))
    return out


_filtfilt_plans = {}


def _filtfilt_plan(b, a):
    """Host-side constants of scipy.signal.filtfilt(b, a, .) with default arguments: normalised coefficients, lfilter_zi initial
    conditions, padlen, and the warm-up length after which a zero-state start is indistinguishable in float64."""
    key = (tuple(np.asarray(b, np.float64)), tuple(np.asarray(a, np.float64)))
    if key not in _filtfilt_plans:
        from scipy.signal import lfilter_zi
        bb, aa = np.asarray(b, np.float64), np.asarray(a, np.float64)
        n = max(len(aa), len(bb))
        bb = np.concatenate([bb, np.zeros(n - len(bb))])
        aa = np.concatenate([aa, np.zeros(n - len(aa))])
        zi = np.ascontiguousarray(lfilter_zi(bb, aa), dtype=np.float64)
        rmax = float(np.max(np.abs(np.roots(aa)))) if n > 1 else 0.0
        if not rmax < 1.0:
            raise ValueError("filtfilt: unstable filter (max |pole| = %g)" % rmax)
        # warm-up: where the envelope of the impulse response has fallen 18 decades (clustered poles -- a Butterworth's -- decay
        # like n^k r^n, so the pole radius alone under-estimates it)
        from scipy.signal import lfilter
        imp = np.zeros(1 << 17)
        imp[0] = 1.0
        env = np.maximum.accumulate(np.abs(lfilter(bb, aa, imp))[::-1])[::-1]
        below = np.nonzero(env < 1e-18 * env[0])[0]
        if len(below) == 0:
            raise ValueError("filtfilt: impulse response too long for the block-parallel recurrence")
        warm = (int(below[0]) + 255) // 256 * 256
        _filtfilt_plans[key] = (np.ascontiguousarray(bb), np.ascontiguousarray(aa), zi, n - 1, 3 * n, warm)
    return _filtfilt_plans[key]


def filtfilt_f64(x, b, a, block=1024):
    """scipy.signal.filtfilt(b, a, x) (default odd padding / lfilter_zi) of a float64 device signal, block-parallel."""
    x = x.contiguous().double()
    bb, aa, zi, order, padlen, warm = _filtfilt_plan(b, a)
    n = x.numel()
    y = torch.empty_like(x)
    ext = torch.empty(n + 2 * padlen, dtype=torch.float64, device=x.device)
    mid = torch.empty_like(ext)
    _check(x)
    _call("aicg_filtfilt_f64", _ptr(x), _ptr(y), n, bb.ctypes.data, aa.ctypes.data, zi.ctypes.data, order, padlen, int(block),
          int(warm), _ptr(ext), _ptr(mid), _stream(x))
    return y


_resample_plans = {}


def _resample_plan(up, down, n_in, device):
    """Filter and trimming of scipy.signal.resample_poly(x float32, up, down) (Kaiser-5 windowed sinc, 10 * max(up, down) zero
    crossings each side), as the polyphase table the kernel reads."""
    g = math.gcd(int(up), int(down))
    up, down = int(up) // g, int(down) // g
    key = (up, down, str(device))
    if key not in _resample_plans:
        from scipy.signal import firwin
        max_rate = max(up, down)
        half_len = 10 * max_rate
        h = firwin(2 * half_len + 1, 1.0 / max_rate, window=("kaiser", 5.0)).astype(np.float32)
        h *= up
        n_pre_pad = down - half_len % down
        hpad = np.concatenate([np.zeros(n_pre_pad, np.float32), h])
        taps = (len(hpad) + up - 1) // up
        table = np.zeros((up, taps), np.float32)
        for ph in range(up):
            col = hpad[ph::up]
            table[ph, :len(col)] = col
        _resample_plans[key] = (torch.from_numpy(table).to(device), taps, (half_len + n_pre_pad) // down)
    table, taps, pre = _resample_plans[key]
    n_out = n_in * up
    n_out = n_out // down + bool(n_out % down)
    return up, down, table, taps, pre, n_out


def resample_poly_mono(x, sr_in, sr_out):
    """(C, N) or (N,) float32 device signal at sr_in -> (n_out,) float32 mono at sr_out: channel mean + polyphase FIR with
    scipy.signal.resample_poly's filter and trimming."""
    x = x.float()
    if x.dim() == 1:
        x = x.unsqueeze(0)
    assert x.stride(1) == 1
    c, n = x.shape
    up, down, table, taps, pre, n_out = _resample_plan(sr_out, sr_in, n, x.device)
    y = torch.empty(n_out, dtype=torch.float32, device=x.device)
    _check(x, table)
    _call("aicg_resample_poly", _ptr(x), _ptr(y), n, n_out, c, x.stride(0), up, down, _ptr(table), taps, pre, _stream(x))
    return y


def resample_poly(x, sr_in, sr_out):
    """(C, n) float32 or (n, C) int16 PCM (read as x / 32768) device signal at sr_in -> (C, n_out) float32 at sr_out, every channel
    for itself: scipy.signal.resample_poly(x, up, down, axis=1) with its default filter and trimming, n_out = ceil(n up / down).
    sr_in == sr_out: the input as float32, nothing is launched."""
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.int16):
        raise TypeError("resample_poly takes (channels, n) float32 or (frames, channels) int16, got %s %s" % (x.dtype, tuple(x.shape)))
    pcm = x.dtype == torch.int16
    if int(sr_in) == int(sr_out):
        return x.t().float().mul_(1.0 / 32768.0).contiguous() if pcm else x
    if not x.is_contiguous():
        raise ValueError("resample_poly takes a contiguous tensor (strides %s of shape %s)" % (x.stride(), tuple(x.shape)))
    n, c = (x.shape[0], x.shape[1]) if pcm else (x.shape[1], x.shape[0])
    up, down, table, taps, pre, n_out = _resample_plan(sr_out, sr_in, n, x.device)
    y = torch.empty((c, n_out), dtype=torch.float32, device=x.device)
    _check(x, table)
    _call("aicg_resample_poly_mc", _ptr(x), STEM_PCM16 if pcm else STEM_F32, _ptr(y), c, n, n_out, up, down, _ptr(table), taps, pre,
          _stream(x))
    return y


def row_sqnorm(v):
    v = v.contiguous().float()
    out = torch.empty(v.shape[0], dtype=torch.float32, device=v.device)
    _check(v)
    _call("aicg_row_sqnorm", _ptr(v), _ptr(out), v.shape[0], v.shape[1], _stream(v))
    return out


def knn8_update(dots, xnorm, qnorm, col_off, best_d, best_i, merge):
    """dots (rows, cols) inner products of one column chunk of the index -> running 8 nearest (squared L2, ascending)."""
    assert dots.dim() == 2 and dots.stride(1) == 1
    _check(dots, xnorm, qnorm, best_d, best_i)
    _call("aicg_knn8", _ptr(dots), dots.stride(0), _ptr(xnorm), _ptr(qnorm), dots.shape[0], dots.shape[1], int(col_off),
          _ptr(best_d), _ptr(best_i), 1 if merge else 0, _stream(dots))


def ivf_scan8(feats, vecs, list_off, probe, nprobe):
    """IndexIVFFlat scan: feats (rows, dim), vecs (N, dim) stored list by list, list_off (nlist + 1,) int64, probe (rows, >= nprobe)
    int64 nearest-first list ids -> (squared distances (rows, 8) ascending, storage positions (rows, 8), -1 where none)."""
    assert feats.is_contiguous() and vecs.is_contiguous() and probe.is_contiguous() and list_off.dtype == torch.int64
    rows, dim = feats.shape
    best_d = torch.empty((rows, 8), dtype=torch.float32, device=feats.device)
    best_p = torch.empty((rows, 8), dtype=torch.int64, device=feats.device)
    _check(feats, vecs, list_off, probe)
    _call("aicg_ivf_scan8", _ptr(feats), _ptr(vecs), _ptr(list_off), _ptr(probe), probe.shape[1], int(nprobe), rows, dim,
          _ptr(best_d), _ptr(best_p), _stream(feats))
    return best_d, best_p


def index_mix_(feats, big, best_d, best_i, rate, recompute=False):
    """feats (rows, dim) <- rate * sum_k w_k big[best_i[k]] + (1 - rate) * feats, w = inverse-square-distance weights (best_i < 0:
    weight 0).  `recompute`: distances re-evaluated directly from the gathered rows first (and stored in best_d)."""
    assert feats.is_contiguous() and big.is_contiguous() and best_d.is_contiguous() and best_i.is_contiguous()
    _check(feats, big, best_d, best_i)
    _call("aicg_index_mix", _ptr(feats), _ptr(big), _ptr(best_d), _ptr(best_i), feats.shape[0], feats.shape[1], float(rate),
          1 if recompute else 0, _stream(feats))
    return feats
