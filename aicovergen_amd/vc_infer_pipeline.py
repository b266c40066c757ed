"""RVC voice-conversion pipeline on the gfx950 kernels behind the reference's `VC` class
(reference src/vc_infer_pipeline.py:63-653; `Pipeline` is the name upstream RVC uses and BASELINE.json quotes).

Kept exactly: chunk geometry from Config (x_pad, x_query, x_center, x_max), the 48 Hz zero-phase high-pass, the
quietest-sample cut search, reflect padding, whole-track f0, per-chunk vc(), RMS mixing, peak limiting and the
truncating int16 conversion, the in-place `times = [hubert, f0, synth]` accounting.
Moved to the device: HuBERT, RMVPE (incl. the salience decode and the coarse-pitch quantiser), the feature
upsample / protect blend and the whole synthesizer.  Host numpy keeps the O(N) pre/post steps.
"""
import functools
import os
import traceback
import warnings
from time import time as ttime

import numpy as np
import torch
import torch.nn.functional as F
from scipy import signal

from . import _env
from . import ops
from . import dist as adist

BASE_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

bh, ah = signal.butter(N=5, Wn=48, btype="high", fs=16000)  # reference :22

input_audio_path2wav = {}

_NO_GROUP = "single"   # sentinel understood by dist.world(): this call must not communicate even if a process group exists


class _HostStream:
    """What the overlapped schedule needs of a torch.cuda.Stream when the kernels run synchronously on the host (the CPU emulator
    of tests/): every hand-over is already ordered."""

    def wait_stream(self, other): pass
    def wait_event(self, ev): pass
    def synchronize(self): pass
    def __enter__(self): return self
    def __exit__(self, *a): return False


class _HostEvent:
    def record(self, stream=None): pass


def _rms_frames(y, frame_length, hop_length):
    """librosa.feature.rms(y=y, frame_length=, hop_length=) of librosa 0.9.1: center=True with reflect padding,
    frame power mean, sqrt; returns (1, n_frames) float32 like librosa does for float32 input."""
    y = np.asarray(y)
    pad = frame_length // 2
    yp = np.pad(y, (pad, pad), mode="reflect")
    n_frames = 1 + (len(yp) - frame_length) // hop_length
    idx = np.arange(frame_length)[None, :] + hop_length * np.arange(n_frames)[:, None]
    power = np.mean(np.abs(yp[idx]) ** 2, axis=1)
    return np.sqrt(power)[None, :].astype(y.dtype if y.dtype in (np.float32, np.float64) else np.float32)


def change_rms(data1, sr1, data2, sr2, rate):
    """RMS-envelope mix of input (1) into output (2) (reference :41-60)."""
    rms1 = _rms_frames(data1, sr1 // 2 * 2, sr1 // 2)
    rms2 = _rms_frames(data2, sr2 // 2 * 2, sr2 // 2)
    rms1 = F.interpolate(torch.from_numpy(rms1).unsqueeze(0), size=data2.shape[0], mode="linear").squeeze()
    rms2 = F.interpolate(torch.from_numpy(rms2).unsqueeze(0), size=data2.shape[0], mode="linear").squeeze()
    rms2 = torch.max(rms2, torch.zeros_like(rms2) + 1e-6)
    data2 *= (torch.pow(rms1, torch.tensor(1 - rate)) * torch.pow(rms2, torch.tensor(rate - 1))).numpy()
    return data2


def _bracket_pipeline(fn):
    """While VC.pipeline runs, the f0 estimators may use the job's process group (VC._f0_group) -- and never outside it,
    whatever happens inside the call."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        self._in_pipeline = True
        try:
            return fn(self, *args, **kwargs)
        finally:
            self._in_pipeline = False
            self._group = None
    return wrapper


class _Call:
    """One VC.pipeline call: the arguments its chunk routine needs (model, net_g, sid, index, big_npy, index_rate, version, protect, if_f0,
    noise_fn, times, f0_args = get_f0's positional arguments), the track (audio_pad, bounds, p_len, mine = this rank's chunks), the schedule
    VC._schedule chose ("serial" | "one_launch" | "progressive", nseg, two_streams; "front" with `front` = the VoiceFront the call was
    given), and what the schedule's steps hand to each other."""

    def __init__(self, **args):
        self.__dict__.update(args)
        self.overlap, self.progressive = self.schedule != "serial", self.schedule == "progressive"
        self.pitch = self.pitchf = self.main = self.side = self.enc = None
        self.pad_dev = None       # overlapped schedules: the padded track as float32 on the device
        self.feats_of, self.pieces = {}, {}
        self.fronts = {}          # two streams: chunk -> (state of its queued encoder half, event, inputs kept alive)
        self.gru_seg, self.f0_bad = None, False    # progressive f0: the recurrence's handle (its exchange-timeout word is polled between chunks)
        self.marks, self.cover = [], (self.p_len, 0)    # progressive f0: (first frame, end frame, event) -- the frame range whose pitch exists once the event has fired
        self.tf0 = self.t2 = self.f0_wait = 0.0    # side stream forked; features (and, unless progressive, f0) exist; of that, waiting for f0

    def noise(self, ci):
        return self.noise_fn(ci, *self.bounds[ci]) if self.noise_fn is not None else None

    def frames_of(self, ci):
        s, e = self.bounds[ci]
        return s // self.window, (self.p_len if ci == len(self.bounds) - 1 else (e - self.window) // self.window)

    def chunk_pitch(self, ci):
        if self.if_f0 != 1:
            return None, None
        fa, fb = self.frames_of(ci)
        return self.pitch[:, fa:fb], self.pitchf[:, fa:fb]

    def publish(self, lo, hi, f0bak, coarse):
        """Progressive f0: write the pitch of frames [lo, hi), queued on `side`; with it the covered range grows to both sides."""
        hi = min(hi, self.p_len)
        if lo < hi:
            self.pitch[0, lo:hi] = coarse[: hi - lo]
            self.pitchf[0, lo:hi] = f0bak[: hi - lo].float()
        self.cover = (min(self.cover[0], lo), max(self.cover[1], hi))
        ev = torch.cuda.Event() if self.on_gpu else _HostEvent()
        ev.record(self.side)
        self.marks.append(self.cover + (ev,))

    def mark_of(self, ci):
        """Index of the first mark whose range covers the chunk's frames."""
        fa, fb = self.frames_of(ci)
        for m, (lo, hi, _) in enumerate(self.marks):
            if lo <= fa and min(fb, self.p_len) <= hi:
                return m
        return len(self.marks) - 1

    def order(self):
        """This rank's chunks in the order the loop takes them: as their pitch is published (middle-out) under the progressive schedule
        -- asked once the whole recurrence has been queued -- and first to last otherwise."""
        return sorted(self.mine, key=lambda ci: (self.mark_of(ci), ci)) if self.progressive else list(self.mine)

    def wait_pitch(self, stream, ci):
        if self.progressive:
            stream.wait_event(self.marks[self.mark_of(ci)][2])      # this chunk's pitch frames exist

    def drain(self):
        """The chunk's work is done (progressive: without waiting for the f0 stream's remaining segments)."""
        if not self.on_gpu:
            return
        if self.progressive:
            torch.cuda.current_stream(self.device).synchronize()
        else:
            torch.cuda.synchronize()


class VoiceFront:
    """What VC.pipeline computes of a track before the voice model matters (VC.front): the filtered track and its chunk plan (`audio`,
    `audio_pad`, `opt_ts`, `p_len`, `bounds`: what plan / chunk_bounds return), the UNTRANSPOSED f0 contour in Hz of the padded track
    (`f0`: float64 (p_len,), the estimate as it left the _estimated_f0 seam -- no key shift, no coarse bins; None for if_f0 != 1) and
    HuBERT's output per chunk (`feats`: [(1, T, C)], after final_proj for v1, before the retrieval mix, the x2 upsample and the protect
    copy).  Everything lives on the device and is only read afterwards.  `key`: what it was built under; pipeline(front=) refuses a
    front whose key differs from its own call in any field."""

    FIELDS = ("audio_len", "audio_sum", "f0_method", "crepe_hop_length", "filter_radius", "if_f0", "version", "x_pad", "x_query",
              "x_center", "x_max")

    def __init__(self, key, audio, audio_pad, opt_ts, p_len, bounds, f0, feats, schedule):
        self.key, self.audio, self.audio_pad, self.opt_ts, self.p_len, self.bounds = key, audio, audio_pad, opt_ts, p_len, bounds
        self.f0, self.feats, self.schedule = f0, feats, schedule

    def nbytes(self):
        ts = [self.audio, self.audio_pad] + ([self.f0] if self.f0 is not None else []) + list(self.feats)
        return sum(t.numel() * t.element_size() for t in ts)

    def check(self, key):
        for f in self.FIELDS:
            if self.key[f] != key[f]:
                raise ValueError("pipeline(front=): the front was built for %s = %r, this call has %r" % (f, self.key[f], key[f]))


class VC(object):
    def __init__(self, tgt_sr, config):
        self.x_pad, self.x_query, self.x_center, self.x_max, self.is_half = (
            config.x_pad, config.x_query, config.x_center, config.x_max, config.is_half)
        self.sr = 16000      # HuBERT input rate
        self.window = 160    # samples per f0 frame
        self.t_pad = self.sr * self.x_pad
        self.t_pad_tgt = tgt_sr * self.x_pad
        self.t_pad2 = self.t_pad * 2
        self.t_query = self.sr * self.x_query
        self.t_center = self.sr * self.x_center
        self.t_max = self.sr * self.x_max
        self.device = config.device
        self.rmvpe_path = None   # resolved on first use (_default_rmvpe_path), or set by the caller

    def get_optimal_torch_device(self, index: int = 0) -> torch.device:
        if torch.cuda.is_available():
            return torch.device(f"cuda:{index % torch.cuda.device_count()}")
        return torch.device("cpu")

    # ---- f0 ---------------------------------------------------------------------------------------------------
    def get_f0_crepe_computation(self, x, f0_min, f0_max, p_len, hop_length=160, model="full", dither=None):
        """mangio-crepe (reference :96-137).  The CREPE network is built lazily from torchcrepe's bundled weights, or
        injected as `self.model_crepe[model]` (tests / benchmarks use seeded parameters)."""
        from . import crepe
        print("Initiating prediction with a crepe_hop_length of: " + str(hop_length))
        x = x.to(self.device) if torch.is_tensor(x) else x   # a tensor stays on the device: crepe.quantile_normalise
        return crepe.mangio_crepe_f0(self._crepe(model), x, p_len, hop_length, dither=dither, group=self._f0_group(False))

    def _crepe(self, model):
        from . import crepe
        if not hasattr(self, "model_crepe"):
            self.model_crepe = {}
        if model not in self.model_crepe:
            self.model_crepe[model] = crepe.load_crepe(model, self.device)
        return self.model_crepe[model]

    def get_f0_official_crepe_computation(self, x, f0_min, f0_max, model="full", dither=None, to_host=True):
        """f0_method 'crepe' / 'crepe-tiny' (reference :139-165): torchcrepe.predict at the 10 ms hop with periodicity, 3-frame
        median of the periodicity, 3-frame mean of f0, unvoiced (periodicity < 0.1) frames zeroed.  `to_host=False` (hybrid on a
        device track): the float32 device tensor instead of numpy."""
        from . import crepe
        return crepe.official_crepe_f0(self._crepe(model), x, self.window, f0_min, f0_max, dither=dither,
                                       group=self._f0_group(False), to_host=to_host)

    HYBRID_METHODS = ("crepe", "crepe-tiny", "mangio-crepe", "mangio-crepe-tiny", "dio")

    def get_f0_hybrid_computation(self, methods_str, input_audio_path, x, f0_min, f0_max, p_len, filter_radius,
                                  crepe_hop_length, time_step):
        """hybrid[m1+m2+...] (reference :175-260): nan-median over the listed estimators on the quantile-normalised signal.
        A tensor x stays on the device (crepe.quantile_normalise: ops.abs_quantile / ops.div_scalar, numpy's bits; under a numpy other
        than 2.x it takes the host route); a numpy x is normalised on the host as before.  The `dio` row (reference :235-245) is DIO,
        StoneMask and the 3-point median of the NORMALISED signal without its first frame; it is computed in full on every rank, the
        crepe rows shard as they do alone.  Rows that are all device tensors (dio, crepe[-tiny] of a tensor x; at most
        ops.NANMEDIAN_MAX_ROWS) are joined by ops.nanmedian_rows, anything else by np.nanmedian: the same bits.  Like the reference,
        estimators of different lengths raise.  -> float64 numpy."""
        from . import crepe
        methods = methods_str.split("hybrid")[1].replace("[", "").replace("]", "").split("+")
        print("Calculating f0 pitch estimations for methods: %s" % str(methods))
        for method in methods:
            if method not in self.HYBRID_METHODS:
                raise NotImplementedError("hybrid f0: method %r is not served inside hybrid[...] (supported there: %s; pm runs alone as "
                                          "f0_method 'pm', harvest is not built for the MI355X yet)" % (method, ", ".join(self.HYBRID_METHODS)))
        on_device = torch.is_tensor(x)
        x = crepe.quantile_normalise(x.to(self.device) if on_device else x)
        on_device = torch.is_tensor(x)
        stack = []
        for method in methods:
            if method in ("crepe", "crepe-tiny"):
                f0 = self.get_f0_official_crepe_computation(x, f0_min, f0_max, "tiny" if method.endswith("tiny") else "full",
                                                            to_host=not on_device)[1:]
            elif method in ("mangio-crepe", "mangio-crepe-tiny"):
                f0 = self.get_f0_crepe_computation(x, f0_min, f0_max, p_len, crepe_hop_length,
                                                   "tiny" if method.endswith("tiny") else "full")
            else:
                f0 = self._dio_track(x, f0_min, f0_max, 10.0)[1:]
            stack.append(f0.double() if torch.is_tensor(f0) else np.asarray(f0, dtype=np.float64))
        for fc in stack:
            print(len(fc))
        print("Calculating hybrid median f0 from the stack of: %s" % str(methods))
        if len(stack) == 1:
            return stack[0].cpu().numpy() if torch.is_tensor(stack[0]) else stack[0]
        if all(torch.is_tensor(f) for f in stack) and len(stack) <= ops.NANMEDIAN_MAX_ROWS:
            if len(set(len(f) for f in stack)) != 1:
                raise ValueError("hybrid f0: the estimators gave %s frames" % [len(f) for f in stack])
            return ops.nanmedian_rows(torch.stack(stack)).cpu().numpy()
        stack = [f.cpu().numpy() if torch.is_tensor(f) else f for f in stack]
        return np.nanmedian(stack, axis=0)   # like the reference, estimators of different lengths raise here

    def get_f0_pm_computation(self, x, f0_min, f0_max, p_len):
        """f0_method 'pm' (reference :279-294): Praat's autocorrelation pitch at the 10 ms step, voicing threshold 0.6, zero-padded to
        p_len frames.  The track stays on the device (ops.pitch_ac); no weights, no communication: every rank computes the whole contour."""
        xd = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
        f0 = ops.pitch_ac(xd.to(self.device), self.sr, self.window / self.sr, float(f0_min), float(f0_max), 0.6)
        pad_size = (p_len - len(f0) + 1) // 2
        if pad_size < 0 or p_len - len(f0) - pad_size < 0:      # np.pad in the reference: "index can't contain negative values"
            raise ValueError("f0_method pm: %d frames do not fit p_len %d" % (len(f0), p_len))
        if pad_size > 0 or p_len - len(f0) - pad_size > 0:
            f0 = torch.nn.functional.pad(f0, (pad_size, p_len - len(f0) - pad_size))
        return f0.cpu().numpy()

    def get_f0_dio_computation(self, x, f0_min, f0_max):
        """f0_method 'dio' (reference :300-309): pyworld.dio at the 10 ms frame period, pyworld.stonemask, scipy's medfilt(f0, 3) ->
        len(x) // window + 1 frames.  The track stays on the device (ops.world_dio, ops.stonemask, ops.medfilt3); no weights, no
        communication: every rank computes the whole contour."""
        return self._dio_track(x, f0_min, f0_max, self.window / self.sr * 1000).cpu().numpy()

    def _dio_track(self, x, f0_min, f0_max, frame_period):
        """DIO, StoneMask, medfilt(3) of x (numpy or tensor) -> float64 device tensor."""
        xd = (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(self.device)
        f0 = ops.world_dio(xd, self.sr, frame_period, float(f0_min), float(f0_max))
        return ops.medfilt3(ops.stonemask(xd, f0, self.sr, frame_period))

    def _f0_group(self, explicit=True):
        """The process group the f0 estimators may communicate over.  Inside pipeline() the ranks of the job cut RMVPE's U-Net
        over time (rmvpe.E2E.features_sharded) and CREPE's frames (crepe.predict); a stand-alone get_f0 /
        get_f0_*_computation call (no pipeline in progress) NEVER communicates, whatever torch.distributed state the process
        has -- the other ranks would not join the collective.
        Returns None outside pipeline() or for a single-rank job.  Inside: the job's group; for the default group that is
        td.group.WORLD when `explicit` (RMVPE tests `group is not None`) and None otherwise (crepe hands it to dist.world())."""
        import torch.distributed as td
        if not getattr(self, "_in_pipeline", False) or not (td.is_available() and td.is_initialized()):
            return _NO_GROUP if not explicit else None
        g = getattr(self, "_group", None)
        if adist.single(td.get_world_size(g) if g is not None else td.get_world_size(), g):
            return _NO_GROUP if not explicit else None
        return g if (g is not None or not explicit) else td.group.WORLD

    _rmvpe_group = _f0_group

    @staticmethod
    def _default_rmvpe_path():
        """Where rmvpe.pt lives.  The reference reads <its checkout>/rvc_models/rmvpe.pt (src/vc_infer_pipeline.py:18,327: BASE_DIR is the
        parent of ITS src/); this module lives in another tree, so behind the shadow modules the file is looked up where main.py keeps its
        models: the `rvc_models_dir` global of the running main module (src/main.py:27), then rvc_models/ beside every sys.path entry
        (python src/main.py puts the reference's src/ there), then this repository's own rvc_models/."""
        import sys
        cands = []
        for name in ("__main__", "main"):
            d = getattr(sys.modules.get(name), "rvc_models_dir", None)
            if isinstance(d, str):
                cands.append(os.path.join(d, "rmvpe.pt"))
        for q in sys.path:
            if q:
                cands.append(os.path.join(os.path.dirname(os.path.abspath(q)), "rvc_models", "rmvpe.pt"))
        cands.append(os.path.join(BASE_DIR, "rvc_models", "rmvpe.pt"))
        for c in cands:
            if os.path.exists(c):
                return c
        return cands[-1]

    def _rmvpe(self):
        if not hasattr(self, "model_rmvpe"):
            from .rmvpe import RMVPE
            self.model_rmvpe = RMVPE(self.rmvpe_path or self._default_rmvpe_path(), is_half=self.is_half, device=self.device)
        return self.model_rmvpe

    def _estimate_f0(self, input_audio_path, x, p_len, f0_method, filter_radius, crepe_hop_length, _raw_f0=None):
        """The estimator's half of get_f0: the untransposed f0 track in Hz (numpy float64), passed through the _estimated_f0 seam.  Nothing
        here depends on the voice: get_f0 goes on with the key shift and the coarse bins, VC.front keeps the track as it is."""
        f0_min, f0_max = 50, 1100
        def host(a):   # crepe[-tiny] alone does no quantile: it takes the track from the host, as it always has
            return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)

        if _raw_f0 is not None:
            f0 = _raw_f0
        elif f0_method == "rmvpe":
            f0 = self._rmvpe().infer_from_audio(x, thred=0.03, group=self._rmvpe_group())
        elif f0_method in ("mangio-crepe", "mangio-crepe-tiny"):
            f0 = self.get_f0_crepe_computation(x, f0_min, f0_max, p_len, crepe_hop_length,
                                               "tiny" if f0_method.endswith("tiny") else "full")
        elif f0_method in ("crepe", "crepe-tiny"):
            f0 = self.get_f0_official_crepe_computation(host(x), f0_min, f0_max, "tiny" if f0_method.endswith("tiny") else "full")
        elif f0_method == "pm":
            f0 = self.get_f0_pm_computation(x, f0_min, f0_max, p_len)
        elif f0_method == "dio":
            f0 = self.get_f0_dio_computation(x, f0_min, f0_max)
        elif "hybrid" in f0_method:
            f0 = self.get_f0_hybrid_computation(f0_method, input_audio_path, x, f0_min, f0_max, p_len, filter_radius,
                                                crepe_hop_length, self.window / self.sr * 1000)
        else:
            raise NotImplementedError(
                "f0_method %r needs pyworld's harvest, which is not built for the MI355X yet "
                "(supported: rmvpe, pm, dio, mangio-crepe[-tiny], crepe[-tiny], hybrid[...] of the crepe methods and dio)" % f0_method)
        return np.asarray(self._estimated_f0(0, len(f0), np.asarray(f0, dtype=np.float64)), dtype=np.float64)

    def get_f0(self, input_audio_path, x, p_len, f0_up_key, f0_method, filter_radius, crepe_hop_length, inp_f0=None,
               _raw_f0=None):
        """-> (f0_coarse int64 (n,), f0 float64 (n,)) (reference :262-370).  `_raw_f0` (internal): the estimator's output
        when pipeline() has already run it on a side stream."""
        f0 = self._estimate_f0(input_audio_path, x, p_len, f0_method, filter_radius, crepe_hop_length, _raw_f0)
        tf0 = self.sr // self.window
        factor = pow(2, f0_up_key / 12)
        if inp_f0 is not None:
            f0 = f0 * factor
            factor = 1.0
            delta_t = np.round((inp_f0[:, 0].max() - inp_f0[:, 0].min()) * tf0 + 1).astype("int16")
            replace_f0 = np.interp(list(range(delta_t)), inp_f0[:, 0] * 100, inp_f0[:, 1])
            shape = f0[self.x_pad * tf0: self.x_pad * tf0 + len(replace_f0)].shape[0]
            f0[self.x_pad * tf0: self.x_pad * tf0 + len(replace_f0)] = replace_f0[:shape]
        f0bak, coarse = self._f0_tail(torch.from_numpy(f0).to(self.device), factor)
        return coarse.cpu().numpy(), f0bak.cpu().numpy()

    def _estimated_f0(self, lo, hi, f0):
        """Seam behind the estimator: EVERY f0 estimate passes through here before the key shift and the coarse quantiser -- the whole
        track (numpy float64, lo = 0) from get_f0 under the serial / one-launch schedules, frame range [lo, hi) (device float64 tensor)
        as the progressive schedule publishes it.  Identity; tests/test_bench_sizes.py replaces it to hold f0 fixed (the reference's own
        track) under whichever schedule pipeline() takes."""
        return f0

    def _f0_tail(self, f0, factor):
        """Key shift + mel-scale coarse bins of an f0 track (device float64) -> (f0 * factor float64, coarse int64), reference :360-370.
        The one place both schedules quantise: get_f0 (whole track) and the progressive schedule's per-range callback."""
        f0_mel_min = 1127 * np.log(1 + 50 / 700)
        f0_mel_max = 1127 * np.log(1 + 1100 / 700)
        return ops.f0_coarse(f0, factor, f0_mel_min, f0_mel_max)

    # ---- one chunk ----------------------------------------------------------------------------------------------
    def vc(self, model, net_g, sid, audio0, pitch, pitchf, times, index, big_npy, index_rate, version, protect,
           noise=None, keep_on_device=False, trim=0):
        """One padded chunk -> float32 waveform at tgt_sr (reference :372-472).  `noise` = (noise_z, noise_src)
        replaces the synthesizer's random draws (parity tests); `keep_on_device` returns the waveform as a device
        tensor instead of the reference's numpy array (used by pipeline(), which post-processes on the device).
        `trim`: return the waveform without its first and last `trim` samples (pipeline(): the chunk's padding) -- a synthesizer with
        the front / back split then does not synthesise them either (_vc_synth_back)."""
        t0 = ttime()
        feats, feats0 = self._vc_features(model, audio0, index, big_npy, index_rate, version,
                                          protect < 0.5 and pitch is not None and pitchf is not None)
        if self._sync():
            torch.cuda.synchronize()
        t1 = ttime()
        o = self._vc_synth(net_g, sid, audio0.shape[0], feats, feats0, pitch, pitchf, protect, noise, trim)
        if keep_on_device:
            if self._sync():
                torch.cuda.synchronize()
            audio1 = o[0, 0]
        else:
            audio1 = o[0, 0].data.cpu().float().numpy()
        t2 = ttime()
        times[0] += t1 - t0
        times[2] += t2 - t1
        return audio1

    def _vc_features(self, model, audio0, index, big_npy, index_rate, version, use_protect):
        """HuBERT features of one chunk (+ optional faiss index mix), reference :379-431.  Needs no pitch."""
        return self._vc_features_many(model, [audio0], index, big_npy, index_rate, version, use_protect)[0]

    def _vc_features_many(self, model, audios, index, big_npy, index_rate, version, use_protect):
        """_vc_features for several chunks -> [(feats, feats0)]: the HuBERT half (_hubert_many, which needs neither the voice nor the pitch)
        and, chunk by chunk, the voice's half (_vc_features_post)."""
        return [self._vc_features_post(model, lg, index, big_npy, index_rate, version, use_protect)
                for lg in self._hubert_many(model, audios, version)]

    def _hubert_many(self, model, audios, version):
        """HuBERT's hidden states of several chunks (layer 9 for v1 models, 12 for v2), before final_proj.  A model with
        `extract_features_many` (aicovergen_amd.hubert) runs the transformer's per-token layers once over all chunks; any other object
        with fairseq's `extract_features` is called chunk by chunk, as the reference does."""
        srcs = []
        for audio0 in audios:
            # audio0: host array (reference contract) or a slice of the track already resident on the device
            feats = audio0.float() if torch.is_tensor(audio0) else torch.from_numpy(np.ascontiguousarray(audio0)).float()
            if feats.dim() == 2:
                feats = feats.mean(-1)
            assert feats.dim() == 1, feats.dim()
            srcs.append(feats.view(1, -1).to(self.device))
        layer = 9 if version == "v1" else 12
        if len(srcs) > 1 and hasattr(model, "extract_features_many"):
            return model.extract_features_many(srcs, layer)
        return [model.extract_features(source=s, padding_mask=torch.zeros(s.shape, dtype=torch.bool), output_layer=layer)[0]
                for s in srcs]

    def _vc_features_post(self, model, logits, index, big_npy, index_rate, version, use_protect):
        return self._vc_features_voice(model.final_proj(logits) if version == "v1" else logits, index, big_npy, index_rate, use_protect)

    def _vc_features_voice(self, feats, index, big_npy, index_rate, use_protect, shared=False):
        """The voice's half of a chunk's features: the copy the protect blend needs and the retrieval mix -> (feats, feats0).
        `shared`: `feats` belongs to a VoiceFront and other calls will read it again -- the device mix works in place, so it gets a copy,
        and the untouched tensor itself serves as feats0."""
        mix = index is not None and index_rate != 0
        if shared:
            feats0 = feats if use_protect else None
            feats = feats.clone() if mix and hasattr(index, "mix_") else feats
        else:
            feats0 = feats.clone() if use_protect else None
        if mix and hasattr(index, "mix_"):
            # device retrieval (aicovergen_amd.retrieval.FeatureIndex): faiss' search for the file's index type (IVF-Flat with
            # its nprobe, or flat) + inverse-square blend, all in HBM
            feats = index.mix_(feats[0].contiguous(), index_rate).unsqueeze(0)
        elif mix and big_npy is not None:
            npy = feats[0].cpu().numpy().astype("float32")
            score, ix = index.search(npy, k=8)
            weight = np.square(1 / score)
            weight /= weight.sum(axis=1, keepdims=True)
            npy = np.sum(big_npy[ix] * np.expand_dims(weight, axis=2), axis=1)
            feats = torch.from_numpy(npy.astype("float32")).unsqueeze(0).to(self.device) * index_rate + (1 - index_rate) * feats
        return feats, feats0

    def _vc_synth(self, net_g, sid, n_samples, feats, feats0, pitch, pitchf, protect, noise, trim=0):
        """Features (+ pitch) of one chunk -> synthesizer output (1, 1, T) on the device, reference :433-466."""
        return self._vc_synth_back(net_g, self._vc_synth_front(net_g, sid, n_samples, feats, feats0, pitch, pitchf, protect, noise), trim)

    def _vc_synth_back(self, net_g, st, trim=0):
        """Vocoder half of a chunk's synthesis (state from _vc_synth_front), without the first and last `trim` samples (the reference
        synthesises the whole padded chunk and slices, :567-649).  The vocoder is convolutional: the kept samples depend on a few frames
        of the padding only (net_g.decoder_reach()), so infer_back is told the kept range and skips the rest of it -- the same samples,
        bit for bit (tests/test_synth_window.py).  AICG_SYNTH_WINDOW=0 (development switch): synthesise everything, then slice."""
        if "front" not in st:
            o = st["o"]
        else:
            n = st["front"]["z"].shape[2] * net_g.upp
            if trim and n > 2 * trim and _env.dev("AICG_SYNTH_WINDOW", "1") != "0":
                return net_g.infer_back(st["front"], st["pitchf"], st["ns"], keep=(trim, n - trim))[0]
            o = net_g.infer_back(st["front"], st["pitchf"], st["ns"])[0]
        return o[:, :, trim: o.shape[2] - trim] if trim else o

    def _vc_synth_front(self, net_g, sid, n_samples, feats, feats0, pitch, pitchf, protect, noise):
        """Encoder half of a chunk's synthesis: nearest x2 upsample + protect blend, text encoder, prior sample, reverse flow.
        Synthesizers without the front / back split (any object with the reference's `infer`) run whole here."""
        p_len = n_samples // self.window
        if 2 * feats.shape[1] < p_len:
            p_len = 2 * feats.shape[1]
        if pitch is not None and pitchf is not None:
            pitch = pitch[:, :p_len]
            pitchf = pitchf[:, :p_len]
        use_protect = feats0 is not None
        # nearest x2 upsample + protect blend, written channel-major for the synthesizer (:433-452)
        phone_ct = ops.feats_prepare(feats[0], p_len, feats0[0] if use_protect else None,
                                     pitchf[0].float() if use_protect else None, protect)
        nz, ns = noise if noise is not None else (None, None)
        if hasattr(net_g, "infer_front"):
            return {"front": net_g.infer_front(phone_ct, pitch, sid, nz), "pitchf": pitchf, "ns": ns}
        lens = torch.tensor([p_len], device=self.device).long()
        if pitch is not None and pitchf is not None:
            return {"o": net_g.infer(None, lens, pitch, pitchf, sid, noise_z=nz, noise_src=ns, phone_ct=phone_ct)[0]}
        return {"o": net_g.infer(None, lens, sid, noise_z=nz, noise_src=ns, phone_ct=phone_ct)[0]}

    def _sync(self):
        return torch.cuda.is_available() and str(self.device).startswith("cuda")

    # ---- whole track ----------------------------------------------------------------------------------------------
    def plan(self, audio):
        """High-pass, cut search and padding (reference :513-534) -> (audio_hp, audio_pad, opt_ts, p_len); audio_hp / audio_pad are
        float64 tensors on self.device.  `audio`: the reference's host array, or a float tensor already resident on the device
        (the opt-in hand-over from the separation stage).
        The zero-phase Butterworth runs block-parallel on the device (ops.filtfilt_f64; AICG_FILTFILT=host keeps scipy's
        sequential recurrence on the host): it agrees with scipy.signal.filtfilt to ~5e-8 of the signal peak, which is the
        rounding-noise floor of this ill-conditioned direct-form filter itself (tests/test_dsp.py compares both against an
        extended-precision run)."""
        dev = self.device if ops._lib.backend() != "emu" else torch.device("cpu")
        if torch.is_tensor(audio):
            a = audio.detach().to(dev).double().view(-1)
        else:
            a = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float64)).to(dev)
        if _env.dev("AICG_FILTFILT", "device") == "host" or a.numel() <= 3 * max(len(ah), len(bh)):
            audio = torch.from_numpy(np.ascontiguousarray(signal.filtfilt(bh, ah, a.cpu().numpy()))).to(dev)
        else:
            audio = ops.filtfilt_f64(a, bh, ah)
        n = audio.numel()

        def reflect_pad(x, k):   # np.pad(x, (k, k), mode="reflect"): a re-indexing (numpy reflects repeatedly when k >= n)
            if k < n:
                return F.pad(x.view(1, 1, -1), (k, k), mode="reflect").view(-1)
            period = max(2 * (n - 1), 1)
            i = (torch.arange(-k, n + k, device=x.device) % period)
            return x[torch.where(i >= n, period - i, i)]

        opt_ts = []
        if n + self.window > self.t_max:
            # 160-tap box sum in the reference's summation order + first-minimum search, on the device (bit-exact)
            audio_sum = ops.box_sum_f64(reflect_pad(audio, self.window // 2), n, self.window)
            centers = list(range(self.t_center, n, self.t_center))
            starts = [t - self.t_query for t in centers]
            lens = [min(t + self.t_query, n) - (t - self.t_query) for t in centers]
            idx = ops.argmin_abs_f64(audio_sum, starts, lens).cpu().numpy()
            opt_ts = [int(s0 + i) for s0, i in zip(starts, idx)]
        audio_pad = reflect_pad(audio, self.t_pad)
        return audio, audio_pad, opt_ts, audio_pad.shape[0] // self.window

    def chunk_bounds(self, audio_pad, opt_ts):
        """[(start, end)] sample ranges of audio_pad handed to vc(), in order (reference :567-637)."""
        bounds = []
        s = 0
        t = None
        for t in opt_ts:
            t = t // self.window * self.window
            bounds.append((s, t + self.t_pad2 + self.window))
            s = t
        bounds.append((t if t is not None else 0, audio_pad.shape[0]))
        return bounds

    # ---- whole track: the schedule's steps -------------------------------------------------------------------------------
    def _seeded_noise(self, net_g, seed):
        inter, upp = net_g.inter_channels, net_g.upp

        def noise_fn(ci, s, e, _seed=int(seed)):
            g = torch.Generator(device=self.device).manual_seed(_seed + ci)
            T = 2 * ((e - s - 400) // 320 + 1)
            return (torch.randn((1, inter, T), generator=g, device=self.device),
                    torch.randn(T * upp, generator=g, device=self.device))
        return noise_fn

    def _load_index(self, file_index, index_rate):
        if file_index == "" or not os.path.exists(file_index) or index_rate == 0:
            return None, None
        try:
            if _env.dev("AICG_GPU_KNN", "1") != "0":
                from . import retrieval
                return retrieval.load_index(file_index, self.device), None   # vectors in HBM, search + mix on the device
            import faiss   # the reference's host path: faiss search per chunk
            index = faiss.read_index(file_index)
            return index, index.reconstruct_n(0, index.ntotal)
        except Exception:
            traceback.print_exc()
            return None, None

    @staticmethod
    def _read_f0_file(f0_file):
        try:
            with open(f0_file.name, "r") as f:
                lines = f.read().strip("\n").split("\n")
            return np.array([[float(i) for i in line.split(",")] for line in lines], dtype="float32")
        except Exception:
            traceback.print_exc()

    def _schedule(self, net_g, if_f0, f0_method, world, inp_f0):
        """-> (schedule, f0 segments, two_streams): which of _f0_serial / _f0_one_launch / _f0_progressive starts this call -- decided here only.
        The f0 estimate does not depend on the HuBERT features and RMVPE's recurrent part occupies a handful of CUs, so on the GPU its
        kernels are queued on a side stream first and the feature extraction of every chunk runs on the main stream on top of them; the
        synthesizer passes start once both are done.  Everything is enqueued from this thread (a helper thread fights the launch loop
        for the GIL).  AICG_OVERLAP_F0=0 restores the reference's serial order (f0, then per chunk: features, synthesis).
        (AICG_F0_SEGMENTS on the host: the CPU tests walk the same progressive schedule, with the streams and events as no-ops;
        "1" = the recurrence as one launch.)  One rank on a GPU takes the progressive schedule too since the f0 chain became the longer
        branch of the phase (r4: HuBERT 74.9 ms, f0 79.4): the chunk loop then starts when HuBERT is done, on the middle chunks, while
        the recurrence finishes the track's ends -- 718.7 -> 713.9 ms per 240 s track at 8 segments (4: 715.5, 16: 715.6)."""
        schedule, nseg = self._f0_schedule(if_f0, f0_method, world, inp_f0)
        if schedule == "serial":
            return "serial", nseg, False
        return schedule, nseg, self._two_streams(net_g)

    def _two_streams(self, net_g):
        # Two streams: the encoder half of chunk i + 1 (text encoder + flow: ~140 short launches that leave most CUs idle and take the host
        # about as long to queue -- 40 us each -- as the GPU to run) is queued on a second stream underneath the vocoder of chunk i
        # (_chunk).  What that buys is small -- 2 ms per 240 s track: short launches running beside the vocoder cost it nearly what they
        # take alone (one stream: 674.7 ms, two: 667) -- and a stream priority changes nothing.  AICG_OVERLAP_SYNTH=0: one stream.
        return self._sync() and hasattr(net_g, "infer_front") and _env.dev("AICG_OVERLAP_SYNTH", "1") != "0"

    def _f0_schedule(self, if_f0, f0_method, world, inp_f0):
        """-> (schedule, f0 segments): the part of _schedule that does not look at the voice model (VC.front takes the same decision)."""
        on_gpu = self._sync()
        env_seg = int(_env.dev("AICG_F0_SEGMENTS", "0"))
        nseg = env_seg or (16 if world > 1 else (8 if on_gpu else 0))
        if not (if_f0 == 1 and f0_method == "rmvpe" and (on_gpu or nseg > 1) and _env.dev("AICG_OVERLAP_F0", "1") != "0"):
            return "serial", nseg
        # an f0 curve file (inp_f0) keeps the one-launch schedule, whose get_f0 splices it
        return ("progressive" if nseg > 1 and inp_f0 is None else "one_launch"), nseg

    def _run_f0(self, c, raw=None):
        pc, pcf = self.get_f0(*c.f0_args, _raw_f0=raw)
        return (torch.tensor(pc[:c.p_len], device=self.device).unsqueeze(0).long(),
                torch.tensor(pcf[:c.p_len], device=self.device).unsqueeze(0).float())

    def _features(self, c):
        many = self._vc_features_many(c.model, [c.pad_dev[c.bounds[ci][0]:c.bounds[ci][1]] for ci in c.mine], c.index, c.big_npy,
                                      c.index_rate, c.version, c.protect < 0.5 and c.if_f0 == 1)
        c.feats_of = dict(zip(c.mine, many))

    def _f0_serial(self, c):
        """The reference's order: f0 of the whole track; features and synthesis then go chunk by chunk through vc()."""
        if c.if_f0 == 1:
            c.pitch, c.pitchf = self._run_f0(c)
        if self._sync():
            torch.cuda.synchronize()
        c.t2 = ttime()
        c.times[1] += c.t2 - c.t1

    def _open_side(self, c):
        c.main = torch.cuda.current_stream(self.device) if c.on_gpu else _HostStream()
        # one side stream per VC object: the caching allocator keeps a block pool per stream, a fresh stream per call
        # would strand RMVPE's working set (a few GB for a 4-minute track) in up to 32 pools
        c.side = getattr(self, "_f0_stream", None) if c.on_gpu else _HostStream()
        if c.side is None:
            # high priority: the f0 branch is a short U-Net followed by a 70 ms recurrence on four CUs; dispatched first it
            # leaves the chip to HuBERT while the GRU runs, dispatched behind HuBERT's launches it finishes 40 ms later
            # (AICG_F0_PRIORITY=0: default priority)
            prio = -1 if _env.dev("AICG_F0_PRIORITY", "1") != "0" else 0
            c.side = self._f0_stream = torch.cuda.Stream(device=self.device, priority=prio)
        # one upload of the padded track: a pageable host->device copy on the default stream waits for the whole device,
        # side stream included, so the chunk loop must not issue any
        c.pad_dev = c.audio_pad.float()

    # ---- whole track: what does not depend on the voice ---------------------------------------------------------------------------
    def _front_key(self, audio, f0_method, crepe_hop_length, filter_radius, if_f0, version):
        """What a VoiceFront is valid for.  The audio is identified by its length and the int64 sum of its float32 bit patterns -- exact in
        any summation order, so a host array and its device copy give the same number; one reduction and a 8-byte read."""
        if torch.is_tensor(audio):
            a = audio.detach().float().contiguous().view(-1)
            n, total = a.numel(), int(a.view(torch.int32).sum(dtype=torch.int64).item())
        else:
            a = np.ascontiguousarray(audio, dtype=np.float32).reshape(-1)
            n, total = a.size, int(a.view(np.int32).sum(dtype=np.int64))
        return {"audio_len": int(n), "audio_sum": total, "f0_method": f0_method, "crepe_hop_length": crepe_hop_length,
                "filter_radius": filter_radius, "if_f0": if_f0, "version": version, "x_pad": self.x_pad, "x_query": self.x_query,
                "x_center": self.x_center, "x_max": self.x_max}

    def front(self, model, audio, input_audio_path, f0_method, if_f0, version, filter_radius, crepe_hop_length):
        """Everything pipeline() computes of a track before the voice model matters -> VoiceFront: plan and chunk bounds, the f0 estimate
        (untransposed) and HuBERT over every chunk.  pipeline(..., front=) then runs the voice's part only -- f0 tail, retrieval mix,
        synthesizer -- and returns what the call without a front returns, bit for bit: this takes the f0 schedule pipeline() would take
        (_f0_schedule; serial: the estimator through get_f0's first half and HuBERT chunk by chunk, overlapped: RMVPE on the side stream --
        in the same segments, so the classifier GEMM sees the same frame ranges -- under HuBERT over all chunks at once), so every kernel
        sees the shapes it sees there.  Never communicates (no process group).  A multi-workgroup BiGRU that timed out waiting for its
        partners is rerun on the single-workgroup kernel here, as _settle / _recover do, before the front is handed out."""
        key = self._front_key(audio, f0_method, crepe_hop_length, filter_radius, if_f0, version)
        audio, audio_pad, opt_ts, p_len = self.plan(audio)
        bounds = self.chunk_bounds(audio_pad, opt_ts)
        schedule, nseg = self._f0_schedule(if_f0, f0_method, 1, None)
        proj = (lambda lg: model.final_proj(lg)) if version == "v1" else (lambda lg: lg)
        f0 = f0_dev = None
        if schedule == "serial":
            if if_f0 == 1:
                f0 = self._estimate_f0(input_audio_path, audio_pad, p_len, f0_method, filter_radius, crepe_hop_length)
            feats = [proj(self._hubert_many(model, [audio_pad[s:e]], version)[0]) for s, e in bounds]
        else:
            c = _Call(device=self.device, on_gpu=self._sync(), window=self.window, audio_pad=audio_pad, bounds=bounds, p_len=p_len,
                      schedule=schedule, nseg=nseg, noise_fn=None)
            self._open_side(c)
            if c.progressive:       # created on `main` before the side stream forks from it, like the pitch tracks of _f0_progressive
                f0 = torch.zeros(p_len, dtype=torch.float64, device=self.device)

            def on_f0(lo, hi, est):
                est, hi = self._estimated_f0(lo, hi, est), min(hi, p_len)
                if lo < hi:
                    f0[lo:hi] = est[: hi - lo]
            c.side.wait_stream(c.main)
            with (torch.cuda.stream(c.side) if c.on_gpu else c.side):      # RMVPE is queued before HuBERT
                if c.progressive:
                    self._rmvpe().infer_progressive(c.pad_dev, 0.03, nseg, on_f0)
                else:
                    f0_dev = self._rmvpe().infer_from_audio_device(c.pad_dev, thred=0.03)
            feats = [proj(lg) for lg in self._hubert_many(model, [c.pad_dev[s:e] for s, e in bounds], version)]
            c.main.synchronize()
            c.side.synchronize()
            c.main.wait_stream(c.side)
            bad = c.progressive and self._rmvpe().last_segments.timed_out()
            if ops.gru_timed_out() or bad:
                warnings.warn("aicovergen_amd: the multi-workgroup BiGRU timed out waiting for its partner workgroups (busy or shared GPU); "
                              "f0 is recomputed on the single-workgroup kernel", RuntimeWarning)
                f0_dev = self._rmvpe().infer_from_audio_device(c.pad_dev, thred=0.03, two_workgroups=False)
            if f0_dev is not None:
                f0 = self._estimate_f0(input_audio_path, audio_pad, p_len, f0_method, filter_radius, crepe_hop_length,
                                       _raw_f0=f0_dev.cpu().numpy())
        if f0 is not None and not torch.is_tensor(f0):
            f0 = torch.from_numpy(np.ascontiguousarray(f0[:p_len])).to(self.device)
        if self._sync():
            torch.cuda.synchronize()
        return VoiceFront(key, audio, audio_pad, opt_ts, p_len, bounds, f0, feats, schedule)

    def _f0_front(self, c):
        """pipeline(front=): the voice's tail of the phase the front holds -- key shift and coarse bins of the cached contour (_f0_tail, on
        the device), this call's retrieval mix and protect copy on the cached HuBERT output -- then the chunk loop of the overlapped
        schedules, encoder halves on their own stream included."""
        c.main = torch.cuda.current_stream(self.device) if c.on_gpu else _HostStream()
        c.tf0 = ttime()
        if c.if_f0 == 1:
            f0bak, coarse = self._f0_tail(c.front.f0, pow(2, c.f0_args[3] / 12))      # f0_up_key
            c.pitch, c.pitchf = coarse.unsqueeze(0), f0bak.float().unsqueeze(0)
        tf1 = ttime()
        use_protect = c.protect < 0.5 and c.if_f0 == 1
        c.feats_of = {ci: self._vc_features_voice(c.front.feats[ci], c.index, c.big_npy, c.index_rate, use_protect, shared=True)
                      for ci in c.mine}
        self._open_enc(c)
        c.main.synchronize()
        c.t2 = ttime()
        c.times[0] += c.t2 - tf1
        c.times[1] += tf1 - c.tf0

    def _f0_one_launch(self, c):
        """f0 on the side stream with the recurrence as one launch, every chunk's features on `main` on top of it; the host joins both."""
        self._open_side(c)
        c.side.wait_stream(c.main)
        c.tf0 = ttime()
        with (torch.cuda.stream(c.side) if c.on_gpu else c.side):      # RMVPE is queued before HuBERT
            f0_dev = self._rmvpe().infer_from_audio_device(c.pad_dev, thred=0.03, group=self._rmvpe_group())
        self._features(c)
        self._settle(c, f0_dev)
        self._open_enc(c)

    def _f0_progressive(self, c):
        """Progressive f0 (multi-GPU: every rank runs the whole-track BiGRU, N x 32 ms for N x 240 s): the recurrence is queued in
        segments, and the pitch of a frame range exists as soon as BOTH directions have passed it -- the middle of the track at half
        the recurrence time, its ends last.  The chunk loop then takes this rank's chunks middle-out and waits per chunk (events), not
        for the whole track.  Same values as the one-launch form (GruSegments); the host never sees f0.
        NOTE: this schedule never calls get_f0 (an override of VC.get_f0 is bypassed; the estimate passes _estimated_f0 and the shared
        _f0_tail instead)."""
        self._open_side(c)
        # the device-resident pitch tracks are created and filled on `main` BEFORE the side stream forks from it -- on_f0 writes
        # slices of them on `side`, and a fill that could run after such a write would erase it
        c.pitch = torch.ones((1, c.p_len), dtype=torch.long, device=self.device)
        c.pitchf = torch.zeros((1, c.p_len), dtype=torch.float32, device=self.device)
        c.side.wait_stream(c.main)
        c.tf0 = ttime()
        factor = pow(2, c.f0_args[3] / 12)      # f0_up_key

        def on_f0(lo, hi, f0):
            c.publish(lo, hi, *self._f0_tail(self._estimated_f0(lo, hi, f0), factor))
        with (torch.cuda.stream(c.side) if c.on_gpu else c.side):      # RMVPE is queued before HuBERT
            self._rmvpe().infer_progressive(c.pad_dev, 0.03, c.nseg, on_f0, group=self._rmvpe_group())
        c.gru_seg = self._rmvpe().last_segments
        self._features(c)
        # the host first queues the first chunk's encoder half and settles THEN -- its ~140 short launches take the host 6 ms to issue,
        # which now pass under the tail of HuBERT instead of in front of the first vocoder
        self._open_enc(c)
        self._settle(c)

    def _settle(self, c, f0_dev=None):
        """The host meets the device: every chunk's features exist.  Under the one-launch schedule (`f0_dev`: the estimate queued on the
        side stream) it waits for f0 as well and turns it into the pitch tracks; the progressive schedule's pitch arrives during the
        chunk loop.  times[1] is the f0 branch's own wall time (it overlaps times[0])."""
        c.main.synchronize()
        tf1 = c.t2 = ttime()
        # an early exchange timeout: do not synthesise a whole track from invalid pitch
        c.f0_bad = bool(c.progressive and c.gru_seg.timed_out())
        if f0_dev is not None:
            c.side.synchronize()
            c.main.wait_stream(c.side)
            f0_host = f0_dev.cpu().numpy()
            if ops.gru_timed_out():  # multi-workgroup GRU starved of its partners under the HuBERT load: single-workgroup rerun
                f0_host = self._rmvpe().infer_from_audio_device(c.pad_dev, thred=0.03, two_workgroups=False).cpu().numpy()
            c.pitch, c.pitchf = self._run_f0(c, f0_host)
            c.t2 = ttime()
        c.f0_wait = c.t2 - tf1
        c.times[0] += tf1 - c.tf0
        c.times[1] += c.t2 - c.tf0

    def _open_enc(self, c):
        """Two streams: fork the encoder-half stream from `main` and queue the first chunk's encoder half on it."""
        if not c.two_streams:
            return
        c.enc = getattr(self, "_enc_stream", None)
        if c.enc is None:
            c.enc = self._enc_stream = torch.cuda.Stream(device=self.device)
        c.enc.wait_stream(c.main)          # features, pitch tracks, sid: everything the fronts read exists on `main` by now
        if c.order():
            self._queue_front(c, c.order()[0])

    def _queue_front(self, c, ci):
        s, e = c.bounds[ci]
        pc, pcf = c.chunk_pitch(ci)
        feats, feats0 = c.feats_of.pop(ci)
        c.wait_pitch(c.enc, ci)
        with torch.cuda.stream(c.enc):
            noise = c.noise(ci)
            st = self._vc_synth_front(c.net_g, c.sid, e - s, feats, feats0, pc, pcf, c.protect, noise)
            ev = torch.cuda.Event()
            ev.record(c.enc)
        c.fronts[ci] = (st, ev, (feats, feats0, pc, pcf, noise))

    def _chunk(self, c, ci, front=None, after=None):
        """Synthesise chunk `ci` and keep its trimmed piece -- the one place a chunk becomes audio, whatever the schedule and in recovery.
        `front`: its encoder half as _queue_front left it (two streams).  Then the HOST queues the vocoder of chunk i first and the
        encoder half of chunk i + 1 behind it: the other way round the main stream stood idle for the 6 ms the host needs to issue the
        short launches (kernel trace of round 5, profiles/r05_timeline.json: 6.5 + 6.1 ms at two chunk boundaries, the first vocoder
        behind TWO encoder halves)."""
        s, e = c.bounds[ci]
        pc, pcf = c.chunk_pitch(ci)
        if not c.overlap:       # serial: vc() runs features and synthesis and accumulates times[0] / times[2] itself
            out = self.vc(c.model, c.net_g, c.sid, c.audio_pad[s:e], pc, pcf, c.times, c.index, c.big_npy, c.index_rate, c.version,
                          c.protect, noise=c.noise(ci), keep_on_device=True, trim=self.t_pad_tgt)
        else:
            noise = c.noise(ci) if front is None else None
            ts0 = ttime()
            if front is not None:
                st, ev, keep = front    # the front's inputs stay referenced until the drain below: nothing is recycled under the other stream
                c.main.wait_event(ev)
                out = self._vc_synth_back(c.net_g, st, self.t_pad_tgt)[0, 0]
                if after is not None:
                    self._queue_front(c, after)
            else:
                feats, feats0 = c.feats_of.pop(ci)
                c.wait_pitch(c.main, ci)
                out = self._vc_synth(c.net_g, c.sid, e - s, feats, feats0, pc, pcf, c.protect, noise, self.t_pad_tgt)[0, 0]
            c.drain()
            c.times[2] += ttime() - ts0
        c.pieces[ci] = out      # already without the chunk's padding (_vc_synth_back)
        return c.pieces[ci]

    def _chunk_loop(self, c):
        order = c.order()
        for ci, after in zip(order, order[1:] + [None]):
            if c.f0_bad:
                break
            self._chunk(c, ci, c.fronts.pop(ci, None), after)
            if c.progressive and c.gru_seg.timed_out():    # polled per chunk (4 bytes): at most one chunk is synthesised from bad pitch
                c.f0_bad = True
        if c.progressive:
            if c.on_gpu:
                torch.cuda.synchronize()
            c.fronts.clear()

    def _recover(self, c):
        """The multi-workgroup recurrence starved of its partners (a busy or shared GPU): this rank's f0 is invalid.  Recompute it locally
        on the single-workgroup kernel (no collective: the other ranks may be fine) and redo this rank's chunks."""
        warnings.warn("aicovergen_amd: the multi-workgroup BiGRU timed out waiting for its partner workgroups (busy or shared GPU); "
                      "f0 and this rank's chunks are recomputed on the single-workgroup kernel -- this call costs about twice "
                      "its usual time", RuntimeWarning)
        c.pitch, c.pitchf = self._run_f0(c, self._rmvpe().infer_from_audio_device(c.pad_dev, thred=0.03, two_workgroups=False).cpu().numpy())
        self._features(c)
        for ci in c.mine:
            self._chunk(c, ci)
        if c.on_gpu:
            torch.cuda.synchronize()

    def _post(self, audio_opt, audio, tgt_sr, resample_sr, rms_mix_rate, device_out=False):
        """The joined float32 track at tgt_sr -> the call's int16 result: RMS mix with the input, peak limit, truncating cast (reference :639-651).
        `device_out`: the int16 tensor stays on the device (the same samples) instead of being copied to a host array."""
        if rms_mix_rate != 1:
            # change_rms on the device: frame RMS envelopes (1 s frames, 0.5 s hop), linear interpolation, power mix
            rms1 = ops.frame_rms(audio, 16000 // 2 * 2, 16000 // 2)
            rms2 = ops.frame_rms(audio_opt, tgt_sr // 2 * 2, tgt_sr // 2)
            ops.rms_mix_(audio_opt, rms1, rms2, rms_mix_rate)
        if resample_sr >= 16000 and tgt_sr != resample_sr:
            # optional output resampling (rvc_infer passes resample_sr=0), after change_rms as in the reference (:639-644)
            audio_opt = ops.resample_poly(audio_opt[None], tgt_sr, resample_sr)[0]
        audio_max = float(ops.absmax(audio_opt).item()) / 0.99
        max_int16 = 32768
        if audio_max > 1:
            max_int16 /= audio_max
        out = ops.to_int16(audio_opt, max_int16)
        return out if device_out else out.cpu().numpy()

    @_bracket_pipeline
    def pipeline(self, model, net_g, sid, audio, input_audio_path, times, f0_up_key, f0_method, file_index, index_rate,
                 if_f0, filter_radius, tgt_sr, resample_sr, rms_mix_rate, version, protect, crepe_hop_length, f0_file=None,
                 noise_fn=None, group=None, noise_seed=None, device_out=False, front=None):
        """Same contract as the reference (:474-653): float32 16 kHz mono in, int16 at tgt_sr out (`device_out`: as an int16 tensor left
        on the device, for a caller that goes on there; the samples are the same).
        `noise_fn(chunk_index, start, end) -> (noise_z, noise_src)` injects the synthesizer noise (tests); `noise_seed`
        instead draws it from a per-chunk seeded device generator, which makes the output independent of how chunks are
        distributed over ranks UP TO fp32 SUMMATION ORDER: the HuBERT transformer runs once over all of a rank's chunks
        (HubertModel.extract_features_many), so the GEMM tiles -- and the order of their fp32 sums -- depend on how many chunks a
        rank owns; outputs of different world sizes agree to ~1e-6 relative (tests/test_dist.py states the bound), ranks of one run
        agree bit for bit; `group` shards the chunk loop over the ranks of a torch.distributed process group.
        `front`: a VoiceFront of this audio (VC.front, same f0 method and model version): plan, f0 estimate and HuBERT are taken from it
        and only the voice's part runs -- the same samples, bit for bit.  ValueError if it was built for something else (the field is
        named), or together with an f0 curve file or a process group."""
        if front is not None and (f0_file is not None or group is not None):
            raise ValueError("pipeline(front=) does not take %s" % ("an f0_file curve" if f0_file is not None else "a process group"))
        if noise_fn is None and noise_seed is not None:
            noise_fn = self._seeded_noise(net_g, noise_seed)
        index, big_npy = self._load_index(file_index, index_rate)
        self._group = group   # the crepe f0 methods shard their frames over it, RMVPE its U-Net
        tp0 = ttime()
        if front is None:
            audio, audio_pad, opt_ts, p_len = self.plan(audio)
        else:
            front.check(self._front_key(audio, f0_method, crepe_hop_length, filter_radius, if_f0, version))
            audio, audio_pad, opt_ts, p_len = front.audio, front.audio_pad, front.opt_ts, front.p_len
        t1 = ttime()
        inp_f0 = self._read_f0_file(f0_file) if hasattr(f0_file, "name") else None
        sid = torch.tensor(sid, device=self.device).unsqueeze(0).long()
        bounds = self.chunk_bounds(audio_pad, opt_ts) if front is None else front.bounds
        rank, world = adist.world(group)
        if front is None:
            schedule, nseg, two_streams = self._schedule(net_g, if_f0, f0_method, world, inp_f0)
        else:
            schedule, nseg, two_streams = "front", 0, self._two_streams(net_g)
        c = _Call(device=self.device, on_gpu=self._sync(), window=self.window, model=model, net_g=net_g, sid=sid, index=index,
                  big_npy=big_npy, index_rate=index_rate, version=version, protect=protect, if_f0=if_f0, noise_fn=noise_fn, times=times,
                  f0_args=(input_audio_path, audio_pad, p_len, f0_up_key, f0_method, filter_radius, crepe_hop_length, inp_f0),
                  audio_pad=audio_pad, bounds=bounds, mine=[ci for ci in range(len(bounds)) if ci % world == rank], p_len=p_len,
                  schedule=schedule, nseg=nseg, two_streams=two_streams, t1=t1, front=front)
        # f0 and features: queued (overlapped schedules) or done (serial) when this returns; c.t2 is set
        {"serial": self._f0_serial, "one_launch": self._f0_one_launch, "progressive": self._f0_progressive,
         "front": self._f0_front}[schedule](c)
        self._chunk_loop(c)
        if c.progressive and (ops.gru_timed_out() or c.f0_bad):
            self._recover(c)
        tc1 = ttime()
        pieces = adist.gather_pieces(c.pieces, len(bounds), self.device, group)
        tj1 = ttime()
        audio_opt = self._post(torch.cat([pieces[i] for i in range(len(bounds))]).contiguous(), audio, tgt_sr, resample_sr, rms_mix_rate,
                               device_out)
        # wall-clock split of this call (host pre-processing, f0, chunk loop, join + host post-processing)
        # (overlapped schedule: f0_s = features of every chunk with the f0 branch underneath, f0_wait_s of it spent waiting for f0)
        self.last_profile = {"plan_s": t1 - tp0, "f0_s": c.t2 - t1, "chunks_s": tc1 - c.t2, "post_s": ttime() - tc1,
                             "f0_wait_s": c.f0_wait, "overlap_f0": float(c.overlap), "join_s": tj1 - tc1,
                             "f0_progressive": float(c.progressive)}
        if front is not None:       # f0_s above: the voice's tail of the front's phase
            self.last_profile["front_reused"] = 1.0
        return audio_opt


Pipeline = VC  # the name BASELINE.json / upstream RVC use for this class
