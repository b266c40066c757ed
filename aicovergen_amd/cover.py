"""The tail of the reference's song_cover_pipeline on the device (src/main.py:206-233): the vocal effects chain of add_audio_effects
(pedalboard HighpassFilter -> Compressor(ratio=4, threshold_db=-15) -> Reverb) and the three-stem mix of combine_audio (pydub).

Array level, on tensors where the bound library runs (device memory for the gfx950 library):
    vocal_effects(x, sr, reverb_rm_size, reverb_wet, reverb_dry, reverb_damping, state=None) -> (y, state)
    mix_stems(main_i16, main_sr, backup_i16, backup_sr, inst_i16, inst_sr, main_gain, backup_gain, inst_gain) -> (int16, sr)
    highpass / compressor / reverb: the three stages one at a time (what src/compat/pedalboard wraps)
File level, with main.py's signatures and output names:
    add_audio_effects(audio_path, reverb_rm_size, reverb_wet, reverb_dry, reverb_damping) -> '<stem>_mixed.wav'
    combine_audio(audio_paths, output_path, main_gain, backup_gain, inst_gain, output_format)
    pitch_shift(audio_path, pitch_change) -> '<stem>_p{pitch_change}.wav'   (main.py:138-147, `-pall N`)
and on a signal: pitch_shift_signal(x, sr, semitones, offsets=None) -> (y, offsets): sox's `pitch` as WSOLA + resampling (csrc/pitch.hip)
The whole cover in one call, stems handed from stage to stage in device memory:
    CoverSession(mdxnet_models_dir, rvc_models_dir, output_dir).song_cover_pipeline(song_input, voice_model, pitch_change, keep_files, ...)
    song_cover_pipeline(...) with a default session, and `python -m aicovergen_amd.cover` with main.py's flags (src/main.py:236-339)

Parameters become coefficients here, in float32 the way JUCE derives them; the recurrences and the mix run in
csrc/fx.hip.  The effects are computed in segments that restart from zero state `warm` samples early; the warm-up is chosen so that
the true state's influence has decayed below 2^-30 of its size (warmup_* below).  `segment=0` runs one segment: the exact
sequential recurrence.
"""
import math
import os
import shutil
import subprocess
import tempfile
import wave

import numpy as np
import torch

from . import _env, _lib, ops

_LN2_30 = 30.0 * math.log(2.0)


def _device():
    return torch.device("cuda", torch.cuda.current_device()) if _lib.backend() == "hip" else torch.device("cpu")


# ---------------------------------------------------------------------------------------------------
# Coefficients (float32, in JUCE's order of operations)
# ---------------------------------------------------------------------------------------------------
def highpass_coefs(sr, cutoff_hz=50.0):
    """IIR::Coefficients::makeFirstOrderHighPass: n = tan(pi fc / sr); (b0, b1, a0, a1) = (1, -1, n + 1, n - 1), normalised by
    multiplying with 1 / a0.  Returns (b0, b1, a1) as float32."""
    f32 = np.float32
    n = np.tan(f32(np.pi) * f32(cutoff_hz) / f32(sr))
    a0inv = f32(1.0) / (n + f32(1.0))
    return f32(1.0) * a0inv, f32(-1.0) * a0inv, (n - f32(1.0)) * a0inv


def compressor_coefs(sr, threshold_db, ratio, attack_ms=1.0, release_ms=100.0):
    """dsp::Compressor + BallisticsFilter: cte(t) = exp(-2 pi 1000 / (sr t)) in double, rounded to float (0 below 1 us);
    threshold = 10^(dB / 20) in float.  Returns (cte_attack, cte_release, threshold, threshold_inv, ratio_inv) as float32."""
    f32 = np.float32
    if ratio < 1.0:
        raise ValueError("compressor ratio must be >= 1, got %r" % (ratio,))
    exp_factor = -2.0 * math.pi * 1000.0 / float(sr)

    def cte(t_ms):
        t = float(f32(t_ms))
        return f32(0.0) if t < 1.0e-3 else f32(math.exp(exp_factor / t))

    thr = np.power(f32(10.0), f32(threshold_db) * f32(0.05)) if f32(threshold_db) > f32(-200.0) else f32(0.0)
    return cte(attack_ms), cte(release_ms), thr, f32(1.0) / thr, f32(1.0) / f32(ratio)


def reverb_coefs(room_size, damping, wet_level, dry_level, width=1.0):
    """juce::Reverb::setParameters / updateDamping.  Returns (gain, damp, feedback, wet1, wet2, dry) as float32."""
    f32 = np.float32
    wet = f32(wet_level) * f32(3.0)
    return (f32(0.015), f32(damping) * f32(0.4), f32(room_size) * f32(0.28) + f32(0.7),
            f32(0.5) * wet * (f32(1.0) + f32(width)), f32(0.5) * wet * (f32(1.0) - f32(width)), f32(dry_level) * f32(2.0))


# ---------------------------------------------------------------------------------------------------
# Warm-up rule: samples after which a wrong initial state has decayed below 2^-30 of its size
# ---------------------------------------------------------------------------------------------------
def _decay_len(r):
    r = abs(float(r))
    if r >= 1.0:
        return None  # does not decay: only the exact sequential run is correct
    if r == 0.0:
        return 1
    return int(math.ceil(_LN2_30 / -math.log(r)))


def warmup_dynamics(hp=None, comp=None):
    """High-pass pole a1; the envelope follower contracts by max(cte) per sample.  The high-pass error feeds the compressor, so the
    two lengths add."""
    w = 0
    for r in ([hp[2]] if hp is not None else []) + ([max(comp[0], comp[1])] if comp is not None else []):
        d = _decay_len(r)
        if d is None:
            return None
        w += d
    return w


def comb_lengths(sr, channel):
    return [int(sr) * (t + 23 * channel) // 44100 for t in (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)]


def allpass_lengths(sr, channel):
    return [int(sr) * (t + 23 * channel) // 44100 for t in (556, 441, 341, 225)]


def warmup_reverb(sr, coefs):
    """A comb loop (delay L, one-pole damping with unit DC gain) shrinks a state error by `feedback` per round trip: k + 1 round
    trips of the longest comb, k = ceil(30 ln 2 / -ln feedback); then every all-pass (coefficient 0.5) forgets its own state in 30
    round trips."""
    k = _decay_len(coefs[2])
    if k is None:
        return None
    return (k + 1) * max(comb_lengths(sr, 1)) + 30 * sum(allpass_lengths(sr, 1))


def _segments(n, warm, segment, default_parallel, minimum):
    """(seg_len, warm) for one call: segment=0 or a non-decaying recurrence -> one segment."""
    if segment == 0 or warm is None or n == 0:
        return 0, 0
    if segment is None:
        segment = max(minimum, -(-n // default_parallel))
    return int(segment), int(warm)


# ---------------------------------------------------------------------------------------------------
# Array level
# ---------------------------------------------------------------------------------------------------
def _as_2d(x):
    if x.dtype != torch.float32:
        raise TypeError("vocal effects take float32 signals, got %s" % x.dtype)
    if x.dim() == 1:
        return x.contiguous().view(1, -1), True
    if x.dim() != 2 or x.shape[0] not in (1, 2):
        raise ValueError("vocal effects take (n,) or (channels, n) signals with 1 or 2 channels, got %s" % (tuple(x.shape),))
    return x.contiguous(), False


def _dyn(x, sr, hp, comp, state, segment):
    x2, flat = _as_2d(x)
    flags = (ops.FX_HPF if hp is not None else 0) | (ops.FX_COMP if comp is not None else 0)
    coefs = tuple(hp if hp is not None else (1.0, 0.0, 0.0)) + tuple(comp if comp is not None else (0.0, 0.0, 0.0, 0.0, 1.0))
    seg, warm = _segments(x2.shape[1], warmup_dynamics(hp, comp), segment, 16384, 512)
    y, st = ops.fx_dynamics(x2, state, seg, warm, coefs, flags)
    return (y.view(-1) if flat else y), st


def highpass(x, sr, cutoff_hz=50.0, state=None, segment=None):
    """pedalboard.HighpassFilter(cutoff_frequency_hz).  x: (n,) or (C, n) float32; state: (C, 2) from a previous call or None.
    Returns (y, state)."""
    return _dyn(x, sr, highpass_coefs(sr, cutoff_hz), None, state, segment)


def compressor(x, sr, threshold_db=0.0, ratio=1.0, attack_ms=1.0, release_ms=100.0, state=None, segment=None):
    """pedalboard.Compressor (peak detector, per channel).  Returns (y, state)."""
    return _dyn(x, sr, None, compressor_coefs(sr, threshold_db, ratio, attack_ms, release_ms), state, segment)


def reverb(x, sr, room_size=0.5, damping=0.5, wet_level=0.33, dry_level=0.4, width=1.0, state=None, segment=None):
    """pedalboard.Reverb (juce::Reverb: mono for one channel, the stereo cross-mix for two).  Returns (y, state)."""
    x2, flat = _as_2d(x)
    coefs = reverb_coefs(room_size, damping, wet_level, dry_level, width)
    seg, warm = _segments(x2.shape[1], warmup_reverb(sr, coefs), segment, 512, 4096)
    y, st = ops.fx_reverb(x2, int(sr), state, seg, warm, coefs)
    return (y.view(-1) if flat else y), st


class FxState:
    """What vocal_effects carries from one call to the next: high-pass + envelope per channel, and the reverb's delay lines."""

    def __init__(self, sr, channels, dyn, rev):
        self.sr, self.channels, self.dyn, self.rev = int(sr), int(channels), dyn, rev


def vocal_effects(x, sr, reverb_rm_size, reverb_wet, reverb_dry, reverb_damping, state=None, segment=None):
    """add_audio_effects' board on a signal: HighpassFilter() -> Compressor(ratio=4, threshold_db=-15) -> Reverb(room_size,
    dry_level, wet_level, damping).  x: (n,) or (C, n) float32 (C = 1 or 2).  Returns (y, FxState); passing the state back in
    continues the signal (main.py's 1-second chunks with reset=False)."""
    x2, _ = _as_2d(x)
    if state is not None and (state.sr != int(sr) or state.channels != x2.shape[0]):
        raise ValueError("vocal_effects: state is for %d Hz x %d channels, signal is %d Hz x %d" % (state.sr, state.channels, sr,
                                                                                                x2.shape[0]))
    hp = highpass_coefs(sr)
    comp = compressor_coefs(sr, -15.0, 4.0)
    z, dyn = _dyn(x, sr, hp, comp, None if state is None else state.dyn, segment)
    y, rev = reverb(z, sr, reverb_rm_size, reverb_damping, reverb_wet, reverb_dry, state=None if state is None else state.rev,
                    segment=segment)
    return y, FxState(sr, x2.shape[0], dyn, rev)


def db_to_float(db):
    """pydub.utils.db_to_float: the amplitude factor audioop.mul receives."""
    return 10 ** (float(db) / 20)


def pydub_slice_frames(frames, rate):
    """Frames of seg[0:] in pydub (overlay slices its first operand so): the length is rounded to whole milliseconds and turned
    back into frames, int(round(1000 (n / rate)) (rate / 1000.0))."""
    return int(round(1000 * (float(frames) / rate)) * (rate / 1000.0))


def ratecv_frames(frames, rate_in, rate_out):
    """Frames audioop.ratecv produces from `frames` input frames with a fresh state (pydub skips the call for equal rates)."""
    if frames == 0 or rate_in == rate_out:
        return frames
    g = math.gcd(rate_in, rate_out)
    return (frames - 1) * (rate_out // g) // (rate_in // g) + 1


def _as_pcm(x):
    if x.dtype != torch.int16:
        raise TypeError("mix_stems takes int16 PCM, got %s" % x.dtype)
    if x.dim() == 1:
        x = x.view(-1, 1)
    if x.dim() != 2 or x.shape[1] not in (1, 2):
        raise ValueError("mix_stems takes (frames,) or (frames, channels) PCM with 1 or 2 channels, got %s" % (tuple(x.shape),))
    return x.contiguous()


def overlay(a, a_sr, a_gains, b, b_sr, b_gains):
    """pydub `a.overlay(b)` where a and b are each followed by two apply_gain factors (1.0 = none).  (frames, C) int16 -> (int16,
    rate)."""
    a, b = _as_pcm(a), _as_pcm(b)
    rate = max(int(a_sr), int(b_sr))
    n = pydub_slice_frames(ratecv_frames(a.shape[0], int(a_sr), rate), rate)
    return ops.pcm16_mix(a, int(a_sr), a_gains, b, int(b_sr), b_gains, n), rate


def mix_stems(main_i16, main_sr, backup_i16, backup_sr, inst_i16, inst_sr, main_gain, backup_gain, inst_gain):
    """combine_audio's arithmetic: (main - 4 + main_gain).overlay(backup - 6 + backup_gain).overlay(inst - 7 + inst_gain), every
    gain a separate audioop.mul pass, pydub's channel / rate sync before each overlay.  Inputs: (frames,) or (frames, C) int16.
    Returns ((frames, C) int16, rate)."""
    one = (1.0, 1.0)
    first, r1 = overlay(main_i16, main_sr, (db_to_float(-4), db_to_float(main_gain)),
                        backup_i16, backup_sr, (db_to_float(-6), db_to_float(backup_gain)))
    return overlay(first, r1, one, inst_i16, inst_sr, (db_to_float(-7), db_to_float(inst_gain)))


def pitch_shift_signal(x, sr, semitones, offsets=None):
    """sox `pitch` by `semitones` on a signal: time-stretch by d = 2^(semitones / 12) with WSOLA (pitch kept), then resample by d
    back to the input's length (pitch moved).  x: (n,) or (C, n) float32 (C = 1 or 2).  offsets: the WSOLA offsets to use instead of
    searching (int32, as returned), or None.  Returns (y with exactly x's frames, the offsets used); semitones == 0 returns a copy."""
    x2, flat = _as_2d(x)
    if semitones == 0:
        return x.clone(), torch.zeros(0, dtype=torch.int32, device=x.device)
    d = 2.0 ** (float(semitones) / 12.0)
    z, offs = ops.tempo_wsola(x2, int(sr), 1.0 / d, offsets)
    y = ops.resample_ratio(z, d, x2.shape[1])
    return (y.view(-1) if flat else y), offs


# ---------------------------------------------------------------------------------------------------
# File level (main.py's signatures)
# ---------------------------------------------------------------------------------------------------
def read_pcm16(path):
    """A 16-bit PCM WAV file -> ((frames, channels) int16 array, rate)."""
    from scipy.io import wavfile
    sr, data = wavfile.read(path)
    if data.dtype != np.int16:
        raise NotImplementedError("%s: only 16-bit PCM WAV is mixed (found %s samples)" % (path, data.dtype))
    return (data.reshape(-1, 1) if data.ndim == 1 else data), int(sr)


def write_pcm16(path, pcm, sr):
    """(frames, channels) int16 -> WAV the way pydub's export(format='wav') writes it (the stdlib wave module)."""
    pcm = np.ascontiguousarray(pcm, dtype=np.int16)
    with wave.open(path, "wb") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(int(sr))
        w.setnframes(pcm.shape[0])
        w.writeframesraw(pcm.astype("<i2").tobytes())


def read_float(path):
    """An audio file as pedalboard.io.AudioFile reads it: ((channels, frames) float32, rate); 16-bit PCM is scaled by 1/32768."""
    from scipy.io import wavfile
    from .audio_io import _to_float
    sr, data = wavfile.read(path)
    x = _to_float(data)
    x = x[:, None] if x.ndim == 1 else x
    return np.ascontiguousarray(x.T, dtype=np.float32), int(sr)


def add_audio_effects(audio_path, reverb_rm_size, reverb_wet, reverb_dry, reverb_damping):
    """main.py:206-226: the effects chain over the whole file, written next to it as '<stem>_mixed.wav' (16-bit PCM, the input's
    rate and channel count)."""
    output_path = f'{os.path.splitext(audio_path)[0]}_mixed.wav'
    x, sr = read_float(audio_path)
    if x.shape[0] not in (1, 2):
        raise NotImplementedError("%s: the reverb takes 1 or 2 channels, found %d" % (audio_path, x.shape[0]))
    xd = torch.from_numpy(x).to(_device())
    y, _ = vocal_effects(xd, sr, reverb_rm_size, reverb_wet, reverb_dry, reverb_damping)
    write_pcm16(output_path, ops.fx_to_pcm16(y).cpu().numpy(), sr)
    return output_path


def pitch_shift(audio_path, pitch_change):
    """main.py:138-147: the file shifted by `pitch_change` semitones, written next to it as '<stem>_p{pitch_change}.wav' (16-bit PCM,
    the input's rate and channel count); an existing output is returned as it is."""
    output_path = f'{os.path.splitext(audio_path)[0]}_p{pitch_change}.wav'
    if not os.path.exists(output_path):
        x, sr = read_float(audio_path)
        if x.shape[0] not in (1, 2):
            raise NotImplementedError("%s: pitch_shift takes 1 or 2 channels, found %d" % (audio_path, x.shape[0]))
        y, _ = pitch_shift_signal(torch.from_numpy(x).to(_device()), sr, pitch_change)
        write_pcm16(output_path, ops.fx_to_pcm16(y).cpu().numpy(), sr)
    return output_path


def _write_bytes(path, data):
    with open(path, "wb") as f:
        f.write(data.tobytes())


def export_flac(pcm, sr, output_path, fetch=None):
    """(frames, channels) int16 on the device -> a FLAC file, encoded on the device (ops.flac_encode): only the file's bytes are copied
    to the host (pinned memory, _Fetch) and written as they are.  With `fetch` the copy and the write are queued on it; without, the
    file exists on return."""
    mine = fetch is None
    if mine:
        fetch = _Fetch(_lib.backend() == "hip")
    fetch.add(_write_bytes, output_path, ops.flac_encode(pcm, sr))
    if mine:
        fetch.flush()
    return output_path


def export(pcm, sr, output_path, output_format):
    """pydub export: WAV directly; FLAC through the device encoder (export_flac; ffmpeg installed or not); any other format through
    ffmpeg (`ffmpeg -y -f wav -i <tmp.wav> -f <format> <out>`)."""
    if output_format == "wav":
        write_pcm16(output_path, pcm, sr)
        return output_path
    if output_format == "flac":     # never ffmpeg's: one bitstream on every machine (export_flac)
        return export_flac(torch.from_numpy(np.array(pcm, dtype=np.int16)).to(_device()), sr, output_path)
    ffmpeg = shutil.which("ffmpeg")
    if ffmpeg is None:
        raise RuntimeError("combine_audio: writing %r needs ffmpeg on PATH (only 'wav' is written without it)" % (output_format,))
    with tempfile.TemporaryDirectory() as d:
        tmp = os.path.join(d, "mix.wav")
        write_pcm16(tmp, pcm, sr)
        r = subprocess.run([ffmpeg, "-y", "-f", "wav", "-i", tmp, "-f", output_format, output_path], capture_output=True)
        if r.returncode != 0:
            raise RuntimeError("ffmpeg failed to write %s: %s" % (output_path, r.stderr.decode(errors="replace")[-2000:]))
    return output_path


def combine_audio(audio_paths, output_path, main_gain, backup_gain, inst_gain, output_format):
    """main.py:229-233: AI vocals (-4 dB + main_gain), backup vocals (-6 + backup_gain) and instrumental (-7 + inst_gain) mixed as
    pydub mixes them, exported as `output_format`."""
    dev = _device()
    stems = [read_pcm16(p) for p in audio_paths[:3]]
    t = [(torch.from_numpy(np.ascontiguousarray(d)).to(dev), sr) for d, sr in stems]
    out, sr = mix_stems(t[0][0], t[0][1], t[1][0], t[1][1], t[2][0], t[2][1], main_gain, backup_gain, inst_gain)
    if output_format == "flac":
        export_flac(out, sr, output_path)
    else:
        export(out.cpu().numpy(), sr, output_path, output_format)


# ---------------------------------------------------------------------------------------------------
# The whole cover in one call (main.py's song_cover_pipeline, src/main.py:236-313)
# ---------------------------------------------------------------------------------------------------
MDX_MODEL_FILES = ("UVR-MDX-NET-Voc_FT.onnx", "UVR_MDXNET_KARA_2.onnx", "Reverb_HQ_By_FoxJoy.onnx")     # main.py:182,185,188
BASE_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOICE_CACHE = 4     # voice models a session keeps (the least recently used one leaves)


def get_hash(filepath):
    """main.py:150-156: the song id of a local file."""
    import hashlib
    h = hashlib.blake2b()
    with open(filepath, "rb") as f:
        for chunk in iter(lambda: f.read(8192), b""):
            h.update(chunk)
    return h.hexdigest()[:11]


def get_audio_paths(song_dir):
    """main.py:105-122: (original song, instrumental, de-reverbed main vocals, backup vocals) found again by suffix, None if absent."""
    orig = inst = dereverb = backup = None
    for file in os.listdir(song_dir):
        if file.endswith("_Instrumental.wav"):
            inst = os.path.join(song_dir, file)
            orig = inst.replace("_Instrumental", "")
        elif file.endswith("_Vocals_Main_DeReverb.wav"):
            dereverb = os.path.join(song_dir, file)
        elif file.endswith("_Vocals_Backup.wav"):
            backup = os.path.join(song_dir, file)
    return orig, inst, dereverb, backup


def get_rvc_model(rvc_models_dir, voice_model):
    """main.py:88-102: (the directory's .pth, its .index or '')."""
    model_dir = os.path.join(rvc_models_dir, voice_model)
    pth = index = None
    for file in os.listdir(model_dir):
        ext = os.path.splitext(file)[1]
        if ext == ".pth":
            pth = file
        if ext == ".index":
            index = file
    if pth is None:
        raise FileNotFoundError(f"No model file exists in {model_dir}.")
    return os.path.join(model_dir, pth), os.path.join(model_dir, index) if index else ""


class _NoStream:
    """The host emulator runs every kernel synchronously: hand-overs between streams are already ordered."""

    def wait_stream(self, other): pass
    def __enter__(self): return self
    def __exit__(self, *a): return False


class _Fetch:
    """Device tensors on their way to files.  Each copy to the host is queued on a stream of its own into pinned memory right after the
    kernel that produced the tensor, so neither the device queue nor the host thread waits for it; the files are written when the
    call has queued everything else."""

    def __init__(self, on_gpu):
        self.stream = torch.cuda.Stream() if on_gpu else None
        self.jobs = []

    def add(self, writer, path, t, *args):
        if self.stream is None:
            self.jobs.append((writer, path, t, None, args))
            return
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            host.copy_(t, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.stream)
        t.record_stream(self.stream)
        self.jobs.append((writer, path, host, done, args))

    def flush(self):
        for writer, path, host, done, args in self.jobs:
            if done is not None:
                done.synchronize()
            writer(path, host.numpy(), *args)
        self.jobs = []

    def paths(self):
        return [job[1] for job in self.jobs]

    def flush_in_background(self):
        """Write the files from a thread of its own (waiting for a copy, writing a file and waiting for ffmpeg all release the GIL) while
        the caller queues the next cover; join() re-raises what went wrong there."""
        import threading
        self.error = None

        def work():
            try:
                self.flush()
            except BaseException as e:      # handed to the thread that joins
                self.error = e
        self.thread = threading.Thread(target=work, name="aicg-cover-files")
        self.thread.start()

    def join(self):
        t, self.thread = getattr(self, "thread", None), None
        if t is not None:
            t.join()
            if self.error is not None:
                raise self.error


def _write_wavfile(path, pcm, sr):      # what run_mdx (soundfile's PCM-16) and rvc_infer leave: scipy's writer on int16 samples
    from scipy.io import wavfile
    wavfile.write(path, int(sr), pcm)


def _planar(pcm):
    """(frames, C) int16 PCM -> (C, frames) float32 / 32768: what read_float makes of the stem's file."""
    return pcm.t().contiguous().to(torch.float32) / 32768.0


class _Song:
    """What a session keeps of the last song, all of it independent of the voice: the three int16 stems the mix and the conversion need
    (device tensors, as _separate leaves them or as their files read), the 16 kHz mono hand-over of the de-reverbed stem, the backing
    stems shifted by `pitch_change_all` (per value seen) and the VoiceFronts (per f0 method / hop / filter radius / if_f0 / version).
    `stamp`: size and mtime of the three stem files when they were cached -- main.py's rules look at the files, so stems somebody
    replaced on disk are read again."""

    def __init__(self, song_id, paths, inst, inst_sr, backup, backup_sr, dereverb):
        self.id, self.paths = song_id, paths
        self.inst, self.inst_sr, self.backup, self.backup_sr, self.dereverb = inst, inst_sr, backup, backup_sr, dereverb
        self.audio16k, self.shifted, self.fronts, self.stamp = None, {}, {}, None

    @staticmethod
    def stamp_of(paths):
        try:
            return tuple((os.path.getsize(p), os.stat(p).st_mtime_ns) for p in paths[1:])
        except OSError:
            return None

    def nbytes(self):
        ts = [self.inst, self.backup, self.dereverb] + ([self.audio16k] if self.audio16k is not None else [])
        ts += [t for pair in self.shifted.values() for t in pair]
        return sum(t.numel() * t.element_size() for t in ts) + sum(f.nbytes() for f in self.fronts.values())


class CoverSession:
    """The models of a cover, loaded once: the three MDX-Net sessions (model_data.json entries looked up by hash, as run_mdx does),
    HuBERT, and a small cache of voice models by directory name.  A second song through the same session reloads nothing."""

    def __init__(self, mdxnet_models_dir, rvc_models_dir, output_dir, device=None, resample_sr=0):
        import json
        from . import mdx, rvc
        self.mdxnet_models_dir, self.rvc_models_dir, self.output_dir = mdxnet_models_dir, rvc_models_dir, output_dir
        self.device = "cuda:0" if device is None else device           # main.py:195
        with open(os.path.join(mdxnet_models_dir, "model_data.json")) as f:
            self.mdx_model_params = json.load(f)
        self.mdx_sessions = [mdx.load_session(self.mdx_model_params, os.path.join(mdxnet_models_dir, name)) for name in MDX_MODEL_FILES]
        self.config = rvc.Config(self.device, True)                      # main.py:196
        self.hubert = rvc.load_hubert(self.device, self.config.is_half, os.path.join(rvc_models_dir, "hubert_base.pt"))
        self.voices = {}                                                 # directory name -> (cpt, version, net_g, tgt_sr, vc, index path)
        self.profile_stages = False      # True: drain the device after every stage and keep the wall-clock split in last_profile
        self.last_profile = {}
        self.song = None                 # the last song's voice-independent part (_Song); capacity: one song
        # VC.pipeline's resample_sr (rvc_infer passes 0): >= 16000 and not the voice's rate -> the AI vocals are resampled to it on the
        # device.  Not part of a cached song: it acts behind the voice-independent front.
        self.resample_sr = int(resample_sr)

    def drop_song(self):
        """Forget the cached song: its stems, hand-over, shifted stems and fronts leave device memory."""
        self.song = None

    @staticmethod
    def _song_cache_on():
        return _env.dev("AICG_SONG_CACHE", "1") != "0"      # development switch: "0" = every call starts from the files, as before the cache

    def voice(self, voice_model):
        from . import rvc
        if voice_model in self.voices:
            self.voices[voice_model] = self.voices.pop(voice_model)      # most recently used last
        else:
            pth, index = get_rvc_model(self.rvc_models_dir, voice_model)
            self.voices[voice_model] = rvc.get_vc(self.device, self.config.is_half, self.config, pth) + (index,)
            rmvpe = os.path.join(self.rvc_models_dir, "rmvpe.pt")          # where main.py keeps it (src/vc_infer_pipeline.py:327)
            if os.path.exists(rmvpe):
                self.voices[voice_model][4].rmvpe_path = rmvpe
            while len(self.voices) > VOICE_CACHE:
                self.voices.pop(next(iter(self.voices)))
        return self.voices[voice_model]

    # ---- stages ------------------------------------------------------------------------------------------------------------
    def _mark(self, name, t0):
        import time
        if self.profile_stages:
            if _lib.backend() == "hip":
                torch.cuda.synchronize()
            self.last_profile[name] = self.last_profile.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    def _separate(self, song_path, song_dir, keep_files, fetch):
        """main.py's preprocess_song (:166-190) on the device -> (instrumental, backup, de-reverbed main) int16 (frames, 2) tensors."""
        from . import audio_io, mdx
        dev = self.mdx_sessions[0].device
        base = os.path.splitext(os.path.basename(song_path))[0]
        if audio_io.wav_rate(song_path) in (None, 44100):
            wave, sr = audio_io.load_wav(song_path, 44100, mono=False)
            song = torch.from_numpy(np.ascontiguousarray(wave, dtype=np.float32)).to(dev)
        else:       # a WAV file at another rate: uploaded as it is, converted and resampled on the device (run_mdx takes the same route)
            song, sr = audio_io.load_device(song_path, 44100, dev), 44100
        path = lambda stem: os.path.join(song_dir, "%s_%s.wav" % (base, stem))
        vocals, inst = mdx.run_mdx_device(self.mdx_sessions[0], song, True)
        fetch.add(_write_wavfile, path("Instrumental"), inst, sr)
        if keep_files:
            fetch.add(_write_wavfile, path("Vocals"), vocals, sr)
        backup, main = mdx.run_mdx_device(self.mdx_sessions[1], vocals, True)
        fetch.add(_write_wavfile, path("Vocals_Backup"), backup, sr)
        if keep_files:
            fetch.add(_write_wavfile, path("Vocals_Main"), main, sr)
        _, dereverb = mdx.run_mdx_device(self.mdx_sessions[2], main, True, exclude_main=True)
        fetch.add(_write_wavfile, path("Vocals_Main_DeReverb"), dereverb, sr)
        return song_path, path("Instrumental"), path("Vocals_Main_DeReverb"), path("Vocals_Backup"), inst, backup, dereverb

    def _convert(self, voice_model, dereverb, dereverb_path, pitch_change, f0_method, index_rate, filter_radius, rms_mix_rate, protect,
                 crepe_hop_length, noise_seed, song=None):
        """main.py's voice_change (:193-203) without the file on either side: the de-reverbed stem -> 16 kHz mono on the device
        (ops.resample_poly_mono, bench.py's hand-over) -> VC.pipeline -> (int16 (n,) device tensor, its rate).
        `song` (the session's cache entry): the hand-over and the voice-independent front of the conversion (VC.front: plan, f0
        estimate, HuBERT) are taken from it, or made once and left there; the samples are the same (tests/test_voice_front.py)."""
        cpt, version, net_g, tgt_sr, vc, index_path = self.voice(voice_model)
        if_f0, front = cpt.get("f0", 1), None
        if song is None:
            audio = ops.resample_poly_mono(_planar(dereverb), 44100, 16000)
        else:
            if song.audio16k is None:
                song.audio16k = ops.resample_poly_mono(_planar(dereverb), 44100, 16000)
            audio = song.audio16k
            key = (f0_method, crepe_hop_length, filter_radius, if_f0, version)
            if key not in song.fronts:
                song.fronts[key] = vc.front(self.hubert, audio, dereverb_path, f0_method, if_f0, version, filter_radius, crepe_hop_length)
            front = song.fronts[key]
        out = vc.pipeline(self.hubert, net_g, 0, audio, dereverb_path, [0, 0, 0], pitch_change, f0_method, index_path, index_rate,
                          if_f0, filter_radius, tgt_sr, self.resample_sr, rms_mix_rate, version, protect, crepe_hop_length,
                          noise_seed=noise_seed, device_out=True, front=front)
        return out, (self.resample_sr if self.resample_sr >= 16000 and self.resample_sr != tgt_sr else tgt_sr)

    def song_cover_pipeline(self, song_input, voice_model, pitch_change, keep_files, is_webui=0, main_gain=0, backup_gain=0,
                            inst_gain=0, index_rate=0.5, filter_radius=3, rms_mix_rate=0.25, f0_method='rmvpe', crepe_hop_length=128,
                            protect=0.33, pitch_change_all=0, reverb_rm_size=0.15, reverb_wet=0.2, reverb_dry=0.8,
                            reverb_damping=0.7, output_format='mp3', progress=None, noise_seed=None):
        """main.py's song_cover_pipeline (src/main.py:236-313) with its parameters, defaults, file names and return value (the
        cover's path); `is_webui` and `progress` are accepted and ignored, `noise_seed` seeds the synthesizer's noise per chunk
        (VC.pipeline).  Every stem stays in device memory from the song file to the cover; only the files main.py leaves behind
        are copied to the host (all of them with keep_files).
        The same song again -- another voice, another `-p` -- finds its voice-independent part in the session (_Song): the stems are
        not read and uploaded again, nor resampled, nor passed through the f0 estimator and HuBERT, nor shifted by `-pall` a second
        time.  main.py's file rules come first: keep_files separates again, missing or replaced stem files are made or read again, an
        existing AI-vocals or `_p{N}.wav` file is used as it is.  The files and their bytes are those of a call on a fresh session."""
        path, fetch = self._cover(song_input, voice_model, pitch_change, keep_files, main_gain, backup_gain, inst_gain, index_rate,
                                  filter_radius, rms_mix_rate, f0_method, crepe_hop_length, protect, pitch_change_all, reverb_rm_size,
                                  reverb_wet, reverb_dry, reverb_damping, output_format, noise_seed)
        t0 = __import__("time").perf_counter()
        fetch.flush()
        self._mark("files_s", t0)
        return path

    @staticmethod
    def _checked_input(song_input, voice_model):
        from urllib.parse import urlparse
        if not song_input or not voice_model:
            raise ValueError("Ensure that the song input field and voice model field is filled.")
        if urlparse(song_input).scheme == "https":
            raise ValueError("%s: downloading a song is not part of this pipeline; pass the path of a local audio file" % song_input)
        song_input = song_input.strip('"')
        if not os.path.exists(song_input):
            raise FileNotFoundError(f"{song_input} does not exist.")
        return song_input

    def _stems(self, song_input, song_id, song_dir, keep_files, fetch, dev):
        """The song's stems and their paths (main.py:252-266) -> (paths, inst, inst_sr, backup, backup_sr, dereverb, cache entry or None,
        whether `fetch` now holds stem files)."""
        cached = None
        if os.path.exists(song_dir):
            paths = get_audio_paths(song_dir)
            if not (any(p is None for p in paths) or keep_files):
                cached = paths
        else:
            os.makedirs(song_dir)
        cache = self._song_cache_on()
        if not cache or (self.song is not None and self.song.id != song_id):
            self.song = None                                                        # capacity: one song
        if cached is not None and self.song is not None and (self.song.paths[1:] != tuple(cached[1:])
                                                             or self.song.stamp != _Song.stamp_of(cached)):
            self.song = None                                                        # the files are not the ones that were cached
        if cached is not None and self.song is not None:
            g = self.song
            return cached, g.inst, g.inst_sr, g.backup, g.backup_sr, g.dereverb, g, False
        if cached is None:
            orig_song_path, inst_path, dereverb_path, backup_path, inst, backup, dereverb = self._separate(song_input, song_dir,
                                                                                                          keep_files, fetch)
            inst_sr = backup_sr = 44100
            paths = (orig_song_path, inst_path, dereverb_path, backup_path)
        else:
            paths = orig_song_path, inst_path, dereverb_path, backup_path = cached
            (inst, inst_sr), (backup, backup_sr), (dereverb, _) = [
                (torch.from_numpy(np.ascontiguousarray(d)).to(dev), sr) for d, sr in map(read_pcm16, (inst_path, backup_path, dereverb_path))]
        self.song = _Song(song_id, tuple(paths), inst, inst_sr, backup, backup_sr, dereverb) if cache else None
        if self.song is not None and cached is not None:
            self.song.stamp = _Song.stamp_of(paths)
        return paths, inst, inst_sr, backup, backup_sr, dereverb, self.song, cached is None

    def _cover(self, song_input, voice_model, pitch_change, keep_files, main_gain, backup_gain, inst_gain, index_rate, filter_radius,
               rms_mix_rate, f0_method, crepe_hop_length, protect, pitch_change_all, reverb_rm_size, reverb_wet, reverb_dry,
               reverb_damping, output_format, noise_seed, before_convert=None):
        """song_cover_pipeline up to the files: everything is queued, the _Fetch that will write them is returned with the cover's path.
        `before_convert(ai_vocals_path)`: called before the file checks of the per-voice part (song_covers joins its writer there)."""
        import time
        song_input = self._checked_input(song_input, voice_model)
        song_id = get_hash(song_input)
        song_dir = os.path.join(self.output_dir, song_id)
        on_gpu = _lib.backend() == "hip"
        dev = self.mdx_sessions[0].device
        fetch = _Fetch(on_gpu)
        self.last_profile = {}
        t0 = time.perf_counter()

        (orig_song_path, inst_path, dereverb_path, backup_path), inst, inst_sr, backup, backup_sr, dereverb, song, fetch.has_stems = \
            self._stems(song_input, song_id, song_dir, keep_files, fetch, dev)
        t0 = self._mark("separate_s", t0)

        pitch_change = pitch_change * 12 + pitch_change_all
        base = os.path.splitext(os.path.basename(orig_song_path))[0]
        hop = "" if f0_method != "mangio-crepe" else f"_{crepe_hop_length}"
        ai_vocals_path = os.path.join(song_dir, f"{base}_{voice_model}_p{pitch_change}_i{index_rate}_fr{filter_radius}_rms{rms_mix_rate}"
                                                f"_pro{protect}_{f0_method}{hop}.wav")
        ai_cover_path = os.path.join(song_dir, f"{base} ({voice_model} Ver).{output_format}")
        if before_convert is not None:
            before_convert(ai_vocals_path)

        # the backing stems' pitch shift does not depend on the conversion: one persistent workgroup per stem, queued on a side stream
        # before the conversion starts and joined before the mix
        shifted, side, from_file = {}, None, False
        if pitch_change_all != 0:
            kept = song.shifted.get(pitch_change_all) if song is not None else None
            main_stream = torch.cuda.current_stream() if on_gpu else _NoStream()
            side = torch.cuda.Stream() if on_gpu else _NoStream()
            side.wait_stream(main_stream)
            with (torch.cuda.stream(side) if on_gpu else side):
                for k, (key, pcm, sr, src) in enumerate((("inst", inst, inst_sr, inst_path), ("backup", backup, backup_sr, backup_path))):
                    out_path = f"{os.path.splitext(src)[0]}_p{pitch_change_all}.wav"
                    if os.path.exists(out_path):                                    # main.py:140: an existing file is used as it is
                        y, from_file = torch.from_numpy(np.ascontiguousarray(read_pcm16(out_path)[0])).to(dev), True
                    else:
                        y = kept[k] if kept is not None else ops.fx_to_pcm16(pitch_shift_signal(_planar(pcm), sr, pitch_change_all)[0])
                        if keep_files:
                            fetch.add(write_pcm16, out_path, y, sr)
                    if on_gpu:
                        pcm.record_stream(side)
                        y.record_stream(main_stream)
                    shifted[key] = y
            if song is not None and kept is None and not from_file:
                song.shifted[pitch_change_all] = (shifted["inst"], shifted["backup"])

        if os.path.exists(ai_vocals_path):                                          # main.py:289
            ai, ai_sr = read_pcm16(ai_vocals_path)
            ai = torch.from_numpy(np.ascontiguousarray(ai)).to(dev)
        else:
            ai, ai_sr = self._convert(voice_model, dereverb, dereverb_path, pitch_change, f0_method, index_rate, filter_radius,
                                      rms_mix_rate, protect, crepe_hop_length, noise_seed, song)
            fetch.add(_write_wavfile, ai_vocals_path, ai, ai_sr)
            ai = ai.view(-1, 1)
        t0 = self._mark("convert_s", t0)

        y, _ = vocal_effects(_planar(ai), ai_sr, reverb_rm_size, reverb_wet, reverb_dry, reverb_damping)
        mixed = ops.fx_to_pcm16(y)
        if keep_files:
            fetch.add(write_pcm16, f"{os.path.splitext(ai_vocals_path)[0]}_mixed.wav", mixed, ai_sr)
        t0 = self._mark("effects_s", t0)

        if pitch_change_all != 0:
            main_stream.wait_stream(side)
            inst, backup = shifted["inst"], shifted["backup"]
        out, sr = mix_stems(mixed, ai_sr, backup, backup_sr, inst, inst_sr, main_gain, backup_gain, inst_gain)
        if output_format == "flac":      # encoded here; the file's bytes are what leaves the device
            export_flac(out, sr, ai_cover_path, fetch)
        else:
            fetch.add(lambda p, pcm, r: export(pcm, r, p, output_format), ai_cover_path, out, sr)
        self._mark("pitch_join_and_mix_s", t0)
        if song is not None and fetch.has_stems:      # stems that this call writes: stamped once their files exist
            flush = fetch.flush

            def flush_and_stamp():
                flush()
                song.stamp = _Song.stamp_of(song.paths)
            fetch.flush = flush_and_stamp
        return ai_cover_path, fetch

    PER_COVER = ("pitch_change", "main_gain", "backup_gain", "inst_gain", "index_rate", "filter_radius", "rms_mix_rate", "f0_method",
                 "crepe_hop_length", "protect", "pitch_change_all", "reverb_rm_size", "reverb_wet", "reverb_dry", "reverb_damping",
                 "output_format", "noise_seed")
    DEFAULTS = dict(main_gain=0, backup_gain=0, inst_gain=0, index_rate=0.5, filter_radius=3, rms_mix_rate=0.25, f0_method="rmvpe",
                    crepe_hop_length=128, protect=0.33, pitch_change_all=0, reverb_rm_size=0.15, reverb_wet=0.2, reverb_dry=0.8,
                    reverb_damping=0.7, output_format="mp3", noise_seed=None)

    def song_covers(self, song_input, voices, keep_files=False, **common):
        """One song, several covers: `voices` is a list of dicts with `voice_model` and any of song_cover_pipeline's per-cover parameters
        (PER_COVER), `common` their defaults for all entries -> the cover paths in order.  The same files, byte for byte, as one
        song_cover_pipeline call per entry; the separation, the front of the conversion and the `-pall` shift are queued once (per f0
        method / `pitch_change_all` where the entries differ), and the files of cover k are written by a thread of their own while
        cover k + 1 is on the device.  Two entries that would write the same cover file raise ValueError before any work (main.py, run
        twice, silently overwrites the first)."""
        unknown = sorted(set(common) - set(self.PER_COVER))
        if unknown:
            raise TypeError("song_covers: unknown parameter(s) %s" % ", ".join(unknown))
        entries, seen = [], {}
        for k, v in enumerate(voices):
            unknown = sorted(set(v) - set(self.PER_COVER) - {"voice_model"})
            if unknown or not v.get("voice_model"):
                raise ValueError("song_covers: entry %d needs a voice_model and takes only per-cover parameters (%s)" % (k, ", ".join(unknown)))
            e = dict(self.DEFAULTS, **common)
            e.update(v)
            if "pitch_change" not in e:
                raise ValueError("song_covers: entry %d (%s) has no pitch_change" % (k, e["voice_model"]))
            name = (e["voice_model"], e["output_format"])         # what the cover's file name is made of (main.py:287)
            if name in seen:
                raise ValueError("song_covers: entries %d and %d would both write '... (%s Ver).%s'" % (seen[name], k, *name))
            seen[name] = k
            entries.append(e)
        self._checked_input(song_input, entries[0]["voice_model"] if entries else "-")
        covers, writer = [], None
        try:
            for e in entries:
                pending = writer.paths() if writer is not None else []

                def before_convert(ai_vocals_path, _w=writer, _p=pending):
                    if _w is not None and (keep_files or ai_vocals_path in _p):      # a file this cover looks for may be on its way
                        _w.join()
                args = [e[k] for k in self.PER_COVER]
                path, fetch = self._cover(song_input, e["voice_model"], args[0], keep_files, *args[1:], before_convert=before_convert)
                if writer is not None:
                    writer.join()
                if fetch.has_stems:       # the next entry finds the song by its stem files (main.py:252-262): they are written now
                    fetch.flush()
                    writer = None
                else:
                    fetch.flush_in_background()
                    writer = fetch
                covers.append(path)
        finally:
            if writer is not None:
                writer.join()
        return covers


_default_session = None


def default_session(mdxnet_models_dir=None, rvc_models_dir=None, output_dir=None):
    """The session behind the module-level song_cover_pipeline: main.py's directories next to the package unless named; made on first
    use and kept while the directories stay the same."""
    global _default_session
    dirs = (mdxnet_models_dir or os.path.join(BASE_DIR, "mdxnet_models"), rvc_models_dir or os.path.join(BASE_DIR, "rvc_models"),
            output_dir or os.path.join(BASE_DIR, "song_output"))
    s = _default_session
    if s is None or (s.mdxnet_models_dir, s.rvc_models_dir, s.output_dir) != dirs:
        _default_session = CoverSession(*dirs)
    return _default_session


def song_cover_pipeline(song_input, voice_model, pitch_change, keep_files, **kwargs):
    """CoverSession.song_cover_pipeline on the default session."""
    return default_session().song_cover_pipeline(song_input, voice_model, pitch_change, keep_files, **kwargs)


class _OneOrMore(__import__("argparse").Action):
    """`-dir A`: the string "A", as main.py parses it; `-dir A -dir B`: the list ["A", "B"]."""

    def __call__(self, parser, namespace, value, option_string=None):
        have = getattr(namespace, self.dest, None)
        setattr(namespace, self.dest, value if have is None else (have if isinstance(have, list) else [have]) + [value])


def build_parser():
    """main.py's command line (src/main.py:320-339: same flags, same defaults) plus the three directories."""
    import argparse
    p = argparse.ArgumentParser(description="Generate a AI cover song in the song_output/id directory.", add_help=True)
    p.add_argument("-i", "--song-input", type=str, required=True, help="Filepath to a local audio file to create an AI cover of")
    p.add_argument("-dir", "--rvc-dirname", type=str, required=True, action=_OneOrMore, help="Name of the folder in the rvc_models directory containing the RVC model file and optional index file to use (repeat the flag for several covers of the song)")
    p.add_argument("-p", "--pitch-change", type=int, required=True, help="Change the pitch of AI Vocals only. Generally, use 1 for male to female and -1 for vice-versa. (Octaves)")
    p.add_argument("-k", "--keep-files", action=argparse.BooleanOptionalAction, help="Whether to keep all intermediate audio files generated in the song_output/id directory")
    p.add_argument("-ir", "--index-rate", type=float, default=0.5, help="How much of the retrieved features to mix in (0 to 1)")
    p.add_argument("-fr", "--filter-radius", type=int, default=3, help="Median filtering radius of the harvested pitch (0 to 7)")
    p.add_argument("-rms", "--rms-mix-rate", type=float, default=0.25, help="How much to use the original vocal's loudness (0) or a fixed loudness (1)")
    p.add_argument("-palgo", "--pitch-detection-algo", type=str, default="rmvpe", help="rmvpe, mangio-crepe, pm, dio or hybrid[dio+mangio-crepe+...] (pm and dio need no rmvpe.pt)")
    p.add_argument("-hop", "--crepe-hop-length", type=int, default=128, help="Hop length of mangio-crepe")
    p.add_argument("-pro", "--protect", type=float, default=0.33, help="Protection of voiceless consonants and breath sounds (0.5 disables it)")
    p.add_argument("-mv", "--main-vol", type=int, default=0, help="Volume change for AI main vocals in decibels")
    p.add_argument("-bv", "--backup-vol", type=int, default=0, help="Volume change for backup vocals in decibels")
    p.add_argument("-iv", "--inst-vol", type=int, default=0, help="Volume change for instrumentals in decibels")
    p.add_argument("-pall", "--pitch-change-all", type=int, default=0, help="Change the pitch/key of vocals and instrumentals (semitones)")
    p.add_argument("-rsize", "--reverb-size", type=float, default=0.15, help="Reverb room size between 0 and 1")
    p.add_argument("-rwet", "--reverb-wetness", type=float, default=0.2, help="Reverb wet level between 0 and 1")
    p.add_argument("-rdry", "--reverb-dryness", type=float, default=0.8, help="Reverb dry level between 0 and 1")
    p.add_argument("-rdamp", "--reverb-damping", type=float, default=0.7, help="Reverb damping between 0 and 1")
    p.add_argument("-oformat", "--output-format", type=str, default="mp3", help="Output format of audio file. mp3 for smaller file size, wav for best quality, flac for both (lossless, encoded on the device, needs no ffmpeg)")
    # Not one of main.py's flags.  SUPPRESS keeps it out of the parsed namespace unless given, so a command line of main.py's parses to
    # exactly main.py's namespace (tests/test_cover_pipeline.py compares the two whole); main() reads it with a default of 0.
    p.add_argument("-osr", "--resample-sr", type=int, default=argparse.SUPPRESS, help="Sample rate of the AI vocals (>= 16000); 0 or absent: the voice model's own rate")
    p.add_argument("--mdx-models-dir", type=str, default=os.path.join(BASE_DIR, "mdxnet_models"), help="Directory of the MDX-Net .onnx files and model_data.json")
    p.add_argument("--rvc-models-dir", type=str, default=os.path.join(BASE_DIR, "rvc_models"), help="Directory of hubert_base.pt, rmvpe.pt and the voice model folders")
    p.add_argument("--output-dir", type=str, default=os.path.join(BASE_DIR, "song_output"), help="Directory the song_id folders are made in")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    dirnames = args.rvc_dirname if isinstance(args.rvc_dirname, list) else [args.rvc_dirname]
    for name in dirnames:
        if not os.path.exists(os.path.join(args.rvc_models_dir, name)):
            raise Exception(f"The folder {os.path.join(args.rvc_models_dir, name)} does not exist.")
    session = CoverSession(args.mdx_models_dir, args.rvc_models_dir, args.output_dir, resample_sr=getattr(args, "resample_sr", 0))
    shared = dict(main_gain=args.main_vol, backup_gain=args.backup_vol,
                  inst_gain=args.inst_vol, index_rate=args.index_rate, filter_radius=args.filter_radius, rms_mix_rate=args.rms_mix_rate,
                  f0_method=args.pitch_detection_algo, crepe_hop_length=args.crepe_hop_length, protect=args.protect,
                  pitch_change_all=args.pitch_change_all, reverb_rm_size=args.reverb_size, reverb_wet=args.reverb_wetness,
                  reverb_dry=args.reverb_dryness, reverb_damping=args.reverb_damping, output_format=args.output_format)
    if len(dirnames) == 1:
        cover_path = session.song_cover_pipeline(args.song_input, dirnames[0], args.pitch_change, args.keep_files, **shared)
        print(f"[+] Cover generated at {cover_path}")
        return cover_path
    cover_paths = session.song_covers(args.song_input, [{"voice_model": name} for name in dirnames], bool(args.keep_files),
                                      pitch_change=args.pitch_change, **shared)
    for cover_path in cover_paths:
        print(f"[+] Cover generated at {cover_path}")
    return cover_paths


if __name__ == "__main__":
    main()
