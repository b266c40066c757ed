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

from . import _lib, ops

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


def export(pcm, sr, output_path, output_format):
    """pydub export: WAV directly; any other format through ffmpeg (`ffmpeg -y -f wav -i <tmp.wav> -f <format> <out>`)."""
    if output_format == "wav":
        write_pcm16(output_path, pcm, sr)
        return output_path
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
    export(out.cpu().numpy(), sr, output_path, output_format)
