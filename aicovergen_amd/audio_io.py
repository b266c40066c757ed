"""WAV file plumbing either side of the hot path (the reference uses librosa.load / soundfile.write / ffmpeg,
src/mdx.py:257,273,280 and src/my_utils.py:14-16; none of them exist in this image).  scipy only; no arithmetic
beyond sample-format conversion and (if a file is not at the requested rate) polyphase resampling."""
import shutil
import struct
import subprocess

import numpy as np
from scipy.io import wavfile
from scipy.signal import resample_poly


def _to_float(data):
    if data.dtype == np.int16:
        return data.astype(np.float32) / 32768.0
    if data.dtype == np.int32:
        return data.astype(np.float32) / 2147483648.0
    if data.dtype == np.uint8:
        return (data.astype(np.float32) - 128.0) / 128.0
    return data.astype(np.float32)


def _ffmpeg_decode(path, sr, mono):
    """Any container / codec ffmpeg reads (main.py hands run_mdx the yt-dlp mp3 or a user's m4a / flac / ogg) -> float32
    (C, N) at `sr`; same command shape as the reference's my_utils.load_audio (src/my_utils.py:14-16)."""
    ch = 1 if mono else 2
    cmd = ["ffmpeg", "-nostdin", "-threads", "0", "-i", path, "-f", "f32le", "-acodec", "pcm_f32le", "-ac", str(ch),
           "-ar", str(int(sr)), "-"]
    out = subprocess.run(cmd, capture_output=True, check=True).stdout
    return np.frombuffer(out, np.float32).reshape(-1, ch).T.copy()


def load_wav(path, sr, mono):
    """-> float32 (channels, N) (or (N,) when mono) at `sr`, like librosa.load(path, mono=mono, sr=sr).
    Plain WAV files are read directly; anything else (or a WAV encoding scipy cannot parse) is decoded through ffmpeg when
    the binary is installed, otherwise a clear error names the file."""
    try:
        file_sr, data = wavfile.read(path)
    except Exception as e:  # not RIFF/WAVE, or an encoding scipy does not know (ADPCM, extensible float64 ...)
        if shutil.which("ffmpeg"):
            x = _ffmpeg_decode(path, sr, mono)
            return (x[0] if mono else x), sr
        raise RuntimeError("cannot read %r: not a WAV file scipy understands (%s) and ffmpeg is not installed to decode "
                           "other containers" % (path, e))
    x = _to_float(data)
    x = x[:, None] if x.ndim == 1 else x
    x = x.T  # (C, N)
    if mono:
        x = x.mean(axis=0, keepdims=True)
    if file_sr != sr:
        g = np.gcd(int(file_sr), int(sr))
        x = resample_poly(x, sr // g, file_sr // g, axis=1).astype(np.float32)
    return (x[0] if mono else x), sr


def wav_rate(path):
    """Sample rate the fmt chunk of a RIFF / RIFX / RF64 WAVE file states, whatever its sample encoding (only the chunk headers in front
    of it are read: the samples stay on disk); None for anything else."""
    try:
        with open(path, "rb") as f:
            head = f.read(12)
            if len(head) < 12 or head[:4] not in (b"RIFF", b"RIFX", b"RF64") or head[8:] != b"WAVE":
                return None
            order = ">" if head[:4] == b"RIFX" else "<"
            while True:
                chunk = f.read(8)
                if len(chunk) < 8:
                    return None
                size = struct.unpack(order + "I", chunk[4:])[0]
                if chunk[:4] == b"fmt ":
                    return struct.unpack(order + "HHI", f.read(8))[2]     # format tag, channels, rate
                f.seek(size + (size & 1), 1)                              # chunks are padded to an even length
    except (OSError, struct.error):
        return None


def load_device(path, sr, device):
    """-> float32 (channels, N) tensor at `sr` on `device`: load_wav(path, sr, mono=False) with the sample-format conversion and the
    resampling done on the device (ops.resample_poly: the same polyphase filter, in float32).  A plain WAV file is uploaded in its file
    format -- 16-bit PCM as int16 (frames, channels), every other encoding as the float32 _to_float makes of it; anything scipy cannot
    parse is decoded by ffmpeg, which already delivers `sr`."""
    import torch
    from . import ops
    try:
        file_sr, data = wavfile.read(path)
    except Exception:
        return torch.from_numpy(np.ascontiguousarray(load_wav(path, sr, mono=False)[0], dtype=np.float32)).to(device)
    data = data[:, None] if data.ndim == 1 else data
    if data.dtype == np.int16:
        x = torch.from_numpy(np.ascontiguousarray(data)).to(device)                  # (frames, C): read as x / 32768 by the kernel
    else:
        x = torch.from_numpy(np.ascontiguousarray(_to_float(data).T)).to(device)      # (C, frames)
    return ops.resample_poly(x, int(file_sr), int(sr))


def write_wav_pcm16(path, data, sr):
    """soundfile.write(path, data (N, C) float, sr) default WAV subtype: 16-bit PCM."""
    y = np.clip(np.asarray(data, dtype=np.float64), -1.0, 32767.0 / 32768.0)
    wavfile.write(path, int(sr), np.rint(y * 32768.0).astype(np.int16))
