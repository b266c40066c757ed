"""pedalboard.io.AudioFile as the reference's add_audio_effects uses it: read a WAV file in chunks as float32 (channels, frames),
write 16-bit PCM WAV (round to nearest, clamp to +-32767).  Other modes and formats raise NotImplementedError."""
import numpy as _np

from . import _unsupported
from aicovergen_amd import cover as _cover


class AudioFile:
    def __init__(self, filename, mode="r", samplerate=None, num_channels=1, **kwargs):
        self.filename, self.mode = filename, mode
        if kwargs:
            raise _unsupported("AudioFile(%s)" % ", ".join(sorted(kwargs)))
        if mode == "r":
            self._data, self.samplerate = _cover.read_float(filename)
            self.num_channels, self.frames = self._data.shape
            self._pos = 0
        elif mode == "w":
            if samplerate is None:
                raise ValueError("AudioFile(..., 'w') needs a samplerate")
            if not str(filename).lower().endswith(".wav"):
                raise _unsupported("writing %r (only .wav)" % (filename,))
            self.samplerate, self.num_channels = samplerate, int(num_channels)
            self._chunks = []
        else:
            raise _unsupported("AudioFile mode %r" % (mode,))
        self.closed = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def tell(self):
        return self._pos

    def read(self, num_frames=None):
        end = self.frames if num_frames is None else min(self.frames, self._pos + int(num_frames))
        out = self._data[:, self._pos:end].copy()
        self._pos = end
        return out

    def write(self, samples):
        a = _np.asarray(samples, dtype=_np.float32)
        a = a.reshape(1, -1) if a.ndim == 1 else a
        if a.shape[0] != self.num_channels:
            raise ValueError("AudioFile: %d channels written to a %d-channel file" % (a.shape[0], self.num_channels))
        self._chunks.append(a)

    def close(self):
        if self.closed:
            return
        self.closed = True
        if self.mode == "w":
            x = _np.concatenate(self._chunks, axis=1) if self._chunks else _np.zeros((self.num_channels, 0), _np.float32)
            pcm = _np.rint(_np.clip(x.astype(_np.float64), -1.0, 1.0) * 32767.0).astype(_np.int16)   # = csrc/fx.hip fx_to_pcm16
            _cover.write_pcm16(self.filename, pcm.T, int(self.samplerate))
