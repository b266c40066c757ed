"""Opt-in stand-in for the part of pydub that the reference's src/main.py uses (combine_audio, :229-233), mixed on the device by
aicovergen_amd.cover with pydub's arithmetic (audioop semantics).  src/run_main.py puts src/compat first on sys.path only when
AICG_DEVICE_POST=1.

Supported: AudioSegment.from_wav (16-bit PCM, 1 or 2 channels), `segment - dB` / `segment + dB`, overlay(other) with its defaults,
export(path, format) ('wav' directly, other formats through ffmpeg), and the channels / frame_rate / sample_width / frame_count /
len() queries.  Anything else raises NotImplementedError."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))))

import numbers as _numbers  # noqa: E402

import numpy as _np  # noqa: E402
import torch as _torch  # noqa: E402

from aicovergen_amd import cover as _cover, ops as _ops  # noqa: E402

SUPPORTED = ("AudioSegment.from_wav", "AudioSegment - dB", "AudioSegment + dB", "AudioSegment.apply_gain", "AudioSegment.overlay",
             "AudioSegment.export")


def _unsupported(what):
    return NotImplementedError("%s is not provided by the device stand-in for pydub (aicovergen_amd src/compat); supported: %s"
                               % (what, ", ".join(SUPPORTED)))


class AudioSegment:
    """16-bit PCM on the device.  Gains are kept pending (pydub applies each as its own audioop.mul pass, and so does the mix
    kernel, two per operand) and are applied by the next overlay or export."""

    sample_width = 2

    def __init__(self, pcm, frame_rate, gains=()):
        self._pcm, self.frame_rate, self._gains = pcm, int(frame_rate), tuple(gains)

    @classmethod
    def from_wav(cls, file, parameters=None):
        if parameters is not None or not isinstance(file, (str, _os.PathLike)):
            raise _unsupported("from_wav of %r with parameters=%r" % (type(file).__name__, parameters))
        pcm, sr = _cover.read_pcm16(_os.fspath(file))
        if pcm.shape[1] not in (1, 2):
            raise _unsupported("%d-channel audio" % pcm.shape[1])
        return cls(_torch.from_numpy(_np.ascontiguousarray(pcm)).to(_cover._device()), sr)

    @property
    def channels(self):
        return int(self._pcm.shape[1])

    @property
    def frame_width(self):
        return 2 * self.channels

    def frame_count(self, ms=None):
        if ms is not None:
            return ms * (self.frame_rate / 1000.0)
        return float(self._pcm.shape[0])

    def __len__(self):
        return round(1000 * (self.frame_count() / self.frame_rate))

    def _applied(self):
        """This segment with its pending gains applied (one mix pass, nothing added)."""
        if not self._gains:
            return self._pcm
        g = self._gains + (1.0,) * (2 - len(self._gains))
        empty = self._pcm[:0]
        return _ops.pcm16_mix(self._pcm, self.frame_rate, g, empty, self.frame_rate, (1.0, 1.0), self._pcm.shape[0])

    def apply_gain(self, volume_change):
        f = _cover.db_to_float(float(volume_change))
        if len(self._gains) == 2:
            return AudioSegment(self._applied(), self.frame_rate, (f,))
        return AudioSegment(self._pcm, self.frame_rate, self._gains + (f,))

    def __sub__(self, arg):
        if isinstance(arg, AudioSegment) or not isinstance(arg, _numbers.Real):
            raise _unsupported("AudioSegment - %s" % type(arg).__name__)
        return self.apply_gain(-arg)

    def __add__(self, arg):
        if isinstance(arg, AudioSegment) or not isinstance(arg, _numbers.Real):
            raise _unsupported("AudioSegment + %s (appending)" % type(arg).__name__)
        return self.apply_gain(arg)

    def overlay(self, seg, position=0, loop=False, times=None, gain_during_overlay=None):
        if position != 0 or loop or times is not None or gain_during_overlay is not None:
            raise _unsupported("overlay(position=%r, loop=%r, times=%r, gain_during_overlay=%r)" % (position, loop, times,
                                                                                                  gain_during_overlay))
        if not isinstance(seg, AudioSegment):
            raise _unsupported("overlay of %s" % type(seg).__name__)
        a, b = self, seg
        ga = a._gains + (1.0,) * (2 - len(a._gains))
        gb = b._gains + (1.0,) * (2 - len(b._gains))
        out, rate = _cover.overlay(a._pcm, a.frame_rate, ga, b._pcm, b.frame_rate, gb)
        return AudioSegment(out, rate)

    def export(self, out_f=None, format="mp3", codec=None, bitrate=None, parameters=None, tags=None, id3v2_version="4",
               cover=None):
        if not isinstance(out_f, (str, _os.PathLike)) or codec or bitrate or parameters or tags or cover:
            raise _unsupported("export to %r with codec / bitrate / parameters / tags / cover" % (type(out_f).__name__,))
        return _cover.export(self._applied().cpu().numpy(), self.frame_rate, _os.fspath(out_f), format)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        raise _unsupported("AudioSegment." + name)


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    raise _unsupported("pydub." + name)
