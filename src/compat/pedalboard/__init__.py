"""Opt-in stand-in for the part of pedalboard that the reference's src/main.py uses (add_audio_effects, :206-226), computed on the
device by aicovergen_amd.cover.  src/run_main.py puts src/compat first on sys.path only when AICG_DEVICE_POST=1.

Supported: Pedalboard([...])(audio, sample_rate, reset=...) with HighpassFilter, Compressor and Reverb (freeze_mode 0); the
plugins keep their state between calls unless reset=True.  Anything else raises NotImplementedError."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))))

import numpy as _np  # noqa: E402
import torch as _torch  # noqa: E402

from aicovergen_amd import cover as _cover  # noqa: E402

SUPPORTED = ("Pedalboard", "HighpassFilter", "Compressor", "Reverb", "io.AudioFile")


def _unsupported(what):
    return NotImplementedError("%s is not provided by the device stand-in for pedalboard (aicovergen_amd src/compat); supported: %s"
                               % (what, ", ".join(SUPPORTED)))


class _Plugin:
    def __init__(self):
        self._state, self._key = None, None

    def reset(self):
        self._state, self._key = None, None

    def _run(self, x, sr):
        key = (int(sr), x.shape[0])
        if key != self._key:
            self._state, self._key = None, key
        # one segment: the chunks of a stream are continued exactly from the carried state
        y, self._state = self._process(x, sr, self._state)
        return y


class HighpassFilter(_Plugin):
    def __init__(self, cutoff_frequency_hz=50):
        super().__init__()
        self.cutoff_frequency_hz = float(cutoff_frequency_hz)

    def _process(self, x, sr, state):
        return _cover.highpass(x, sr, self.cutoff_frequency_hz, state=state, segment=0)


class Compressor(_Plugin):
    def __init__(self, threshold_db=0, ratio=1, attack_ms=1.0, release_ms=100):
        super().__init__()
        self.threshold_db, self.ratio = float(threshold_db), float(ratio)
        self.attack_ms, self.release_ms = float(attack_ms), float(release_ms)

    def _process(self, x, sr, state):
        return _cover.compressor(x, sr, self.threshold_db, self.ratio, self.attack_ms, self.release_ms, state=state, segment=0)


class Reverb(_Plugin):
    def __init__(self, room_size=0.5, damping=0.5, wet_level=0.33, dry_level=0.4, width=1.0, freeze_mode=0.0):
        super().__init__()
        if freeze_mode >= 0.5:
            raise _unsupported("Reverb(freeze_mode=%r)" % (freeze_mode,))
        self.room_size, self.damping, self.wet_level, self.dry_level, self.width = (
            float(room_size), float(damping), float(wet_level), float(dry_level), float(width))

    def _process(self, x, sr, state):
        return _cover.reverb(x, sr, self.room_size, self.damping, self.wet_level, self.dry_level, self.width, state=state,
                             segment=0)


class Pedalboard:
    def __init__(self, plugins=None):
        plugins = list(plugins or [])
        for p in plugins:
            if not isinstance(p, _Plugin):
                raise _unsupported(type(p).__name__)
        self.plugins = plugins

    def reset(self):
        for p in self.plugins:
            p.reset()

    def __call__(self, input_array, sample_rate, buffer_size=None, reset=True):
        return self.process(input_array, sample_rate, buffer_size, reset)

    def process(self, input_array, sample_rate, buffer_size=None, reset=True):
        """(channels, frames) or (frames,) float32 -> the same shape, float32 (pedalboard's layout for 2-D input)."""
        a = _np.asarray(input_array, dtype=_np.float32)
        if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[0] not in (1, 2)):
            raise _unsupported("audio of shape %s (use (channels, frames) with 1 or 2 channels)" % (a.shape,))
        if reset:
            self.reset()
        x = _torch.from_numpy(_np.ascontiguousarray(a.reshape(1, -1) if a.ndim == 1 else a)).to(_cover._device())
        for p in self.plugins:
            x = p._run(x, sample_rate)
        y = x.cpu().numpy()
        return y.reshape(-1) if a.ndim == 1 else y


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    raise _unsupported("pedalboard." + name)
