"""Opt-in stand-in for the part of pysox that the reference's src/main.py uses (pitch_shift, :138-147), computed on the device by
aicovergen_amd.cover.  src/run_main.py puts src/compat first on sys.path only when AICG_DEVICE_POST=1.

Supported: Transformer().pitch(n_semitones, quick=False) and Transformer().build_array(input_array=, sample_rate_in=) on a
(frames, channels) or (frames,) float array with 1 or 2 channels; the result has the input's shape and dtype.  Anything else raises
NotImplementedError."""
import os as _os
import sys as _sys

_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))))

import numpy as _np  # noqa: E402
import torch as _torch  # noqa: E402

from aicovergen_amd import cover as _cover  # noqa: E402

SUPPORTED = ("Transformer().pitch(n_semitones, quick=False)", "Transformer().build_array(input_array=, sample_rate_in=)")


def _unsupported(what):
    return NotImplementedError("%s is not provided by the device stand-in for sox (aicovergen_amd src/compat); supported: %s"
                               % (what, ", ".join(SUPPORTED)))


class Transformer:
    def __init__(self):
        self._semitones = []

    def pitch(self, n_semitones, quick=False):
        if quick:
            raise _unsupported("Transformer().pitch(quick=True)")
        if isinstance(n_semitones, bool) or not isinstance(n_semitones, (int, float)):
            raise ValueError("n_semitones must be a number, got %r" % (n_semitones,))
        self._semitones.append(n_semitones)
        return self

    def build_array(self, input_filepath=None, input_array=None, sample_rate_in=None, extra_args=None):
        if input_filepath is not None or extra_args is not None:
            raise _unsupported("Transformer().build_array(input_filepath= / extra_args=)")
        if input_array is None or sample_rate_in is None:
            raise ValueError("build_array needs input_array and sample_rate_in")
        a = _np.asarray(input_array)
        if a.dtype.kind != "f":
            raise _unsupported("audio of dtype %s (use a float array)" % a.dtype)
        if a.ndim not in (1, 2) or (a.ndim == 2 and a.shape[1] not in (1, 2)):
            raise _unsupported("audio of shape %s (use (frames, channels) with 1 or 2 channels)" % (a.shape,))
        x = _torch.from_numpy(_np.ascontiguousarray((a.reshape(-1, 1) if a.ndim == 1 else a).T, dtype=_np.float32)).to(_cover._device())
        for n in self._semitones:
            x, _ = _cover.pitch_shift_signal(x, int(sample_rate_in), n)
        return _np.ascontiguousarray(x.cpu().numpy().T).reshape(a.shape).astype(a.dtype)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        raise _unsupported("Transformer()." + name)


def __getattr__(name):
    if name.startswith("__"):
        raise AttributeError(name)
    raise _unsupported("sox." + name)
