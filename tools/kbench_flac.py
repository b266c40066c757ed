"""Time the two ways a finished cover leaves the device, on a 240 s stereo 44.1 kHz mix (three song-like stems through
cover.mix_stems) that lives there, in one process: the FLAC route (ops.flac_encode, the download of the file's bytes through pinned
memory, the file write; csrc/flac.hip) and the WAV route (the download of the PCM, cover.write_pcm16); median of 10 wall-clock runs
after warm-up, the encoder's device time beside them, and the compression ratio.  Decodes nothing: tests/test_flac.py does.
Writes profiles/flac_kbench.json and prints the same JSON line.
usage: python tools/kbench_flac.py [seconds]"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from aicovergen_amd import cover, ops  # noqa: E402
from kbench_pitch_ac import timed, wall  # noqa: E402
from synthetic.inputs import song_like  # noqa: E402


def main():
    seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 240.0
    sr = 44100
    stems = [torch.from_numpy(np.ascontiguousarray(np.rint(song_like(seconds, sr, seed=s).T * 0.5 * 32767).astype(np.int16))).cuda()
             for s in (31, 32, 33)]
    mix, sr = cover.mix_stems(stems[0], sr, stems[1], sr, stems[2], sr, 0, 0, 0)
    d = tempfile.mkdtemp()
    flac_path, wav_path = os.path.join(d, "cover.flac"), os.path.join(d, "cover.wav")

    def flac_route():
        cover.export_flac(mix, sr, flac_path)

    def wav_route():
        cover.write_pcm16(wav_path, mix.cpu().numpy(), sr)

    flac_route()
    wav_route()
    res = {"seconds": seconds, "frames": int(mix.shape[0]), "channels": int(mix.shape[1]),
           "flac_bytes": os.path.getsize(flac_path), "wav_bytes": os.path.getsize(wav_path),
           "ratio": os.path.getsize(flac_path) / os.path.getsize(wav_path),
           "flac_route_ms": wall(flac_route, reps=10),
           "wav_route_ms": wall(wav_route, reps=10),
           "flac_encode_gpu_ms": timed(lambda: ops.flac_encode(mix, sr), reps=10)}
    line = json.dumps(res)
    with open(os.path.join(ROOT, "profiles", "flac_kbench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
