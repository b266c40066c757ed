"""csrc/flac.hip (ops.flac_encode, the cover's `-oformat flac`) against tests/flac_decode_ref.py, a decoder written from RFC 9639: every
file must decode -- both CRCs, frame numbering, STREAMINFO's sizes and totals are checked there -- to exactly the samples that went in.
The encoder picks by exact bit count from a candidate set that holds every FIXED predictor with one Rice parameter for the block and
VERBATIM, so no frame may be larger than the best of those: a condition without a margin."""
import os
import wave

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import flac_decode_ref as ref
from aicovergen_amd import _lib, cover, ops
from test_cover_pipeline import world  # noqa: F401  (the miniature models, the 3 s song and one keep_files cover; a fixture)

SR = 44100
LENGTHS = (0, 1, 3, 255, 256, 257, 4097)
_made = {}


def signal(kind, n, ch):
    """One array per (kind, n, channels), shared by the tests and never written to."""
    key = (kind, n, ch)
    if key not in _made:
        rng = np.random.default_rng(1000 * len(kind) + n + ch)
        t = np.arange(n)
        if kind == "zeros":
            x = np.zeros((n, ch))
        elif kind == "lowest":
            x = np.full((n, ch), -32768.0)
        elif kind == "alternating":
            x = np.repeat(np.where(t % 2 == 0, 32767.0, -32768.0)[:, None], ch, 1)
        elif kind == "noise":
            x = rng.integers(-32768, 32768, (n, ch)).astype(np.float64)
        elif kind == "uniform8":
            x = rng.integers(-128, 128, (n, ch)).astype(np.float64)
        elif kind == "sine":
            x = np.stack([12000 * np.sin(2 * np.pi * 440 * (1 + 0.5 * c) * t / SR + c) + rng.normal(0, 2, n) for c in range(ch)], 1)
        elif kind == "ramp":
            x = np.stack([(-30000 + (7 + 4 * c) * t) % 60000 - 30000 for c in range(ch)], 1).astype(np.float64)
        elif kind == "equal":       # R = L
            x = np.repeat((9000 * np.sin(2 * np.pi * 300 * t / SR) + rng.normal(0, 40, n))[:, None], 2, 1)
        else:                       # "opposite": R = -L
            l = 9000 * np.sin(2 * np.pi * 300 * t / SR) + rng.normal(0, 40, n)
            x = np.stack([l, -l], 1)
        _made[key] = np.clip(np.rint(x), -32768, 32767).astype(np.int16).reshape(n, ch)
    return _made[key]


def encode(dev, pcm, block, sr=SR):
    out = ops.flac_encode(dev.t(torch.from_numpy(pcm)), sr, block)
    assert out.dtype == torch.uint8 and out.dim() == 1 and out.device.type == dev.device.type
    return out.cpu().numpy().tobytes()


def round_trip(dev, pcm, block, sr=SR):
    data = encode(dev, pcm, block, sr)
    got, info, frames = ref.decode(data)
    assert got.dtype == np.int16 and got.shape == pcm.shape and got.tobytes() == pcm.tobytes()
    assert (info["sample_rate"], info["channels"], info["bits_per_sample"], info["total_samples"]) == (sr, pcm.shape[1], 16, len(pcm))
    assert info["min_blocksize"] == info["max_blocksize"] == block and info["md5"] == bytes(16) and info["metadata_blocks"] == 1
    assert len(frames) == -(-len(pcm) // block) and len(data) == 42 + sum(f["size"] for f in frames)
    return data, frames


def verbatim_size(n, ch, block):
    """The file with every subframe VERBATIM and independent channels: 42 bytes, and per frame at most 16 header and 2 CRC bytes."""
    return 42 + sum(18 + -(-ch * (8 + 16 * min(block, n - s)) // 8) for s in range(0, n, block))


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("kind", ["zeros", "lowest", "alternating", "noise", "sine", "ramp", "uniform8"])
def test_round_trip_bit_for_bit(dev, kind, ch):
    for n in LENGTHS:
        pcm = signal(kind, n, ch)
        data, frames = round_trip(dev, pcm, 256)
        subs = [s for f in frames for s in f["subframes"]]
        types = {s["type"] for s in subs}
        if n == 0:
            assert len(data) == 42
        if kind in ("zeros", "lowest") and n:
            assert types == {"CONSTANT"}
        if kind == "alternating":       # differences of 65535: a FIXED predictor's residuals are the largest there are, so none wins with a
            # Rice code.  (x[i] = -x[i - 1] - 1 is a first-order recurrence: where the block is long enough to pay for the coefficient,
            # LPC order 1 predicts it and is the cheapest by exact count.)
            assert all(s["type"] in ("VERBATIM", "LPC") or s["escapes"] > 0 for s in subs if s["type"] != "CONSTANT")
            assert n != 3 or types <= {"VERBATIM", "CONSTANT"}         # (stereo: the side of two equal channels is constant)
        if kind == "uniform8" and n >= 255:         # flat over 8 bits: raw bits are shorter than any Rice code
            assert any(s["escapes"] > 0 for s in subs)
        if kind == "noise":
            assert len(data) <= verbatim_size(n, ch, 256)
        if kind == "sine" and n >= 256:
            assert "LPC" in types
        if kind == "ramp" and n >= 256:
            assert "FIXED" in types
        if n and n % 256:                           # the last, short block carries its size in the tail field
            assert frames[-1]["blocksize"] == n % 256 and frames[-1]["blocksize_code"] in (6, 7)
        for s, f in ((s, f) for f in frames for s in f["subframes"]):
            assert s["order"] < f["blocksize"] or s["order"] == 0


@pytest.mark.parametrize("kind,modes", [("equal", {"left/side", "side/right"}), ("opposite", {"left/side", "side/right", "mid/side"})])
def test_stereo_decorrelation(dev, kind, modes):
    for n in LENGTHS:
        _, frames = round_trip(dev, signal(kind, n, 2), 256)
        if n >= 255:
            assert {f["assignment"] for f in frames if f["blocksize"] >= 255} <= modes
    if kind == "opposite":      # mid = 0: a CONSTANT subframe next to the side channel
        assert any(f["assignment"] == "mid/side" and f["subframes"][0]["type"] == "CONSTANT" for f in frames)


@pytest.mark.parametrize("ch", [1, 2])
def test_default_block_size(dev, ch):
    pcm = signal("sine", 3 * 4096 + 17, ch)
    data = ops.flac_encode(dev.t(torch.from_numpy(pcm)), SR).cpu().numpy().tobytes()
    got, info, frames = ref.decode(data)
    assert got.tobytes() == pcm.tobytes() and info["max_blocksize"] == 4096 and [f["blocksize"] for f in frames] == [4096] * 3 + [17]
    assert len(data) < 0.75 * pcm.nbytes
    for block in (512, 1024, 2048):
        round_trip(dev, pcm[:2 * block + 300], block)
    for sr in (8000, 40000, 12345, 123450, 700001):     # table code, kHz tail, Hz tail, tens-of-Hz tail, "see STREAMINFO"
        round_trip(dev, pcm[:300], 256, sr)


@pytest.mark.parametrize("frames", [129, 2049])
def test_frame_number_coding(dev, frames):
    """Frame numbers 127 -> 128 and 2047 -> 2048: the coded number grows to two and to three bytes."""
    n = frames * 256
    pcm = signal("sine", 524544, 1)[:n]
    _, recs = round_trip(dev, pcm, 256)
    assert [r["number"] for r in recs] == list(range(frames))
    assert recs[127]["header_bytes"] + 1 == recs[128]["header_bytes"]
    if frames > 2048:
        assert recs[2047]["header_bytes"] + 1 == recs[2048]["header_bytes"]


def baseline_bits(x, bps=16):
    """The simple encoder for one channel of one block: the best FIXED order 0..4 with ONE Rice parameter (partition order 0), by
    exact count, against VERBATIM."""
    x = x.astype(np.int64)
    best = 8 + bps * len(x)
    for order in range(0, min(4, len(x) - 1) + 1):
        r = np.diff(x, order)
        z = np.where(r >= 0, 2 * r, -2 * r - 1)
        rice = min(int(np.sum((z >> k) + 1 + k)) for k in range(15))
        best = min(best, 8 + bps * order + 2 + 4 + 4 + rice)
    return best


@pytest.mark.parametrize("ch", [1, 2])
@pytest.mark.parametrize("kind", ["sine", "ramp", "noise"])
def test_never_worse_than_the_simple_encoder(dev, kind, ch):
    pcm = signal(kind, 4097, ch)
    for block in (256, 4096):
        _, frames = round_trip(dev, pcm, block)
        for f in frames:
            x = pcm[f["number"] * block:f["number"] * block + f["blocksize"]]
            simple = f["header_bytes"] + -(-sum(baseline_bits(x[:, c]) for c in range(ch)) // 8) + 2
            assert f["size"] <= simple, (kind, ch, block, f["number"], f["size"], simple)


def test_bad_arguments(dev):
    x = dev.t(torch.zeros(300, 2, dtype=torch.int16))
    with pytest.raises(ValueError):
        ops.flac_encode(dev.t(torch.zeros(300, 3, dtype=torch.int16)), SR)
    with pytest.raises(TypeError):
        ops.flac_encode(x.float(), SR)
    with pytest.raises(ValueError):
        ops.flac_encode(x, SR, 300)
    with pytest.raises(ValueError):
        ops.flac_encode(x, 0)
    lib = _lib.get()
    geom = torch.zeros(4, dtype=torch.int64)
    assert lib.aicg_flac_geometry(300, 3, SR, 256, geom.data_ptr()) == -1
    assert lib.aicg_flac_geometry(-1, 2, SR, 256, geom.data_ptr()) == -1
    assert lib.aicg_flac_geometry(1 << 36, 2, SR, 4096, geom.data_ptr()) == -1
    assert lib.aicg_flac_geometry(300, 2, SR, 300, geom.data_ptr()) == -2
    assert lib.aicg_flac_geometry(300, 2, 1 << 20, 256, geom.data_ptr()) == -2
    assert lib.aicg_flac_geometry(300, 2, SR, 256, None) == -2
    assert lib.aicg_flac_geometry(300, 2, SR, 256, geom.data_ptr()) == 0 and geom[0] == 2
    ws = dev.t(torch.zeros(int(geom[1]), dtype=torch.uint8))
    out = dev.t(torch.zeros(int(geom[2]), dtype=torch.uint8))
    size = dev.t(torch.zeros(1, dtype=torch.int64))
    args = lambda n, ch, block, cap, pcm=x: (pcm.data_ptr() if pcm is not None else None, n, ch, SR, block, ws.data_ptr(), out.data_ptr(), cap,
                                             size.data_ptr(), None)
    assert lib.aicg_flac_encode(*args(300, 3, 256, int(geom[2]))) == -1
    assert lib.aicg_flac_encode(*args(300, 2, 300, int(geom[2]))) == -2
    assert lib.aicg_flac_encode(*args(300, 2, 256, int(geom[2]) - 1)) == -2
    assert lib.aicg_flac_encode(*args(300, 2, 256, int(geom[2]), None)) == -2
    assert b"aicg_flac_encode" in lib.aicg_last_error()
    assert lib.aicg_flac_encode(*args(300, 2, 256, int(geom[2]))) == 0


@pytest.mark.skipif(ref.other_decoder() is None, reason="neither soundfile nor a flac binary on this machine")
def test_another_decoder_agrees(dev, tmp_path):
    for kind, n, ch, block in (("sine", 4097, 2, 256), ("opposite", 4097, 2, 256), ("noise", 257, 1, 256), ("sine", 3 * 4096 + 17, 2, 4096)):
        pcm = signal(kind, n, ch)
        assert ref.decode_with_other(encode(dev, pcm, block), tmp_path).tobytes() == pcm.tobytes()


# ---- the cover --------------------------------------------------------------------------------------------------------------------
def _pcm(seconds, rate, channels, seed, amp=0.5):       # tests/test_cover_mix.py's stems
    rng = np.random.default_rng(seed)
    n = int(seconds * rate)
    t = np.arange(n) / rate
    x = np.stack([amp * np.sin(2 * np.pi * (300 + 50 * c) * t) + 0.2 * amp * rng.standard_normal(n) for c in range(channels)], 1)
    return np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)


def _wav_frames(path):
    with wave.open(path, "rb") as w:
        return w.getnchannels(), w.getframerate(), w.readframes(w.getnframes())


def test_combine_audio_writes_flac(dev, tmp_path):
    paths = []
    for name, (s, r, c), seed in (("v", (0.5, 40000, 1), 6), ("b", (0.5, 44100, 2), 7), ("i", (0.5, 44100, 2), 8)):
        p = str(tmp_path / (name + ".wav"))
        wavfile.write(p, r, _pcm(s, r, c, seed)[:, 0] if c == 1 else _pcm(s, r, c, seed))
        paths.append(p)
    cover.combine_audio(paths, str(tmp_path / "cover.wav"), 1, -1, 0, "wav")
    cover.combine_audio(paths, str(tmp_path / "cover.flac"), 1, -1, 0, "flac")
    ch, sr, want = _wav_frames(str(tmp_path / "cover.wav"))
    got, info, frames = ref.decode(open(str(tmp_path / "cover.flac"), "rb").read())
    assert (info["channels"], info["sample_rate"]) == (ch, sr) and got.tobytes() == want and len(want) > 80000
    assert all(f["blocksize"] == 4096 for f in frames[:-1]) and os.path.getsize(str(tmp_path / "cover.flac")) < len(want)
    # the pydub stand-in's export goes through cover.export: the same route, the same bytes
    cover.export(np.frombuffer(want, dtype=np.int16).reshape(-1, ch), sr, str(tmp_path / "again.flac"), "flac")
    assert open(str(tmp_path / "again.flac"), "rb").read() == open(str(tmp_path / "cover.flac"), "rb").read()


def test_cover_pipeline_writes_flac(world, monkeypatch):  # noqa: F811
    import test_cover_pipeline as tcp
    w = world
    monkeypatch.setattr(cover.shutil, "which", lambda name: None)        # flac needs no ffmpeg, installed or not
    ch, sr, want = _wav_frames(w.cover)
    kw = dict(tcp.KW, output_format="flac")
    path = w.session.song_cover_pipeline(w.song, "Voice", 0, False, **kw)
    assert path == os.path.join(w.dir, "song (Voice Ver).flac")
    data = open(path, "rb").read()
    got, info, _ = ref.decode(data)
    assert (info["channels"], info["sample_rate"]) == (ch, sr) and got.tobytes() == want and len(data) < len(want)
    os.remove(path)
    again = cover.main(["-i", w.song, "-dir", "Voice", "-p", "0", "-pall", "2", "-oformat", "flac", "--mdx-models-dir", w.mdx_dir,
                        "--rvc-models-dir", w.rvc_dir, "--output-dir", w.out_dir])
    assert again == path and open(path, "rb").read() == data
