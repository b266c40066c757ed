"""csrc/pitch.hip at every launch form the sample rates reach, and at its edges in length and content, against the float64 restatement
in tests/pitch_restated.py.  tempo_wsola_kernel derives its whole launch geometry from the rate -- search width and
overlap, the cut of the overlap into S slices of L frames, the walk of the (slice, 4 candidates) items over the threads, the size of
the prefetch -- and tests/test_cover_pitch.py runs two rates.  Here: the host geometry at every common rate, the tie model and the
arithmetic with injected offsets at one rate per code path (the table in test_launch_arithmetic_puts_each_rate_on_its_path), the
edges in length and content, and resample_ratio_kernel on signals shorter than its filter and outputs beyond the input's end.

No bound is new: tie_eps, the 6 u cross-fade bound of test_arithmetic_with_offsets_injected, table_error_bound and one 16-bit step.
Every parity test exists on the emulator and, marked gpu, on the MI355X."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import pitch_restated as R
from aicovergen_amd import ops
from test_cover_pitch import _tie_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RATES = (8000, 11025, 16000, 22050, 24000, 32000, 40000, 44100, 48000, 88200, 96000, 176400, 192000, 384000)
# (rate, channels): one per path of the search (see the table below), mono and stereo where the path depends on the channel count
FORMS = ((16000, 1), (16000, 2), (22050, 2), (48000, 1), (48000, 2), (96000, 2), (192000, 1), (384000, 2))
FREE = [(sr, c, n) for sr, c in FORMS for n in (2, -3)] + [(48000, 2, n) for n in (12, -12, 1, -1)]
EDGE_FORMS = ((8000, 1), (48000, 2), (22050, 1))
STEPS = 6


def _ratio(n):
    return 2.0 ** (n / 12.0)


def _tempo(semitones):
    return 1.0 / _ratio(semitones)


def _shortest(sr, f, n_out):
    """The shortest input whose output has at least n_out frames."""
    n = max(0, int(math.floor((n_out - 1) * f)) - 2)
    while R.geometry(sr, f, n)["n_out"] < n_out:
        n += 1
    return n


def _six_steps(sr, f):
    """The longest input of STEPS steps: the last step is full, or short by a frame where no input length fills it."""
    n = _shortest(sr, f, STEPS * R.geometry(sr, f, 0)["adv"] + 1) - 1
    g = R.geometry(sr, f, n)
    assert g["steps"] == STEPS and g["n_out"] > STEPS * g["adv"] - 3
    return n


def _exactly(sr, f, extra):
    """An input whose output is exactly k adv + extra frames (for f < 1 not every output length exists: the first k that has one)."""
    adv = R.geometry(sr, f, 0)["adv"]
    for k in range(2, 64):
        n = _shortest(sr, f, k * adv + extra)
        if R.geometry(sr, f, n)["n_out"] == k * adv + extra:
            return n
    raise AssertionError("no input length gives k adv + %d output frames at %d Hz, tempo %g" % (extra, sr, f))


def _seconds(n, sr):
    """What R.stems and _tie_model turn back into exactly n frames."""
    s = (n + 0.5) / sr
    assert int(s * sr) == n
    return s


def _signal(n, sr, channels, seed):
    x = R.stems(_seconds(n, sr), sr, channels, seed)
    assert x.shape == (channels, n)
    return x


def _wsola(dev, x, sr, f, offsets=None):
    inj = None if offsets is None else dev.t(torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int32)))
    y, offs = ops.tempo_wsola(dev.t(torch.from_numpy(np.ascontiguousarray(x))), sr, f, inj)
    dev.sync()
    return y.cpu().numpy(), offs.cpu().numpy()


def _assert_arithmetic(y, ref):
    """test_arithmetic_with_offsets_injected's check: frames copied from the input are its bits; a cross-faded frame is
    fl(fl(o fl(1 - a)) + fl(x a)) with a = fl(fl(1 / ovl) j), within 6 u max(|o|, |x|) of the float64 value (u = 2^-24)."""
    assert y.shape == ref["y"].shape and y.dtype == np.float32
    cp = ref["copied"]
    assert np.array_equal(y[:, cp], ref["y"][:, cp].astype(np.float32)), "copied frames must be the input's bits"
    err = np.abs(y[:, ~cp].astype(np.float64) - ref["y"][:, ~cp])
    scale = ref["scale"][:, ~cp]
    assert np.all(err <= 6.0 * R.U * (1.0 + 1e-6) * scale), "worst %.2f u" % float((err / np.maximum(scale, 1e-30)).max() / R.U)


def _assert_geometry(sr, f, n, g):
    assert tuple(ops.tempo_wsola_geometry(sr, f, n)) == (g["seg"], g["search"], g["ovl"], g["skip"], g["steps"], g["n_out"])


def _free(dev, x, sr, f):
    """Free search on the device; the restatement walks along the device's offsets: the tie model of
    test_offsets_obey_the_tie_model, and the output's arithmetic along those offsets."""
    y, offs = _wsola(dev, x, sr, f)
    ref = R.wsola(x, sr, f, offsets=offs)
    g = ref["geom"]
    _assert_geometry(sr, f, x.shape[1], g)
    assert offs.shape == (g["steps"],) and offs.dtype == np.int32
    if g["steps"]:
        assert offs[0] == 0 and offs.min() >= 0 and offs.max() < g["search"]
    eps = R.tie_eps(g["ovl"], x.shape[0])
    assert np.all(ref["chosen"][1:] <= ref["best"][1:] * (1.0 + eps)), (offs, ref["argmin"], ref["chosen"], ref["best"])
    _assert_arithmetic(y, ref)
    return y, offs, ref


def _injected(dev, x, sr, f):
    """The offsets of an independent float64 run are injected: no near-tie can move a segment."""
    ref = R.wsola(x, sr, f)
    _assert_geometry(sr, f, x.shape[1], ref["geom"])
    y, used = _wsola(dev, x, sr, f, ref["offsets"])
    assert used.shape == ref["offsets"].shape and np.array_equal(used, ref["offsets"])
    _assert_arithmetic(y, ref)
    return y, ref


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- 1. geometry -------------------------------------------------------------------------------------------------------------------
def test_geometry_at_every_rate_matches_the_restatement(dev):
    """No kernel, the host arithmetic of whichever library is bound.  seg, search, ovl, skip, steps and n_out for every common rate, tempo factors from an octave down to an octave up,
    and the lengths around one step and one segment: llround against the restatement's floor(v + 0.5) at every .5 the list holds."""
    for sr in RATES:
        for semis in (-12, -7, -1, 1, 5, 12):
            f = 2.0 ** (-semis / 12.0)
            g0 = R.geometry(sr, f, 0)
            adv, seg, search = g0["adv"], g0["seg"], g0["search"]
            assert adv == seg - g0["ovl"] and g0["ovl"] % 8 == 0
            for n in (0, 1, adv - 1, adv, adv + 1, seg, seg + search, 3 * sr):
                _assert_geometry(sr, f, n, R.geometry(sr, f, n))


def _constant(name):
    text = open(os.path.join(ROOT, "aicovergen_amd", "csrc", "pitch.hip")).read()
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, "csrc/pitch.hip no longer states %s as a plain constant: restate the launch arithmetic of this test" % name
    return int(m.group(1))


def _launch(sr, channels):
    """aicg_tempo_wsola's launch arithmetic restated, with the kernel's two tuning constants read from its source."""
    nt, pre = _constant("kWsolaThreads"), _constant("kWsolaPre")
    g = R.geometry(sr, 1.0, 0)
    search, ovl = g["search"], g["ovl"]
    Gp = (search + 3) & ~3
    G = Gp // 4
    s_want = max(1, min(nt // G, ovl // 4))
    L = (-(-ovl // s_want) + 3) & ~3
    S = -(-ovl // L)
    return dict(search=search, ovl=ovl, Gp=Gp, G=G, S=S, L=L, tot=2 * channels * (search + ovl), nt=nt, held=pre * nt)


def test_launch_arithmetic_puts_each_rate_on_its_path():
    """Host only.  Why each rate is in FORMS: with the kernel's present kWsolaThreads and kWsolaPre, the rate reaches the path named.
    A retuning of either constant that moves a rate off its path fails here, by name, instead of the cover silently going."""
    table = {  # rate: (search, ovl, G, S, L)
        8000: (117, 96, 30, 24, 4), 16000: (235, 192, 59, 16, 12), 22050: (324, 264, 81, 11, 24), 44100: (647, 528, 162, 6, 88),
        48000: (705, 576, 177, 5, 116), 88200: (1295, 1056, 324, 3, 352), 96000: (1409, 1152, 353, 2, 576),
        192000: (2819, 2304, 705, 1, 2304), 384000: (5637, 4608, 1410, 1, 4608)}
    for sr, want in table.items():
        a = _launch(sr, 1)
        assert (a["search"], a["ovl"], a["G"], a["S"], a["L"]) == want, (sr, a)
        assert a["L"] % 4 == 0 and a["S"] * a["L"] >= a["ovl"] > (a["S"] - 1) * a["L"]
    assert (_launch(88200, 2)["tot"], _launch(96000, 2)["tot"]) == (9404, 10244)
    a = _launch(16000, 2)
    assert a["nt"] % a["G"] != 0 and a["S"] > 1, "16 kHz: several slices, and G does not divide the threads: tid / G, tid % G"
    for sr in table:                                 # S <= nt / G: a thread has at most one item, a second turn only where G > nt
        assert _launch(sr, 1)["S"] * _launch(sr, 1)["G"] <= a["nt"] or sr == 384000, sr
    assert a["tot"] <= a["held"], "16 kHz stereo: the prefetch fits the registers (the form without the tail loop)"
    a = _launch(22050, 2)
    assert a["Gp"] == a["search"], "22.05 kHz: no padded candidates"
    for sr, c in FORMS:
        if sr != 22050:
            assert _launch(sr, c)["Gp"] > _launch(sr, c)["search"]
    a = _launch(48000, 2)
    assert a["S"] * a["L"] > a["ovl"], "48 kHz: the last slice is clipped"
    for sr in (8000, 16000, 22050, 44100):
        assert _launch(sr, 1)["S"] * _launch(sr, 1)["L"] == _launch(sr, 1)["ovl"], sr
    a = _launch(96000, 2)
    assert a["tot"] > a["held"] and _launch(96000, 1)["tot"] <= a["held"], "96 kHz: the prefetch tail runs in stereo only"
    a = _launch(192000, 1)
    assert a["S"] == 1 and a["G"] <= a["nt"] and a["tot"] > a["held"], "192 kHz: one slice, one item per thread, the tail in mono"
    a = _launch(384000, 2)
    assert a["S"] == 1 and a["G"] > a["nt"], "384 kHz: more candidate groups than threads"
    lds = 4 * (2 * (a["Gp"] + a["ovl"] + 4) + 2 * a["ovl"] + a["S"] * a["Gp"] + 2 * (a["nt"] // 64))
    assert 128 * 1024 < lds <= 160 * 1024, "384 kHz stereo: 141 568 bytes of LDS, inside the 160 KiB the entry point allows"


# ---- 2. free search ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,channels,semitones", FREE)
def test_free_search_obeys_the_tie_model_at_every_launch_form(dev, sr, channels, semitones):
    """test_cover_pitch's tie model, unchanged, at one rate per path of the search: the shortest signal with six steps, so the
    prefetch for step k + 1, the stash shifted by i_k and every turn of the item walk occur five times."""
    f = _tempo(semitones)
    n = _six_steps(sr, f)
    _tie_model(dev, _seconds(n, sr), sr, channels, semitones, 100 + channels)


@pytest.mark.parametrize("sr,channels", FORMS)
@pytest.mark.parametrize("which", ["first", "last"])
def test_the_first_and_the_last_candidate_can_win(dev, sr, channels, which):
    """The overlap of step 1 is planted in the search window at offset 0 / search - 1: that candidate costs exactly 0 in any
    precision, every other one more, so the device must take it.  search - 1 is in the last group of four candidates, whatever
    padding follows it (none at 22.05 kHz), and at 384 kHz in a group a thread reaches on its second turn."""
    f = 2.0
    g = R.geometry(sr, f, 0)
    adv, ovl, search, skip = g["adv"], g["ovl"], g["search"], g["skip"]
    x = _signal(skip + g["seg"] + search, sr, channels, 170 + channels)
    at = skip + (0 if which == "first" else search - 1)
    assert adv + ovl <= skip
    x[:, at:at + ovl] = x[:, adv:adv + ovl]
    y, offs, ref = _free(dev, x, sr, f)
    assert ref["geom"]["steps"] == 2 and ref["best"][1] == 0.0
    assert offs[1] == at - skip == ref["argmin"][1]


def test_a_batch_is_its_signals_where_the_prefetch_tail_runs(dev):
    """96 kHz stereo, three different signals in one launch: each equals its own single-signal call bit for bit, output and offsets
    (the tail loop's fetches and the outputs are strided by the signal)."""
    sr, f = 96000, _tempo(2)
    n = _six_steps(sr, f)
    xs = np.stack([_signal(n, sr, 2, 110 + s) for s in range(3)])
    assert not np.array_equal(xs[0], xs[1]) and not np.array_equal(xs[1], xs[2])
    yb, ob = ops.tempo_wsola(dev.t(torch.from_numpy(xs)), sr, f)
    yb, ob = yb.cpu().numpy(), ob.cpu().numpy()
    assert yb.shape[:2] == (3, 2) and ob.shape == (3, STEPS)
    for s in range(3):
        y1, o1 = _wsola(dev, xs[s], sr, f)
        assert np.array_equal(_bits(yb[s]), _bits(y1)) and np.array_equal(ob[s], o1), s
    # and with the offsets injected, rotated among the signals so that a wrong stride shows
    inj = np.ascontiguousarray(np.roll(ob, 1, axis=0))
    yi, ui = ops.tempo_wsola(dev.t(torch.from_numpy(xs)), sr, f, dev.t(torch.from_numpy(inj)))
    assert np.array_equal(ui.cpu().numpy(), inj)
    for s in range(3):
        y1, _ = _wsola(dev, xs[s], sr, f, inj[s])
        assert np.array_equal(_bits(yi[s].cpu().numpy()), _bits(y1)), s


# ---- 3. offsets injected -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,channels", FORMS)
@pytest.mark.parametrize("semitones", [2, -3])
def test_arithmetic_with_offsets_injected_at_every_launch_form(dev, sr, channels, semitones):
    f = _tempo(semitones)
    x = _signal(_six_steps(sr, f), sr, channels, 120 + channels)
    _injected(dev, x, sr, f)


@pytest.mark.parametrize("sr,channels", FORMS)
def test_injected_offsets_are_clamped_to_the_search_range(dev, sr, channels):
    """Offsets below 0 and at or above `search` are used as 0 and search - 1: the offsets returned say so, and the output is the
    output of the clamped vector, bit for bit, and the restatement's along it."""
    f = _tempo(2)
    x = _signal(_six_steps(sr, f), sr, channels, 130 + channels)
    search = R.geometry(sr, f, 0)["search"]
    inj = np.array([0, -1, search, search - 1, -2 ** 31, 2 ** 31 - 1], np.int32)
    assert len(inj) == STEPS
    clamped = np.clip(inj.astype(np.int64), 0, search - 1).astype(np.int32)
    y, used = _wsola(dev, x, sr, f, inj)
    assert np.array_equal(used, clamped)
    y2, used2 = _wsola(dev, x, sr, f, clamped)
    assert np.array_equal(used2, clamped) and np.array_equal(_bits(y), _bits(y2))
    _assert_arithmetic(y, R.wsola(x, sr, f, offsets=clamped))


# ---- 4. edges in length and content --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,channels", EDGE_FORMS)
@pytest.mark.parametrize("semitones", [2, -3])
def test_edges_in_length(dev, sr, channels, semitones):
    """Nothing, one frame, one step less / exactly / more than a frame, a last step that is exactly full and one of one frame, and
    an input one frame short of a segment and a search width (past which step 1's window reads when the tempo factor is above 1):
    free search (tie model) and injected offsets."""
    f = _tempo(semitones)
    g = R.geometry(sr, f, 0)
    adv, seg, search = g["adv"], g["seg"], g["search"]
    full, one = _exactly(sr, f, 0), _exactly(sr, f, 1)
    assert R.geometry(sr, f, full)["n_out"] % adv == 0 and R.geometry(sr, f, one)["n_out"] % adv == 1
    assert R.geometry(sr, f, seg + search - 1)["steps"] >= 2
    if f > 1.0:                                     # (skip > adv: step 1's window ends past seg + search - 1)
        assert g["skip"] + search + g["ovl"] - 1 > seg + search - 1
    for n in (0, 1, adv - 1, adv, adv + 1, full, one, seg + search - 1):
        x = _signal(n, sr, channels, 140 + channels)
        y, offs, _ = _free(dev, x, sr, f)
        _injected(dev, x, sr, f)
        if n == 0:
            assert y.shape == (channels, 0) and offs.shape == (0,)


@pytest.mark.parametrize("sr,channels", EDGE_FORMS)
def test_windows_past_the_end_of_a_short_signal_at_twice_the_tempo(dev, sr, channels):
    """f = 2.0, the largest skip: the last step's search window begins two frames before the input's end, and the overlap it is
    compared with lies wholly past it.  And a tempo factor whose skip rounds up, far enough along that (steps - 1) skip >= n: the
    whole window of the last step is zeros.  The restatement reads zeros there, the kernel relies on the buffer range check."""
    g = R.geometry(sr, 2.0, 0)
    adv, skip = g["adv"], g["skip"]
    assert skip == 2 * adv
    n = 2 * (2 * adv + 1)
    g = R.geometry(sr, 2.0, n)
    assert g["steps"] == 3 and (g["steps"] - 1) * skip == n - 2
    x = _signal(n, sr, channels, 150 + channels)
    _free(dev, x, sr, 2.0)
    _injected(dev, x, sr, 2.0)
    f = (adv + 0.501) / adv                          # skip = adv + 1: each step gains 0.499 frames on its share of the input
    k = int(math.ceil(f / 0.5)) + 2
    n = _shortest(sr, f, k * adv + 1)
    g = R.geometry(sr, f, n)
    assert g["skip"] == adv + 1 and g["steps"] == k + 1 and k * g["skip"] >= n, (g, n)
    x = _signal(n, sr, channels, 152 + channels)
    y, offs, ref = _free(dev, x, sr, f)
    assert offs[-1] == 0 and ref["best"][-1] == ref["chosen"][-1]
    _injected(dev, x, sr, f)


@pytest.mark.parametrize("sr,channels", EDGE_FORMS)
def test_silence_and_a_constant(dev, sr, channels):
    """All zeros: every candidate ties, the lowest wins, the output is zeros.  A constant: the offsets obey the tie model, and
    wherever every frame a step can read lies inside the input the output is the constant within the cross-fade's 6 u."""
    f = _tempo(2)
    g = R.geometry(sr, f, 0)
    n = _six_steps(sr, f)
    y, offs = _wsola(dev, np.zeros((channels, n), np.float32), sr, f)
    assert offs.shape == (STEPS,) and not offs.any() and y.shape == (channels, R.geometry(sr, f, n)["n_out"]) and not _bits(y).any()
    c = np.float32(0.3)
    y, offs, ref = _free(dev, np.full((channels, n), c, np.float32), sr, f)
    inside = [k for k in range(STEPS) if k * g["skip"] + g["search"] + g["seg"] <= n]
    assert len(inside) >= 3
    interior = y[:, :(inside[-1] + 1) * g["adv"]].astype(np.float64)
    assert not offs[:inside[-1] + 1].any()
    assert np.all(np.abs(interior - float(c)) <= 6.0 * R.U * (1.0 + 1e-6) * float(c))


def test_one_infinite_sample_stays_where_it_is_and_nan_falls_back_to_offset_0(dev):
    """8 kHz mono, ten steps, one +inf in the middle.  The call returns and every offset is in [0, search).  A step whose search
    window and overlap do not hold the sample, and whose predecessor took the clean run's offset, takes the clean run's offset too
    (the search is deterministic), and all of its frames that are not computed from the sample are the clean run's bits.  The
    steps before the sample are such steps by geometry alone; behind it the chain may have moved, so the offsets say which are."""
    sr, f = 8000, _tempo(2)
    g = R.geometry(sr, f, 0)
    adv, ovl, search, skip = g["adv"], g["ovl"], g["search"], g["skip"]
    x = _signal(_shortest(sr, f, 10 * adv), sr, 1, 160)
    n = x.shape[1]
    bad = 5 * skip + search // 2 + 40                 # in step 5's search window, in nobody's overlap
    assert n // 2 - adv < bad < n // 2 + adv
    y0, o0 = _wsola(dev, x, sr, f)
    xb = x.copy()
    xb[0, bad] = np.inf
    y1, o1 = _wsola(dev, xb, sr, f)
    assert o1.shape == (10,) and o1.min() >= 0 and o1.max() < search and y1.shape == y0.shape
    # step 0 copies input frames 0 .. adv
    same = np.ones(y0.shape[1], bool)
    same[:adv] = np.arange(adv) != bad
    in_sync, before = [True], 0
    for k in range(1, 10):
        p, prev = k * skip, (k - 1) * skip + int(o1[k - 1]) + adv
        clean = not (p <= bad < p + search + ovl) and not (prev <= bad < prev + ovl)
        ok = clean and o1[k - 1] == o0[k - 1]
        in_sync.append(bool(ok))
        j = np.arange(adv)
        touched = (p + int(o1[k]) + j == bad) | ((j < ovl) & (prev + j == bad))
        same[k * adv:(k + 1) * adv] = ~touched if ok else False
        if ok:
            assert o1[k] == o0[k], (k, o1, o0)
        if p + search + ovl <= bad and (k - 1) * skip + search + adv + ovl <= bad:
            before += 1
            assert ok
    assert before == 4 and not in_sync[5], (before, in_sync)
    assert np.array_equal(_bits(y1)[:, same], _bits(y0)[:, same])
    assert np.isfinite(y1[:, same]).all() and not np.isfinite(y1).all()
    # no finite cost at all: two NaN samples of which step 5's overlap holds one whichever offset step 4 took (the overlap begins
    # 4 skip + adv + i_4 and has ovl frames), so every candidate of step 5 costs NaN and the kernel falls back to offset 0
    base = 4 * skip + adv
    assert all(any(i <= d < i + ovl for d in (60, 150)) for i in range(search))
    xn = x.copy()
    xn[0, [base + 60, base + 150]] = np.nan
    y2, o2 = _wsola(dev, xn, sr, f)
    assert o2.min() >= 0 and o2.max() < search and o2[5] == 0 and np.array_equal(o2[:5], o0[:5])
    assert np.array_equal(_bits(y2)[:, :4 * adv], _bits(y0)[:, :4 * adv])


@pytest.mark.parametrize("sr,channels", [(96000, 2), (16000, 2)])
def test_two_calls_give_the_same_bits(dev, sr, channels):
    """One form whose prefetch overflows the registers into the tail loop, one whose prefetch fits."""
    assert (_launch(sr, channels)["tot"] > _launch(sr, channels)["held"]) == (sr == 96000)
    f = _tempo(-3)
    x = _signal(_six_steps(sr, f), sr, channels, 180)
    y, offs = _wsola(dev, x, sr, f)
    y2, offs2 = _wsola(dev, x, sr, f)
    assert np.array_equal(_bits(y), _bits(y2)) and np.array_equal(offs, offs2)


# ---- 5. resample_ratio at its edges --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table_bound(d):
    return R.table_error_bound(d)


def _resample(dev, x, d, n_out):
    y = ops.resample_ratio(dev.t(torch.from_numpy(np.ascontiguousarray(x))), d, n_out)
    dev.sync()
    return y.cpu().numpy()


def _assert_resampled(y, x, d, n_out):
    """test_resampler_against_the_exact_filter's two checks, and exact zeros where no tap reaches a sample."""
    ref = R.resample(x, d, n_out)
    assert y.shape == ref.shape == (x.shape[0], n_out) and y.dtype == np.float32
    peak = float(np.abs(x).max()) if x.size else 0.0
    err = np.abs(y.astype(np.float64) - ref)
    assert np.all(err <= _table_bound(d) * peak + R.U * np.abs(ref)), (x.shape, d, n_out, float(err.max()))
    if n_out:
        assert np.abs(R.to_int16(y).astype(np.int32) - R.to_int16(ref)).max() <= 1
    half = ops.resample_ratio_design(d)[2]
    t0 = np.floor(np.arange(n_out, dtype=np.float64) * d)
    unreached = t0 - half >= x.shape[1]
    assert not ref[:, unreached].any() and not _bits(y)[:, unreached].any()
    return unreached


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("semitones", [-12, -1, 1, 12])
def test_resampler_on_signals_shorter_than_its_filter(dev, channels, semitones):
    """n_in from one sample to just over the filter's length: the first and the last tap are both clipped for every output.  n_out
    from one frame to three filter half lengths beyond the input's end: the outputs there follow the restatement and are exactly 0
    from where no tap reaches a sample."""
    d = _ratio(semitones)
    half = ops.resample_ratio_design(d)[2]
    assert half == R.design(d)["half"]
    for n_in in (1, 2, half, 2 * half, 2 * half + 1, 2 * half + 2):
        x = _signal(n_in, 8000, channels, 200 + channels)
        for n_out in (1, int(round(n_in / d)), int(round(n_in / d)) + 3 * half):
            unreached = _assert_resampled(_resample(dev, x, d, n_out), x, d, n_out)
            if n_out > n_in / d + 2 * half and 3 * half - 2.5 >= half / d:
                assert unreached.any()


def test_resampler_batch_is_its_signals(dev):
    d = _ratio(-1)
    half = ops.resample_ratio_design(d)[2]
    xs = np.stack([_signal(2 * half + 1, 8000, 2, 210 + s) for s in range(3)])
    n_out = int(round(xs.shape[2] / d)) + 3 * half
    yb = ops.resample_ratio(dev.t(torch.from_numpy(xs)), d, n_out).cpu().numpy()
    assert yb.shape == (3, 2, n_out)
    for s in range(3):
        assert np.array_equal(_bits(yb[s]), _bits(_resample(dev, xs[s], d, n_out))), s


def test_the_filter_and_its_bound_exist_at_the_ratio_limits():
    """Host only.  The design and the table's error bound are functions of the ratio through nu = min(1, 1 / ratio) alone: below 1
    the filter is the one of any ratio below 1, at 4 it is the 2.0 filter stretched by two.  Nothing in table_error_bound's
    derivation (interpolation error, the window's jump at the edge, the table's rounding, each summed over the taps present) is
    particular to a ratio, so it covers 0.25 and 4.0 as it covers 0.5 and 2.0."""
    assert R.design(0.25) == R.design(0.5) and R.design(0.25)["half"] == ops.resample_ratio_design(0.25)[2]
    assert R.design(4.0)["half"] == ops.resample_ratio_design(4.0)[2] and R.design(4.0)["nu"] == 0.25
    for d in (0.25, 4.0):
        b = R.table_error_bound(d)
        assert np.isfinite(b) and 0.0 < b < 2.0 ** -16, (d, b)
    assert R.table_error_bound(0.25) == R.table_error_bound(0.5)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("d", [0.25, 4.0])
def test_resampler_at_the_ratio_limits_and_just_outside(dev, channels, d):
    x = _signal(2400, 8000, channels, 220 + channels)
    n_out = int(round(x.shape[1] / d))
    _assert_resampled(_resample(dev, x, d, n_out), x, d, n_out)
    xt = dev.t(torch.from_numpy(x))
    for out in (0.2499, 4.001):
        with pytest.raises(RuntimeError, match="ratio"):
            ops.resample_ratio(xt, out, 100)


@pytest.mark.parametrize("channels", [1, 2])
def test_resampler_with_nothing_to_write_or_nothing_to_read(dev, channels):
    """n_out = 0: an empty result, no launch.  n_in = 0 with n_out > 0: every output's tap range is empty (jlo > jhi), zeros."""
    d = _ratio(2)
    x = _signal(500, 8000, channels, 230)
    assert _resample(dev, x, d, 0).shape == (channels, 0)
    y = _resample(dev, np.zeros((channels, 0), np.float32), d, 300)
    assert y.shape == (channels, 300) and not _bits(y).any()
    _assert_resampled(y, np.zeros((channels, 0), np.float32), d, 300)
