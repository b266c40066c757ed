"""Float64 restatement of the pitch-shift definition that tests/test_cover_pitch.py holds csrc/pitch.hip against: the
WSOLA chain with sox's `tempo` music defaults, and the Kaiser-windowed-sinc resampler.  Written from the definition, not from the
kernels: plain numpy, every sum in float64."""
import math

import numpy as np

U = 2.0 ** -24                      # float32 unit roundoff
ATT_DB, PASS, PHASES = 100.0, 0.90, 1024


def _round(v):
    return int(math.floor(v + 0.5))


def geometry(sr, tempo, n):
    seg, search = _round(sr * 0.082), _round(sr * 0.01468)
    ovl = max(_round(sr * 0.012), 16) & ~7
    adv = seg - ovl
    skip, n_out = _round(tempo * adv), _round(n / tempo)
    return dict(seg=seg, search=search, ovl=ovl, adv=adv, skip=skip, n_out=n_out, steps=-(-n_out // adv))


def wsola(x, sr, tempo, offsets=None):
    """x: (C, n).  offsets None: the chain chooses its own argmin (lowest offset on ties); otherwise it walks along `offsets`.
    Returns dict(y (C, n_out) float64, offsets, chosen / best (the float64 cost at the offset taken / the minimum, per step),
    argmin, copied (n_out,) bool: frames that are plain copies of input, scale (C, n_out): max(|o|, |x|) of a cross-faded sample)."""
    x = np.asarray(x, np.float64)
    C, n = x.shape
    g = geometry(sr, tempo, n)
    seg, search, ovl, adv, skip, n_out, steps = (g[k] for k in ("seg", "search", "ovl", "adv", "skip", "n_out", "steps"))
    xp = np.zeros((C, max(n, steps * skip) + seg + search + ovl))
    xp[:, :n] = x
    y = np.zeros((C, steps * adv))
    copied = np.ones(steps * adv, bool)
    scale = np.zeros((C, steps * adv))
    offs = np.zeros(steps, np.int64)
    chosen, best, argmin = np.zeros(steps), np.zeros(steps), np.zeros(steps, np.int64)
    w = np.arange(ovl) / ovl
    if steps:
        y[:, :adv] = xp[:, :adv]
    prev = adv                                     # where o_k starts in the input
    for k in range(1, steps):
        p = k * skip
        o = xp[:, prev:prev + ovl]
        sw = np.lib.stride_tricks.sliding_window_view(xp[:, p:p + search + ovl - 1], ovl, axis=1)     # (C, search, ovl)
        cost = ((sw - o[:, None, :]) ** 2).sum(axis=(0, 2))
        argmin[k] = int(np.argmin(cost))
        i = int(offsets[k]) if offsets is not None else int(argmin[k])
        offs[k], chosen[k], best[k] = i, cost[i], cost[argmin[k]]
        xin = xp[:, p + i:p + i + adv]
        b = k * adv
        y[:, b:b + ovl] = o * (1.0 - w) + xin[:, :ovl] * w
        y[:, b + ovl:b + adv] = xin[:, ovl:]
        copied[b:b + ovl] = False
        scale[:, b:b + ovl] = np.maximum(np.abs(o), np.abs(xin[:, :ovl]))
        prev = p + i + adv
    return dict(y=y[:, :n_out], offsets=offs, chosen=chosen, best=best, argmin=argmin, copied=copied[:n_out], scale=scale[:, :n_out],
                geom=g)


def tie_eps(ovl, channels):
    """Both compared costs are float32 sums of ovl * C non-negative terms, each a rounded square of a rounded difference: relative
    error at most (ovl C + 3) u each."""
    return 2.0 * (ovl * channels + 3) * U


# ---- resampler ---------------------------------------------------------------------------------------------------------------------
def design(ratio):
    nu = min(1.0, 1.0 / ratio)
    beta = 0.1102 * (ATT_DB - 8.7)
    width = (1.0 - PASS) * nu / 2.0
    half = int(math.ceil((ATT_DB - 7.95) / (2.285 * 2.0 * math.pi * width) / 2.0))
    return dict(nu=nu, fc=(1.0 + PASS) / 2.0 * nu / 2.0, beta=beta, half=half)


def h(tau, ratio):
    d = design(ratio)
    tau = np.asarray(tau, np.float64)
    u = 1.0 - (tau / d["half"]) ** 2
    w = np.where(u > 0.0, np.i0(d["beta"] * np.sqrt(np.maximum(u, 0.0))) / np.i0(d["beta"]), 0.0)
    return 2.0 * d["fc"] * np.sinc(2.0 * d["fc"] * tau) * w


def resample(x, ratio, n_out, chunk=8192):
    """y[c][m] = sum_t h(m ratio - t) x[c][t] with the exact filter, float64."""
    x = np.asarray(x, np.float64)
    C, n_in = x.shape
    half = design(ratio)["half"]
    xp = np.zeros((C, n_in + 2 * half + 2))
    y = np.zeros((C, n_out))
    j = np.arange(-half, half + 1)
    for m0 in range(0, n_out, chunk):
        m = np.arange(m0, min(n_out, m0 + chunk), dtype=np.float64)
        pos = m * np.float64(ratio)
        t0 = np.floor(pos)
        hv = h((pos - t0)[:, None] + j[None, :], ratio)                    # (m, taps)
        t = t0.astype(np.int64)[:, None] - j[None, :]
        ok = (t >= 0) & (t < n_in)
        xv = x[:, np.clip(t, 0, max(n_in - 1, 0))] * ok[None] if n_in else np.zeros((C,) + t.shape)
        y[:, m0:m0 + len(m)] = (xv * hv[None]).sum(-1)
    return y


def table_error_bound(ratio):
    """What reading the filter from the float32 table with linear interpolation between PHASES rows per sample can add to one output
    sample of a signal bounded by 1: the interpolation error h'' / (8 P^2) summed over the taps, the jump of the Kaiser window at the
    filter's edge (one tap is interpolated across it), and the table's float32 rounding u sum |h|.  The sums are maxima over a grid
    of 256 phases, taken 10 % larger to cover the phases between the grid points."""
    half = design(ratio)["half"]
    phi = np.arange(256)[:, None] / 256.0
    tau = phi + np.arange(-half, half + 1)[None, :]
    e = 1e-3
    h2 = (h(tau + e, ratio) - 2.0 * h(tau, ratio) + h(tau - e, ratio)) / e ** 2
    H1 = 1.1 * np.abs(h(tau, ratio)).sum(1).max()
    H2 = 1.1 * np.abs(h2).sum(1).max()
    edge = abs(float(h(half - 1e-9, ratio)))
    return H2 / (8.0 * PHASES ** 2) + edge + U * H1


def to_int16(y):
    return np.rint(np.clip(y, -1.0, 1.0) * 32767.0).astype(np.int16)


def stems(seconds, sr, channels, seed):
    """A seeded music-like signal in [-1, 1]: a few tones with vibrato under a slow envelope, plus noise; channels differ."""
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    t = np.arange(n) / sr
    out = []
    for c in range(channels):
        s = 0.02 * rng.standard_normal(n)
        for f0, a in ((220.0 + 30 * c, 0.25), (331.0, 0.15), (523.0 + 11 * c, 0.1)):
            s += a * np.sin(2 * np.pi * f0 * t + 2.0 * np.sin(2 * np.pi * (4.0 + c) * t) + rng.uniform(0, 6))
        out.append(s * (0.4 + 0.6 * np.sin(2 * np.pi * 0.7 * t + c) ** 2))
    return np.stack(out).astype(np.float32)
