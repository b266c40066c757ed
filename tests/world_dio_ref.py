"""f0_method "dio" restated in numpy: WORLD's DIO (Morise, Kawahara, Katayose 2009; Morise et al. 2016), StoneMask and the 3-point median,
as the reference calls them (src/vc_infer_pipeline.py:300-309).  The float64 run is the authority csrc/world_dio.hip is held to
(DESIGN 10); `dtype=np.float32` runs the arithmetic of the filters, the crossings, the candidates and StoneMask's sums in float32 (same
operands, another rounding) and gives the tolerances of tests/test_world_dio.py.  Every place where the description leaves freedom is
marked DECISION.  No WORLD source was at hand: the steps are restated from the papers and the library's documented behaviour, and
tests/test_world_dio.py::test_pyworld_pin holds them to pyworld where it is installed."""
import numpy as np

EPS = 1e-12              # the safeguard added to denominators
BIG = 100000.0           # score of a rejected candidate before the division by (0 + EPS)
CUTOFF = 50.0            # low-cut
NUTTALL = (0.355768, -0.487396, 0.144232, -0.012604)
STONEMASK_FLOOR = 40.0


def mround(v):
    """round half away from zero"""
    return int(v + 0.5) if v > 0 else int(v - 0.5)


def geometry(n, fs=16000, frame_period=10.0, f0_floor=50.0, f0_ceil=1100.0, channels_in_octave=2.0):
    n_bands = 1 + int(np.log2(f0_ceil / f0_floor) * channels_in_octave)
    boundary = f0_floor * 2.0 ** ((np.arange(n_bands) + 1.0) / channels_in_octave)
    cut = mround(fs / CUTOFF)
    return {"n_frames": int(1000.0 * n / fs / frame_period) + 1, "n_bands": n_bands, "boundary": boundary,
            "half": [mround(fs / b / 2.0) for b in boundary], "lowcut": 2 * cut + 1,
            "vrm": 2 * int(0.5 + 1000.0 / frame_period / f0_floor) + 1}


def lowcut_taps(N):
    """1 at the centre minus the Hanning low-pass normalised to sum 1; N odd, the delay (N - 1) / 2 is taken out by the caller"""
    h = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, N + 1, dtype=np.float64) / (N + 1))
    h = -h / h.sum()
    h[(N - 1) // 2] += 1.0
    return h


def nuttall_taps(h):
    """DECISION: the window of length 4 h is sampled at i / (4 h - 1), i = 0 .. 4 h - 1 (both ends included, not normalised); the delay
    taken out is 2 h, half a sample more than the window's centre -- as the library does."""
    t = np.arange(4 * h, dtype=np.float64) / (4 * h - 1.0)
    return sum(c * np.cos(2.0 * np.pi * k * t) for k, c in enumerate(NUTTALL))


def _conv(a, b, T):
    if T == np.float64:
        from scipy.signal import fftconvolve
        return fftconvolve(a, b)                    # zero-padded FFT = linear convolution
    return np.convolve(a.astype(T), b.astype(T))    # the direct sum in T


def prefilter(x, g, T=np.float64):
    """-> the low-cut signal at the positions -c .. n + c - 1 (c = (N - 1) / 2): the whole linear convolution.
    DECISION: the mean is the plain mean of the n samples.  DECISION: nothing is cut between the low-cut and the band filter -- a band
    sees the low-cut signal's tails outside [0, n), as a product of spectra does."""
    x = np.asarray(x, T)
    y = x - T(np.mean(x.astype(np.float64))) if len(x) else x
    return _conv(y, lowcut_taps(g["lowcut"]), T).astype(T)


def band_signal(lc, g, band, n, T=np.float64):
    """the band's low-passed signal at 0 .. n - 1"""
    h = g["half"][band]
    full = _conv(lc, nuttall_taps(h), T)
    off = 2 * h + (g["lowcut"] - 1) // 2
    return full[off:off + n].astype(T)


def crossings(u):
    """negative-going zero crossings of u: between u[i] > 0 and u[i + 1] <= 0 -> (ip int64, frac), position ip + frac.
    DECISION: ip = i + 1, the ONE-based index of sample i, as the library's MATLAB heritage has it (all locations sit one sample late;
    frame times are zero-based).  frac = u[i] / (u[i] - u[i + 1]) in (0, 1]."""
    if len(u) < 2:
        return np.zeros(0, np.int64), np.zeros(0, u.dtype)
    i = np.nonzero((u[:-1] > 0) & (u[1:] <= 0))[0]
    a, b = u[i], u[i + 1]
    return (i + 1).astype(np.int64), (a / (a - b)).astype(u.dtype)


def four_kinds(s):
    """the four signals whose negative-going crossings are taken: s, -s, the forward difference (peaks) and its negative (dips)"""
    d = s[1:] - s[:-1]
    return s, -s, d, -d


def interp_kind(ip, frac, tpos, fs, T):
    """interval f0 between successive crossings, interpolated linearly at the frame positions tpos (samples, float64); outside the first
    and the last interval the end segment's line goes on.  The integer parts are subtracted as integers (an absolute position
    in float32 loses the fraction on a long track).  DECISION: the bracket is looked for in samples, not seconds."""
    dist = (ip[1:] - ip[:-1]).astype(T) + (frac[1:] - frac[:-1])
    f = T(fs) / dist
    loc = ((ip[1:] + ip[:-1]).astype(np.float64) + frac[1:].astype(np.float64) + frac[:-1].astype(np.float64)) / 2.0
    j = np.clip(np.searchsorted(loc, tpos, side="right") - 1, 0, len(loc) - 2)
    s = ((tpos - loc[j]) / (loc[j + 1] - loc[j])).astype(T)
    return f[j] + s * (f[j + 1] - f[j])


def candidates(x, fs=16000, frame_period=10.0, f0_floor=50.0, f0_ceil=1100.0, channels_in_octave=2.0, dtype=np.float64, full=False):
    """-> cand, score (n_bands, n_frames) float32 and counts (n_bands, 4) of crossings [, raw candidate, raw score, range distance]"""
    T = dtype
    n = len(x)
    g = geometry(n, fs, frame_period, f0_floor, f0_ceil, channels_in_octave)
    nf, nb = g["n_frames"], g["n_bands"]
    tpos = np.arange(nf, dtype=np.float64) * frame_period / 1000.0 * fs
    cand = np.zeros((nb, nf), np.float32)
    score = np.full((nb, nf), np.float32(BIG / EPS), np.float32)
    counts = np.zeros((nb, 4), np.int64)
    raw_c = np.full((nb, nf), np.nan)
    raw_s = np.full((nb, nf), np.nan)
    rdist = np.full((nb, nf), np.inf)
    lc = prefilter(x, g, T) if n else None
    for b in range(nb):
        if n == 0:
            continue
        s = band_signal(lc, g, b, n, T)
        ev = [crossings(u) for u in four_kinds(s)]
        counts[b] = [len(e[0]) for e in ev]
        if min(counts[b]) - 1 <= 2:               # a set with <= 2 intervals: the band is unvoiced throughout
            continue
        y = [interp_kind(ip, fr, tpos, fs, T) for ip, fr in ev]
        with np.errstate(all="ignore"):
            c = (((y[0] + y[1]) + y[2]) + y[3]) / T(4)
            sd = np.sqrt(((((y[0] - c) ** 2 + (y[1] - c) ** 2) + (y[2] - c) ** 2) + (y[3] - c) ** 2) / T(3))
            B = g["boundary"][b]
            bad = (c > T(B)) | (c < T(B / 2.0)) | (c > T(f0_ceil)) | (c < T(f0_floor)) | ~np.isfinite(c)
            sc = sd / (c + T(EPS))
            cand[b] = np.where(bad, 0, c)
            score[b] = np.where(bad, np.float32(BIG / EPS), sc)
            raw_c[b], raw_s[b] = c, sc
            c64 = c.astype(np.float64)
            rdist[b] = np.min(np.abs(np.stack([c64 / B, c64 / (B / 2.0), c64 / f0_ceil, c64 / f0_floor]) - 1.0), axis=0)
    if full:
        return cand, score, counts, raw_c, raw_s, rdist
    return cand, score, counts


def _select(ref, col):
    """the candidate of this frame nearest `ref` (first minimum), its error and the next distinct value's error"""
    err = np.abs(ref - col)
    k = int(np.argmin(err))
    other = err[col != col[k]]
    return col[k], err[k], (other.min() if len(other) else np.inf)


def repair(cand, score, frame_period=10.0, f0_floor=50.0, allowed_range=0.1, sel_margin=None, want_margins=False, extra=None):
    """best contour and the four repair steps on (n_bands, n_frames) tables, float64 arithmetic on the float32 entries.
    -> f0 float64 (n_frames,) [, margin per frame].
    DECISION (step 3): the forward extension from the end of section i runs up to the END of section i + 1 (the last frame after the
    last section), writing over that section while it finds candidates, as the library does; step 4 mirrors it down to the START of
    section i - 1 (frame 1 before the first).  Sections are those of step 2 in both.
    DECISION: n_frames <= vrm gives zeros."""
    cand = np.asarray(cand, np.float32).astype(np.float64)
    score = np.asarray(score, np.float32).astype(np.float64)
    nb, L = cand.shape
    vrm = 2 * int(0.5 + 1000.0 / frame_period / f0_floor) + 1
    big = np.inf
    mg = np.full(L, big) if sel_margin is None else np.array(sel_margin, np.float64)
    if L <= vrm:
        f0 = np.zeros(L)
        return (f0, np.full(L, big)) if want_margins else f0
    bi = np.argmin(score, axis=0)                    # first minimum: ties to the lowest band
    best = cand[bi, np.arange(L)]
    if sel_margin is None and want_margins:          # tables alone: the gap between the best and the second-best score
        for i in range(L):
            o = np.delete(score[:, i], bi[i])
            o = o[cand[np.arange(nb) != bi[i], i] != best[i]]
            if len(o):
                mg[i] = min(mg[i], o.min() - score[bi[i], i])
    # step 1
    base = best.copy()
    base[:vrm] = 0
    base[max(0, L - vrm):] = 0
    f1 = np.zeros(L)
    m1 = mg.copy()
    for i in range(vrm, L):
        if base[i] != 0:
            jump = abs((base[i] - base[i - 1]) / (EPS + base[i]))
            f1[i] = base[i] if jump < allowed_range else 0.0
            m1[i] = min(mg[i], mg[i - 1], abs(jump - allowed_range))
    m1[:vrm] = big                                   # zeroed whatever was found
    m1[max(0, L - vrm):] = big
    # step 2
    c = (vrm - 1) // 2
    f2 = f1.copy()
    m2 = m1.copy()
    for i in range(c, L - c):
        w = np.arange(i - c, i + c + 1)
        z = w[f1[w] == 0]
        if len(z):
            f2[i] = 0.0
            m2[i] = m1[z].max()                      # every unvoiced frame of the window would have to turn
        else:
            m2[i] = m1[w].min()
    ends = [i - 1 for i in range(1, L) if f2[i] == 0 and f2[i - 1] != 0]
    starts = [i for i in range(1, L) if f2[i - 1] == 0 and f2[i] != 0]

    def extend(f, m, frm, limit, step):
        mu = min(m[frm], m[frm - step])
        j = frm
        while j != limit:
            t = j + step
            ref = (3.0 * f[j] - f[j - step]) / 2.0
            v, e1, e2 = _select(ref, cand[:, t])
            with np.errstate(all="ignore"):
                rel = abs(1.0 - v / ref)
                mu = min(mu, (e2 - e1) / abs(ref), abs(rel - allowed_range))
            if extra is not None:
                raw_c, rdist = extra
                k = int(np.argmin(np.abs(ref - cand[:, t])))
                if v != 0:
                    mu = min(mu, rdist[k, t])
                nearer = np.abs(ref - raw_c[:, t]) < e1
                nearer &= cand[:, t] == 0
                if nearer.any():
                    mu = min(mu, rdist[nearer, t].min())
            if not rel <= allowed_range:
                v = 0.0
            f[t] = v
            m[t] = mu
            if v == 0:
                k = t
                while k != limit:                    # the frames a longer extension would have reached
                    k += step
                    m[k] = min(m[k], mu)
                break
            j = t

    f3, m3 = f2.copy(), m2.copy()
    for i, e in enumerate(ends):
        extend(f3, m3, e, L - 1 if i == len(ends) - 1 else ends[i + 1], 1)
    f4, m4 = f3.copy(), m3.copy()
    for i in range(len(starts) - 1, -1, -1):
        extend(f4, m4, starts[i], 1 if i == 0 else starts[i - 1], -1)
    return (f4, m4) if want_margins else f4


def dio(x, fs=16000, frame_period=10.0, f0_floor=50.0, f0_ceil=1100.0, channels_in_octave=2.0, allowed_range=0.1, dtype=np.float64,
        full=False):
    """-> f0 float64 (n_frames,) [, margin, cand, score, counts]"""
    cand, score, counts, raw_c, raw_s, rdist = candidates(x, fs, frame_period, f0_floor, f0_ceil, channels_in_octave, dtype, full=True)
    if not full:
        return repair(cand, score, frame_period, f0_floor, allowed_range)
    nb, L = cand.shape
    sel = np.full(L, np.inf)
    s64 = score.astype(np.float64)
    bi = np.argmin(s64, axis=0)
    for i in range(L):
        b0 = bi[i]
        sb = s64[b0, i]
        for b in range(nb):
            if not np.isfinite(rdist[b, i]):
                continue                             # no candidate was computed: no comparison
            if cand[b, i] != 0:
                sel[i] = min(sel[i], rdist[b, i] if b == b0 else s64[b, i] - sb)
            elif raw_s[b, i] < sb or not np.isfinite(raw_s[b, i]):
                sel[i] = min(sel[i], rdist[b, i])    # a rejected band that would win if it were accepted
    f0, m = repair(cand, score, frame_period, f0_floor, allowed_range, sel_margin=sel, want_margins=True, extra=(raw_c, rdist))
    return f0, np.minimum(m, 1.0), cand, score, counts


# ---- StoneMask ------------------------------------------------------------------------------------------------------------------------
def stonemask_geometry(f0, fs):
    half = int(1.5 * fs / f0 + 1.0)
    return half, 2 ** (2 + int(np.log2(2.0 * half + 1.0)))


def _fix_f0(P, Q, fft_size, fs, f0, nh, T):
    num = den = T(0)
    for k in range(1, nh + 1):
        b = mround(f0 * fft_size / fs * k)
        p = P[b]
        inst = T(0) if p == 0 else T(b * fs / fft_size) + Q[b] / p * T(fs / 2.0 / np.pi)
        a = np.sqrt(p)
        num += a * inst
        den += a * T(k)
    return float(num) / (float(den) + EPS)


def stonemask_frame(x, fs, t, f0, T=np.float64):
    """-> (refined f0, margin).  x float64 or float32 samples, t the frame time in seconds.
    DECISION: the first sample index is round((t - half / fs) fs + 0.001), the others follow one by one; these indices are ONE-based:
    sample index - 1 is read (clamped to the signal) and the windows are evaluated at (index - 1) / fs - t.
    DECISION: an initial f0 <= 40 Hz or above fs / 12 gives 0.  The bins of the zero-padded FFT are direct sums."""
    if not (f0 > STONEMASK_FLOOR and f0 <= fs / 12.0):
        return 0.0, np.inf
    n = len(x)
    half, fft_size = stonemask_geometry(f0, fs)
    W = 2 * half + 1
    idx = mround((t - half / fs) * fs + 0.001) + np.arange(W)
    tm = ((idx - 1.0) / fs - t) / (W / fs)
    win = (0.42 + 0.5 * np.cos(2.0 * np.pi * tm) + 0.08 * np.cos(4.0 * np.pi * tm)).astype(T)
    dwin = np.zeros(W, T)
    dwin[0] = -win[1] / T(2)
    dwin[1:-1] = -(win[2:] - win[:-2]) / T(2)
    dwin[-1] = win[-2] / T(2)
    seg = np.asarray(x, T)[np.clip(idx - 1, 0, n - 1)]
    P, Q = {}, {}

    def bins(f, nh):
        for k in range(1, nh + 1):
            b = mround(f * fft_size / fs * k)
            if b not in P:
                ph = 2.0 * np.pi * ((b * np.arange(W)) % fft_size) / fft_size
                cs, sn = np.cos(ph).astype(T), np.sin(ph).astype(T)
                re, im = np.sum(seg * win * cs), -np.sum(seg * win * sn)
                dre, dim = np.sum(seg * dwin * cs), -np.sum(seg * dwin * sn)
                P[b] = re * re + im * im
                Q[b] = re * dim - im * dre

    bins(f0, 2)
    tent = _fix_f0(P, Q, fft_size, fs, f0, 2, T)
    margin = min(abs(tent / f0), abs(tent / (2.0 * f0) - 1.0))
    mean = 0.0
    if tent > 0.0 and tent <= 2.0 * f0:
        nh = min(int(fs / 2.0 / tent), 6)
        bins(tent, nh)
        mean = _fix_f0(P, Q, fft_size, fs, tent, nh, T)
    margin = min(margin, abs(abs(mean - f0) / f0 - 0.2))
    if mean <= 0.0 or mean > fs / 12.0 or abs(mean - f0) > 0.2 * f0:
        mean = f0
    return mean, margin


def stonemask(x, f0, fs=16000, frame_period=10.0, dtype=np.float64, want_margins=False):
    out = np.zeros(len(f0))
    mg = np.full(len(f0), np.inf)
    for i, f in enumerate(np.asarray(f0, np.float64)):
        if f > 0:
            out[i], mg[i] = stonemask_frame(x, fs, i * frame_period / 1000.0, f, dtype)
    return (out, mg) if want_margins else out


def medfilt3(f0):
    """scipy.signal.medfilt(f0, 3): zeros beyond both ends"""
    p = np.concatenate([[0.0], np.asarray(f0, np.float64), [0.0]])
    return np.median(np.stack([p[:-2], p[1:-1], p[2:]]), axis=0) if len(f0) else np.zeros(0)


def dio_stonemask_median(x, fs=16000, frame_period=10.0, f0_floor=50.0, f0_ceil=1100.0, dtype=np.float64, full=False):
    """the reference's whole `dio` branch -> f0 [, margin]: a frame's margin is the smallest of its own and its two neighbours'
    (the median reads all three)"""
    f0, m, _, _, _ = dio(x, fs, frame_period, f0_floor, f0_ceil, dtype=dtype, full=True)
    r, ms = stonemask(np.asarray(x, np.float64), f0, fs, frame_period, dtype, want_margins=True)
    out = medfilt3(r)
    if not full:
        return out
    m = np.minimum(np.minimum(m, ms), 1.0)
    p = np.concatenate([[1.0], m, [1.0]])
    return out, np.minimum(np.minimum(p[:-2], p[1:-1]), p[2:])
