"""TEST HELPER: Praat's autocorrelation pitch (`Sound: To Pitch (ac)...`, Boersma 1993) restated in plain numpy, float64 -- what
csrc/pitch_ac.hip is held to.  `dtype=np.float32` runs the frame stage (window, FFT, normalisation, interpolation, search)
in float32 through scipy.fft; that run only measures how far float32 arithmetic moves the result.  It is never taken from the kernel.

Where the paper leaves freedom, the choice is a named constant or a small function here, marked DECISION; the kernel follows."""
import numpy as np
import scipy.fft

PERIODS_PER_WINDOW = 3.0
MAX_CANDIDATES = 15
SILENCE_THRESHOLD = 0.03
OCTAVE_COST = 0.01
OCTAVE_JUMP_COST = 0.35
VOICED_UNVOICED_COST = 0.14
DEPTH_STRENGTH = 30          # sinc interpolation depth of a maximum's first strength
DEPTH_REFINE = 70            # ... of the refinement
DEPTH_REFINE_HIGH = 700      # ... for candidates above 0.3 sr
# DECISION (the maximiser's stopping rule): golden-section search of the bracket [k - 1, k + 1], a fixed 20 steps, the result is the
# middle of the last bracket (2 * 0.618^20 = 1.3e-4 samples wide).  Praat runs Brent's method to a tolerance of 1e-10.
GOLDEN_STEPS = 20
GOLDEN = 0.61803398874989484820


def geometry(n, sr=16000, time_step=0.01, pitch_floor=50.0):
    """dict of the framing, or ValueError for a signal shorter than one window."""
    dx = 1.0 / sr
    nw = int(np.floor(PERIODS_PER_WINDOW / pitch_floor / dx))
    half = nw // 2 - 1
    nw = 2 * half
    maxlag = min(nw // 3 + 2, nw)
    dur = n * dx
    if dur < PERIODS_PER_WINDOW / pitch_floor:
        raise ValueError("%d samples are shorter than one window" % n)
    n_frames = int(np.floor((dur - PERIODS_PER_WINDOW / pitch_floor) / time_step)) + 1
    nfft = 1
    while nfft < 1.5 * nw:
        nfft *= 2
    step = time_step * sr
    # DECISION (frame positions): everything in samples -- t1s = n / 2 - (n_frames - 1) step / 2; frame i starts at sample
    # floor(t1s + i step - 0.5) + 1 - nw / 2 (Praat's Sampled_xToLowIndex of the frame time, samples at (k + 0.5) dx)
    t1s = 0.5 * n - 0.5 * (n_frames - 1) * step
    return dict(nw=nw, nfft=nfft, maxlag=maxlag, brent=nw // 2, n_frames=n_frames, t1s=t1s, step=step)


def frame_start(g, i):
    return int(np.floor(g["t1s"] + i * g["step"] - 0.5)) + 1 - g["nw"] // 2


def frame_times(g, sr=16000):
    return (g["t1s"] + np.arange(g["n_frames"]) * g["step"]) / sr


def tables(g):
    nw, nfft = g["nw"], g["nfft"]
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, nw + 1, dtype=np.float64) / (nw + 1))
    wr = np.fft.irfft(np.abs(np.fft.rfft(w, nfft)) ** 2, nfft)
    return w, wr[:g["brent"] + 1] / wr[0]


def sinc_interp(r, brent, lag, depth, dtype=np.float64):
    """Hann-tapered sinc interpolation of the even sequence r[-brent .. brent] at `lag` (Praat's NUM_interpolate_sinc).
    DECISION (the taper at the array ends): the depth is cut to the samples the array has on either side; below one sample the nearest
    value is taken; Praat's linear / cubic special cases at depths 1 and 2 are not restated (no lag of the scan comes that close)."""
    T = dtype
    lag = T(lag)
    if lag >= brent or lag <= -brent:
        return T(r[brent])
    ml = int(np.floor(lag))
    phi = T(lag - T(ml))
    if phi == 0:
        return T(r[abs(ml)])
    depth = min(depth, ml + brent + 1, brent - ml)
    if depth < 1:
        return T(r[min(brent, abs(int(np.floor(lag + T(0.5)))))])
    t = np.arange(depth)
    sg = np.where(t & 1, -1.0, 1.0).astype(T)
    pi = T(np.pi)
    tt = t.astype(T)
    ul, ur = phi + tt, (T(1) - phi) + tt
    dl = sg * (T(0.5) * np.sin(pi * phi)) / (pi * ul) * (T(1) + np.cos(pi * (ul * (T(1) / (phi + T(depth))))))
    dr = sg * (T(0.5) * np.sin(pi * (T(1) - phi))) / (pi * ur) * (T(1) + np.cos(pi * (ur * (T(1) / (T(1) - phi + T(depth))))))
    rl = r[np.minimum(np.abs(ml - t), brent)].astype(T)
    rr = r[np.minimum(np.abs(ml + 1 + t), brent)].astype(T)
    return T(np.sum(rl * dl + rr * dr, dtype=T))


def refine(r, brent, k, depth, dtype=np.float64):
    """-> (lag, value) of the maximum of the interpolation inside [k - 1, k + 1]."""
    T = dtype
    g = T(GOLDEN)
    a, b = T(k - 1), T(k + 1)
    x1, x2 = b - g * (b - a), a + g * (b - a)
    f1, f2 = sinc_interp(r, brent, x1, depth, T), sinc_interp(r, brent, x2, depth, T)
    for _ in range(GOLDEN_STEPS):
        if f1 > f2:
            b, x2, f2 = x2, x1, f1
            x1 = b - g * (b - a)
            f1 = sinc_interp(r, brent, x1, depth, T)
        else:
            a, x1, f1 = x1, x2, f2
            x2 = a + g * (b - a)
            f2 = sinc_interp(r, brent, x2, depth, T)
    xm = T(0.5) * (a + b)
    return xm, sinc_interp(r, brent, xm, depth, T)


def candidates(x, sr=16000, time_step=0.01, pitch_floor=50.0, pitch_ceiling=1100.0, voicing_threshold=0.6,
               max_candidates=MAX_CANDIDATES, silence_threshold=SILENCE_THRESHOLD, octave_cost=OCTAVE_COST, dtype=np.float64):
    """-> (cand float32 (n_frames, max_candidates, 2), count int32 (n_frames,)): the table the device kernel writes."""
    T = dtype
    x = np.asarray(x, np.float32)   # the device reads the track as float32
    n = len(x)
    g = geometry(n, sr, time_step, pitch_floor)
    nw, nfft, brent, nf = g["nw"], g["nfft"], g["brent"], g["n_frames"]
    w64, wr64 = tables(g)
    w, wr = w64.astype(np.float32).astype(T), wr64.astype(np.float32).astype(T)
    gmean = np.float32(x.astype(np.float64).sum() / n)
    gpeak = np.abs(x - gmean).max()
    kmax = min(g["maxlag"], brent)
    cand = np.zeros((nf, max_candidates, 2), np.float32)
    count = np.zeros(nf, np.int32)
    vthr, sil, oc, fl, srT = T(voicing_threshold), T(silence_threshold), T(octave_cost), T(pitch_floor), T(sr)
    for i in range(nf):
        s0 = frame_start(g, i)
        seg = x[s0:s0 + nw].astype(T)
        assert len(seg) == nw
        seg = seg - T(seg.sum(dtype=T) / T(nw))
        lpeak = np.abs(seg).max()
        inten = lpeak / gpeak if gpeak > 0 else 0.0
        cand[i, 0] = (0.0, vthr + max(T(0), T(2) - T(inten) / (sil / (T(1) + vthr))))
        kept = []   # [k, f, strength]
        F = scipy.fft.rfft(seg * w, nfft)
        ac = scipy.fft.irfft((F.real * F.real + F.imag * F.imag).astype(T), nfft)
        assert ac.dtype == T
        if lpeak > 0 and ac[0] > 0:
            r = (ac[:brent + 1] / (ac[0] * wr)).astype(T)
            for k in range(2, kmax):
                if r[k] > T(0.5) * vthr and r[k] > r[k - 1] and r[k] >= r[k + 1]:
                    dr = T(0.5) * (r[k + 1] - r[k - 1])
                    d2r = T(2) * r[k] - r[k - 1] - r[k + 1]
                    lag = T(k) + dr / d2r
                    st = sinc_interp(r, brent, lag, DEPTH_STRENGTH, T)
                    if st > 1:
                        st = T(1) / st
                    f = srT / lag
                    if len(kept) < max_candidates - 1:
                        kept.append([k, f, st])
                    else:
                        ls = [c[2] - oc * np.log2(fl / c[1]) for c in kept]
                        weakest, place = T(2), -1
                        for c, v in enumerate(ls):
                            if v < weakest:
                                weakest, place = v, c
                        if st - oc * np.log2(fl / f) > weakest and place >= 0:
                            kept[place] = [k, f, st]
            for c, (k, f, st) in enumerate(kept):
                lag, val = refine(r, brent, k, DEPTH_REFINE_HIGH if f > T(0.3) * srT else DEPTH_REFINE, T)
                if val > 1:
                    val = T(1) / val
                cand[i, 1 + c] = (srT / lag, val)
        count[i] = 1 + len(kept)
    return cand, count


UNVOICED = -1.0e30


def _nodes(cand, count, pitch_ceiling, octave_cost):
    nf, K = cand.shape[:2]
    f = cand[:, :, 0].astype(np.float64)
    s = cand[:, :, 1].astype(np.float64)
    voiced = (f > 0) & (f < pitch_ceiling)
    lf = np.where(voiced, np.log2(np.where(voiced, f, 1.0)), UNVOICED)
    # DECISION: log2(ceiling / f) and log2(f1 / f2) are taken as differences of log2 f, one logarithm per candidate
    node = np.where(voiced, s - octave_cost * (np.log2(pitch_ceiling) - lf), s[:, :1])
    valid = np.arange(K)[None, :] < np.clip(count, 1, K)[:, None]
    return node, lf, voiced, valid


def _trans(lf1, v1, lf2, v2, ojc, vuc):
    """cost[i][j] of going from candidate i of one frame to candidate j of the next"""
    both = v1[:, None] & v2[None, :]
    mixed = v1[:, None] != v2[None, :]
    return np.where(both, ojc * np.abs(lf1[:, None] - lf2[None, :]), np.where(mixed, vuc, 0.0))


def path(cand, count, time_step=0.01, pitch_ceiling=1100.0, octave_cost=OCTAVE_COST, octave_jump_cost=OCTAVE_JUMP_COST,
         voiced_unvoiced_cost=VOICED_UNVOICED_COST, want_margins=False):
    """Praat's Pitch_pathFinder in float64 -> (f0 float64 (n_frames,), states) [, predecessor margin, frame margin].
    predecessor margin: the smallest nonzero gap between the best and the second-best predecessor over all valid nodes (inf if none;
    an exact tie is between states that carry the same value by construction -- two unvoiced candidates of a frame -- and index order
    settles it);
    frame margin[t]: the best path value through the chosen node minus the best through any other node of frame t.
    DECISION (selected_array for a chosen candidate at or above the ceiling): its frequency is written as it stands."""
    cand = np.asarray(cand, np.float32)
    nf, K = cand.shape[:2]
    c = 0.01 / time_step
    ojc, vuc = octave_jump_cost * c, voiced_unvoiced_cost * c
    node, lf, voiced, valid = _nodes(cand, count, pitch_ceiling, octave_cost)
    NEG = -np.inf
    delta = np.full((nf, K), NEG)
    psi = np.zeros((nf, K), np.int64)
    delta[0] = np.where(valid[0], 0.0 + node[0], NEG)
    pmargin = np.inf
    for t in range(1, nf):
        v = np.where(valid[t - 1][:, None], delta[t - 1][:, None] - _trans(lf[t - 1], voiced[t - 1], lf[t], voiced[t], ojc, vuc), NEG)
        bi = np.argmax(v, axis=0)          # first maximum: ties to the lowest index
        best = v[bi, np.arange(K)]
        psi[t] = bi
        delta[t] = np.where(valid[t], best + node[t], NEG)
        if want_margins:
            for j in np.nonzero(valid[t])[0]:
                col = np.sort(v[valid[t - 1], j])
                if len(col) > 1 and col[-1] > col[-2]:
                    pmargin = min(pmargin, col[-1] - col[-2])
    states = np.zeros(nf, np.int64)
    states[-1] = int(np.argmax(delta[-1]))
    for t in range(nf - 1, 0, -1):
        states[t - 1] = psi[t, states[t]]
    f0 = cand[np.arange(nf), states, 0].astype(np.float64)
    if not want_margins:
        return f0, states
    # best continuation after node j of frame t (without its own value)
    beta = np.zeros((nf, K))
    for t in range(nf - 2, -1, -1):
        v = np.where(valid[t + 1][None, :], beta[t + 1][None, :] + node[t + 1][None, :] -
                     _trans(lf[t], voiced[t], lf[t + 1], voiced[t + 1], ojc, vuc), NEG)
        beta[t] = v.max(axis=1)
    through = np.where(valid, delta + beta, NEG)
    fm = np.full(nf, np.inf)
    for t in range(nf):
        others = np.delete(through[t], states[t])
        others = others[np.isfinite(others)]
        if len(others):
            fm[t] = through[t, states[t]] - others.max()
    return f0, states, pmargin, fm


def pitch_ac(x, sr=16000, time_step=0.01, pitch_floor=50.0, pitch_ceiling=1100.0, voicing_threshold=0.6, dtype=np.float64, full=False):
    cand, count = candidates(x, sr, time_step, pitch_floor, pitch_ceiling, voicing_threshold, dtype=dtype)
    if full:
        return (cand, count) + path(cand, count, time_step, pitch_ceiling, want_margins=True)
    return path(cand, count, time_step, pitch_ceiling)[0]
