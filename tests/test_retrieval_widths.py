"""Feature retrieval at the widths it ships at.  ivf_scan8 walks a vector as `for (c = lane * 4; c < dim; c += 256)`, index_mix and
row_sqnorm as `c += 64`, the blend as `c = threadIdx.x; c += 256` (csrc/dsp.hip); tests/test_retrieval.py stops at dim 64, where
none of these loops runs a second pass and most lanes idle.  Here: dim 4 (the minimum), 256 (one full pass, every lane live: v1
voices), 260 (a ragged second pass) and 768 (three passes: v2 voices), against oracle/faiss_ivf.py (float64).

Bars.  IVF distance: ivf_scan8 sums `dim` non-negative fp32 terms (q_c - x_c)^2 in some order.  Each term carries one rounded
subtraction (squared: 2 u) and one rounded square (u), u = 2^-24; any order of the dim - 1 additions adds at most (dim - 1) u to
first order; together (dim + 2) u, taken as rtol = (dim + 3) * 2^-24 against the float64 distance, no absolute term.  row_sqnorm
has no subtraction: (dim + 1) * 2^-24.  Exhaustive search and blend: test_retrieval.py's, the absolute part scaled with |x|^2."""
import numpy as np
import pytest
import torch

from aicovergen_amd import ops, retrieval
from oracle import faiss_ivf

DIMS = [4, 256, 260, 768]
NLIST, SMALL, EMPTY = 6, 5, 4
U = 2.0 ** -24


def _data(dim):
    """test_retrieval._clustered's construction: vectors around NLIST centres, each assigned to its nearest centroid and stored list
    by list; list SMALL keeps 3 vectors (fewer than k), list EMPTY none.  40 queries near stored vectors; query 0 sits on the small
    list's centroid, query 1 EQUALS a stored vector, query 2 sits on the empty list's centroid."""
    rng = np.random.default_rng(100 + dim)
    n = 440
    cent = rng.standard_normal((NLIST, dim)).astype(np.float32) * 2.0
    x = (cent[rng.integers(0, NLIST, n)] + rng.standard_normal((n, dim)).astype(np.float32) * 0.9).astype(np.float32)
    assign = ((x[:, None, :].astype(np.float64) - cent[None].astype(np.float64)) ** 2).sum(-1).argmin(1)
    keep = np.ones(n, bool)
    keep[np.nonzero(assign == SMALL)[0][3:]] = False
    keep[assign == EMPTY] = False
    x, assign = x[keep], assign[keep]
    ids_by_list = [np.nonzero(assign == l)[0].astype(np.int64) for l in range(NLIST)]
    sizes = np.array([len(i) for i in ids_by_list], np.int64)
    ids = np.concatenate(ids_by_list)
    t = 40
    feats = (x[rng.integers(0, len(x), t)] + rng.standard_normal((t, dim)).astype(np.float32) * 0.7).astype(np.float32)
    feats[0] = cent[SMALL] + 0.01
    feats[1] = x[17]
    feats[2] = cent[EMPTY]
    return cent, sizes, ids, x[ids], x, feats


def _candidates(feats, cent, sizes, stored, nprobe):
    """Per query: float64 distances of every vector in its probed lists, ascending (for the 9th candidate), and the float64 gap
    between the last probed centroid and the first one left out."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    q, c, v = feats.astype(np.float64), cent.astype(np.float64), stored.astype(np.float64)
    out, gaps = [], []
    for t in range(len(q)):
        cd = ((c - q[t]) ** 2).sum(1)
        order = np.argsort(cd, kind="stable")
        gaps.append(cd[order[nprobe]] - cd[order[nprobe - 1]])
        rows = np.concatenate([np.arange(off[l], off[l + 1]) for l in order[:nprobe]])
        out.append(np.sort(((v[rows] - q[t]) ** 2).sum(1)))
    return out, np.array(gaps)


def _both_sides(clear):
    """clear[r, k]: rank k is clear of rank k + 1.  A rank is firm when it is clear of BOTH neighbours: a near-tie of ranks k, k + 1
    may swap them, which moves rank k + 1 as well although ITS gap to rank k + 2 is wide."""
    firm = clear.copy()
    firm[:, 1:] &= clear[:, :-1]
    return firm


def _firm(D, found, ninth, tol):
    """Ranks whose gap to the next candidate (and from the previous one) exceeds the distance tolerance of both ends (2 tol x the
    farther one)."""
    nxt = np.concatenate([D[:, 1:], ninth[:, None]], axis=1)
    with np.errstate(invalid="ignore"):
        return found & _both_sides(~np.isfinite(nxt) | (nxt - D > 2 * tol * nxt))


def _blend_want(feats, by_label, D, I, rate):
    """faiss_ivf.mix, with the two rows the reference turns into NaN stated as index_mix_kernel documents them: a zero distance
    takes the whole weight (shared among the zero-distance rows), no neighbour at all leaves the frame as it is."""
    with np.errstate(invalid="ignore", divide="ignore"):
        want = faiss_ivf.mix(feats, by_label, D, I, rate)
    f = feats.astype(np.float64)
    for r in range(len(f)):
        zero = (D[r] == 0) & (I[r] >= 0)
        if zero.any():
            want[r] = rate * by_label[I[r][zero]].astype(np.float64).mean(0) + (1 - rate) * f[r]
        elif not (I[r] >= 0).any():
            want[r] = f[r]
    assert np.isfinite(want).all()
    return want


@pytest.mark.parametrize("nprobe", [1, 3])
@pytest.mark.parametrize("dim", DIMS)
def test_ivf_search_and_blend_at_width(dev, dim, nprobe):
    cent, sizes, ids, stored, by_label, feats = _data(dim)
    assert 280 <= len(stored) <= 320 and sizes[SMALL] == 3 and sizes[EMPTY] == 0
    rtol = (dim + 3) * U
    D, I = faiss_ivf.ivf_search(feats, cent, sizes, stored, ids, nprobe)
    found = I >= 0
    cand, coarse_gap = _candidates(feats, cent, sizes, stored, nprobe)
    # conditions on the inputs (CPU only) ------------------------------------------------------------------------------------------
    # the coarse quantizer ranks centroids by the fp32 GEMM expansion: the probed set must not hang on its noise
    norm = float((by_label.astype(np.float64) ** 2).sum(1).max())
    assert (coarse_gap > 1e-3 * norm / 64).all()
    # one component dropped or doubled moves a distance by its share (q_c - x_c)^2 / d: 1 / dim on average, and for the typical
    # component well above the bar
    pairs = [(r, k) for r in range(len(feats)) for k in range(8) if found[r, k] and D[r, k] > 0]
    share = np.stack([(feats[r].astype(np.float64) - by_label[I[r, k]].astype(np.float64)) ** 2 / D[r, k] for r, k in pairs])
    assert abs(share.mean() * dim - 1) < 1e-9 and 1.0 / dim > 25 * rtol and np.median(share) > 10 * rtol
    ninth = np.array([c[8] if len(c) > 8 else np.inf for c in cand])
    firm = _firm(D, found, ninth, rtol)
    assert firm.sum() >= 0.95 * found.sum()
    assert D[1, 0] == 0 and I[1, 0] == 17
    if nprobe == 1:
        assert (I[0, 3:] == -1).all() and (I[0, :3] >= 0).all() and (I[2] == -1).all()
    # the device ------------------------------------------------------------------------------------------------------------------
    idx = retrieval.FeatureIndex(stored, dev.device, lists=(cent, sizes, ids, nprobe), exact=False)
    assert idx.ivf and idx.nprobe == nprobe and idx.dim == dim
    d, lab = idx.search(dev.t(torch.from_numpy(feats)))
    d, lab = d.cpu().numpy().astype(np.float64), lab.cpu().numpy()
    assert np.array_equal(found, lab >= 0) and np.isinf(d[~found]).all()
    err = np.abs(d[found] - D[found]) / np.maximum(D[found], 1e-300)
    print("dim %d nprobe %d: worst distance error %.3g (bar %.3g), firm %d of %d" % (dim, nprobe, err.max(), rtol, firm.sum(), found.sum()))
    assert (np.abs(d[found] - D[found]) <= rtol * D[found]).all()
    assert (lab[firm] == I[firm]).all()
    f = dev.t(torch.from_numpy(feats.copy()))
    mixed = idx.mix_(f, 0.6).cpu().numpy()
    want = _blend_want(feats, by_label, D, I, 0.6)
    assert np.abs(mixed - want).max() < 2e-5 * np.abs(want).max()
    assert np.allclose(mixed[1], feats[1], rtol=3e-7, atol=0)                 # the duplicate: rate x itself + (1 - rate) x itself, two roundings
    if nprobe == 1:
        assert np.array_equal(mixed[2], feats[2])                             # nothing found: untouched


@pytest.mark.parametrize("dim", DIMS)
def test_exhaustive_search_and_blend_at_width(dev, dim):
    """IndexFlatL2 semantics with the index cut into three column chunks, the last one ragged; test_exhaustive_search_and_mix's bars
    (rtol 1e-4, atol 1e-3 at |x|^2 ~ 64: the GEMM expansion's fp32 noise) with the absolute part scaled by |x|^2 / 64."""
    cent, sizes, ids, stored, by_label, feats = _data(dim)
    n, t = len(by_label), len(feats)
    old = retrieval.CHUNK
    retrieval.CHUNK = 128
    assert 2 * 128 < n < 3 * 128 and n % 128
    try:
        D, I = faiss_ivf.flat_search(feats, by_label)
        d64 = ((feats[:, None, :].astype(np.float64) - by_label[None].astype(np.float64)) ** 2).sum(-1)
        atol = 1e-3 * max(float((by_label.astype(np.float64) ** 2).sum(1).max()), float((feats.astype(np.float64) ** 2).sum(1).max()), 64.0) / 64
        nxt = np.take_along_axis(d64, np.lexsort((np.arange(n)[None].repeat(t, 0), d64), axis=1)[:, 1:9], 1)
        firm = _both_sides(nxt - D > 2 * atol)
        assert firm.mean() >= 0.95 and I[1, 0] == 17 and D[1, 0] == 0
        idx = retrieval.FeatureIndex(by_label, dev.device)
        assert not idx.ivf
        d, i = idx.search(dev.t(torch.from_numpy(feats)))
        got_i = i.cpu().numpy()
        print("dim %d: worst |d - D| %.3g (atol %.3g)" % (dim, np.abs(d.cpu().numpy() - D).max(), atol))
        assert np.allclose(d.cpu().numpy(), D, rtol=1e-4, atol=atol)
        assert (got_i[firm] == I[firm]).all() and got_i[1, 0] == 17
        f = dev.t(torch.from_numpy(feats.copy()))
        mixed = idx.mix_(f, 0.6).cpu().numpy()
        Dg = np.take_along_axis(d64, got_i, 1)                                # the blend uses DIRECT distances of the neighbours found
        want = _blend_want(feats, by_label, Dg, got_i, 0.6)
        assert np.abs(mixed - want).max() < 2e-5 * np.abs(want).max()
        assert np.allclose(mixed[1], feats[1], rtol=3e-7, atol=0)
    finally:
        retrieval.CHUNK = old


@pytest.mark.parametrize("dim", DIMS + [1, 67])
def test_row_sqnorm_at_width(dev, dim):
    """dim squares, dim - 1 additions in any order: (dim + 1) * 2^-24 covers dim u to first order."""
    rng = np.random.default_rng(dim)
    v = rng.standard_normal((37, dim)).astype(np.float32) * 3
    got = ops.row_sqnorm(dev.t(torch.from_numpy(v))).cpu().numpy().astype(np.float64)
    ref = (v.astype(np.float64) ** 2).sum(1)
    assert (np.abs(got - ref) <= (dim + 1) * U * ref).all()


def test_knn8_merge_breaks_ties_by_the_lower_column(dev):
    """aicg_knn8 over three column chunks (70, 70, 60 columns: more than one column per lane, a ragged last pass) of hand-made inner
    products whose distances are small integers, exact in fp32 (|x|^2 = |q|^2 = 0, d = -2 dot): ties everywhere, inside a lane's own
    list, across lanes, across chunk boundaries (columns 69 | 70, 139 | 140) and between the running best and a new chunk.  The lower
    column wins; the result is the (distance, column) lexicographic top 8."""
    rng = np.random.default_rng(1)
    rows, cols, bounds = 5, 200, [0, 70, 140, 200]
    dist = rng.integers(1, 6, (rows, cols)).astype(np.float64)
    dist[1] = 3.0                                                             # all equal: columns 0..7
    dist[2] = 5.0
    dist[2, [69, 70, 139, 140, 199]] = 1.0                                    # the only small ones straddle both boundaries
    dist[3] = np.arange(cols, 0, -1)                                          # strictly descending: every chunk replaces the whole best
    dist[4, :] = 4.0
    dist[4, 150:] = 0.0                                                       # zeros only in the last chunk
    dots = dev.t(torch.from_numpy((-dist / 2).astype(np.float32)))
    zc, zr = dev.t(torch.zeros(cols)), dev.t(torch.zeros(rows))
    best_d = torch.empty((rows, 8), dtype=torch.float32, device=dev.device)
    best_i = torch.empty((rows, 8), dtype=torch.int64, device=dev.device)
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        ops.knn8_update(dots[:, c0:c1], zc[c0:c1], zr, c0, best_d, best_i, merge=c0 > 0)
    order = np.lexsort((np.arange(cols)[None].repeat(rows, 0), dist), axis=1)[:, :8]
    assert np.array_equal(best_i.cpu().numpy(), order)
    assert np.array_equal(best_d.cpu().numpy().astype(np.float64), np.take_along_axis(dist, order, 1))
    assert list(order[2][:5]) == [69, 70, 139, 140, 199] and list(order[1]) == list(range(8))
