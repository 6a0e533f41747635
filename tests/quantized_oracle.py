"""NumPy restatement of fn_quantize_rows and fn_qgallery_search and the inputs their tests share.

Quantisation: m = max |x_e|, c_e = rint(x_e * 127 / m) in fp64 (half to even), scale = (float)(m / 127), rho = ||x - scale c|| and
norm = ||x|| as sequential fp64 sums of rounded squares, the IEEE square root, rounded up to fp32.  Shortlist: idot the exact
integer dot product of two code rows, s^ = (sq sg) (float) idot in fp32, key = bits(2 (1 - clip(s^))) << 32 | row, the R smallest.
Re-rank: identify_oracle's chain and distances over the shortlisted rows, cut to k.  Certificate: fp64, in the written order."""
from __future__ import annotations

import numpy as np

from tests import identify_oracle as io

U = 2.0 ** -24
NONE = io.NONE


def padded(E):
    return (E + 63) // 64 * 64


def float_not_below(v):
    """The smallest float32 >= v (fp64 >= 0)."""
    f = np.asarray(v, dtype=np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def seq_norm(t):
    """sqrt of the sequential ascending fp64 sum from 0.0 of the rounded squares of t [N, E]."""
    sq = t * t
    acc = np.zeros(t.shape[0], dtype=np.float64)
    for e in range(t.shape[1]):
        acc = acc + sq[:, e]
    return np.sqrt(acc)


def quantize(x):
    """-> dict: codes int8 [N, Ep], scale / rho / norm float32 [N], and rho64 / norm64 (the fp64 values before rounding up)."""
    x = np.asarray(x, dtype=np.float32)
    N, E = x.shape
    xd = x.astype(np.float64)
    m = np.abs(xd).max(axis=1)
    safe = np.where(m > 0, m, 1.0)
    c = np.where(m[:, None] > 0, np.rint(xd * 127.0 / safe[:, None]), 0.0)
    scale = np.where(m > 0, (m / 127.0).astype(np.float32), np.float32(0)).astype(np.float32)
    t = xd - scale.astype(np.float64)[:, None] * c
    rho64, norm64 = seq_norm(t), seq_norm(xd)
    codes = np.zeros((N, padded(E)), dtype=np.int8)
    codes[:, :E] = c.astype(np.int8)
    return {"codes": codes, "scale": scale, "rho": float_not_below(rho64), "norm": float_not_below(norm64), "rho64": rho64, "norm64": norm64}


def estimates(qq, gq):
    """s^ [Q, G] float32 of two quantised tables."""
    idot = qq["codes"].astype(np.int64) @ gq["codes"].astype(np.int64).T
    assert np.abs(idot).max(initial=0) < 2 ** 24
    return ((qq["scale"][:, None] * gq["scale"][None, :]).astype(np.float32) * idot.astype(np.float32)).astype(np.float32)


def shortlist_keys(est, R, skip=None):
    """uint64 [Q, R]: the R smallest keys of every query, ascending, all ones behind their number."""
    Q, G = est.shape
    _, d = io.distances(est)
    keys = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(G, dtype=np.uint64)[None, :]
    if skip is not None:
        skip = np.asarray(skip)
        hit = (skip >= 0) & (skip < G)
        keys[np.nonzero(hit)[0], skip[hit]] = NONE
    keys = np.sort(keys, axis=1)[:, :R]
    if R > G:
        keys = np.concatenate([keys, np.full((Q, R - G), NONE, dtype=np.uint64)], axis=1)
    return keys


def bound(rq, nq, rho_max, norm_max, E):
    """B, in fp64 in the written order (rq, nq: the query's stored rho and norm as fp64)."""
    eu = E * U
    gamma = eu / (1.0 - eu)
    t1 = rq * norm_max
    t2 = (nq + rq) * rho_max
    t3 = (gamma * nq) * norm_max
    return ((t1 + t2) + t3) + 4.0 * U


def search(q, g, k, R, metric=0, skip=None, s=None):
    """-> dict: keys uint64 [Q, R] (the shortlist), dist / rows as identify_oracle.search reports them, certified bool [Q],
    range (lo, hi) of the chain values re-ranked (None without one), est [Q, G], s [Q, G] the chain values, qq / gq."""
    q, g = np.asarray(q, dtype=np.float32), np.asarray(g, dtype=np.float32)
    Q, G, E = q.shape[0], g.shape[0], q.shape[1]
    qq, gq = quantize(q), quantize(g)
    est = estimates(qq, gq)
    keys = shortlist_keys(est, R, skip)
    s = io.chain_similarities(q, g) if s is None else s
    sc, d0 = io.distances(s)
    rho_max, norm_max = float(gq["rho"].max()), float(gq["norm"].max())
    dist = np.full((Q, k), np.inf, dtype=np.float32 if metric == 0 else np.float64)
    rows = np.full((Q, k), -1, dtype=np.int32)
    certified = np.zeros(Q, dtype=bool)
    seen = []
    for i in range(Q):
        cand = (keys[i][keys[i] != NONE] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        seen.append(s[i, cand])
        k2 = np.sort((d0[i, cand].view(np.uint32).astype(np.uint64) << np.uint64(32)) | cand.astype(np.uint64))[:k]
        best = (k2 & np.uint64(0xFFFFFFFF)).astype(np.int64)
        rows[i, :len(best)] = best
        dist[i, :len(best)] = d0[i, best] if metric == 0 else np.arccos(sc[i, best].astype(np.float64))
        if len(cand) < R:
            certified[i] = True
            continue
        rq, nq = float(qq["rho"][i]), float(qq["norm"][i])
        d_R = float((keys[i, R - 1] >> np.uint64(32)).astype(np.uint32).view(np.float32))
        rhs = (d_R - 2.0 * bound(rq, nq, rho_max, norm_max, E)) - 8.0 * U
        in_domain = (nq + rq) * (norm_max + rho_max) <= 1.05
        certified[i] = bool(in_domain and float(d0[i, best[k - 1]]) < rhs)
    seen = np.concatenate(seen) if seen else np.zeros(0, np.float32)
    return {"keys": keys, "dist": dist, "rows": rows, "certified": certified, "est": est, "s": s, "qq": qq, "gq": gq,
            "range": (float(seen.min()), float(seen.max())) if len(seen) else None}


def near_duplicates(classes, per_class, E, seed, spread=2e-3):
    """classes * per_class unit rows: every class a random direction with ``per_class`` copies perturbed by ``spread``."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((classes, E))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = np.repeat(centres, per_class, axis=0) + spread * rng.standard_normal((classes * per_class, E))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def small_integer_codes(n, E, seed):
    """n fp32 rows whose codes are the distinct small integers they are built from: entry e of row r is an integer in [-127, 127],
    its maximum magnitude exactly 127, scaled by 2^-13, so that c_e = the integer itself and s^ = idot 2^-26 exactly.  A different
    integer at every (row, e): a wrong k pairing or a swapped row / column changes the dot products."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-126, 127, (n, E))
    c[np.arange(n), rng.integers(0, E, n)] = 127
    return (c * 2.0 ** -13).astype(np.float32), c
