"""NumPy restatement of fn_gallery_search and the inputs its tests share.

s(q, g) is the ascending-e fp32 fmaf chain from 0.0f (oracle.facenet_oracle._fma32 is a correctly rounded fp32 FMA), sc = s clipped
to [-1, 1], the rank key d0 = 2 (1 - sc) in fp32, order ascending (d0, gallery row), tail row -1 / distance +inf."""
from __future__ import annotations

import numpy as np

from oracle.facenet_oracle import _fma32

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def chain_similarities(q, g):
    """[Q, G] fp32: acc = fma(q[:, e], g[:, e], acc) for e = 0 .. E-1, from 0."""
    q, g = np.asarray(q, dtype=np.float32), np.asarray(g, dtype=np.float32)
    acc = np.zeros((q.shape[0], g.shape[0]), dtype=np.float32)
    for e in range(q.shape[1]):
        acc = _fma32(q[:, e, None], g[None, :, e], acc)
    return acc


def distances(s):
    """(sc, d0) of the chain values, every operation in fp32."""
    sc = np.minimum(np.maximum(np.asarray(s, dtype=np.float32), np.float32(-1)), np.float32(1))
    return sc, (np.float32(2) * (np.float32(1) - sc)).astype(np.float32)


def search(q, g, k, metric=0, skip=None, s=None):
    """-> dict: dist float32 [Q, k] (metric 0: d0 bit for bit; metric 1: float64 arccos of the bit-exact sc, for a tolerance
    check), rows int32 [Q, k], sc float32 [Q, k] (NaN in the tail), s [Q, G] the chain values."""
    s = chain_similarities(q, g) if s is None else s
    sc, d0 = distances(s)
    Q, G = s.shape
    keys = (d0.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(G, dtype=np.uint64)[None, :]
    if skip is not None:
        skip = np.asarray(skip)
        hit = (skip >= 0) & (skip < G)
        keys[np.nonzero(hit)[0], skip[hit]] = NONE
    order = np.argsort(keys, axis=1, kind="stable")[:, :k]
    best = np.take_along_axis(keys, order, axis=1)
    rows = np.where(best == NONE, -1, order).astype(np.int32)
    if k > G:
        pad = k - G
        rows = np.concatenate([rows, np.full((Q, pad), -1, np.int32)], axis=1)
        order = np.concatenate([order, np.zeros((Q, pad), order.dtype)], axis=1)
    valid = rows >= 0
    sel_sc = np.where(valid, np.take_along_axis(sc, order, axis=1), np.float32(np.nan)).astype(np.float32)
    sel_d0 = np.where(valid, np.take_along_axis(d0, order, axis=1), np.float32(np.inf)).astype(np.float32)
    dist = sel_d0 if metric == 0 else np.where(valid, np.arccos(sel_sc.astype(np.float64)), np.inf)
    return {"dist": dist, "rows": rows, "sc": sel_sc, "s": s}


def unit_rows(n, E, seed):
    """n random rows of norm 1 (to fp32 rounding)."""
    x = np.random.default_rng(seed).standard_normal((n, E))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


TIE_E = 64


def tie_pool(n, seed):
    """n rows of 64 entries +-1/8: every row has norm exactly 1 and every partial sum of a dot product is a multiple of 1/64
    of magnitude <= 1, so the fp32 chain is exact and equal dot products are equal bit for bit."""
    signs = np.random.default_rng(seed).integers(0, 2, (n, TIE_E)) * 2 - 1
    return (signs * 0.125).astype(np.float32)


def adversarial_order(G, E, seed, nq=3):
    """(queries [nq, E], gallery [G, E]): gallery rows at decreasing angles to query 0 and ordered by the chain distance so that
    each row is nearer to query 0 than all before it (every tile beats every threshold: the prune path runs every time); the
    other queries are query 0 nudged, so almost the same holds for them."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(E)
    q /= np.linalg.norm(q)
    noise = rng.standard_normal((G, E))
    noise -= (noise @ q)[:, None] * q
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    theta = np.linspace(1.5, 0.05, G)[:, None]
    gallery = (np.cos(theta) * q + np.sin(theta) * noise).astype(np.float32)
    queries = q[None, :] + 1e-4 * rng.standard_normal((nq, E)) * (np.arange(nq) > 0)[:, None]
    queries = (queries / np.linalg.norm(queries, axis=1, keepdims=True)).astype(np.float32)
    _, d0 = distances(chain_similarities(queries[:1], gallery))
    return queries, gallery[np.argsort(-d0[0].astype(np.float64), kind="stable")]
