"""The reference's two greedy loops over false examples (facenet/statistics.py:334-421) in NumPy, over an
fp32 distance matrix of rows sorted by class and ``starts``.  Written from the semantics, not from the kernel:

false negatives, per class with at least 2 rows: over the pairs (i < k) of rows not yet excluded take the largest d, ties to the
smallest i, then k; emit it and exclude both rows when d > threshold, else stop; at most max_fneg picks.
false positives, per pair of classes a < b: over (i in a, k in b), row i and column k not yet excluded, take the smallest d, ties
to the smallest i, then k; emit it and exclude row i and column k when d < threshold, else stop; at most max_fpos picks.

Both return [(distance fp32, row1, row2)] with global rows, in the order (class or pair of classes, pick)."""
import numpy as np

from tests import pair_lattice as pl


def false_negatives(D, starts, threshold, max_fneg=10):
    D, t, out = np.asarray(D, np.float32), np.float32(threshold), []
    for c in range(len(starts) - 1):
        a0, n = int(starts[c]), int(starts[c + 1] - starts[c])
        m = D[a0:a0 + n, a0:a0 + n].astype(np.float64)
        m[np.tril_indices(n)] = -np.inf                       # i < k only
        for _ in range(max_fneg):
            if n < 2:
                break
            i, k = np.unravel_index(np.argmax(m), m.shape)    # the first in row-major order
            if not np.float32(m[i, k]) > t:
                break
            out.append((np.float32(m[i, k]), a0 + int(i), a0 + int(k)))
            m[[i, k], :] = -np.inf
            m[:, [i, k]] = -np.inf
    return out


def false_positives(D, starts, threshold, max_fpos=2):
    D, t, out = np.asarray(D, np.float32), np.float32(threshold), []
    C = len(starts) - 1
    for a in range(C):
        for b in range(a + 1, C):
            a0, b0 = int(starts[a]), int(starts[b])
            m = D[a0:int(starts[a + 1]), b0:int(starts[b + 1])].astype(np.float64)
            for _ in range(max_fpos):
                if m.size == 0:
                    break
                i, k = np.unravel_index(np.argmin(m), m.shape)
                if not np.float32(m[i, k]) < t:
                    break
                out.append((np.float32(m[i, k]), a0 + int(i), b0 + int(k)))
                m[i, :] = np.inf
                m[:, k] = np.inf
    return out


def false_pairs(D, starts, threshold, max_fneg=10, max_fpos=2):
    return false_negatives(D, starts, threshold, max_fneg), false_positives(D, starts, threshold, max_fpos)


def lattice_distances(H, metric, E0=64, scale=1.0):
    """fp32 distances of lattice rows: exact at metric 0."""
    return pl.distance32(pl.exact_dots(H, E0, scale).astype(np.float32), metric)


def chain_distances(emb, metric=0):
    """fp32 distances of any rows from the host's restatement of the kernels' fmaf chain: the kernels' bits at metric 0."""
    return pl.distance32(pl.fp32_chain(emb, emb), metric)


def records_bound(sizes, max_fneg, max_fpos):
    """sum over classes of min(max_fneg, n // 2) + sum over pairs of classes of min(max_fpos, n_a, n_b), term by term."""
    sizes = [int(n) for n in sizes]
    return (sum(min(max_fneg, n // 2) for n in sizes)
            + sum(min(max_fpos, sizes[a], sizes[b]) for a in range(len(sizes)) for b in range(a + 1, len(sizes))))
