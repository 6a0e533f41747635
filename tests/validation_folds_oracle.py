"""NumPy restatement of the one-pass k-fold count tables (the arithmetic of fn_confidence_counts_folds).

Every pair distance of a class pair is binned ONCE.  A pair of rows held out in folds fa and fb belongs to the training part
of every fold except fa and fb, so the histogram of fold f's training part is ``total - touch_f`` with ``touch_f`` the
histogram of the pairs with ``fa == f or fb == f``; the weights use the rows and classes left in that training part."""
import numpy as np
from sklearn.model_selection import KFold

# (class sizes, E, folds, (class, fold) cells with no training row): the input sets of the one-pass tests
CASES = [
    ([6] * 12 + [9, 3, 14], 64, 4, 0),
    ([1, 2, 1, 5, 9, 2, 1, 3, 30, 1], 32, 5, 4),
    ([3] * 20, 48, 10, 0),
    ([70, 45], 24, 2, 0),
    ([4, 1, 1, 6], 16, 3, 2),
    ([5, 7, 4, 6], 512, 4, 0),             # the embedding size of the real models
    ([150, 3, 40], 100, 3, 0),             # E not a multiple of 4, a class larger than two 64-row tiles
]


def pool(sizes, E, seed, spread=0.5):
    """The ``_pool`` recipe of tests/test_gpu_validation.py: unit-norm fp32 rows around one centre per class, shuffled."""
    rng = np.random.default_rng(seed)
    emb, labels = [], []
    for c, n in enumerate(sizes):
        cen = rng.normal(size=(1, E))
        emb.append(cen * 0.6 + rng.normal(size=(n, E)) * spread)
        labels += [c * 3 + 7] * n
    emb = np.concatenate(emb).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    labels = np.array(labels)
    p = rng.permutation(len(labels))
    return emb[p], labels[p]


def kfold(n, F):
    """(fold each index is held out in, the (train, test) splits) of KFold(F, shuffle=True, random_state=0)."""
    splits = list(KFold(n_splits=F, shuffle=True, random_state=0).split(np.arange(n)))
    fold = np.empty(n, np.int64)
    for f, (_, te) in enumerate(splits):
        fold[te] = f
    return fold, splits


def tables(labels, fold, F):
    """Brute force: (train_rows [C, F], train_classes [F]) over the sorted unique labels."""
    uniq = np.unique(labels)
    rows = np.array([[int(np.sum((labels == u) & (fold != f))) for f in range(F)] for u in uniq])
    return rows, np.array([len(np.unique(labels[fold != f])) for f in range(F)])


def onepass(emb, labels, fold, thr, F, metric=0):
    """out [F, 4, T] (tp / tn / fp / fn per fold's training part) and the number of (class, fold) cells without a training row."""
    emb = np.asarray(emb, dtype=np.float64)
    order = np.argsort(labels, kind="stable")
    emb, labels, fold = emb[order], labels[order], fold[order]
    uniq, cnt = np.unique(labels, return_counts=True)
    C, T = len(uniq), len(thr)
    start = np.concatenate([[0], np.cumsum(cnt)])
    held = np.zeros((C, F), np.int64)
    for c in range(C):
        held[c] = np.bincount(fold[start[c]:start[c + 1]], minlength=F)
    ntrain = cnt[:, None] - held                       # rows of class c in the training part of fold f
    Cf = (ntrain > 0).sum(0)                           # classes present in the training part of fold f
    out = np.zeros((F, 4, T))
    for i in range(C):
        A, fa = emb[start[i]:start[i + 1]], fold[start[i]:start[i + 1]]
        for k in range(i + 1):
            B, fb = emb[start[k]:start[k + 1]], fold[start[k]:start[k + 1]]
            s = np.clip(A @ B.T, -1, 1)
            d = 2 * (1 - s) if metric == 0 else np.arccos(s)
            FA, FB = np.broadcast_arrays(fa[:, None], fb[None, :])
            if i == k:
                iu = np.triu_indices(len(A), 1)
                d, FA, FB = d[iu], FA[iu], FB[iu]
            else:
                d, FA, FB = d.ravel(), FA.ravel(), FB.ravel()
            b = np.searchsorted(thr, d, side="right")            # first n with thr[n] > d
            total = np.bincount(b, minlength=T + 1)
            for f in range(F):
                touch = np.bincount(b[(FA == f) | (FB == f)], minlength=T + 1)
                h = np.cumsum((total - touch)[:T])               # count(d < thr[n]) over the training pairs of fold f
                P = ntrain[i, f] * (ntrain[i, f] - 1) // 2 if i == k else ntrain[i, f] * ntrain[k, f]
                if P < 1:
                    continue
                w = P * (Cf[f] if i == k else Cf[f] * (Cf[f] - 1) / 2)
                if i == k:
                    out[f, 0] += h / w
                    out[f, 3] += (P - h) / w
                else:
                    out[f, 2] += h / w
                    out[f, 1] += (P - h) / w
    return out, int((ntrain == 0).sum())
