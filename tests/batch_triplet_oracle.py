"""fp64 NumPy reference of fn_batch_triplet_fwd_bwd (csrc/batch_triplet.hip) with derived error bounds.

Mining runs on a GIVEN distance matrix.  Handed the fp32 matrix the device itself produced, every decision -- the farthest positive
and nearest negative of batch hard (ties to the lowest index), the strict ``> 0`` of a hinge -- is taken on the device's own bits,
and both sides form a term by the same IEEE operations, l = ((double) d_ap - (double) d_an) + (double) alpha.  For a hinge ``coef``
(+-1, or integer counts <= 1023) and ``info`` are therefore compared EXACTLY; only ``loss``, the soft-margin ``coef`` and ``demb``
carry rounding, and their bounds are counted off the kernel, not chosen (u = 2^-24, the fp32 unit roundoff):

loss    Every term is >= 0, so sum |term| / Z = loss.  The budget is one fp32 rounding per term computed from the fp32
        dist, u * sum |term| / Z = u * loss.  The kernel forms the terms in fp64 and spends that budget once per ANCHOR: an
        anchor's fp64 partial sum is rounded to fp32 to cross the kernel boundary (sum_a u * partial_a / Z = u * loss).  One more
        rounding stores loss[0] (u * loss).  The fp64 sums -- at most n_max terms per anchor, then a tree over N anchors -- and
        the fp64 exp / log1p of a soft margin (a few fp64 ulps) add (n_max + N + 16) * 2^-53 * loss, which is negligible and
        kept for completeness.   e_loss = (2 u + (n_max + N + 16) 2^-53) * loss.

coef    Soft margin only.  sigma(l) is evaluated in fp64 and the sum over a pair's triplets is an fp64 sum in a fixed order,
        rounded to fp32 once:   e_coef = (u + (n + 16) 2^-53) * |coef|,   n the number of triplets that use the pair.

demb    demb[r][e] = (2/Z) sum_j w_rj (x_re - x_je), j ascending over the terms_r non-zero w_rj = coef[r][j] + coef[j][r].  One
        fp32 rounding per difference, per product and per add of the chain (terms_r - 1 adds), one for the scale (formed in fp64,
        rounded once):   (terms_r + 2) * u * (2/Z) * sum_j |w_rj| |x_re - x_je|.   For a hinge w_rj is an exact integer.  For a soft
        margin it carries the error of both coefficients and the rounding of their fp32 sum, e_w = e_coef[r][j] + e_coef[j][r] +
        u |w_rj|, which propagates as (2/Z) * sum_j e_w |x_re - x_je|.

``triple_loop`` is the definition written out literally over (a, p, n), for small N: the host test holds ``mine`` to it."""
import numpy as np

U = 2.0 ** -24
D = 2.0 ** -53


def softplus(l):
    return np.maximum(l, 0.0) + np.log1p(np.exp(-np.abs(l)))


def sigmoid(l):
    e = np.exp(-np.abs(l))
    return np.where(l >= 0, 1.0, e) / (1.0 + e)


def sqdist64(x):
    """[N,N] squared distances of fp64 rows in the difference form."""
    x = np.asarray(x, np.float64)
    d = x[:, None, :] - x[None, :, :]
    return (d * d).sum(-1)


def normaliser(info, strategy, soft):
    return int(info[0] if strategy == 0 else (info[1] if soft else info[2]))


def mine(dist, labels, alpha, strategy, soft, emb=None):
    """dist [N,N] (the device's fp32 matrix, or any fp64 one), labels [N], alpha (taken as its fp32 value, as the kernel gets it).
    -> dict(coef fp64 [N,N], e_coef, info int64 [8], loss, e_loss, Z) and, with emb [N,E]: demb fp64 [N,E], e_demb."""
    d = np.asarray(dist)
    lab = np.asarray(labels).reshape(-1)
    N = len(lab)
    assert d.shape == (N, N)
    d64 = d.astype(np.float64)
    alpha64 = float(np.float32(alpha))
    coef, uses = np.zeros((N, N)), np.zeros((N, N))
    anchors = terms = active = nonfinite = n_max = 0
    total = 0.0
    for a in range(N):
        same = lab == lab[a]
        neg = ~same
        same[a] = False
        if not same.any() or not neg.any():
            continue
        anchors += 1
        P, Q = np.flatnonzero(same), np.flatnonzero(neg)
        if not (np.isfinite(d[a, P]).all() and np.isfinite(d[a, Q]).all()):
            nonfinite = 1
        if strategy == 0:
            P, Q = P[[np.argmax(d[a, P])]], Q[[np.argmin(d[a, Q])]]              # first occurrence: the lowest index on ties
        l = d64[a, P][:, None] - d64[a, Q][None, :]
        if soft:
            value, sg = softplus(l), sigmoid(l)
            act = np.ones(l.shape, bool)
        else:
            l = l + alpha64
            act = l > 0
            value, sg = np.where(act, l, 0.0), act.astype(np.float64)
        terms += l.size
        active += int(act.sum())
        n_max = max(n_max, l.size)
        total += float(value.sum())
        coef[a, P], coef[a, Q] = sg.sum(1), -sg.sum(0)
        uses[a, P], uses[a, Q] = len(Q), len(P)
    info = np.array([anchors, terms, active, nonfinite, 0, 0, 0, 0], np.int64)
    Z = normaliser(info, strategy, soft)
    loss = total / Z if Z else 0.0
    out = dict(coef=coef, e_coef=(U + (uses + 16) * D) * np.abs(coef) if soft else np.zeros((N, N)), info=info, Z=Z,
               loss=float("nan") if nonfinite else loss, e_loss=(2 * U + (n_max + N + 16) * D) * loss)
    if emb is not None:
        x = np.asarray(emb).astype(np.float64)
        W = coef + coef.T
        EW = out["e_coef"] + out["e_coef"].T + (U * np.abs(W) if soft else 0.0)
        demb, e_demb = np.zeros_like(x), np.zeros_like(x)
        if Z:
            for r in range(N):
                diff = x[r][None, :] - x
                absd = np.abs(diff)
                demb[r] = (2.0 / Z) * (W[r][:, None] * diff).sum(0)
                e_demb[r] = (2.0 / Z) * ((np.count_nonzero(W[r]) + 2) * U * (np.abs(W[r])[:, None] * absd).sum(0) + (EW[r][:, None] * absd).sum(0))
        out.update(demb=demb, e_demb=e_demb)
    return out


def triple_loop(dist, labels, alpha, strategy, soft):
    """The definition, literally: -> (coef, info[:3], loss).  O(N^3): small N only."""
    d = np.asarray(dist, np.float64)
    lab = list(np.asarray(labels).reshape(-1))
    N = len(lab)
    alpha64 = float(np.float32(alpha))
    coef = np.zeros((N, N))
    anchors = terms = active = 0
    total = 0.0
    for a in range(N):
        triplets = [(p, n) for p in range(N) if p != a and lab[p] == lab[a] for n in range(N) if lab[n] != lab[a]]
        if not triplets:
            continue
        anchors += 1
        if strategy == 0:
            p_star = n_star = None
            for p, n in triplets:
                if p_star is None or d[a, p] > d[a, p_star]:
                    p_star = p
                if n_star is None or d[a, n] < d[a, n_star]:
                    n_star = n
            triplets = [(p_star, n_star)]
        for p, n in triplets:
            terms += 1
            l = d[a, p] - d[a, n]
            if soft:
                value, g = float(softplus(np.float64(l))), float(sigmoid(np.float64(l)))
            else:
                l += alpha64
                value, g = (l, 1.0) if l > 0 else (0.0, 0.0)
            if soft or l > 0:
                active += 1
            total += value
            coef[a, p] += g
            coef[a, n] -= g
    Z = anchors if strategy == 0 else (terms if soft else active)
    return coef, [anchors, terms, active], (total / Z if Z else 0.0)


def ragged_labels(n, seed, sizes=(1, 2, 3, 7)):
    """n identity ids in classes of sizes cycling through ``sizes``: unsorted, non-contiguous and partly negative."""
    rng = np.random.default_rng(seed)
    lab, c = [], 0
    while len(lab) < n:
        lab += [c * 37 - 1000] * sizes[c % len(sizes)]
        c += 1
    return rng.permutation(np.array(lab[:n], np.int64))
