"""fp64 NumPy reference of fn_xbm_triplet_fwd_bwd and a host model of fn_xbm_enqueue (csrc/batch_triplet.hip),
built on tests/batch_triplet_oracle.py, with derived error bounds.

Batch hard over a UNION of candidates: for anchor a the batch columns j != a (union index j) and the slots s < valid of the memory
(union index N + s).  As in section 31, mining runs on GIVEN distance matrices -- the device's own fp32 ``dist`` [N,N] and
``mem_dist`` [N,M] -- so the farthest positive and the nearest negative (compared as the stored fp32 values, ties to the lowest union
index: np.argmax / np.argmin return the first occurrence), and the strict ``> 0`` of a hinge, are decided on the device's bits.  Both
sides form the anchor's single term by the same IEEE operations, l = ((double) d_ap - (double) d_an) + (double) alpha.  Hinge
``coef``, ``mpick``, hinge ``mcoef`` and ``info`` are therefore compared EXACTLY.  Slots at or beyond ``valid`` are sliced away before
anything is read: whatever they hold, NaN included, cannot matter.

The bounds are section 31's with the chain lengthened (u = 2^-24, the fp32 unit roundoff):

loss    One term per anchor (n_max = 1), every term >= 0.  The term is formed in fp64 and rounded once to fp32 to cross the kernel
        boundary on coef's diagonal (u * loss over the anchors); one more rounding stores loss[0] (u * loss).  The fp64 tree over N
        diagonal words, the division and the fp64 exp / log1p of a soft margin add (1 + N + 16) * 2^-53 * loss.
            e_loss = (2 u + (N + 17) 2^-53) * loss.

coef / mcoef    Soft margin only: sigma(l) in fp64 (a few fp64 ulps, counted as 16), one pair per coefficient (n = 1), rounded to
        fp32 once:   e_c = (u + 17 * 2^-53) * |c|.   The same c goes, with its sign, to coef or mcoef.

demb    demb[r] = (2/Z) (sum_j w_rj (x_r - x_j) + mcoef[r][0] (x_r - mem[mpick[r][0]]) + mcoef[r][1] (x_r - mem[mpick[r][1]])), one
        chain in that order, zero weights skipped, T_r non-zero weights in all (memory picks included).  One fp32 rounding per
        difference, per product and per add (T_r - 1 adds), one for the scale (formed in fp64, rounded once):
            (T_r + 2) * u * (2/Z) * sum |w| |diff|.
        A hinge's weights are exact integers.  A soft batch weight w_rj = coef[r][j] + coef[j][r] carries e_c of both and the
        rounding of their fp32 sum; a soft memory weight is mcoef itself and carries its e_c alone.  Either propagates as
        (2/Z) * sum e_w |diff|.

``literal_loop`` is the definition written out over (a, candidates), for small N: the host test holds ``mine`` to it.
``Ring`` is the host model of the ring buffer that fn_xbm_enqueue keeps on the device."""
import numpy as np

from tests import batch_triplet_oracle as bo

U, D = bo.U, bo.D


def mine(dist, mem_dist, labels, mem_labels, valid, alpha, soft, emb=None, mem=None):
    """dist [N,N], mem_dist [N,M] (the device's fp32 matrices, or any fp64 ones), labels [N], mem_labels [M], valid = mem_state[1].
    -> dict(coef fp64 [N,N], e_coef, mpick int [N,2], mcoef fp64 [N,2], e_mcoef, info int64 [8], loss, e_loss, Z) and, with
    emb [N,E] and mem [M,E]: demb fp64 [N,E], e_demb."""
    d, dm = np.asarray(dist), np.asarray(mem_dist)
    lab, mlab = np.asarray(labels).reshape(-1), np.asarray(mem_labels).reshape(-1)
    N, M = len(lab), len(mlab)
    assert d.shape == (N, N) and dm.shape == (N, M) and 0 <= valid <= M
    alpha64 = float(np.float32(alpha))
    coef, mcoef, mpick = np.zeros((N, N)), np.zeros((N, 2)), np.full((N, 2), -1, np.int64)
    anchors = active = nonfinite = mem_pos = mem_neg = 0
    total = 0.0
    ulab = np.concatenate([lab, mlab[:valid]])
    for a in range(N):
        du = np.concatenate([d[a], dm[a, :valid]])                    # by union index
        same = ulab == lab[a]
        neg = ~same
        same[a] = False
        if not same.any() or not neg.any():
            continue
        anchors += 1
        P, Q = np.flatnonzero(same), np.flatnonzero(neg)
        if not (np.isfinite(du[P]).all() and np.isfinite(du[Q]).all()):
            nonfinite = 1
        p, n = int(P[np.argmax(du[P])]), int(Q[np.argmin(du[Q])])     # first occurrence: the lowest union index on ties
        l = float(np.float64(du[p]) - np.float64(du[n]))
        if soft:
            value, c = float(bo.softplus(np.float64(l))), float(bo.sigmoid(np.float64(l)))
            active += 1
        else:
            l = l + alpha64
            value, c = (l, 1.0) if l > 0 else (0.0, 0.0)
            active += int(l > 0)
        total += value
        if p < N:
            coef[a, p] = c
        else:
            mpick[a, 0], mcoef[a, 0] = p - N, c
            mem_pos += 1
        if n < N:
            coef[a, n] = -c
        else:
            mpick[a, 1], mcoef[a, 1] = n - N, -c
            mem_neg += 1
    info = np.array([anchors, anchors, active, nonfinite, mem_pos, mem_neg, valid, 0], np.int64)
    Z = anchors
    loss = total / Z if Z else 0.0
    rel = (U + 17 * D) if soft else 0.0
    out = dict(coef=coef, e_coef=rel * np.abs(coef), mpick=mpick, mcoef=mcoef, e_mcoef=rel * np.abs(mcoef), info=info, Z=Z,
               loss=float("nan") if nonfinite else loss, e_loss=(2 * U + (N + 17) * D) * loss)
    if emb is not None:
        x, m = np.asarray(emb).astype(np.float64), np.asarray(mem).astype(np.float64)
        W = coef + coef.T
        EW = out["e_coef"] + out["e_coef"].T + (U * np.abs(W) if soft else 0.0)
        demb, e_demb = np.zeros_like(x), np.zeros_like(x)
        if Z:
            for r in range(N):
                rows = [x[j] for j in range(N)] + [m[max(s, 0)] for s in mpick[r]]
                w = np.concatenate([W[r], np.where(mpick[r] >= 0, mcoef[r], 0.0)])
                ew = np.concatenate([EW[r], out["e_mcoef"][r]])
                diff = x[r][None, :] - np.array(rows)
                absd = np.abs(diff)
                demb[r] = (2.0 / Z) * (w[:, None] * diff).sum(0)
                e_demb[r] = (2.0 / Z) * ((np.count_nonzero(w) + 2) * U * (np.abs(w)[:, None] * absd).sum(0) + (ew[:, None] * absd).sum(0))
        out.update(demb=demb, e_demb=e_demb)
    return out


def literal_loop(dist, mem_dist, labels, mem_labels, valid, alpha, soft):
    """The definition, literally, one candidate at a time in union order: -> (coef, mpick, mcoef, info[:7], loss)."""
    d, dm = np.asarray(dist, np.float64), np.asarray(mem_dist, np.float64)
    lab, mlab = list(np.asarray(labels).reshape(-1)), list(np.asarray(mem_labels).reshape(-1))
    N = len(lab)
    alpha64 = float(np.float32(alpha))
    coef, mcoef, mpick = np.zeros((N, N)), np.zeros((N, 2)), np.full((N, 2), -1, np.int64)
    anchors = active = mem_pos = mem_neg = 0
    total = 0.0
    for a in range(N):
        cands = [(j, d[a, j], lab[j]) for j in range(N) if j != a] + [(N + s, dm[a, s], mlab[s]) for s in range(valid)]
        p = n = None
        for u, dist_u, lab_u in cands:
            if lab_u == lab[a]:
                if p is None or dist_u > p[1]:
                    p = (u, dist_u)
            elif n is None or dist_u < n[1]:
                n = (u, dist_u)
        if p is None or n is None:
            continue
        anchors += 1
        l = p[1] - n[1]
        if soft:
            value, c = float(bo.softplus(np.float64(l))), float(bo.sigmoid(np.float64(l)))
        else:
            l += alpha64
            value, c = (l, 1.0) if l > 0 else (0.0, 0.0)
        active += int(bool(soft) or l > 0)
        total += value
        for k, (u, sign) in enumerate(((p[0], 1.0), (n[0], -1.0))):
            if u < N:
                coef[a, u] = sign * c
            else:
                mpick[a, k], mcoef[a, k] = u - N, sign * c
                mem_pos, mem_neg = mem_pos + (k == 0), mem_neg + (k == 1)
    return coef, mpick, mcoef, [anchors, anchors, active, 0, mem_pos, mem_neg, valid], (total / anchors if anchors else 0.0)


class Ring:
    """fn_xbm_enqueue on the host: emb fp32 [M,E], labels int32 [M], state int32 [4] = cursor | valid | calls seen | 0."""

    def __init__(self, M, E):
        self.M, self.E = M, E
        self.emb, self.labels, self.state = np.zeros((M, E), np.float32), np.zeros(M, np.int32), np.zeros(4, np.int32)

    def enqueue(self, emb, labels, start=0):
        emb, labels = np.asarray(emb, np.float32), np.asarray(labels, np.int32)
        n = len(labels)
        if not 1 <= n <= self.M or emb.shape != (n, self.E) or start < 0:
            raise ValueError("xbm_enqueue: 1 <= N <= M, emb [N,E], start >= 0")
        cursor, valid, calls = (int(v) for v in self.state[:3])
        if calls >= start:
            for i in range(n):
                self.emb[(cursor + i) % self.M] = emb[i]
                self.labels[(cursor + i) % self.M] = labels[i]
            self.state[0], self.state[1] = (cursor + n) % self.M, min(valid + n, self.M)
        self.state[2] = min(calls + 1, 2 ** 31 - 1)
