"""NumPy restatement of the softmax-training embedding regularisers: the center loss of
facenet/facenet.py:204-217 and the prelogits-norm loss of apps/configs/train_softmax.yaml:73-78.

x = the fp32 prelogits [N, E], y = int labels [N], centers = fp32 [C, E] as they were BEFORE this step's update.
Losses and gradients are float64 (the kernel computes them in double); the center update is float32 with every rounding of
the kernel, so it is compared bit for bit."""
import numpy as np


def _a(x):
    """a = |x| + 1e-4, formed in float32 like the kernel (x is float32)."""
    x = np.asarray(x)
    if x.dtype == np.float32:
        return (np.abs(x) + np.float32(1e-4)).astype(np.float64)
    return np.abs(x) + 1e-4


def center_loss(x, y, centers):
    """mean_{i,e} (x - c_old[y])^2 and its gradient 2 (x - c_old[y]) / (N E) (the centers get none)."""
    x = np.asarray(x, np.float64) if np.asarray(x).dtype != np.float64 else np.asarray(x)
    d = x - np.asarray(centers, np.float64)[np.asarray(y)]
    return float(np.mean(d * d)), 2.0 * d / d.size


def prelogits_norm(x, p):
    """mean_i (sum_e a^p)^(1/p), a = |x| + 1e-4, and its gradient sign(x) a^(p-1) n_i^(1-p) / N with sign(0) = 0."""
    xd = np.asarray(x, np.float64)
    a = _a(x)
    n = np.sum(a ** p, axis=1) ** (1.0 / p)
    g = np.sign(xd) * a ** (p - 1.0) * (n ** (1.0 - p))[:, None] / xd.shape[0]
    return float(np.mean(n)), g


def regularizer_grad(x, y, centers, center_factor, norm_factor, p):
    """The gradient fn_center_loss_fwd_bwd adds into demb (a factor of 0 contributes nothing).  The factors and p reach the
    kernel as float32 arguments: they are rounded to float32 here too."""
    cf, nf, p = (float(np.float32(v)) for v in (center_factor, norm_factor, p))
    g = np.zeros(np.shape(x), np.float64)
    if cf:
        g += cf * center_loss(x, y, centers)[1]
    if nf:
        g += nf * prelogits_norm(x, p)[1]
    return g


def add_grad(demb, g):
    """demb + g rounded once to float32 (what the kernel stores)."""
    return (np.asarray(demb, np.float64) + g).astype(np.float32)


def center_update(centers, x, y, alfa):
    """facenet.py:212-213 in the fixed order: for each class, the rows j carrying it in ascending order,
    c <- c - k (c_old - x_j), k = float32(1 - alfa), every operation rounded to float32."""
    out = np.array(centers, dtype=np.float32, copy=True)
    old = np.array(centers, dtype=np.float32, copy=True)
    x = np.asarray(x, np.float32)
    k = np.float32(1.0 - alfa)
    for j, cls in enumerate(np.asarray(y)):
        t = old[cls] - x[j]
        u = (k * t).astype(np.float32)
        out[cls] = (out[cls] - u).astype(np.float32)
    return out
