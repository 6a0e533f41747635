"""float64 NumPy restatement of the pair classifiers and their training, line by line from
facenet/faceclass.py:8-118, facenet/facenet.py:89-123 and apps/train_classifier.py:17-125 of the reference."""
import random

import numpy as np

MODE_DISTANCE, MODE_NORMALIZED = 0, 1


def distance(x, y=None, mode=MODE_DISTANCE, theta=1.0):
    """faceclass.py:45-77 (distance classifier) / :102-110 (normalized classifier)."""
    x = np.asarray(x, np.float64)
    y = x if y is None else np.asarray(y, np.float64)
    if mode == MODE_NORMALIZED:
        return 2 * (1 - x @ y.T)
    y = y.T
    norm_x = np.linalg.norm(x, axis=1, keepdims=True)
    norm_y = np.linalg.norm(y, axis=0, keepdims=True)
    x1, y1 = x / norm_x, y / norm_y
    return 2 * (1 - x1 @ y1) + theta * pow(2 * (norm_x - norm_y) / (norm_x + norm_y), 2)


def ratio2(x, y=None):
    """(2 (n_x - n_y) / (n_x + n_y))^2, the factor of theta."""
    x = np.asarray(x, np.float64)
    y = x if y is None else np.asarray(y, np.float64)
    nx = np.linalg.norm(x, axis=1)[:, None]
    ny = np.linalg.norm(y, axis=1)[None, :]
    return (2 * (nx - ny) / (nx + ny)) ** 2


def logits(x, y=None, mode=MODE_DISTANCE, alpha=10.0, threshold=1.0, theta=1.0):
    """faceclass.py:23-27."""
    return alpha * (threshold - distance(x, y, mode, theta))


def pair_labels(P, K):
    """train_classifier.py:62-72: upper-triangle pairs i < k of a batch of P K rows and their labels."""
    batch_size = P * K
    triu = np.triu_indices(batch_size, k=1)
    labels = [1 if (i // K) == (k // K) else 0 for i, k in zip(*triu)]
    return triu, np.asarray(labels, np.float64)


def pos_weight(P, K):
    """train_classifier.py:74."""
    _, labels = pair_labels(P, K)
    return len(labels) / sum(labels) - 1


def weighted_bce(z, s, q):
    """tf.nn.weighted_cross_entropy_with_logits(labels=z, logits=s, pos_weight=q), the numerically stable form."""
    w = 1 + (q - 1) * z
    return (1 - z) * s + w * (np.log1p(np.exp(-np.abs(s))) + np.maximum(-s, 0))


def pair_loss(batch, P, K, mode=MODE_DISTANCE, alpha=10.0, threshold=1.0, theta=1.0, q=None):
    """train_classifier.py:60-84: loss = mean of the weighted BCE over the pairs, and its analytic gradient
    {d/dalpha, d/dthreshold, d/dtheta}; also the sums of |term| that scale a tolerance."""
    q = pos_weight(P, K) if q is None else q
    triu, z = pair_labels(P, K)
    d = distance(batch, None, mode, theta)[triu]
    r2 = ratio2(batch)[triu] if mode == MODE_DISTANCE else np.zeros_like(d)
    u = threshold - d
    s = alpha * u
    ce = weighted_bce(z, s, q)
    n = len(z)
    g = ((1 - z) - (1 + (q - 1) * z) / (1 + np.exp(s))) / n       # dL/ds per pair
    grads = np.array([np.sum(g * u), np.sum(g * alpha), -np.sum(g * alpha * r2) if mode == MODE_DISTANCE else 0.0])
    scale = np.array([np.sum(np.abs(g * u)), np.sum(np.abs(g * alpha)), np.sum(np.abs(g * alpha * r2))])
    return float(np.mean(ce)), grads, scale


def adam(w, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=0.1):
    """TF1 AdamOptimizer (= tf.keras Adam): one update with step count t (1-based)."""
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    lr_t = lr * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    return w - lr_t * m / (np.sqrt(v) + eps), m, v


def learning_rate(initial_value, decay_rate, decay_steps, global_step):
    """train_classifier.py:114-125."""
    return initial_value * pow(decay_rate, np.floor(float(global_step) / decay_steps))


def reference_batches(embeddings, P, K):
    """facenet.py:116-121, the reference generator: the rows themselves (lists)."""
    while True:
        embs = []
        for embeddings_per_class in random.sample(embeddings, P):
            embs += random.sample(embeddings_per_class.tolist(), K)
        yield embs


def reference_subsample(embeddings, nrof_classes, max_nrof_images):
    """facenet.py:237-253 on the per-class arrays."""
    if nrof_classes and len(embeddings) > nrof_classes:
        labels = random.sample([_ for _ in range(len(embeddings))], nrof_classes)
        embeddings = [embeddings[label] for label in labels]
    if max_nrof_images:
        for idx, emb in enumerate(embeddings):
            if emb.shape[0] > max_nrof_images:
                labels = random.sample([_ for _ in range(emb.shape[0])], max_nrof_images)
                embeddings[idx] = embeddings[idx][labels, :]
    return embeddings


def confusion_matrix(embeddings, mode=MODE_DISTANCE, threshold=1.0, theta=1.0):
    """train_classifier.py:18-49 with classifier.predict = distance < threshold."""
    nrof_classes = len(embeddings)
    nrof_positive_class_pairs = nrof_classes
    nrof_negative_class_pairs = nrof_classes * (nrof_classes - 1) / 2
    tp = tn = fp = fn = 0
    for i in range(nrof_classes):
        for k in range(i):
            mean = np.mean(distance(embeddings[i], embeddings[k], mode, theta) < threshold)
            fp += mean
            tn += 1 - mean
        mean = np.mean(distance(embeddings[i], None, mode, theta) < threshold)
        tp += mean
        fn += 1 - mean
    tp /= nrof_positive_class_pairs
    fn /= nrof_positive_class_pairs
    fp /= nrof_negative_class_pairs
    tn /= nrof_negative_class_pairs
    return dict(tp=tp, tn=tn, fp=fp, fn=fn, accuracy=(tp + tn) / (tp + fp + tn + fn), precision=tp / (tp + fp),
                tp_rate=tp / (tp + fn), tn_rate=tn / (tn + fp))


def clustered(sizes, E, seed, spread=0.35, norm_jitter=0.3, dtype=np.float32):
    """Per-class arrays: a random unit center per class plus noise, rows scaled by 1 +- norm_jitter."""
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        c = rng.standard_normal(E)
        c /= np.linalg.norm(c)
        x = c + spread * rng.standard_normal((n, E)) / np.sqrt(E)
        x *= (1 + norm_jitter * (rng.random((n, 1)) * 2 - 1))
        out.append(x.astype(dtype))
    return out
