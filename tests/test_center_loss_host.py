"""CPU checks of the softmax-training embedding regularisers: the reference's config defaults
(apps/configs/train_softmax.yaml:73-78), the NumPy oracle's gradients against torch.autograd and its fixed update order for
repeated labels (facenet/facenet.py:204-217)."""
import numpy as np
import pytest
import torch

from facenet_amd.config import load_config
from tests import center_loss_oracle as co


def test_config_carries_the_reference_loss_defaults():
    loss = load_config().loss
    assert loss.center_factor == 0.0 and loss.center_alfa == 0.95
    assert loss.prelogits_norm_factor == 0.0 and loss.prelogits_norm_p == 1.0
    assert loss.alpha == 0.2
    over = load_config(overrides={"loss": {"center_factor": 0.01}}).loss
    assert over.center_factor == 0.01 and over.center_alfa == 0.95


def _torch_terms(x, y, centers, p):
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    c = torch.tensor(centers, dtype=torch.float64)[torch.as_tensor(y)]
    cl = ((xt - c) ** 2).mean()
    a = xt.abs() + 1e-4
    pn = (a ** p).sum(dim=1).pow(1.0 / p).mean()
    g_c, = torch.autograd.grad(cl, xt, retain_graph=True)
    g_n, = torch.autograd.grad(pn, xt)
    return float(cl), float(pn), g_c.numpy(), g_n.numpy()


@pytest.mark.parametrize("p", [1.0, 1.5, 2.0])
def test_oracle_gradients_match_autograd(p):
    rng = np.random.default_rng(int(p * 10))
    N, E, C = 9, 16, 5
    x = rng.standard_normal((N, E))
    x[0, :3] = 0.0                                   # exact zeros: sign(0) = 0, the gradient torch (and TF) give abs at 0
    x[4, 7] = 0.0
    y = np.array([0, 1, 1, 2, 4, 1, 0, 3, 1])
    centers = rng.standard_normal((C, E))
    cl, pn, g_c, g_n = _torch_terms(x, y, centers, p)
    ocl, og_c = co.center_loss(x, y, centers)
    opn, og_n = co.prelogits_norm(x, p)
    assert abs(ocl - cl) <= 1e-12 * abs(cl) and abs(opn - pn) <= 1e-12 * abs(pn)
    np.testing.assert_allclose(og_c, g_c, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(og_n, g_n, rtol=1e-12, atol=1e-15)
    assert np.all(og_n[0, :3] == 0.0) and og_n[4, 7] == 0.0
    g = co.regularizer_grad(x, y, centers, 0.5, 0.25, p)
    np.testing.assert_allclose(g, 0.5 * g_c + 0.25 * g_n, rtol=1e-12, atol=1e-15)
    assert np.array_equal(co.regularizer_grad(x, y, centers, 0.0, 0.25, p), 0.25 * og_n)   # factor 0: nothing added


def test_oracle_update_order_for_repeated_labels():
    """Each class: c <- c - k (c_old - x_j) over its rows in ascending order, k = float32(1 - alfa), float32 roundings."""
    rng = np.random.default_rng(3)
    E, alfa = 8, 0.95
    centers = rng.standard_normal((4, E)).astype(np.float32)
    x = rng.standard_normal((6, E)).astype(np.float32)
    y = np.array([2, 0, 2, 3, 2, 0])
    got = co.center_update(centers, x, y, alfa)
    k = np.float32(1.0 - alfa)
    assert k == np.float32(0.05000000000000004)
    want = centers.copy()
    for cls in (0, 2, 3):
        c = centers[cls].copy()
        for j in np.flatnonzero(y == cls):           # ascending row order
            c = np.float32(c - np.float32(k * np.float32(centers[cls] - x[j])))
        want[cls] = c
    assert np.array_equal(got, want)
    assert np.array_equal(got[1], centers[1])        # a class absent from the batch keeps its center
    # with a single row per class the update is TF's: c - (1 - alfa)(c - x)
    single = co.center_update(centers, x[:2], y[:2], alfa)
    assert np.array_equal(single[0], np.float32(centers[0] - np.float32(k * np.float32(centers[0] - x[1]))))
