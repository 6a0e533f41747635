"""The margin-softmax oracle (tests/margin_oracle.py) without a GPU: its fp64 statement agrees with torch autograd on the textbook
formula, the fp32 restatement of every kernel stays inside the derived bounds on the GPU tests' inputs, each planted error falls
outside them, and the settings are checked and carried from the config to the trainer."""
import types

import numpy as np
import pytest
import torch

from facenet_amd.config import load_config
from tests import elementwise_oracle as eo
from tests import margin_oracle as mo

BF, HF = eo.BF, eo.HF
RNORM_SHAPES = [(37, 128), (1000, 512), (8, 8)]


# ---- the oracle against autograd ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,m_arc,m_cos", mo.SETTINGS)
def test_oracle_matches_autograd_in_fp64(scale, m_arc, m_cos):
    """The textbook head (cosine logits, phi = c cos m2 - sqrt(1 - c^2) sin m2 - m3 above th, the linear continuation below) in
    torch autograd, fp64, N = 7, C = 37, E = 16; the constants are the fp32-rounded ones the kernel receives."""
    N, C, E = 7, 37, 16
    g = torch.Generator().manual_seed(3)
    xn = torch.nn.functional.normalize(torch.randn(N, E, generator=g, dtype=torch.float64), dim=1).requires_grad_(True)
    W = (torch.randn(C, E, generator=g, dtype=torch.float64) * 0.4).requires_grad_(True)
    labels = torch.randint(0, C, (N,), generator=g)
    labels[2] = labels[5]
    cos_m, sin_m, th, mm = mo.constants(m_arc)
    c = xn @ torch.nn.functional.normalize(W, dim=1).t()
    assert float(c.detach().abs().max()) < mo.T_CLAMP                                      # inside both clamps
    ct = c[torch.arange(N), labels]
    if m_arc > 0:
        with torch.no_grad():                                                      # one target below th: the fallback is covered
            W[labels[0]] = -xn[0] * 0.3 + 0.02 * W[labels[0]]
        c = xn @ torch.nn.functional.normalize(W, dim=1).t()
        ct = c[torch.arange(N), labels]
        assert bool((ct <= th).any()) and bool((ct > th).any())
    phi = torch.where(ct > th, ct * cos_m - (1 - ct * ct).sqrt() * sin_m, ct - mm) - mo.f32(m_cos)
    logits = (scale * c).scatter(1, labels.view(N, 1), (scale * phi).view(N, 1))
    loss = torch.nn.functional.cross_entropy(logits, labels)
    dxn, dW = torch.autograd.grad(loss, (xn, W))
    o_loss, o_dW, o_dxn = mo.head_fp64(xn.detach(), W.detach(), labels, scale, m_arc, m_cos)
    for got, ref in ((o_loss, loss.detach()), (o_dW, dW), (o_dxn, dxn)):
        assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max())
    assert float((o_dW * W.detach()).sum(1).abs().max()) <= 1e-12 * float(o_dW.abs().max())      # dW_j . w_j = 0


# ---- the restatements inside the bounds --------------------------------------------------------------------------------------
def _check_margin(z, r, labels, C, setting, grad_scale, dt, plant=None):
    """Compare the (possibly planted) fp32 restatement with the oracle; returns the names of the outputs outside their bound."""
    ref = mo.margin_ref(z, r, labels, C, *setting, grad_scale, dt)
    assert ref["margin_ok"]
    loss, dz, t, x = mo.margin_f32(z, r, labels, C, *setting, grad_scale, dt, plant=plant)
    N = z.shape[0]
    main = ref["main"].view(N)
    pairs = {"loss": (loss, ref["loss"], ref["e_loss"]), "dz": (dz, ref["dz"], ref["e_dz"]),
             "t": (t.double() * 2.0 ** -mo.ACC_GRAD_BITS, ref["t"], ref["e_t"]),
             "phi": (x["phi"], ref["phi"].view(N), ref["e_phi"].view(N)), "D": (x["D"], ref["D"].view(N), ref["e_D"].view(N)),
             "q": (torch.from_numpy(x["q"])[main], ref["q"].view(N)[main], ref["e_q"].view(N)[main])}      # q feeds the main branch only
    return [k for k, (got, want, bound) in pairs.items() if not eo.inside(torch.as_tensor(got), want, bound)], ref


@pytest.mark.parametrize("dt", [BF, HF])
@pytest.mark.parametrize("setting", mo.SETTINGS)
@pytest.mark.parametrize("N,C,ld,ld_d", mo.SHAPES)
def test_margin_restatement_stays_inside_the_bounds(N, C, ld, ld_d, setting, dt):
    z, r, labels = mo.margin_inputs(N, C, ld, seed=N, m_arc=setting[1])
    outside, ref = _check_margin(z, r, labels, C, setting, 1.0 / N, dt)
    assert outside == []
    main = ref["main"].view(N)
    assert bool(main[0]) and bool(main[2])                                          # every branch is hit on purpose
    if setting[1] > 0:
        assert not bool(main[1]) and not bool(main[3]) and not bool(main[4])
        assert float(ref["D"][2]) > 300                                             # ct = T: the derivative at its cap, cos + 2^9.5 sin
        assert float(ref["D"].max()) <= mo.constants(setting[1])[0] + 725 * mo.constants(setting[1])[1]
    else:
        assert bool(main.all())                                                     # th = -1 < -T: no fallback to take


@pytest.mark.parametrize("C,E", RNORM_SHAPES)
def test_rnorm_and_correction_restatements_stay_inside_the_bounds(C, E):
    w = mo.rnorm_inputs(C, E, seed=C)
    ref, bound = mo.rnorm_ref(w)
    got = mo.rnorm_f32(w)
    assert eo.inside(got, ref, bound)
    assert float(got[2]) == 1.0 and float(got[1]) == float(np.float32(1.0) / np.sqrt(np.float32(mo.EPS)))
    assert not eo.inside(got * (1 + 8 * eo.U), ref, bound)                          # the bound is a few ulps, not a tolerance
    dw, w2, rn, t = mo.wgrad_fix_inputs(C, E, seed=E)
    ref, bound = mo.wgrad_fix_ref(dw, w2, rn, t)
    assert eo.inside(mo.wgrad_fix_f32(dw, w2, rn, t), ref, bound)
    assert not eo.inside(dw.double() - (rn.double().view(-1, 1) * t.double().view(-1, 1) * 2.0 ** -40) * w2.double(), ref, bound)   # r, not r^2


# ---- planted errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plant,hit", [("ge", "loss"), ("no_D", "dz"), ("no_r", "dz"), ("t_no_c", "t"), ("sub", "q")])
def test_planted_errors_fall_outside_the_bounds(plant, hit):
    N, C, ld, _ = mo.SHAPES[0]
    setting = mo.SETTINGS[0]                                                        # ArcFace: D != 1, th inside the clamp
    z, r, labels = mo.margin_inputs(N, C, ld, seed=N, m_arc=setting[1])
    for dt in (BF, HF):
        outside, _ = _check_margin(z, r, labels, C, setting, 1.0 / N, dt, plant=plant)
        assert hit in outside, (plant, outside)


# ---- settings ----------------------------------------------------------------------------------------------------------------
def test_check_loss_arguments_refuses_bad_margin_settings():
    from facenet_amd.train import check_loss_arguments
    net = types.SimpleNamespace(nrof_classes=19)
    base = (0.0, 0.95, 0.0, 1.0)
    check_loss_arguments(net, 6, "softmax", *base)
    check_loss_arguments(net, 6, "softmax", *base, margin_scale=64.0, margin_arc=0.5, margin_cos=0.0)
    check_loss_arguments(net, 6, "softmax", *base, margin_scale=30.0, margin_cos=0.35)
    check_loss_arguments(net, 6, "triplet", *base)
    for loss, kw in (("triplet", dict(margin_scale=30.0)), ("triplet", dict(margin_scale=30.0, margin_cos=0.35)),
                     ("softmax", dict(margin_scale=-1.0)), ("softmax", dict(margin_scale=30.0, margin_arc=-0.1)),
                     ("softmax", dict(margin_scale=30.0, margin_cos=-0.1)), ("softmax", dict(margin_scale=30.0, margin_arc=np.pi / 2)),
                     ("softmax", dict(margin_scale=30.0, margin_arc=2.0)), ("softmax", dict(margin_arc=0.5)),
                     ("softmax", dict(margin_cos=0.35)), ("softmax", dict(margin_scale=float("nan")))):
        with pytest.raises(ValueError):
            check_loss_arguments(net, 6, loss, *base, **kw)


def test_config_defaults_and_the_apps_key_passing():
    from facenet_amd.apps.train_softmax import _loss_key
    from facenet_amd.config import Config
    loss = load_config().loss
    assert loss.margin_scale == 0.0 and loss.margin_arc == 0.0 and loss.margin_cos == 0.0
    cfg = load_config(overrides={"loss": {"margin_scale": 30, "margin_cos": 0.35}})
    assert [_loss_key(cfg, k) for k in ("margin_scale", "margin_arc", "margin_cos", "center_alfa")] == [30, 0.0, 0.35, 0.95]
    bare = Config({"loss": {"alpha": 0.2}})                                         # a settings tree not built by load_config
    assert [_loss_key(bare, k) for k in ("margin_scale", "margin_arc", "margin_cos")] == [0.0, 0.0, 0.0]
