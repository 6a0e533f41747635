"""The update rules of train.optimizer besides Adam restated in fp32 NumPy, in the operation order written
next to opt_keras_kernel (facenet_amd/csrc/optim.hip), every operation an IEEE fp32 operation rounded on its own:

    g = G * grad_scale;  g = g + (2 * l2) * w                               on [0, n_decay)
    ADAGRAD   a = a + g * g;  w = w - (lr * g) / (sqrt(a) + eps)
    ADADELTA  ag = rho * ag + (1 - rho) * (g * g);  u = sqrt(av + eps) / sqrt(ag + eps) * g;  w = w - lr * u;
              av = rho * av + (1 - rho) * (u * u)
    RMSPROP   ms = rho * ms + (1 - rho) * (g * g);  mom = mu * mom + (lr * g) / sqrt(ms + eps);  w = w - mom
    MOM       acc = mu * acc - lr * g;  w = w + (mu * acc - lr * g)

``step64`` is the same recurrence in float64, the closed form the fp32 restatement is checked against.  The constants come
from the one table of them, ``facenet_amd.train.OPTIMIZERS``."""
import numpy as np

from facenet_amd.train import OPTIMIZERS

F = np.float32
RULES = ("ADAGRAD", "ADADELTA", "RMSPROP", "MOM")


def initial_slots(name, n):
    return [np.full(n, init, F) for _, init in OPTIMIZERS[name].slots]


def gradient(G, w, grad_scale=1.0, l2=0.0, n_decay=0):
    g = np.asarray(G, F) * F(grad_scale)
    g[:n_decay] = g[:n_decay] + (F(2.0) * F(l2)) * np.asarray(w, F)[:n_decay]
    return g


def step(name, w, G, slots, lr, grad_scale=1.0, l2=0.0, n_decay=0):
    """One fp32 step of rule `name`: (new w, [new slots])."""
    r = OPTIMIZERS[name]
    w = np.asarray(w, F)
    g = gradient(G, w, grad_scale, l2, n_decay)
    lr, rho, mu, eps = F(lr), F(r.rho), F(r.momentum), F(r.epsilon)
    one_minus_rho = F(1.0) - rho
    s = [np.asarray(x, F) for x in slots]
    if name == "ADAGRAD":
        a = s[0] + g * g
        return w - (lr * g) / (np.sqrt(a) + eps), [a]
    if name == "ADADELTA":
        ag = rho * s[0] + one_minus_rho * (g * g)
        u = np.sqrt(s[1] + eps) / np.sqrt(ag + eps) * g
        w = w - lr * u
        return w, [ag, rho * s[1] + one_minus_rho * (u * u)]
    if name == "RMSPROP":
        ms = rho * s[0] + one_minus_rho * (g * g)
        mom = mu * s[1] + (lr * g) / np.sqrt(ms + eps)
        return w - mom, [ms, mom]
    if name == "MOM":
        st = lr * g
        acc = mu * s[0] - st
        return w + (mu * acc - st), [acc]
    raise ValueError(name)


def step64(name, w, G, slots, lr, grad_scale=1.0, l2=0.0, n_decay=0):
    """The same rule in float64 from the same (fp32-representable) constants."""
    r = OPTIMIZERS[name]
    f = lambda x: np.float64(np.float32(x))
    w = np.asarray(w, np.float64)
    g = np.asarray(G, np.float64) * f(grad_scale)
    g[:n_decay] += 2.0 * f(l2) * w[:n_decay]
    lr, rho, mu, eps = f(lr), f(r.rho), f(r.momentum), f(r.epsilon)
    s = [np.asarray(x, np.float64) for x in slots]
    if name == "ADAGRAD":
        a = s[0] + g ** 2
        return w - lr * g / (np.sqrt(a) + eps), [a]
    if name == "ADADELTA":
        ag = rho * s[0] + (1 - rho) * g ** 2
        u = np.sqrt(s[1] + eps) / np.sqrt(ag + eps) * g
        return w - lr * u, [ag, rho * s[1] + (1 - rho) * u ** 2]
    if name == "RMSPROP":
        ms = rho * s[0] + (1 - rho) * g ** 2
        mom = mu * s[1] + lr * g / np.sqrt(ms + eps)
        return w - mom, [ms, mom]
    if name == "MOM":
        acc = mu * s[0] - lr * g
        return w + mu * acc - lr * g, [acc]
    raise ValueError(name)
