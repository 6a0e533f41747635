"""The moving average of the weights restated in fp32 NumPy: TF1's
``ExponentialMovingAverage(decay, num_updates=t)`` with ``zero_debias=False``, as ``fn_adam_keras_ema`` applies it after Adam:

    d = min(decay, (1 + t) / (10 + t))        t = Keras ``iterations`` after the step's tick (>= 1)
    s = s - (s - w) * (1 - d)

every operation an IEEE fp32 operation rounded on its own (no fused multiply-add)."""
import numpy as np

F = np.float32


def decay_at(t: int, decay: float) -> np.float32:
    tf = F(t)
    return np.minimum(F(decay), (F(1.0) + tf) / (F(10.0) + tf))


def update(shadow: np.ndarray, w: np.ndarray, t: int, decay: float) -> np.ndarray:
    s, w = np.asarray(shadow, F), np.asarray(w, F)
    one_minus_d = F(1.0) - decay_at(t, decay)
    return (s - (s - w) * one_minus_d).astype(F)


def switch_point(decay: float) -> int:
    """The first t at which d stops following (1 + t) / (10 + t) in fp32 and equals the configured decay."""
    d = F(decay)
    ramp = lambda t: (F(1.0) + F(t)) / (F(10.0) + F(t))
    lo, hi = 1, 1
    while ramp(hi) < d:            # the fp32 ramp is non-decreasing in t: bracket, then bisect
        lo, hi = hi, 2 * hi
    while lo < hi:
        mid = (lo + hi) // 2
        if ramp(mid) < d:
            lo = mid + 1
        else:
            hi = mid
    return lo
