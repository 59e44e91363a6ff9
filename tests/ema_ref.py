"""NumPy specification of the weight average (tf.train.ExponentialMovingAverage as TrainSession(ema_decay=...) keeps it).  Test infrastructure only:
the product never imports it."""
import numpy as np


def decay_at(ema_decay, t):
    """Decay of the update whose 1-based count is ``t`` ([TF-sem] the num_updates rule): min(decay, (1 + t) / (10 + t)), in Python floats."""
    return min(float(ema_decay), (1.0 + t) / (10.0 + t))


def update(ema, w, one_minus_decay):
    """[TF-sem] assign_moving_average, variable -= (variable - value) * (1 - decay): three f32 operations, each rounded once."""
    ema, w, omd = np.asarray(ema, np.float32), np.asarray(w, np.float32), np.float32(one_minus_decay)
    with np.errstate(all='ignore'):          # NaN and inf propagate as IEEE says
        d = np.subtract(ema, w, dtype=np.float32)
        d = np.multiply(d, omd, dtype=np.float32)
        return np.subtract(ema, d, dtype=np.float32)


def run(w0, history, ema_decay):
    """Shadows after every step: they start at the initial parameters ``w0`` (no zero-debias); step t = 1, 2, ... averages ``history[t - 1]``
    (the parameters after that step's optimizer update) with decay_at(ema_decay, t).  Returns the list of shadow arrays, one per step."""
    ema = np.array(w0, np.float32, copy=True)
    out = []
    for t, w in enumerate(history, 1):
        ema = update(ema, w, np.float32(1.0 - decay_at(ema_decay, t)))
        out.append(ema)
    return out
