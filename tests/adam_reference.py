"""A numpy restatement of include/bloomscene_adam.h: the Adam step per element in fp32, in the header's order, every
operation rounded once, and bpow in python floats (IEEE doubles) with the header's order of multiplications.  Test
infrastructure only: the product never imports it."""
import math

import numpy as np

F32 = np.float32


def bpow(b, t):
    """b^t for t >= 0: binary exponentiation, least significant bit first (the header's definition)."""
    r, x, t = 1.0, float(b), int(t)
    while t > 0:
        if t & 1:
            r = r * x
        t >>= 1
        if t > 0:
            x = x * x
    return r


def step_scalars(lr, beta1, beta2, t):
    """-> (ss, bc2s): each formed in fp64 and rounded once to fp32."""
    with np.errstate(all="ignore"):
        ss = F32(np.float64(lr) / np.float64(1.0 - bpow(beta1, t)))
    return ss, F32(math.sqrt(1.0 - bpow(beta2, t)))


def adam_step(p, g, m, v, lr, t, beta1=0.9, beta2=0.999, eps=1e-8):
    """One step, t >= 1 being the step taken.  -> (p', m', v'), new fp32 arrays; the inputs are left unchanged."""
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    b2, w1, w2, e = F32(beta2), F32(1.0 - beta1), F32(1.0 - beta2), F32(eps)
    ss, bc2s = step_scalars(lr, beta1, beta2, t)
    with np.errstate(all="ignore"):
        m1 = m + w1 * (g - m)
        v1 = b2 * v + w2 * (g * g)
        den = np.sqrt(v1) / bc2s + e
        p1 = p - ss * (m1 / den)
    assert p1.dtype == m1.dtype == v1.dtype == F32
    return p1, m1, v1


def adam_step_f64(p, g, m, v, lr, t, beta1=0.9, beta2=0.999, eps=1e-8):
    """The same step in float64 with the mathematical beta ** t: the yardstick distances are measured from."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        m1 = beta1 * m + (1.0 - beta1) * g
        v1 = beta2 * v + (1.0 - beta2) * g * g
        den = np.sqrt(v1) / math.sqrt(1.0 - beta2 ** t) + eps
        p1 = p - lr / (1.0 - beta1 ** t) * (m1 / den)
    return p1, m1, v1


def bits_equal(a, b):
    """Bit for bit, except that any NaN equals any NaN (the header leaves sign and payload of a NaN open)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))
