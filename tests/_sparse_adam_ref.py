"""kge_sparse_adam_step_touched (include/kge_amd.h; kge_amd/csrc/touched.hip) restated in plain numpy for the tests (no
torch, no GPU).

The clock: a kge_adam_clock record (t, beta1_pow, beta2_pow, step_size, bias_correction2_sqrt); a tick is, in float64
with IEEE division and square root,
    t += 1;  beta1_pow *= beta1;  beta2_pow *= beta2;  root = sqrt(1 - beta2_pow)
    step_size = float32((lr * root) / (1 - beta1_pow));  bias_correction2_sqrt = float32(root)
A fresh record is (T, beta1 ** T, beta2 ** T, 0, 0) with Python's float power, as kge_amd.optim.SparseAdam seeds it.
The clock ticks once per call, whatever the bitmap holds.

The update (`step_touched`, float32: every operation rounded on its own, in the header's order), for every set bit
r < num_rows, with omb1 = float32(1 - beta1), omb2 = float32(1 - beta2) (the difference formed in float64):
    u1 = (g - m) * omb1;  m = m + u1;  u2 = (g * g - v) * omb2;  v = v + u2
    p = p + (-step_size) * (m / (sqrt(v) + eps));  copy = bf16 bits of p (RNE)
then grad[r] = 0 and the whole bitmap zero.  Rows whose bit is clear are not looked at.  `step_touched_f64` is the same
in float64 with nothing rounded to float32 (step size included).

`error_step`: how far two runs of that update can drift apart -- see its docstring; tests/test_gpu_sparse_adam_model.py
holds the GPU model step to torch's CPU step with it."""
import struct

import numpy as np

from _touched_ref import _QUIET, bf16_rne_bits, marked_rows

U32 = 2.0 ** -24  # unit roundoff of float32


def clock_seed(T, beta1, beta2):
    """-> (t, beta1_pow, beta2_pow, step_size, bias_correction2_sqrt) of a fresh record at step count T."""
    return (int(T), float(beta1) ** int(T), float(beta2) ** int(T), np.float32(0), np.float32(0))


def clock_tick(clock, lr, beta1, beta2):
    t, b1, b2, _, _ = clock
    b1 = np.float64(b1) * np.float64(beta1)
    b2 = np.float64(b2) * np.float64(beta2)
    with np.errstate(**_QUIET):
        root = np.sqrt(np.float64(1.0) - b2)
        step_size = np.float32((np.float64(lr) * root) / (np.float64(1.0) - b1))
    return (t + 1, float(b1), float(b2), step_size, np.float32(root))


def clock_bytes(clock):
    """The 32 bytes of the record (kge_adam_clock: int64, two doubles, two floats; little endian)."""
    return struct.pack("<qddff", clock[0], clock[1], clock[2], float(clock[3]), float(clock[4]))


def _step(dtype, param, grad, m1, m2, bitmap, step_size, beta1, beta2, eps, copy):
    p, g, a, b = (np.array(x, dtype=dtype) for x in (param, grad, m1, m2))
    c = None if copy is None else np.array(copy, dtype=np.uint16)
    omb1, omb2, eps = dtype(1.0 - float(beta1)), dtype(1.0 - float(beta2)), dtype(eps)
    neg = -dtype(step_size)
    with np.errstate(**_QUIET):
        for r in marked_rows(bitmap, p.shape[0]):
            ge = g[r]
            u1 = (ge - a[r]) * omb1
            ae = a[r] + u1
            u2 = (ge * ge - b[r]) * omb2
            be = b[r] + u2
            pe = p[r] + neg * (ae / (np.sqrt(be) + eps))
            a[r], b[r], p[r] = ae, be, pe
            g[r] = dtype(0)
            if c is not None:
                c[r] = bf16_rne_bits(pe.astype(np.float32))
    return p, g, a, b, np.zeros_like(np.asarray(bitmap, dtype=np.uint32)), c


def step_touched(param, grad, exp_avg, exp_avg_sq, bitmap, clock, lr, beta1, beta2, eps, copy=None):
    """One kge_sparse_adam_step_touched call.  param, grad, exp_avg, exp_avg_sq: float32 [E, dim]; bitmap: uint32 words;
    clock: the record before the call; copy: uint16 [E, dim] or None.
    -> (param, grad, exp_avg, exp_avg_sq, bitmap, copy, clock) after the call (new arrays)."""
    clock = clock_tick(clock, lr, beta1, beta2)
    return _step(np.float32, param, grad, exp_avg, exp_avg_sq, bitmap, clock[3], beta1, beta2, eps, copy) + (clock,)


def step_touched_f64(param, grad, exp_avg, exp_avg_sq, bitmap, t, lr, beta1, beta2, eps):
    """The same update in float64 at step count `t` (after the tick), step size lr sqrt(1 - beta2^t) / (1 - beta1^t)
    unrounded -> (param, grad, exp_avg, exp_avg_sq)."""
    step_size = float(lr) * np.sqrt(1.0 - float(beta2) ** t) / (1.0 - float(beta1) ** t)
    return _step(np.float64, param, grad, exp_avg, exp_avg_sq, bitmap, step_size, beta1, beta2, eps, None)[:4]


def error_step(g, dg, m, dm, v, dv, p_new, dp, t, lr, beta1, beta2, eps):
    """How far a float32 run of one update can be from the float64 run `step_touched_f64`, element by element.

    Given, for the marked rows, the float64 run's inputs g, m, v (before the step), its new parameter p_new, and bounds
    dg, dm, dv, dp on |float32 run - float64 run| of gradient, moments and parameter BEFORE the step -> (dm', dv', dp')
    after it.  Every line is an inequality of real arithmetic plus the standard model fl(x op y) = (x op y)(1 + e),
    |e| <= u = 2^-24, for the float32 run's own operations; nothing is fitted.  With c1 = 1 - beta1, c2 = 1 - beta2,
    m' = m + c1 (g - m), v' = v + c2 (g^2 - v), D = sqrt(v') + eps, s = the step size:
      dm' = (1 - c1) dm + c1 dg + 4 u (|g| + dg + |m| + dm)
            -- the map is linear in (m, g); u1 takes a subtraction, a multiplication by a rounded constant and the
               sum m + u1 a third rounding, each on quantities below |g| + |m| (of the float32 run: + dg + dm)
      dv' = (1 - c2) dv + c2 (2 |g| dg + dg^2) + 5 u ((|g| + dg)^2 + v + dv)
            -- g^2 moves by at most 2 |g| dg + dg^2; four roundings and the rounded constant on g^2 + v
      dD  = min(sqrt(dv'), dv' / sqrt(v')) + 2 u (D + dD)
            -- |sqrt a - sqrt b| <= sqrt|a - b| and <= |a - b| / max(sqrt a, sqrt b); the square root and the sum round
      D_lo = max(D - dD, eps)    (v >= 0 in either run, so either denominator is at least eps)
      dq  = dm' / D_lo + |m'| dD / (D D_lo)
            -- |m1/D1 - m2/D2| <= |m1 - m2| / D1 + |m2| |D1 - D2| / (D1 D2)
      dp' = dp + s (dq + 4 u (|m'| + dm') / D_lo) + u (|p_new| + dp + s (|m'| + dm') / D_lo)
            -- the quotient, the product with the float32 step size (itself rounded once, after a float64 recurrence
               whose error is below u by orders of magnitude: 2 u in all) and the final sum round
    Two float32 runs (the kernel's and torch's) are each within these bounds of the float64 run when each one's
    gradient is within dg of the float64 gradient: they differ by at most twice the bounds."""
    u = U32
    g, dg, m, dm, v, dv, p_new, dp = (np.asarray(x, dtype=np.float64) for x in (g, dg, m, dm, v, dv, p_new, dp))
    c1, c2 = 1.0 - float(beta1), 1.0 - float(beta2)
    s = float(lr) * np.sqrt(1.0 - float(beta2) ** t) / (1.0 - float(beta1) ** t)
    m_new = m + c1 * (g - m)
    v_new = v + c2 * (g * g - v)
    D = np.sqrt(v_new) + eps
    dm_new = (1.0 - c1) * dm + c1 * dg + 4 * u * (np.abs(g) + dg + np.abs(m) + dm)
    dv_new = (1.0 - c2) * dv + c2 * (2 * np.abs(g) * dg + dg * dg) + 5 * u * ((np.abs(g) + dg) ** 2 + v + dv)
    with np.errstate(**_QUIET):
        dD = np.minimum(np.sqrt(dv_new), np.where(v_new > 0, dv_new / np.sqrt(v_new), np.inf))
    dD = dD + 2 * u * (D + dD)
    D_lo = np.maximum(D - dD, eps)
    dq = dm_new / D_lo + np.abs(m_new) * dD / (D * D_lo)
    big = (np.abs(m_new) + dm_new) / D_lo
    dp_new = dp + s * (dq + 4 * u * big) + u * (np.abs(p_new) + dp + s * big)
    return dm_new, dv_new, dp_new
