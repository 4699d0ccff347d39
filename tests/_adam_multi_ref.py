"""kge_adam_step_multi (kge_amd/csrc/optim.hip: adam_clock_kernel, adam_multi_kernel) restated in plain numpy for the
tests (no torch, no GPU).

The clock: a record (t, beta1_pow, beta2_pow, step_size, bias_correction2_sqrt); a tick is, in float64 with IEEE
division and square root,
    t += 1;  beta1_pow *= beta1;  beta2_pow *= beta2
    step_size = float32(lr / (1 - beta1_pow));  bias_correction2_sqrt = float32(sqrt(1 - beta2_pow))
A fresh record is (T, beta1 ** T, beta2 ** T, 0, 0) with Python's float power, as kge_amd.optim.Adam seeds it.

The update of a segment: the penalty's gradient (as _optim_ref.adagrad_penalty restates it for kinds 1 and 2; a segment
of kind 0 is the plain update, nothing is added to its gradient) added to the gradient in float32, then
_optim_ref.adam with the record's two floats.  The penalty's value: float32 per-thread partials (four consecutive
elements or complex pairs per thread) added in float64."""
import struct

import numpy as np

import _optim_ref as orf


def clock_seed(T, beta1, beta2):
    """-> (t, beta1_pow, beta2_pow, step_size, bias_correction2_sqrt) of a fresh record at step count T."""
    return (int(T), float(beta1) ** int(T), float(beta2) ** int(T), np.float32(0), np.float32(0))


def clock_tick(clock, lr, beta1, beta2):
    t, b1, b2, _, _ = clock
    b1 = np.float64(b1) * np.float64(beta1)
    b2 = np.float64(b2) * np.float64(beta2)
    with np.errstate(**orf._QUIET):
        step_size = np.float32(np.float64(lr) / (np.float64(1.0) - b1))
        bc2_sqrt = np.float32(np.sqrt(np.float64(1.0) - b2))
    return (t + 1, float(b1), float(b2), step_size, bc2_sqrt)


def clock_bytes(clock):
    """The 32 bytes of the record (kge_adam_clock: int64, two doubles, two floats; little endian)."""
    return struct.pack("<qddff", clock[0], clock[1], clock[2], float(clock[3]), float(clock[4]))


def penalty_gradient(param, kind, p, weight, row_dim):
    """-> (the term's gradient per element in float32, or None for kind 0; sum |x|^p (sum |z|^3) as the kernel sums
    it up to the order of the float64 additions)."""
    dtype = np.float32
    x, w = orf._flat(param, dtype), dtype(weight)
    with np.errstate(**orf._QUIET):
        if kind == 0:
            return None, 0.0
        if kind == 1:
            a = np.abs(x)
            if p == 1:
                terms, pg = a, np.where(x > 0, w, np.where(x < 0, -w, dtype(0))).astype(dtype)
            elif p == 2:
                terms, pg = x * x, w * x
            elif p == 3:
                terms, pg = (a * a) * a, w * (x * a)
            else:
                raise ValueError(p)
        elif kind == 2:
            h = row_dim // 2
            assert row_dim % 8 == 0 and x.size % row_dim == 0
            xr = x.reshape(-1, 2, h)
            re, im = xr[:, 0, :], xr[:, 1, :]
            z = np.sqrt(re * re + im * im + dtype(1e-14))
            terms = ((z * z) * z).reshape(-1)
            pg = np.stack([w * (z * re), w * (z * im)], axis=1).reshape(-1)
        else:
            raise ValueError(kind)
        return pg, float(orf._thread_partials(terms, dtype).astype(np.float64).sum())


def adam_multi_segment(param, grad, m1, m2, clock, lr, beta1, beta2, weight_decay, eps, kind=0, p=0, weight=0.0,
                       row_dim=0):
    """One non-empty segment of a kge_adam_step_multi call -> (param, m1, m2, value, clock) after it."""
    clock = clock_tick(clock, lr, beta1, beta2)
    g = orf._flat(grad, np.float32)
    pg, value = penalty_gradient(param, kind, p, weight, row_dim)
    if pg is not None:
        with np.errstate(**orf._QUIET):
            g = g + pg
    pn, a, b = orf.adam(param, g, m1, m2, clock[3], clock[4], beta1, beta2, weight_decay, eps)
    return pn, a, b, value, clock
