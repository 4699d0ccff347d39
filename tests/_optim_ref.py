"""The optimizer kernels of kge_amd/csrc/optim.hip restated in plain numpy for the tests (no torch, no GPU).

float32 (the default `dtype`): op by op, every intermediate an np.float32 array, in the order the kernels' code writes
the operations -- the library is built with -ffp-contract=off, IEEE division and square root, denormals kept, so a
kernel must give these bits.  The scalar arguments are rounded to float32 the way ctypes hands a Python float to a
`float` parameter of the C ABI; Adam's `1 - beta` is formed in double and then rounded (api.hip: kge_adam_step).

float64 (`dtype=np.float64`, or the `*64` names): the same formulas with arrays and scalars in double -- what
torch.optim's CPU optimizers compute on float64 parameters (tests/test_optim_ref_cpu.py holds them to a few float64 ulp).

  adagrad          kge_adagrad_step, a segment of kge_adagrad_step_multi
  adagrad_penalty  a segment of kge_adagrad_step_multi_penalty (kind 0 none, 1 lp with p in 1..3, 2 n3 over complex pairs)
  adam             kge_adam_step
  adagrad_rows     kge_adagrad_step_rows
  bf16_rne_bits    the bf16 copy the kernels write beside the new parameter (common.hpp: f32_to_bf16)
"""
import numpy as np

_QUIET = dict(over="ignore", under="ignore", invalid="ignore", divide="ignore")


def _flat(x, dtype):
    return np.array(x, dtype=dtype).reshape(-1)


def _step(p, ge, s, minus_clr, weight_decay, eps):
    """ge = ge + wd * p (if wd != 0);  s = s + ge * ge;  p = p + (minus_clr * ge) / (sqrt(s) + eps)"""
    if weight_decay != 0:
        ge = ge + weight_decay * p
    s = s + ge * ge
    p = p + (minus_clr * ge) / (np.sqrt(s) + eps)
    return p, s


def adagrad(param, grad, sum, minus_clr, weight_decay, eps, dtype=np.float32):
    """-> (param, sum) after the step."""
    p, g, s = _flat(param, dtype), _flat(grad, dtype), _flat(sum, dtype)
    minus_clr, weight_decay, eps = dtype(minus_clr), dtype(weight_decay), dtype(eps)
    with np.errstate(**_QUIET):
        return _step(p, g, s, minus_clr, weight_decay, eps)


def _thread_partials(terms, dtype):
    """One partial per thread: its (up to) four terms added in element order, starting from 0, in `dtype`."""
    n = terms.size
    pad = np.zeros((-n) % 4, dtype=dtype)  # + 0 leaves a non-negative partial as it is
    t = np.concatenate([terms.astype(dtype), pad]).reshape(-1, 4)
    v = np.zeros(t.shape[0], dtype=dtype)
    for e in range(4):
        v = v + t[:, e]
    return v


def adagrad_penalty(param, grad, sum, minus_clr, weight_decay, eps, kind, p, weight, row_dim, dtype=np.float32):
    """-> (param, sum, value).  The penalty's gradient -- lp: w * sign(x) |x|^(p-1) written as w or -w or 0 (p = 1),
    w * x (p = 2), w * (x * a) with a = |x| (p = 3); n3: w * (z * re), w * (z * im) with z = sqrt(re*re + im*im + 1e-14f),
    im = re's column + row_dim / 2 -- is added to the gradient FIRST (before weight decay), then the step as in adagrad.

    value = sum |x|^p (p = 3: (a*a)*a; n3: (z*z)*z) of the pre-step parameters, summed as the kernel sums it: every
    thread adds its own terms (4 consecutive elements, 4 consecutive complex pairs, or the up-to-3 tail elements) in
    `dtype` in element order, the per-thread partials are then added in float64 (here: in array order; the kernel: by
    wave, workgroup and atomic add -- the same non-negative terms in another order).

    kind 0 inside a penalty launch: the four-element body adds a penalty gradient of +0 to the gradient (-0 becomes
    +0), the scalar tail does not; both are restated."""
    x, g, s = _flat(param, dtype), _flat(grad, dtype), _flat(sum, dtype)
    minus_clr, weight_decay, eps, w = dtype(minus_clr), dtype(weight_decay), dtype(eps), dtype(weight)
    n = x.size
    with np.errstate(**_QUIET):
        if kind == 0:
            body = n - n % 4
            ge = g.copy()
            ge[:body] = g[:body] + dtype(0)
            value = 0.0
        elif kind == 1:
            a = np.abs(x)
            if p == 1:
                terms = a
                pg = np.where(x > 0, w, np.where(x < 0, -w, dtype(0))).astype(dtype)
            elif p == 2:
                terms = x * x
                pg = w * x
            elif p == 3:
                terms = (a * a) * a
                pg = w * (x * a)
            else:
                raise ValueError(p)
            ge = g + pg
            value = float(_thread_partials(terms, dtype).astype(np.float64).sum())
        elif kind == 2:
            h = row_dim // 2
            assert row_dim % 8 == 0 and n % row_dim == 0
            xr = x.reshape(-1, 2, h)
            re, im = xr[:, 0, :], xr[:, 1, :]
            z = np.sqrt(re * re + im * im + dtype(1e-14))
            terms = (z * z) * z
            pg = np.stack([w * (z * re), w * (z * im)], axis=1).reshape(-1)
            ge = g + pg
            value = float(_thread_partials(terms.reshape(-1), dtype).astype(np.float64).sum())
        else:
            raise ValueError(kind)
        pn, sn = _step(x, ge, s, minus_clr, weight_decay, eps)
    return pn, sn, value


def adam(param, grad, m1, m2, step_size, bc2_sqrt, beta1, beta2, weight_decay, eps, dtype=np.float32):
    """-> (param, m1, m2):
        g  = g + wd * p                     (if wd != 0)
        m1 = m1 + (g - m1) * (1 - beta1)
        m2 = m2 * beta2 + ((1 - beta2) * g) * g
        p  = p + (-step_size) * (m1 / (sqrt(m2) / bc2_sqrt + eps))"""
    p, g, a, b = _flat(param, dtype), _flat(grad, dtype), _flat(m1, dtype), _flat(m2, dtype)
    step_size, bc2_sqrt, weight_decay, eps = dtype(step_size), dtype(bc2_sqrt), dtype(weight_decay), dtype(eps)
    omb1, omb2, beta2 = dtype(1.0 - float(beta1)), dtype(1.0 - float(beta2)), dtype(beta2)
    with np.errstate(**_QUIET):
        if weight_decay != 0:
            g = g + weight_decay * p
        a = a + (g - a) * omb1
        b = b * beta2 + (omb2 * g) * g
        denom = np.sqrt(b) / bc2_sqrt + eps
        p = p + (-step_size) * (a / denom)
    return p, a, b


def adagrad_rows(param, grows, sum, rows, minus_clr, eps, dtype=np.float32):
    """param, sum: [E, dim]; grows: [len(rows), dim], row r the gradient of table row rows[r] (unique ids).
    -> (param, sum) with the listed rows stepped (no weight decay), every other row as it was."""
    p, s = np.array(param, dtype=dtype), np.array(sum, dtype=dtype)
    g = np.array(grows, dtype=dtype).reshape(len(rows), -1)
    rows = np.asarray(rows, dtype=np.int64)
    assert np.unique(rows).size == rows.size
    minus_clr, eps = dtype(minus_clr), dtype(eps)
    with np.errstate(**_QUIET):
        se = s[rows] + g * g
        pe = p[rows] + (minus_clr * g) / (np.sqrt(se) + eps)
    s[rows] = se
    p[rows] = pe
    return p, s


def bf16_rne_bits(x):
    """float32 array -> uint16 bf16 bits, round to nearest even; NaN -> a quiet NaN (sign and high payload kept)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    r = (u + (np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)  # (no wrap: not a NaN)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x0040), r).astype(np.uint16)


def adagrad64(*a, **k):
    return adagrad(*a, dtype=np.float64, **k)


def adagrad_penalty64(*a, **k):
    return adagrad_penalty(*a, dtype=np.float64, **k)


def adam64(*a, **k):
    return adam(*a, dtype=np.float64, **k)


def adagrad_rows64(*a, **k):
    return adagrad_rows(*a, dtype=np.float64, **k)
