"""tests/_sparse_adam_ref.py without a GPU: the float32 restatement of kge_sparse_adam_step_touched against
torch.optim.SparseAdam on coalesced sparse gradients, and its clock against the closed form."""
import numpy as np
import pytest
import torch

import _sparse_adam_ref as sar
import _touched_ref as tr


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("lr,betas,eps", [(1e-3, (0.9, 0.999), 1e-8), (0.05, (0.5, 0.99), 1e-6)])
def test_restatement_equals_torch_sparse_adam_bit_for_bit(lr, betas, eps):
    """Three steps with changing row sets (duplicated ids in the uncoalesced gradient, a row that comes back, a row
    whose gradient is exactly zero).  BIT EQUALITY holds and is required: torch's CPU step is a sequence of separate
    element-wise float32 kernels (sub, mul by a scalar rounded to float32, add, pow(2) = g * g, sqrt, div), none of
    which can contract with its neighbour, and -step_size is rounded to float32 once, as the clock does -- the
    restatement's operations one for one.  The step size itself is float32(lr sqrt(1 - beta2 ** t) / (1 - beta1 ** t))
    in torch and a product recurrence in the clock; test_clock_is_the_closed_form holds the two together."""
    E, d = 70, 5
    gen = torch.Generator().manual_seed(5)
    w = torch.randn(E, d, generator=gen).requires_grad_(True)
    opt = torch.optim.SparseAdam([w], lr=lr, betas=betas, eps=eps)
    p = w.detach().numpy().copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    clock = sar.clock_seed(0, *betas)
    row_sets = [[3, 3, 31, 32, 64, 69], [0, 3, 33, 64, 64, 64], [3, 5, 69]]
    for step, rows in enumerate(row_sets):
        idx = torch.tensor(rows)
        vals = torch.randn(len(rows), d, generator=gen)
        if step == 1:
            vals[0] = 0.0  # row 0: present in the gradient, exactly zero
        w.grad = torch.sparse_coo_tensor(idx[None], vals, (E, d))
        dense = w.grad.coalesce().to_dense().numpy()  # the values the kernel finds in its persistent buffer
        before = p.copy()
        p, g, m, v, bm, _, clock = sar.step_touched(p, dense, m, v, tr.mark(rows, E), clock, lr, betas[0], betas[1], eps)
        opt.step()
        st = opt.state[w]
        assert (_bits(p) == _bits(w.detach().numpy())).all()
        assert (_bits(m) == _bits(st["exp_avg"].numpy())).all()
        assert (_bits(v) == _bits(st["exp_avg_sq"].numpy())).all()
        assert clock[0] == st["step"] == step + 1
        assert not g.any() and not bm.any()
        untouched = sorted(set(range(E)) - set(rows))
        assert (_bits(p[untouched]) == _bits(before[untouched])).all()


def test_a_marked_row_with_zero_gradient_moves_and_an_unmarked_row_does_not():
    E, d = 40, 4
    rng = np.random.default_rng(2)
    p = rng.standard_normal((E, d)).astype(np.float32)
    m = rng.standard_normal((E, d)).astype(np.float32)
    v = rng.random((E, d)).astype(np.float32)
    g = np.zeros((E, d), np.float32)
    g[9] = 1.0  # row 9 has a gradient but is NOT marked
    clock = sar.clock_seed(4, 0.9, 0.999)
    pn, gn, mn, vn, bm, _, clock = sar.step_touched(p, g, m, v, tr.mark([7, 33], E), clock, 1e-2, 0.9, 0.999, 1e-8)
    for r in (7, 33):  # marked, gradient exactly zero: the moments decay and the parameter moves
        assert (mn[r] != m[r]).all() and (vn[r] != v[r]).all() and (pn[r] != p[r]).all()
        assert (np.abs(mn[r]) < np.abs(m[r])).all() and (vn[r] < v[r]).all()
    rest = [r for r in range(E) if r not in (7, 33)]
    for a, b in ((pn, p), (mn, m), (vn, v), (gn, g)):
        assert (_bits(a[rest]) == _bits(b[rest])).all()
    assert clock[0] == 5 and not bm.any()
    # the float64 version: the same rows, values within float32 rounding of the float32 run
    p64, _, m64, v64 = sar.step_touched_f64(p, g, m, v, tr.mark([7, 33], E), 5, 1e-2, 0.9, 0.999, 1e-8)
    assert np.abs(p64 - pn).max() < 1e-5 and (p64[rest] == p[rest]).all()


@pytest.mark.parametrize("beta1,beta2,lr", [(0.9, 0.999, 1e-3), (0.5, 0.99, 0.05), (0.0, 0.9999, 0.2)])
def test_clock_is_the_closed_form(beta1, beta2, lr):
    """t = 1..1000.  The record's powers are a product recurrence, Python's beta ** t is libm's pow: each of the t - 1
    multiplications rounds once (relative 2^-53) and pow is within one unit in the last place of beta^t, so
    |beta_pow - beta ** t| <= (t + 1) 2^-53 beta ** t, and since beta_pow <= 1 / 2 or 1 - beta_pow is exact up to one
    rounding, |(1 - beta_pow) - (1 - beta ** t)| <= (t + 2) 2^-53: asserted.  The float32 step size the update reads
    must be the very float32 torch computes, float32(lr * sqrt(1 - beta2 ** t) / (1 - beta1 ** t)): asserted bit for
    bit (the two float64 values differ by parts in 10^13 at most, a float32 rounding boundary between them would be a
    one-in-a-million event per t; none exists for these betas)."""
    c = sar.clock_seed(0, beta1, beta2)
    for t in range(1, 1001):
        c = sar.clock_tick(c, lr, beta1, beta2)
        assert c[0] == t
        for got, beta in ((c[1], beta1), (c[2], beta2)):
            assert abs((1.0 - got) - (1.0 - beta ** t)) <= (t + 2) * 2.0 ** -53
        want = np.float32(lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t))
        assert c[3].view(np.uint32) == want.view(np.uint32), t
        assert c[4].view(np.uint32) == np.float32(np.sqrt(1.0 - beta2 ** t)).view(np.uint32), t
    assert len(sar.clock_bytes(c)) == 32
    # a record restored at T continues the recurrence from Python's power
    r = sar.clock_tick(sar.clock_seed(7, beta1, beta2), lr, beta1, beta2)
    assert r[0] == 8 and r[3].view(np.uint32) == np.float32(lr * np.sqrt(1.0 - beta2 ** 8) / (1.0 - beta1 ** 8)).view(np.uint32)
