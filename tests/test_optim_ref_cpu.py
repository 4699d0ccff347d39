"""tests/_optim_ref.py, the numpy restatement of the optimizer kernels that tests/test_gpu_optim_exact.py holds the
MI355X to bit for bit, verified without a GPU:

* its float64 form against torch's own CPU optimizers on float64 parameters (Adagrad with lr_decay / weight decay /
  initial accumulator, Adagrad's sparse path, Adam) over several steps: a few float64 ulp;
* its float32 form against the float64 form on the same inputs, with torch's float32 CPU optimizer as the yardstick;
* the penalty's value and gradient against float64 autograd of the reference's term;
* the bf16 bit recipe against torch's cast over every upper half of a float32."""
import numpy as np
import pytest
import torch

import _optim_ref as orf

RTOL64 = 1e-13  # both sides float64, a handful of operations per element: a few ulp (2.2e-16 each)


def _close64(got, want, what, before=None):
    """Relative to max(|result|, |value before the step|): the last operation adds the update to the old value, both
    carrying the rounding of what came before, so where the two nearly cancel the error stays at THEIR scale."""
    got, want = np.asarray(got), np.asarray(want)
    scale = np.abs(want) if before is None else np.maximum(np.abs(want), np.abs(before))
    bad = np.abs(got - want) > RTOL64 * scale
    assert not bad.any(), (what, int(bad.sum()), float((np.abs(got - want) / np.maximum(scale, 1e-300)).max()))


@pytest.mark.parametrize("lr_decay,weight_decay,init_acc", [(0.0, 0.0, 0.0), (0.01, 1e-3, 0.1), (0.3, 0.0, 2.0)])
def test_float64_adagrad_is_torch_adagrad(lr_decay, weight_decay, init_acc):
    rng = np.random.default_rng(0)
    n, lr, eps = 301, 0.1, 1e-10
    p0 = rng.standard_normal(n)
    t = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adagrad([t], lr=lr, lr_decay=lr_decay, weight_decay=weight_decay,
                              initial_accumulator_value=init_acc, eps=eps)
    p, s = p0.copy(), np.full(n, init_acc)
    for step in range(1, 5):
        g = rng.standard_normal(n)
        t.grad = torch.tensor(g)
        opt.step()
        minus_clr = -lr / (1.0 + (step - 1.0) * lr_decay)  # what kge_amd.optim.Adagrad hands to the kernel
        before = p
        p, s = orf.adagrad64(p, g, s, minus_clr, weight_decay, eps)
        _close64(p, t.detach().numpy(), f"param, step {step}", before)
        _close64(s, opt.state[t]["sum"].numpy(), f"sum, step {step}")


def test_float64_adagrad_rows_is_torch_sparse_adagrad():
    rng = np.random.default_rng(1)
    E, d, lr, lr_decay, eps = 40, 7, 0.1, 0.01, 1e-10
    p0 = rng.standard_normal((E, d))
    t = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adagrad([t], lr=lr, lr_decay=lr_decay, eps=eps)
    p, s = p0.copy(), np.zeros((E, d))
    for step in range(1, 5):
        rows = rng.permutation(E)[:9]  # unsorted, unique
        if step == 2:
            rows = np.concatenate([[E - 1, 0], 1 + rng.permutation(E - 2)[:7]])
        g = rng.standard_normal((rows.size, d))
        t.grad = torch.sparse_coo_tensor(torch.tensor(rows)[None], torch.tensor(g), (E, d))
        opt.step()
        before = p
        p, s = orf.adagrad_rows64(p, g, s, rows, -lr / (1.0 + (step - 1.0) * lr_decay), eps)
        _close64(p, t.detach().numpy(), f"param, step {step}", before)
        _close64(s, opt.state[t]["sum"].numpy(), f"sum, step {step}")


@pytest.mark.parametrize("betas,weight_decay", [((0.9, 0.999), 0.0), ((0.3, 0.99), 1e-3)])
def test_float64_adam_is_torch_adam(betas, weight_decay):
    rng = np.random.default_rng(2)
    n, lr, eps = 301, 0.05, 1e-8
    p0 = rng.standard_normal(n)
    t = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([t], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    p, m1, m2 = p0.copy(), np.zeros(n), np.zeros(n)
    for step in range(1, 6):
        g = rng.standard_normal(n)
        t.grad = torch.tensor(g)
        opt.step()
        step_size = lr / (1.0 - betas[0] ** step)  # kge_amd.optim.Adam's launch arguments
        bc2_sqrt = (1.0 - betas[1] ** step) ** 0.5
        before, before1 = p, m1
        p, m1, m2 = orf.adam64(p, g, m1, m2, step_size, bc2_sqrt, betas[0], betas[1], weight_decay, eps)
        _close64(p, t.detach().numpy(), f"param, step {step}", before)
        _close64(m1, opt.state[t]["exp_avg"].numpy(), f"exp_avg, step {step}", before1)
        _close64(m2, opt.state[t]["exp_avg_sq"].numpy(), f"exp_avg_sq, step {step}")


def _ulps(got32, want64):
    """Largest |got - want| in float32 ulps of the float64 result."""
    want64 = np.asarray(want64, dtype=np.float64)
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return float((np.abs(np.asarray(got32, dtype=np.float64) - want64) / ulp).max())


def _inputs32(n, seed):
    """Normal magnitudes and no cancellation, so that an error in ulps of the RESULT means something: |p| in [1, 2]
    (the update stays below 1), |g| in [0.25, 2], the accumulators in [0.5, 2], Adam's first moment on the gradient's
    side in [0.1, 0.5]; float32 values, so all three computations start from the same numbers."""
    rng = np.random.default_rng(seed)
    sign = lambda: rng.choice([-1.0, 1.0], n)
    p = (sign() * rng.uniform(1.0, 2.0, n)).astype(np.float32)
    g = (sign() * rng.uniform(0.25, 2.0, n)).astype(np.float32)
    s = rng.uniform(0.5, 2.0, n).astype(np.float32)
    m = (np.sign(g) * rng.uniform(0.1, 0.5, n)).astype(np.float32)
    return p, g, s, m


def _torch_adagrad32(p, g, s, lr, weight_decay, eps, rows=None):
    t = torch.tensor(p, requires_grad=True)
    opt = torch.optim.Adagrad([t], lr=lr, weight_decay=weight_decay, eps=eps, foreach=False)
    opt.state[t]["sum"].copy_(torch.tensor(s))
    t.grad = torch.tensor(g) if rows is None else torch.sparse_coo_tensor(torch.tensor(rows)[None], torch.tensor(g), p.shape)
    opt.step()
    return t.detach().numpy(), opt.state[t]["sum"].numpy()


def test_float32_restatements_are_as_close_to_float64_as_torch_float32():
    """One step from the same float32 inputs, three ways: the float64 form (the yardstick), torch's float32 CPU
    optimizer, the float32 restatement.  Errors in float32 ulps of the float64 result, the maximum over all elements;
    the restatement may be at most twice as far off as torch (torch's kernels may contract sum + g*g and g + wd*p into
    an fma, which moves an ulp either way; the restatement rounds every operation).

    Measured (torch float32 -> restatement), n = 20000; the maximum over everything: torch 1.591, restatement 2.127:
      adagrad, wd = 0        param 0.667 -> 0.667    sum 0.500 -> 0.998
      adagrad, wd = 1e-3     param 0.668 -> 0.668    sum 1.560 -> 2.127
      adagrad rows           param 0.615 -> 0.626    sum 0.999 -> 0.999
      adam, wd = 0           param 0.565 -> 0.579    exp_avg 1.000 -> 1.200    exp_avg_sq 1.428 -> 1.498
      adam, wd = 1e-3        param 0.570 -> 0.603    exp_avg 1.343 -> 1.488    exp_avg_sq 1.591 -> 1.591
    (sum, wd = 0: torch's fused sum + g*g is one rounding, 0.5 ulp; two roundings of non-negative terms stay below 1.)
    The bound is applied to every output on its own, which asks more than the two overall maxima would.
    """
    n, lr, eps = 20000, 0.1, 1e-10
    p, g, s, m = _inputs32(n, 3)
    worst = {}

    def record(tag, names, got_t, got_r, want):
        for name, a, b, w in zip(names, got_t, got_r, want):
            e_t, e_r = _ulps(a, w), _ulps(b, w)
            print(f"ULPS {tag} {name}: torch float32 {e_t:.3f} restatement {e_r:.3f}")
            worst[(tag, name)] = (e_t, e_r)

    for wd in (0.0, 1e-3):
        want = orf.adagrad64(p, g, s, -lr, wd, eps)
        record(f"adagrad wd={wd}", ("param", "sum"), _torch_adagrad32(p, g, s, lr, wd, eps),
               orf.adagrad(p, g, s, -lr, wd, eps), want)
    E, d = 200, 100
    rows = np.random.default_rng(4).permutation(E)[:77]
    p2, s2, g2 = p.reshape(E, d), s.reshape(E, d), g[:rows.size * d].reshape(rows.size, d)
    want = orf.adagrad_rows64(p2, g2, s2, rows, -lr, eps)
    got_t = _torch_adagrad32(p2, g2, s2, lr, 0.0, eps, rows=rows)
    got_r = orf.adagrad_rows(p2, g2, s2, rows, -lr, eps)
    record("adagrad rows", ("param", "sum"), [x[rows] for x in got_t], [x[rows] for x in got_r], [x[rows] for x in want])
    assert np.array_equal(got_r[0][~np.isin(np.arange(E), rows)], p2[~np.isin(np.arange(E), rows)])

    betas, lr_a, eps_a, step = (0.9, 0.999), 0.05, 1e-8, 3
    m2 = s * 0.01
    for wd in (0.0, 1e-3):
        step_size, bc2_sqrt = lr_a / (1.0 - betas[0] ** step), (1.0 - betas[1] ** step) ** 0.5
        want = orf.adam64(p, g, m, m2, step_size, bc2_sqrt, betas[0], betas[1], wd, eps_a)
        t = torch.tensor(p, requires_grad=True)
        opt = torch.optim.Adam([t], lr=lr_a, betas=betas, eps=eps_a, weight_decay=wd, foreach=False)
        opt.state[t] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.tensor(m), "exp_avg_sq": torch.tensor(m2)}
        t.grad = torch.tensor(g)
        opt.step()
        assert float(opt.state[t]["step"]) == step
        got_t = (t.detach().numpy(), opt.state[t]["exp_avg"].numpy(), opt.state[t]["exp_avg_sq"].numpy())
        record(f"adam wd={wd}", ("param", "exp_avg", "exp_avg_sq"), got_t,
               orf.adam(p, g, m, m2, step_size, bc2_sqrt, betas[0], betas[1], wd, eps_a), want)
    for key, (e_t, e_r) in worst.items():
        assert e_t > 0.0 and e_r <= 2.0 * e_t, (key, e_t, e_r)


def _term64(x, kind, p, weight, row_dim):
    """LookupEmbedder.penalty's unweighted term on a [rows, row_dim] float64 table."""
    if kind == 2:
        re, im = x.view(-1, row_dim).chunk(2, dim=1)
        x = torch.sqrt(re ** 2 + im ** 2 + 1e-14)
    return weight / p * x.norm(p=p) ** p


@pytest.mark.parametrize("kind,p", [(1, 1), (1, 2), (1, 3), (2, 3)])
def test_penalty_value_and_gradient_are_float64_autograd_of_the_term(kind, p):
    rng = np.random.default_rng(5 + p)
    row_dim, weight = 8, 0.37
    n = 21 * row_dim + (3 if kind == 1 else 0)  # lp: with a scalar tail
    x = rng.standard_normal(n)
    x[[0, 5, 9, 13, 40, 44, n - 1]] = 0.0  # sign(0) = 0; (9, 13) and (40, 44) are whole complex pairs: |z| = 1e-7
    g = 0.1 * rng.standard_normal(n)
    s = rng.uniform(0.5, 2.0, n)
    t = torch.tensor(x, requires_grad=True)
    term = _term64(t, kind, p, weight, row_dim)
    term.backward()
    # the float64 form: the step with the folded penalty == the plain step on grad + d term
    pn, sn, value = orf.adagrad_penalty64(x, g, s, -0.1, 1e-3, 1e-10, kind, p, weight, row_dim)
    want_p, want_s = orf.adagrad64(x, g + t.grad.numpy(), s, -0.1, 1e-3, 1e-10)
    _close64(pn, want_p, "param", x)
    _close64(sn, want_s, "sum")
    assert abs(value * weight / p - float(term.detach())) <= RTOL64 * float(term.detach())
    assert (t.grad.numpy()[[0, 5, n - 1]] == 0.0).all()
    # the float32 form: the value within float32 rounding of the 4-term partials (2 ulp each), param / sum close
    p32, s32, v32 = orf.adagrad_penalty(x, g, s, -0.1, 1e-3, 1e-10, kind, p, weight, row_dim)
    x32 = x.astype(np.float32).astype(np.float64)
    want32 = float(_term64(torch.tensor(x32), kind, p, weight, row_dim)) * p / weight
    assert abs(v32 - want32) <= 8 * 2.0 ** -24 * want32
    assert p32.dtype == np.float32 and s32.dtype == np.float32
    np.testing.assert_allclose(p32, want_p, rtol=1e-5, atol=1e-6)


def test_penalty_kind_0_is_the_plain_step():
    rng = np.random.default_rng(6)
    n = 23
    x, g, s = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    s = np.abs(s)
    a = orf.adagrad_penalty(x, g, s, -0.1, 1e-3, 1e-10, 0, 0, 0.0, 0)
    b = orf.adagrad(x, g, s, -0.1, 1e-3, 1e-10)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == 0.0


def test_bf16_bits_are_torch_cast_over_every_upper_half():
    hi = np.arange(65536, dtype=np.uint32) << np.uint32(16)
    lo = np.array([0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff], dtype=np.uint32)
    u = (hi[:, None] | lo[None, :]).reshape(-1)
    f = u.view(np.float32)
    got = orf.bf16_rne_bits(f)
    want = torch.from_numpy(f.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(f)
    assert np.array_equal(got[~nan], want[~nan])
    got_f = (got.astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert np.isnan(got_f[nan]).all() and nan.sum() == 2 * 127 * 6 + 2 * 5
    # the edges by hand: ties to even, carry into the exponent, overflow to inf, bf16 subnormals, -0
    for bits, want_bits in [(0x3f808000, 0x3f80), (0x3f818000, 0x3f82), (0x3f808001, 0x3f81), (0x3f807fff, 0x3f80),
                            (0x3fffffff, 0x4000), (0x7f7fffff, 0x7f80), (0x00008000, 0x0000), (0x00018000, 0x0002),
                            (0x00008001, 0x0001), (0x80000000, 0x8000), (0x7f800000, 0x7f80), (0xff800000, 0xff80)]:
        assert int(orf.bf16_rne_bits(np.array([bits], dtype=np.uint32).view(np.float32))[0]) == want_bits, hex(bits)
