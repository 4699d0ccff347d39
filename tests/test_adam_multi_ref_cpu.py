"""kge_adam_step_multi without a GPU: the clock recurrence of tests/_adam_multi_ref.py against the host path's bias
correction, the restatement against torch.optim.Adam, the entry point's argument validation (returns before any launch)
and the GraphedStep gate for kge_amd.optim.Adam(device_step=True)."""
import ctypes

import numpy as np
import pytest
import torch

import _adam_multi_ref as amr


@pytest.mark.parametrize("beta1,beta2,lr", [(0.9, 0.999, 1e-3), (0.9, 0.99, 0.05), (0.5, 0.9999, 0.2)])
def test_clock_recurrence_gives_the_host_paths_two_floats(beta1, beta2, lr):
    """kge_amd.optim.Adam.step() (host step) hands the kernel float32(lr / (1 - beta1 ** t)) and
    float32((1 - beta2 ** t) ** 0.5).  The clock multiplies instead of calling pow: the float64 powers differ in their
    last bits, the two float32 results must not -- at every t in 1..200,000, bit for bit."""
    n = 200000
    b1 = b2 = 1.0
    p1, p2 = np.empty(n), np.empty(n)
    for k in range(n):  # the recurrence: one float64 multiplication per step
        b1 *= beta1
        b2 *= beta2
        p1[k], p2[k] = b1, b2
    got_ss = (np.float64(lr) / (1.0 - p1)).astype(np.float32)
    got_bc = np.sqrt(1.0 - p2).astype(np.float32)
    want_ss = np.array([lr / (1.0 - beta1 ** float(t)) for t in range(1, n + 1)]).astype(np.float32)
    want_bc = np.array([(1.0 - beta2 ** float(t)) ** 0.5 for t in range(1, n + 1)]).astype(np.float32)
    assert (got_ss.view(np.uint32) != want_ss.view(np.uint32)).sum() == 0
    assert (got_bc.view(np.uint32) != want_bc.view(np.uint32)).sum() == 0
    # ... and clock_tick is that recurrence
    c = amr.clock_seed(0, beta1, beta2)
    for k in range(50):
        c = amr.clock_tick(c, lr, beta1, beta2)
        assert c[0] == k + 1 and c[1] == p1[k] and c[2] == p2[k]
        assert c[3].view(np.uint32) == got_ss[k].view(np.uint32) and c[4].view(np.uint32) == got_bc[k].view(np.uint32)
    assert len(amr.clock_bytes(c)) == 32


@pytest.mark.parametrize("weight_decay", [0.0, 1e-3])
def test_restatement_matches_torch_adam_over_five_steps(weight_decay):
    """Tolerances: tests/test_gpu_optim.py::test_adam_matches_torch."""
    torch.manual_seed(1)
    lr, betas, eps = 0.05, (0.9, 0.99), 1e-8
    shapes = [(777, 64), (9, 31), (6,)]
    ref = [torch.randn(s).requires_grad_(True) for s in shapes]
    opt = torch.optim.Adam(ref, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    got = [(r.detach().numpy().copy().reshape(-1), np.zeros(r.numel(), np.float32), np.zeros(r.numel(), np.float32),
            amr.clock_seed(0, *betas)) for r in ref]
    for step in range(5):
        for k, r in enumerate(ref):
            r.grad = torch.randn_like(r)
            p, a, b, c = got[k]
            p, a, b, _, c = amr.adam_multi_segment(p, r.grad.numpy(), a, b, c, lr, betas[0], betas[1], weight_decay, eps)
            got[k] = (p, a, b, c)
        opt.step()
        for r, (p, a, b, c) in zip(ref, got):
            st = opt.state[r]
            torch.testing.assert_close(torch.from_numpy(p).view(r.shape), r.detach(), rtol=5e-6, atol=2e-6)
            torch.testing.assert_close(torch.from_numpy(a).view(r.shape), st["exp_avg"], rtol=5e-6, atol=2e-7)
            torch.testing.assert_close(torch.from_numpy(b).view(r.shape), st["exp_avg_sq"], rtol=5e-6, atol=1e-9)
            assert c[0] == step + 1 == float(st["step"])


def test_entry_point_validates_arguments_without_a_device():
    from kge_amd import _lib
    from kge_amd._lib import KgeAdamClock, KgeAdamSeg, KgePenaltySeg
    _lib.build()
    lib = _lib.lib()
    assert ctypes.sizeof(KgeAdamClock) == 32 and KgeAdamClock.step_size.offset == 24
    assert ctypes.sizeof(KgeAdamSeg) == 88 and KgeAdamSeg.clock.offset == 40 and KgeAdamSeg.lr.offset == 56
    assert KgeAdamSeg.weight_decay.offset == 80
    assert _lib.ADAM_MAX_SEGS == 8

    def seg(count=64, param=16, grad=16, m1=16, m2=16, copy=None, clock=32, beta1=0.9, beta2=0.999):
        return KgeAdamSeg(param, grad, m1, m2, copy, clock, count, 1e-3, beta1, beta2, 0.0, 1e-8)
    call = lambda segs, pens=None: lib.kge_adam_step_multi(
        (KgeAdamSeg * len(segs))(*segs), None if pens is None else (KgePenaltySeg * len(pens))(*pens), len(segs), None)
    empty = seg(count=0, param=None, grad=None, m1=None, m2=None, clock=None)
    # nothing to do: no launch (there is no device here)
    assert lib.kge_adam_step_multi(None, None, 0, None) == 0
    assert call([empty]) == 0 and call([empty] * 8) == 0
    # the number of segments
    assert lib.kge_adam_step_multi(None, None, 1, None) == -1
    assert lib.kge_adam_step_multi(None, None, -1, None) == -1
    assert call([empty] * 9) == -1
    # NULL / misaligned arrays of a non-empty segment
    for name in ("param", "grad", "m1", "m2"):
        assert call([seg(**{name: None})]) == -1, name
        assert call([seg(**{name: 24})]) == -1, name
        assert call([empty, seg(**{name: 20})]) == -1, name
    assert call([seg(copy=12)]) == -1
    assert call([seg(count=-1)]) == -1
    # the clock: NULL, misaligned, shared by two non-empty segments
    assert call([seg(clock=None)]) == -1
    assert call([seg(clock=36)]) == -1
    assert call([seg(clock=32), seg(clock=64), seg(clock=32)]) == -1
    # betas outside [0, 1)
    assert call([seg(beta1=1.0)]) == -1 and call([seg(beta2=-0.1)]) == -1 and call([seg(beta2=float("nan"))]) == -1
    # penalties
    one = lambda pen, count=64: call([seg(count=count)], [pen])
    assert one(KgePenaltySeg(3, 2, 0.1, 0, 8)) == -1          # unknown kind
    assert one(KgePenaltySeg(-1, 2, 0.1, 0, 8)) == -1
    assert one(KgePenaltySeg(1, 2, 0.1, 0, None)) == -1       # no accumulator
    assert one(KgePenaltySeg(1, 2, 0.1, 0, 12)) == -1         # misaligned accumulator
    assert one(KgePenaltySeg(1, 4, 0.1, 0, 8)) == -2          # exponent outside 1..3: unsupported
    assert one(KgePenaltySeg(2, 3, 0.1, 12, 8)) == -1         # complex rows: row_dim % 8 != 0
    assert one(KgePenaltySeg(2, 3, 0.1, 48, 8)) == -1         # ... count not a multiple of row_dim
    assert one(KgePenaltySeg(2, 3, 0.1, 0, 8)) == -1
    # past 2^31 workgroups (checked before the launch; the arrays are never touched)
    assert call([seg(count=1024 << 31)]) == -2
    assert call([seg(count=1 << 40, clock=32), seg(count=1 << 40, clock=64)]) == -2


def test_graphed_step_admits_the_device_step_adam_only():
    from kge_amd import optim as kopt
    from kge_amd.train_graph import GraphedStep
    w = [torch.nn.Parameter(torch.zeros(4, 4))]
    f = lambda *a: None
    opt = kopt.Adam(w, lr=0.1, device_step=True)
    st = GraphedStep(f, opt)
    assert st.enabled and st.disabled_reason is None and opt.graph_capturable
    st = GraphedStep(f, kopt.Adam(w, lr=0.1))
    assert not st.enabled and "step count" in st.disabled_reason
    assert kopt.Adam.graph_capturable is False
    # the penalty interface belongs to the device step; the clock is not part of the checkpoint
    with pytest.raises(ValueError, match="device_step"):
        kopt.Adam(w, lr=0.1).set_penalty(w[0], "lp", 2, 0.1)
    assert not opt.has_penalties()
    opt.state[w[0]].update(step=torch.tensor(3.0), exp_avg=torch.zeros(4, 4), exp_avg_sq=torch.zeros(4, 4),
                           clock=torch.zeros(4, dtype=torch.int64))
    sd = opt.state_dict()
    assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"] and "clock" in opt.state[w[0]]
    fresh = kopt.Adam(w, lr=0.1, device_step=True)
    fresh.load_state_dict(sd)
    assert sorted(fresh.state[w[0]]) == ["exp_avg", "exp_avg_sq", "step"] and float(fresh.state[w[0]]["step"]) == 3.0
    for bad in (dict(amsgrad=True),):
        with pytest.raises(NotImplementedError):
            kopt.Adam(w, lr=0.1, device_step=True, **bad)
