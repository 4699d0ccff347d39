"""kge_amd.optim.Adam(device_step=True) under GraphedStep on a model: the 1vsAll step of ComplEx (fused cross entropy
of both directions, its backward, the one-launch Adam) replayed as one hipGraph, with and without folded penalty terms,
against the eager host-step Adam -- the case of tests/test_gpu_train_graph.py::
test_graphed_step_refuses_adam_and_counts_adagrad_steps, where the host-step Adam has to stay eager.

The bound.  The gradient scatter uses float atomics, so no bound can be derived: it is MEASURED.  Two eager host-step
runs of this case (the same kernels, the same launches) differ in their losses by up to SPREAD relative (DESIGN.md 24
has the measurement); a replay orders the atomics differently again, so four times that is allowed.  The losses are float32
numbers: a spread below half a unit in the last place of one (2^-24 relative) cannot be observed, so that is the floor
of the figure that is multiplied."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# Measured on the MI355X, on EAGER runs of the HOST-STEP Adam alone (the code this file tests takes no part in it):
# max over the 8 steps of |l1 - l2| / |l1|, over all pairs of 32 runs in 16 fresh processes, for the two forms of this
# case the tests below compare against:
#   plain (no penalty)                        0.0       one loss sequence in 32 runs (and in 40 more runs of one process)
#   lp terms of both tables through autograd  3.556e-6  two loss sequences, 27 and 5 of 32 runs, parting at the sixth
#                                                       loss (133.02187 / 133.02139); 3 of 16 processes saw both
# The second form's scatter meets a sum of three or more float atomics whose order decides a rounding; the first does
# not happen to within its 8 steps.  One bound serves both tests (the issue: "at the same bound"), so SPREAD is the
# case's spread over both forms.  A first version of this file took SPREAD from the plain form only (0.0) and its
# penalty test then failed whenever its two runs landed on different sequences.
SPREAD = 3.556e-6
BOUND = 4.0 * max(SPREAD, 2.0 ** -24)
WEIGHT = 0.05


def _batches():
    g = torch.Generator().manual_seed(3)
    return [torch.stack([torch.randint(hi, (128,), generator=g) for hi in (900, 5, 900)], 1).to(DEV) for _ in range(8)]


def _run(device_step, graphed, penalty=None):
    """penalty: None, "folded" (set_penalty on both tables, lp p = 2) or "autograd" (weight / 2 * sum x^2 of both tables
    added to the loss).  -> (batch losses, penalty values per step and table, optimizer, step)"""
    from kge_amd import model as km, optim as kopt
    from kge_amd.train_graph import GraphedStep
    torch.manual_seed(0)
    m = km.create("complex", 900, 5, 256, device=DEV, score_dtype=torch.bfloat16)
    params = list(m.parameters())
    opt = kopt.Adam(params, lr=0.01, bf16_copies=True, device_step=device_step)
    if penalty == "folded":
        for p in params:
            opt.set_penalty(p, "lp", 2, WEIGHT)
    pens, last = [], {}

    def loss_fn(s, p, o):
        loss = m.loss_sp_po(s, p, o).sum() / len(s)
        if penalty == "autograd":
            terms = [WEIGHT / 2 * (q * q).sum() for q in params]
            # (the values that are compared: the same terms of the same parameters summed in float64)
            last["batch"] = loss.detach()
            last["terms"] = [WEIGHT / 2 * (q.detach().double() ** 2).sum() for q in params]
            loss = loss + sum(terms)
        return loss
    step = GraphedStep(loss_fn, opt, warmup=2, enabled=graphed)
    losses = []
    for b in _batches():
        loss = float(step(b[:, 0], b[:, 1], b[:, 2]))
        if penalty == "autograd":
            loss = float(last["batch"])
            pens.append([float(t) for t in last["terms"]])
        elif penalty == "folded":
            pens.append([float(opt.penalty_value(p)) for p in params])
        losses.append(loss)
    return losses, pens, opt, step


def _close(a, b):
    return abs(a - b) <= BOUND * abs(b)


@pytest.fixture(scope="module")
def eager_host():
    return _run(False, False)[0]


def test_device_step_adam_replays_and_takes_the_eager_host_steps(eager_host):
    losses, _, opt, step = _run(True, True)
    assert step.disabled_reason is None and step.replays == 6
    print("host-step eager:", eager_host, "\ndevice-step graph:", losses)
    assert all(_close(a, b) for a, b in zip(losses, eager_host)), (losses, eager_host)
    assert eager_host[0] > eager_host[-1]  # it trains
    for p in opt.state:
        assert float(opt.state[p]["step"]) == 8 == opt.device_step_count(p)


def test_folded_penalty_takes_the_autograd_terms_steps():
    l_ref, v_ref, _, _ = _run(True, False, "autograd")
    l_got, v_got, opt, step = _run(True, True, "folded")
    assert step.disabled_reason is None and step.replays == 6 and opt.has_penalties()
    print("autograd terms:", l_ref, v_ref, "\nfolded:", l_got, v_got)
    assert all(_close(a, b) for a, b in zip(l_got, l_ref)), (l_got, l_ref)
    for got, ref in zip(v_got, v_ref):
        assert all(_close(a, b) for a, b in zip(got, ref)), (v_got, v_ref)
