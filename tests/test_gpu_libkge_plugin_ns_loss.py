"""`hip_negative_sampling.fused_other_losses` through an UNMODIFIED LibKGE on the MI355X: train.loss kl /
margin_ranking / soft_margin / se with the job's loss object replaced by the one-kernel stand-in (_HipNsLoss ->
kge_ns_loss), one epoch on the toy dataset of tests/test_gpu_libkge_plugin_shared.py (16 batches of 256, 2 x 64
per-triple negatives, dim 128) against the same job with the option off -- the reference's loss object on the same
scoring kernels, from the same initial parameters and samples.

Bounds: the epoch loss fused against reference loss within 1e-4 relative -- the bound of the negative-sampling cases of
tests/test_gpu_libkge_plugin.py (test_b2_negative_sampling_with_the_fused_bce_losses, line 216; test_b_negative_sampling_jobs,
line 237); the captured step against the eager one within 1e-5 -- case b3's bound (line 919: the replay orders the float
atomics of the gradient scatter differently).  Needs the reference package, like the harness it uses."""
import pytest
import torch

import ref_harness as rh
from test_gpu_libkge_plugin_shared import _rel, _train_epoch, data  # noqa: F401  (`data`: the toy dataset fixture)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]

PER_TRIPLE = {"negative_sampling.shared": False, "negative_sampling.implementation": "triple"}
ON = {"hip_negative_sampling.fused_other_losses": True}
OFF = {"hip_negative_sampling.fused_other_losses": False}
NO_GRAPH = {"hip_negative_sampling.graph_step": False}
HIP_ADAGRAD = {"train.optimizer.default.type": "HipAdagrad"}


def _run(data, tag, model, loss, *opts, init_from=None):
    root, folder = data
    o = dict(PER_TRIPLE, **{"train.loss": loss})
    for extra in opts:
        o.update(extra)
    return _train_epoch(root, folder, tag, model, "hip_negative_sampling", "default", opts=o, init_from=init_from)


# (soft_margin on hip_distmult: on TransE's scores -- minus an L1 distance, about -100 at initialisation -- the
# reference's float32 log(1 + exp(z)) overflows and the reference trainer stops with "Cost became nan": the case below)
@pytest.mark.parametrize("model,loss", [("hip_rotate", "kl"), ("hip_distmult", "soft_margin"), ("hip_transe", "se")])
def test_fused_other_losses_against_the_reference_loss_object(data, model, loss):
    """Eager steps (torch's Adagrad is not capturable): the stand-in's block form, once per slot and batch."""
    off, l_off, st = _run(data, f"off_{loss}", model, loss, OFF)
    on, l_on, _ = _run(data, f"on_{loss}", model, loss, ON, init_from=st)
    assert type(off.loss).__name__ != "_HipNsLoss" and type(off.loss).__module__ == "kge.util.loss"
    assert type(on.loss).__name__ == "_HipNsLoss" and on.loss.kind == loss and on.loss.fused_calls == 2 * 16
    assert on.graph_batches == 0
    print(f"{model} {loss}: loss reference object {l_off:.8g} stand-in {l_on:.8g} rel {_rel(l_on, l_off):.3e}")
    assert _rel(l_on, l_off) <= 1e-4, (l_on, l_off)


def test_soft_margin_stand_in_trains_where_the_float32_reference_form_overflows(data):
    """hip_transe + soft_margin: a positive's score is minus a distance of about 100, z = -x is past float32 exp
    overflow, and the reference's loss object gives nan in the first batch (its trainer raises FloatingPointError).  The
    stand-in's max(z, 0) + log1p(exp(-|z|)) takes the epoch with a finite loss."""
    with pytest.raises(FloatingPointError):
        _run(data, "sm_off_transe", "hip_transe", "soft_margin", OFF)
    on, l_on, _ = _run(data, "sm_on_transe", "hip_transe", "soft_margin", ON)
    assert type(on.loss).__name__ == "_HipNsLoss" and on.loss.fused_calls == 2 * 16
    print(f"hip_transe soft_margin: stand-in epoch loss {l_on:.8g}")
    assert l_on > 0 and l_on < float("inf")


def test_margin_ranking_gets_the_captured_step_with_the_option_on_only(data):
    """hip_transe + margin_ranking (margin = train.loss_arg) + HipAdagrad.  Option off: the reference's loss object, no
    captured step (its nonzero() calls wait on the device) -- unchanged behaviour.  Option on: the stand-in, and the
    batches go through the GraphedStep (positives and the slots' blocks straight into kge_ns_loss: the parts form);
    the epoch loss equals the eager stand-in's to 1e-5 and the reference loss object's to 1e-4."""
    margin = {"train.loss_arg": 4.0}
    off, l_off, st = _run(data, "mr_off", "hip_transe", "margin_ranking", OFF, HIP_ADAGRAD, margin)
    gra, l_gra, _ = _run(data, "mr_graph", "hip_transe", "margin_ranking", ON, HIP_ADAGRAD, margin, init_from=st)
    eag, l_eag, _ = _run(data, "mr_eager", "hip_transe", "margin_ranking", ON, HIP_ADAGRAD, margin, NO_GRAPH, init_from=st)
    assert type(off.loss).__name__ == "MarginRankingKgeLoss" and off.graph_batches == 0 and off._graph_step is None
    for job in (gra, eag):
        assert type(job.loss).__name__ == "_HipNsLoss" and job.loss.kind == "margin_ranking" and job.loss.arg == 4.0
        assert job.loss.fused_calls > 0
    gs = gra._graph_step
    assert gra.graph_batches > 0 and gs is not None and gs.disabled_reason is None and gs.replays > 0, vars(gs)
    assert eag.graph_batches == 0 and eag._graph_step is None
    print(f"margin_ranking: loss reference object {l_off:.8g} stand-in eager {l_eag:.8g} captured {l_gra:.8g} "
          f"(batches through the step {gra.graph_batches}, replays {gs.replays}); rel eager vs reference "
          f"{_rel(l_eag, l_off):.3e}, captured vs eager {_rel(l_gra, l_eag):.3e}")
    assert l_off > 0 and torch.isfinite(torch.tensor(l_gra))
    assert _rel(l_eag, l_off) <= 1e-4, (l_eag, l_off)
    assert _rel(l_gra, l_eag) <= 1e-5, (l_gra, l_eag)
