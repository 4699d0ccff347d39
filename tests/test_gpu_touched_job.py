"""`hip_negative_sampling.touched_rows` through an UNMODIFIED LibKGE on the MI355X: test b3's
job (tests/test_gpu_libkge_plugin.py: hip_transe + hip_negative_sampling + HipAdagrad, 64 + 48 negatives, 100 batches of
512 at the FB15k-237 shape, train.loss bce_self_adversarial) with the option on against off, from the same initial
parameters, once eager and once with graph_step.

The row step is the dense step on the rows that have a gradient, so the two runs differ only in the order of the float
atomics of the gradient scatter: epoch loss within 1e-5 relative, the bar b3 holds a replayed run to against an eager
one.  No test here asserts a time."""
import os

import pytest
import torch

import ref_harness as rh
from test_gpu_libkge_plugin import DEVICE, _rel, _train_epoch, data  # noqa: F401  (data: the module's dataset fixture)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]

OPTS = {"negative_sampling.num_samples.s": 64, "negative_sampling.num_samples.o": 48,
        "negative_sampling.implementation": "triple", "train.loss": "bce_self_adversarial",
        "train.optimizer.default.type": "HipAdagrad"}


def _entity_weight(job):
    return job.model.get_s_embedder()._embeddings.weight


def _run(data, tag, graph, touched, init_from=None, extra=None):
    root, folder = data
    opts = dict(OPTS, **{"hip_negative_sampling.graph_step": graph, "hip_negative_sampling.touched_rows": touched})
    opts.update(extra or {})
    return _train_epoch(root, folder, tag, "hip_transe", "hip_negative_sampling", 128, opts, init_from=init_from)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph_step"])
def test_touched_rows_takes_the_dense_jobs_steps(data, graph):
    if DEVICE == "cpu":
        pytest.skip("needs the GPU")
    dense, l_dense, st = _run(data, f"touched_off_{graph}", graph, False)
    rows, l_rows, _ = _run(data, f"touched_on_{graph}", graph, True, init_from=st)
    assert dense.touched_rows is False and dense.touched_rows_declined is None
    assert rows.touched_rows is True and rows.touched_rows_declined is None, rows.touched_rows_declined
    w, w0 = _entity_weight(rows), _entity_weight(dense)
    pair = rows.optimizer.touched_rows(w)
    assert pair is not None and dense.optimizer.touched_rows(w0) is None
    assert w.grad is None                                   # the entity gradient never reached .grad
    torch.cuda.synchronize()
    assert not pair[0].any() and not pair[1].any()          # buffer and bitmap are zero between steps
    batches = len(rows.loader)
    print(f"touched_rows {'graph_step' if graph else 'eager'}: loss on {l_rows!r} off {l_dense!r} "
          f"rel {_rel(l_rows, l_dense):.3e}, batches {batches}")
    assert _rel(l_rows, l_dense) <= 1e-5, (l_rows, l_dense)
    # the checkpoint's step count: one per batch, for the touched-row table as for the dense one
    assert float(rows.optimizer.state[w]["step"]) == batches
    assert float(dense.optimizer.state[w0]["step"]) == batches
    rel_w = rows.model.get_p_embedder()._embeddings.weight
    assert float(rows.optimizer.state[rel_w]["step"]) == batches
    gs = rows._graph_step
    if graph:
        assert gs is not None and gs.disabled_reason is None and gs.captures == 1 and gs.replays >= 90, vars(gs)
    else:
        assert gs is None
    # (printed, not asserted: Adagrad turns a coordinate whose gradient is atomic-order noise into a +-lr move)
    diff = float((w.detach() - w0.detach()).norm() / w0.detach().norm())
    print(f"  entity table relative difference {diff:.3e}")


def test_an_ineligible_job_runs_the_dense_path_and_says_why(data):
    if DEVICE == "cpu":
        pytest.skip("needs the GPU")
    job, loss, _ = _run(data, "touched_ineligible", True, True,
                        extra={"hip_transe.entity_embedder.regularize_weight": 1e-6})
    assert job.touched_rows is False
    assert "regularize_weight" in (job.touched_rows_declined or ""), job.touched_rows_declined
    w = _entity_weight(job)
    assert job.optimizer.touched_rows(w) is None
    assert float(job.optimizer.state[w]["step"]) == len(job.loader)   # the dense path stepped it
    assert loss == loss and os.path.isdir(job.config.folder)
