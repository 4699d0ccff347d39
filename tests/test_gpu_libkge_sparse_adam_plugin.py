"""`train.optimizer.default.type: HipSparseAdam` with `hip_negative_sampling.touched_rows: true` through an UNMODIFIED
LibKGE on the MI355X: hip_distmult on the toy dataset of tests/test_abi_sparse_adam_cpu.py, two
epochs, once eager and once with graph_step, from the same initial parameters and the same batches.

The two runs take the same steps up to the order of the float atomics of the gradient scatter (the eager job
back-propagates slot by slot, the captured step through one node): epoch losses within 1e-5 relative, the bar
tests/test_gpu_touched_job.py and test b3 hold a replayed run to against an eager one.  The job's checkpoint -- step,
exp_avg, exp_avg_sq, no clock record -- then loads into the REFERENCE's own job (model distmult with
lookup_embedder.sparse: true, train.type negative_sampling, optimizer SparseAdam), which continues from it."""
import os

import pytest
import torch

import ref_harness as rh
from test_abi_sparse_adam_cpu import _job

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]

OPTS = {"train.optimizer.default.type": "HipSparseAdam", "train.optimizer.default.args.lr": 0.01,
        "hip_negative_sampling.touched_rows": True, "negative_sampling.implementation": "triple"}


def _two_epochs(tmp_path, tag, graph, init=None):
    torch.manual_seed(17)
    job = _job(tmp_path, tag, dict(OPTS, **{"hip_negative_sampling.graph_step": graph}), device="cuda")
    if init is not None:
        job.model.load_state_dict(init)
    state0 = {k: v.detach().clone() for k, v in job.model.state_dict().items()}
    torch.manual_seed(23)  # batch order / negative samples
    losses = [job.run_epoch()["avg_loss"] for _ in range(2)]
    torch.cuda.synchronize()
    return job, losses, state0


def test_eager_and_graph_step_take_the_same_steps_and_the_reference_continues(tmp_path):
    from kge_amd import optim as kopt
    eager, l_eager, st = _two_epochs(tmp_path, "eager", False)
    graph, l_graph, _ = _two_epochs(tmp_path, "graph", True, init=st)
    batches = len(eager.loader)
    for job in (eager, graph):
        assert isinstance(job.optimizer, kopt.SparseAdam)
        assert job.touched_rows is True and job.touched_rows_declined is None, job.touched_rows_declined
        for emb in (job.model.get_s_embedder(), job.model.get_p_embedder()):
            w = emb._embeddings.weight
            pair = job.optimizer.touched_rows(w)
            assert pair is not None and w.grad is None
            assert not pair[0].any() and not pair[1].any()      # buffer and bitmap are zero between steps
            assert job.optimizer.state[w]["step"] == 2 * batches == job.optimizer.device_step_count(w)
    gs = graph._graph_step
    assert eager._graph_step is None
    assert gs is not None and gs.disabled_reason is None and gs.captures == 1 and gs.replays >= 2 * batches - 3, vars(gs)
    for a, b in zip(l_eager, l_graph):
        print(f"HipSparseAdam touched_rows: epoch loss eager {a!r} graph_step {b!r} rel {abs(a - b) / max(1.0, abs(b)):.3e}")
        assert a == a and abs(a - b) / max(1.0, abs(b)) <= 1e-5, (l_eager, l_graph)
    assert l_eager[1] < l_eager[0]
    # the checkpoint into the reference's job: SparseAdam on sparse embedders
    path = os.path.join(str(tmp_path), "checkpoint_hip.pt")
    graph.epoch = 2
    graph.save(path)
    ckpt = torch.load(path, map_location="cuda", weights_only=False)
    assert all(sorted(s) == ["exp_avg", "exp_avg_sq", "step"] for s in ckpt["optimizer_state_dict"]["state"].values())
    ref = _job(tmp_path, "ref", {"train.optimizer.default.type": "SparseAdam", "train.optimizer.default.args.lr": 0.01,
                                 "lookup_embedder.sparse": True, "negative_sampling.implementation": "triple"},
               device="cuda", model="distmult", train_type="negative_sampling")
    assert type(ref.optimizer) is torch.optim.SparseAdam
    ref.model.load(ckpt["model"])
    ckpt["file"] = path
    ref._load(ckpt)
    w_ref = ref.model.get_s_embedder()._embeddings.weight
    w_hip = graph.model.get_s_embedder()._embeddings.weight
    assert torch.equal(w_ref.detach(), w_hip.detach())
    assert torch.equal(ref.optimizer.state[w_ref]["exp_avg_sq"], graph.optimizer.state[w_hip]["exp_avg_sq"])
    assert ref.optimizer.state[w_ref]["step"] == 2 * batches and ref.epoch == 2
    loss3 = ref.run_epoch()["avg_loss"]
    print(f"  reference job continued from the checkpoint: epoch loss {loss3!r} after {l_graph!r}")
    assert ref.optimizer.state[w_ref]["step"] == 3 * batches and w_ref.grad is None or w_ref.grad.is_sparse
    assert loss3 == loss3 and loss3 < l_graph[0]
