"""hip_1vsAll through an unmodified LibKGE with train.optimizer.default.type: HipAdam and args.device_step: true: the
job captures its step (the host-step HipAdam kept it eager), the embedders' penalty terms are folded into the
optimizer's launch (kge_adam_step_multi), and two epochs of the graphed job follow two epochs of the same job with
hip_1vsAll.graph_step: false (eager steps of the same kernels, the reference's autograd penalty terms).

Needs the reference package (oracle/_ref/, as tests/test_gpu_libkge_plugin.py, whose helpers are used here).  The
bound is the measured one of tests/test_gpu_adam_model_step.py.

That bound is 4 * 3.556e-6 = 1.42e-5, from eager host-step runs of the 900-entity case.  What this job shows against
it (MI355X; 14,541 entities, 512 triples per batch, 200 Adam steps; second-epoch avg_loss, relative):
    two eager runs of the host-step HipAdam                 4.2e-7
    two eager runs with device_step                         3.3e-7
    two graphed runs with device_step                       1.7e-6
    graphed against eager (this test), five runs            1.8e-6, 5.5e-7, 2.3e-7, 2.1e-6, 4.0e-7
    penalty values, graphed against eager                   5.1e-9 (entities), 2.7e-8 (relations)
The differences are the scatter atomics' order, not the clock (tests/test_gpu_adam_multi.py holds the update and the
captured step to bits)."""
import pytest
import torch

import ref_harness as rh
from test_gpu_adam_model_step import BOUND
from test_gpu_libkge_plugin import DEVICE, _train_epoch, data  # noqa: F401  (data: the module's dataset fixture)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]


def test_hip_1vsall_captures_its_step_under_device_step_adam_with_folded_penalties(data):  # noqa: F811
    if DEVICE == "cpu":
        pytest.skip("needs the GPU")
    root, folder = data
    opts = {"lookup_embedder.regularize": "lp", "lookup_embedder.regularize_args.p": 2,
            "hip_complex.entity_embedder.regularize_weight": 2e-4, "hip_complex.relation_embedder.regularize_weight": 5e-3,
            "train.optimizer.default.type": "HipAdam", "train.optimizer.default.args.lr": 0.003,
            "train.optimizer.default.args.device_step": True, "train.optimizer.default.args.bf16_copies": True,
            "hip_complex.score_dtype": "bfloat16"}
    gra, _, st = _train_epoch(root, folder, "adam_graph", "hip_complex", "hip_1vsAll", dim=256, opts=opts)
    eag, _, _ = _train_epoch(root, folder, "adam_eager", "hip_complex", "hip_1vsAll", dim=256, init_from=st,
                             opts=dict(opts, **{"hip_1vsAll.graph_step": False}))
    traces = []
    for job in (gra, eag):
        torch.manual_seed(29)  # the second epoch's batch order
        traces.append(job.run_epoch())
    torch.cuda.synchronize()
    tr_gra, tr_eag = traces
    gs = gra._graph_step
    assert gs is not None and gs.disabled_reason is None and gs.replays > 0 and gs.captures == 1, vars(gs)
    assert gra.optimizer.device_step and gra.optimizer.graph_capturable
    assert gra.optimizer.has_penalties() and len(gra._folded_penalties) == 2
    assert eag._graph_step is None and not eag.optimizer.has_penalties()
    for p, state in gra.optimizer.state.items():
        assert float(state["step"]) == gra.optimizer.device_step_count(p) == 200  # 2 epochs of 100 batches
    print("second epoch:", tr_gra["avg_loss"], tr_eag["avg_loss"], tr_gra["avg_penalties"], tr_eag["avg_penalties"],
          "replays", gs.replays)
    assert abs(tr_gra["avg_loss"] - tr_eag["avg_loss"]) <= BOUND * abs(tr_eag["avg_loss"]), (tr_gra["avg_loss"],
                                                                                              tr_eag["avg_loss"])
    keys = sorted(tr_eag["avg_penalties"])
    assert keys == sorted(tr_gra["avg_penalties"]) and len(keys) == 2
    for k in keys:
        a, b = tr_gra["avg_penalties"][k], tr_eag["avg_penalties"][k]
        assert abs(a - b) <= BOUND * abs(b), (k, a, b)
