"""`hip_KvsAll.fused_f32_loss` through an UNMODIFIED LibKGE on the MI355X: one epoch of float32 hip_complex /
hip_distmult with the option on (kge_kl_f32_* / kge_bce_f32_*, no [n, E] matrix; label smoothing on the fused path)
against the same job with the option off (score_sp / score_po + the reference's loss) from the same initial parameters,
on the dataset of tests/test_gpu_libkge_plugin_multilabel_dist.py (no repeated training triples: label ids unique per
row).

Compared, each within 2e-5 relative (the project's bound for job-level loss agreement): batch 0 of the training epoch
(identical parameters), every batch and the avg_loss of a forward-only epoch on the parameters the fused run ended
with, and the avg_loss of the SGD-trained epoch.  The training epochs step with plain SGD, whose step is continuous in
the gradient; the dist module's docstring has the measurements that ruled Adagrad out (its first step is lr * sign(g),
so noise-sized gradients move elements by +-lr differently from run to run).

Needs the reference package (oracle/ref_harness.py)."""
import os
import shutil

import pytest
import torch

import ref_harness as rh
from test_gpu_libkge_plugin_multilabel_dist import MODULES, _batch_losses, _rel, data  # noqa: F401  (`data`: a fixture)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]
BOUND = 2e-5


def _train_epoch(root, folder, tag, model, loss, smoothing, option, init_from=None, base=None, forward_only=False):
    """-> (job, avg_loss, initial state, number of (batch, query type) pairs of the epoch)"""
    rh.import_reference()
    from kge import Config, Dataset
    from kge.job import TrainingJob
    config = Config()
    config.folder = os.path.join(root, tag)
    shutil.rmtree(config.folder, ignore_errors=True)
    os.makedirs(config.folder)
    config.set("console.quiet", True)
    config.set("modules", MODULES)
    config.set("model", model)
    config._import(model)
    if base is not None:
        config._import(base)
        config.set(f"{model}.base_model.type", base)
    config.set("dataset.name", "small")
    config.set("job.device", "cuda")
    config.set("train.max_epochs", 1)
    config.set("train.batch_size", 256)
    config.set("train.num_workers", 0)
    config.set("train.loss", loss)
    config.set("KvsAll.label_smoothing", smoothing)
    config.set("train.optimizer.default.type", "SGD")  # (the module docstring)
    config.set("train.optimizer.default.args.lr", 0.1, create=True)
    config.set("lookup_embedder.dim", 128)
    for key in ("default", "torch", "numpy", "python"):
        config.set("random_seed." + key, 17)
    config.set("valid.every", 0)
    config.set("train.trace_level", "batch")
    config._import("hip_KvsAll")
    config.set("train.type", "hip_KvsAll")
    config.set("hip_KvsAll.fused_f32_loss", option)
    torch.manual_seed(17)
    job = TrainingJob.create(config, Dataset.create(config, folder=folder), forward_only=forward_only)
    if init_from is not None:
        job.model.load_state_dict(init_from)
    state0 = {k: v.detach().clone() for k, v in job.model.state_dict().items()}
    pairs = [0]
    inner = job._process_subbatch

    def counted(batch_index, batch, subbatch_slice, result):
        pairs[0] += int(torch.unique(batch["query_type_indexes"][subbatch_slice]).numel())
        return inner(batch_index, batch, subbatch_slice, result)

    job._process_subbatch = counted
    torch.manual_seed(23)
    job._prepare()
    trace = job.run_epoch()
    torch.cuda.synchronize()
    job.batch_losses = _batch_losses(config.folder)
    return job, trace["avg_loss"], state0, pairs[0]


@pytest.fixture
def entered(monkeypatch):
    """Times the fused autograd functions' forward was entered (kge_amd.model._FusedKLF32 / _FusedBCEF32) and times
    score_sp / score_po of the scoring model class were asked."""
    rh.import_reference()
    from kge_amd import model as km
    from kge_amd.libkge_plugin import models as pm
    calls = {"kl": 0, "bce": 0, "score": 0}
    for key, cls in (("kl", km._FusedKLF32), ("bce", km._FusedBCEF32)):
        def forward(ctx, *a, _orig=cls.forward, _key=key, **k):
            calls[_key] += 1
            return _orig(ctx, *a, **k)
        monkeypatch.setattr(cls, "forward", staticmethod(forward))
    for nm in ("score_sp", "score_po"):
        def counted(self, *a, _f=getattr(pm._FusedScoring, nm), **k):
            calls["score"] += 1
            return _f(self, *a, **k)
        monkeypatch.setattr(pm._FusedScoring, nm, counted)
    return calls


def _on_against_off(data, entered, tag, model, loss, smoothing, base=None):
    root, folder = data
    other = "bce" if loss == "kl" else "kl"
    off, l_off, st, pairs_off = _train_epoch(root, folder, f"off_{tag}", model, loss, smoothing, False, base=base)
    assert type(off).__name__ == "HipTrainingJobKvsAll"
    assert entered["kl"] == entered["bce"] == 0 and entered["score"] == pairs_off, (entered, pairs_off)
    on, l_on, _, pairs = _train_epoch(root, folder, f"on_{tag}", model, loss, smoothing, True, init_from=st, base=base)
    assert pairs == pairs_off and pairs >= len(on.loader)
    # the fused functions were entered once per query type per batch; score_sp / score_po were not asked again
    assert entered[loss] == pairs and entered[other] == 0 and entered["score"] == pairs_off, (entered, pairs)
    assert len(on.batch_losses) == len(off.batch_losses) == len(on.loader)
    per_batch = [_rel(a, b) for a, b in zip(on.batch_losses, off.batch_losses)]
    print(f"{tag}: relative difference of the batch losses, batch 0 .. last: " + " ".join(f"{x:.1e}" for x in per_batch))
    rel = _rel(l_on, l_off)
    print(f"JOB {tag}: avg_loss off {l_off:.8g} on {l_on:.8g} rel {rel:.3e} ({pairs} fused calls, {len(on.loader)} batches)")
    assert per_batch[0] <= BOUND, per_batch[0]   # identical parameters
    trained = {k: v.detach().clone() for k, v in on.model.state_dict().items()}
    before = dict(entered)
    f_off, lf_off, _, _ = _train_epoch(root, folder, f"fwd_off_{tag}", model, loss, smoothing, False, init_from=trained,
                                       base=base, forward_only=True)
    assert entered["kl"] == before["kl"] and entered["bce"] == before["bce"]
    scored = entered["score"]
    f_on, lf_on, _, f_pairs = _train_epoch(root, folder, f"fwd_on_{tag}", model, loss, smoothing, True, init_from=trained,
                                           base=base, forward_only=True)
    assert entered[loss] == before[loss] + f_pairs and entered["score"] == scored
    assert all(torch.equal(v, trained[k]) for k, v in f_on.model.state_dict().items()), "a forward-only epoch moved parameters"
    fwd = [_rel(a, b) for a, b in zip(f_on.batch_losses, f_off.batch_losses)]
    print(f"JOB {tag}: forward only on the trained parameters, batch 0 .. last: " + " ".join(f"{x:.1e}" for x in fwd)
          + f"; avg_loss rel {_rel(lf_on, lf_off):.3e}")
    assert len(fwd) == len(f_on.loader) and max(fwd) <= BOUND and _rel(lf_on, lf_off) <= BOUND, (max(fwd), lf_on, lf_off)
    assert rel <= BOUND, (l_on, l_off)   # the SGD-trained epoch


@pytest.mark.parametrize("loss,smoothing", [("kl", 0.0), ("kl", 0.1), ("bce", 0.0)])
@pytest.mark.parametrize("model", ["hip_complex", "hip_distmult"])
def test_one_kvsall_epoch_with_the_option_on_and_off(data, entered, model, loss, smoothing):
    _on_against_off(data, entered, f"{model}_{loss}_{smoothing}", model, loss, smoothing)


def test_kvsall_under_the_reciprocal_wrapper(data, entered):
    _on_against_off(data, entered, "reciprocal_complex_kl", "hip_reciprocal_relations_model", "kl", 0.1, base="hip_complex")
