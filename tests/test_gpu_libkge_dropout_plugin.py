"""`hip_negative_sampling.fused_dropout` driven by an unmodified LibKGE on the GPU: hip_complex and hip_rotate with
embedder dropout 0.2 / 0.1 train on the fused dropout kernels -- no scorer's score_emb runs, the number of fused dropout
calls is batches x slots x 2 -- and with the option off the composed path runs (the trap fires).  The epoch loss of the
fused job lies within the spread of five option-off jobs on other seeds: the generators differ, so only the reference's
own spread can be the yardstick.  Needs the reference package under oracle/_ref (tests/ref_harness.py), else skipped."""
import json
import os
import shutil
import sys

import pytest
import torch

import ref_harness as rh

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]

E, R, TRAIN, DIM, BATCH, K = 300, 12, 2048, 32, 256, 8
MODULES = ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from kge_amd.synthetic import make_splits, write_libkge_dataset
    root = tmp_path_factory.mktemp("libkge_dropout")
    splits = make_splits(E, R, TRAIN, 64, 64, seed=3)
    return str(root), write_libkge_dataset(str(root / "toy"), "toy", E, R, splits)


def _train_epoch(root, folder, tag, model, fused, seed=23):
    rh.import_reference()
    from kge import Config, Dataset
    from kge.job import TrainingJob
    from kge.util.seed import seed_from_config
    config = Config()
    config.folder = os.path.join(root, tag)
    shutil.rmtree(config.folder, ignore_errors=True)
    os.makedirs(config.folder)
    config.set("console.quiet", True)
    config.set("modules", MODULES)
    config.set("model", model)
    config._import(model)
    config._import("hip_negative_sampling")
    for k, v in {"dataset.name": "toy", "job.device": "cuda", "train.max_epochs": 1, "train.batch_size": BATCH,
                 "train.num_workers": 0, "lookup_embedder.dim": DIM, "random_seed.default": 17, "random_seed.torch": 17,
                 "random_seed.numpy": 17, "random_seed.python": 17, "valid.every": 0,
                 "train.type": "hip_negative_sampling", "negative_sampling.num_samples.s": K,
                 "negative_sampling.num_samples.o": K, "negative_sampling.implementation": "triple",
                 f"{model}.entity_embedder.dropout": 0.2, f"{model}.relation_embedder.dropout": 0.1}.items():
        config.set(k, v)
    config.set("hip_negative_sampling.fused_dropout", bool(fused), create=True)
    seed_from_config(config)
    torch.manual_seed(17)
    job = TrainingJob.create(config, Dataset.create(config, folder=folder))
    torch.manual_seed(seed)  # batch order, negative samples, torch's dropout masks
    job._prepare()
    job._is_prepared = True
    trace = job.run_epoch()
    torch.cuda.synchronize()
    return job, float(trace["avg_loss"])


@pytest.fixture
def composed_path_trap(monkeypatch):
    """the composed path of a model with active dropout ends in a scorer's score_emb on n K gathered rows -- the
    reference scorers' (hip_transe / hip_rotate) or the plugin scorers' kge_score_emb front end (hip_complex /
    hip_distmult): all raise for the duration of the test"""
    rh.import_reference()
    from kge.model.complex import ComplExScorer
    from kge.model.distmult import DistMultScorer
    from kge.model.rotate import RotatEScorer
    from kge.model.transe import TransEScorer
    from kge_amd.libkge_plugin import models as pm
    hit = []

    def trap(name):
        def raiser(*a, **kw):
            hit.append(name)
            raise AssertionError(f"{name} was reached: the composed path ran")
        return raiser
    for cls in (ComplExScorer, DistMultScorer, TransEScorer, RotatEScorer, pm._HipScorer):
        monkeypatch.setattr(cls, "score_emb", trap(cls.__name__ + ".score_emb"))
    return hit


@pytest.mark.parametrize("model", ["hip_complex", "hip_rotate"])
def test_fused_dropout_keeps_the_step_on_the_fused_kernels(data, composed_path_trap, model):
    from kge_amd import model as km
    root, folder = data
    calls0 = km.DROPOUT_CALLS
    job, loss = _train_epoch(root, folder, f"fused_{model}", model, True)
    batches = -(-TRAIN // BATCH)
    assert composed_path_trap == []
    assert km.DROPOUT_CALLS - calls0 == batches * 2 * 2  # per batch and slot: the positives and the slot's block
    assert loss == loss and loss > 0
    for prm in job.model.parameters():
        assert bool(torch.isfinite(prm).all())


@pytest.mark.parametrize("model", ["hip_complex", "hip_rotate"])
def test_with_the_option_off_the_composed_path_runs(data, composed_path_trap, model):
    from kge_amd import model as km
    root, folder = data
    calls0 = km.DROPOUT_CALLS
    with pytest.raises(AssertionError, match="the composed path ran"):
        _train_epoch(root, folder, f"off_{model}", model, False)
    assert composed_path_trap and km.DROPOUT_CALLS == calls0


@pytest.mark.parametrize("model", ["hip_complex", "hip_rotate"])
def test_epoch_loss_lies_within_the_spread_of_the_option_off_job(data, model):
    root, folder = data
    off = [_train_epoch(root, folder, f"spread_{model}_{seed}", model, False, seed)[1] for seed in (23, 24, 25, 26, 27)]
    fused = _train_epoch(root, folder, f"spread_{model}_fused", model, True, 23)[1]
    lo, hi = min(off), max(off)
    rec = dict(case="fused_dropout epoch loss", model=model, option_off=off, fused=fused, lo=lo - (hi - lo),
               hi=hi + (hi - lo))
    print("DROPOUT_PLUGIN " + json.dumps(rec, sort_keys=True), file=sys.stderr)
    out = os.environ.get("KGE_DROPOUT_PLUGIN_LOG")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps(rec, sort_keys=True) + "\n")
    assert lo - (hi - lo) <= fused <= hi + (hi - lo), rec
