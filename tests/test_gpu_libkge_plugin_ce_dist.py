"""`hip_1vsAll.fused_dist_loss` through an UNMODIFIED LibKGE on the MI355X: one epoch of hip_transe / hip_rotate with
the option on (kge_ce_dist_fwd / kge_ce_dist_bwd, no [n, E] matrix) against the same job with the option off (score_sp /
score_po + the reference's loss) from the same initial parameters.  Needs the reference package (oracle/ref_harness.py),
like tests/test_gpu_libkge_plugin_shared.py."""
import os
import shutil

import pytest
import torch

import ref_harness as rh

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]

E, R = 2000, 20
MODULES = ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from kge_amd.synthetic import make_splits, write_libkge_dataset
    root = tmp_path_factory.mktemp("libkge_gpu_ce_dist")
    splits = make_splits(E, R, 4096, 256, 256, seed=3)
    folder = write_libkge_dataset(str(root / "small"), "small", E, R, splits)
    return str(root), folder


def _train_epoch(root, folder, tag, model, option, init_from=None):
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
    config.set("dataset.name", "small")
    config.set("job.device", "cuda")
    config.set("train.max_epochs", 1)
    config.set("train.batch_size", 256)
    config.set("train.num_workers", 0)
    config.set("lookup_embedder.dim", 128)
    for key in ("default", "torch", "numpy", "python"):
        config.set("random_seed." + key, 17)
    config.set("valid.every", 0)
    config._import("hip_1vsAll")
    config.set("train.type", "hip_1vsAll")
    config.set("hip_1vsAll.fused_dist_loss", option)
    torch.manual_seed(17)
    job = TrainingJob.create(config, Dataset.create(config, folder=folder))
    if init_from is not None:
        job.model.load_state_dict(init_from)
    state0 = {k: v.detach().clone() for k, v in job.model.state_dict().items()}
    torch.manual_seed(23)
    job._prepare()
    trace = job.run_epoch()
    torch.cuda.synchronize()
    return job, trace["avg_loss"], state0


@pytest.fixture
def entered(monkeypatch):
    """Times the fused autograd function's forward was entered (kge_amd.model._FusedCEDist)."""
    from kge_amd import model as km
    calls = {"fused": 0}
    orig = km._FusedCEDist.forward

    def forward(ctx, *a, **k):
        calls["fused"] += 1
        return orig(ctx, *a, **k)

    monkeypatch.setattr(km._FusedCEDist, "forward", staticmethod(forward))
    return calls


@pytest.mark.parametrize("model", ["hip_transe", "hip_rotate"])
def test_one_epoch_with_the_option_on_and_off(data, entered, model):
    """16 batches of 256: the epoch's avg_loss of the two runs within 2e-5 relative (the README's bound for job-level
    loss agreement); the fused function was entered for both directions of every batch with the option on, never with
    it off."""
    root, folder = data
    off, l_off, st = _train_epoch(root, folder, "off_" + model, model, False)
    assert type(off).__name__ == "HipTrainingJob1vsAll" and entered["fused"] == 0
    on, l_on, _ = _train_epoch(root, folder, "on_" + model, model, True, init_from=st)
    assert entered["fused"] == 2 * 16, entered
    rel = abs(l_on - l_off) / max(1.0, abs(l_off))
    print(f"{model}: avg_loss off {l_off:.8g} on {l_on:.8g} rel {rel:.3e}")
    assert rel <= 2e-5, (l_on, l_off)
