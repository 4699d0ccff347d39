"""`hip_1vsAll.fused_f32_loss` through an UNMODIFIED LibKGE on the MI355X: float32 hip_complex (alone and under
hip_reciprocal_relations_model) with the option on (kge_ce_f32_fwd / kge_ce_f32_bwd, no [n, E] matrix) against the same
job with the option off (score_sp / score_po + the reference's loss) from the same initial parameters: batch 0, one
forward-only epoch, one epoch of SGD (Adagrad's first steps are +-lr whatever the gradient's size: rounding-level
differences of a gradient near zero become whole steps).  A small synthetic dataset (the reference's toy dataset is not
shipped).  Needs the reference package (oracle/ref_harness.py), like tests/test_gpu_libkge_plugin_ce_dist.py."""
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
    root = tmp_path_factory.mktemp("libkge_gpu_ce_f32")
    splits = make_splits(E, R, 4096, 256, 256, seed=3)
    folder = write_libkge_dataset(str(root / "small"), "small", E, R, splits)
    return str(root), folder


def _train_epoch(root, folder, tag, model, option, init_from=None, base=None, forward_only=False, batches=None,
                 extra=(), create_only=False):
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
    config.set("train.optimizer.default.type", "SGD")
    config.set("train.optimizer.default.args.lr", 0.5)
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
    config.set("hip_1vsAll.fused_f32_loss", option)
    for k, v in extra:
        config.set(k, v)
    torch.manual_seed(17)
    job = TrainingJob.create(config, Dataset.create(config, folder=folder), forward_only=forward_only)
    if create_only:
        return job
    if init_from is not None:
        job.model.load_state_dict(init_from)
    state0 = {k: v.detach().clone() for k, v in job.model.state_dict().items()}
    torch.manual_seed(23)
    job._prepare()
    if batches is not None:  # the first `batches` batches only, as run_epoch processes them
        losses = []
        for i, batch in enumerate(job.loader):
            if i >= batches:
                break
            job.optimizer.zero_grad()
            losses.append(job._process_batch(i, batch).avg_loss)
            job.optimizer.step()
        torch.cuda.synchronize()
        return job, sum(losses) / len(losses), state0
    trace = job.run_epoch()
    torch.cuda.synchronize()
    return job, trace["avg_loss"], state0


@pytest.fixture
def entered(monkeypatch):
    """Times the fused autograd function's forward was entered (kge_amd.model._FusedCEF32)."""
    from kge_amd import model as km
    calls = {"fused": 0}
    orig = km._FusedCEF32.forward

    def forward(ctx, *a, **k):
        calls["fused"] += 1
        return orig(ctx, *a, **k)

    monkeypatch.setattr(km._FusedCEF32, "forward", staticmethod(forward))
    return calls


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


@pytest.mark.parametrize("model,base", [("hip_complex", None), ("hip_reciprocal_relations_model", "hip_complex")])
def test_option_on_against_off(data, entered, model, base):
    """Batch 0, a forward-only epoch and an epoch of SGD (16 batches of 256): the avg_loss of the two runs within 2e-5
    relative (the bound of tests/test_gpu_libkge_plugin_ce_dist.py); after batch 0 the parameters within the same bound of
    their largest element.  The fused function is entered for both directions of every batch with the option on, never
    with it off."""
    root, folder = data
    tag = "rr_" if base else ""
    off0, l_off0, st = _train_epoch(root, folder, tag + "off0", model, False, base=base, batches=1)
    assert type(off0).__name__ == "HipTrainingJob1vsAll" and entered["fused"] == 0
    on0, l_on0, _ = _train_epoch(root, folder, tag + "on0", model, True, init_from=st, base=base, batches=1)
    assert entered["fused"] == 2, entered
    print(f"{model} batch 0: off {l_off0:.8g} on {l_on0:.8g} rel {_rel(l_on0, l_off0):.3e}")
    assert _rel(l_on0, l_off0) <= 2e-5
    for (k, x), (_, y) in zip(on0.model.state_dict().items(), off0.model.state_dict().items()):
        err = float((x - y).abs().max()) / max(1.0, float(y.abs().max()))
        print(f"{model} batch 0 {k}: max |diff| / scale {err:.3e}")
        assert err <= 2e-5, (k, err)
    for what, kw in (("forward-only epoch", {"forward_only": True}), ("SGD epoch", {})):
        entered["fused"] = 0
        _, l_off, _ = _train_epoch(root, folder, tag + "off", model, False, init_from=st, base=base, **kw)
        assert entered["fused"] == 0
        _, l_on, _ = _train_epoch(root, folder, tag + "on", model, True, init_from=st, base=base, **kw)
        assert entered["fused"] == 2 * 16, entered
        print(f"{model} {what}: avg_loss off {l_off:.8g} on {l_on:.8g} rel {_rel(l_on, l_off):.3e}")
        assert _rel(l_on, l_off) <= 2e-5, (what, l_on, l_off)


@pytest.mark.parametrize("extra", [(("lookup_embedder.dim", 36),),
                                   (("lookup_embedder.dim", 40), ("hip_complex.score_dtype", "bfloat16"))])
def test_unsupported_configurations_return_none(data, entered, extra):
    """Option on, parameters on the GPU, a dimension that is no multiple of 8 / tables scored in bfloat16 (at a dimension
    the bf16 loss kernels do not take either): `_ce_f32_tables()` is None and the model's loss hooks return None -- the
    job composes the loss from score_sp / score_po, the fused function is never entered."""
    root, folder = data
    job = _train_epoch(root, folder, "unsupported", "hip_complex", True, extra=extra, create_only=True)
    m = job.model.train()
    assert m._fused_f32_loss is True and m._fused() and m._ce_f32_tables() is None
    tri = torch.tensor([[1, 2, 3], [4, 5, 6]], device="cuda")
    assert m.loss_sp(tri[:, 0], tri[:, 1], tri[:, 2]) is None and m.loss_po(tri[:, 1], tri[:, 2], tri[:, 0]) is None
    assert m.loss_sp_po(tri[:, 0], tri[:, 1], tri[:, 2]) is None
    job._prepare()
    assert torch.isfinite(torch.tensor(job.run_epoch()["avg_loss"])) and entered["fused"] == 0
