"""`model: hip_transh` inside an unmodified LibKGE on the GPU, against the reference's `transh` on the same weights: the
pattern (and the way to find the reference package) of tests/test_gpu_libkge_plugin.py, on a toy dataset -- the
reference's score_sp / score_po hold [m, n, d]."""
import os
import shutil

import pytest
import torch

import ref_harness as rh

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]

E, R, D = 60, 5, 33
MODULES = ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from kge_amd.synthetic import make_splits, write_libkge_dataset
    root = tmp_path_factory.mktemp("libkge_transh")
    splits = make_splits(E, R, 400, 60, 60, seed=3)
    return str(root), write_libkge_dataset(str(root / "toy"), "toy", E, R, splits)


def _config(root, tag, model, opts=None):
    rh.import_reference()
    from kge import Config
    config = Config()
    config.folder = os.path.join(root, tag)
    shutil.rmtree(config.folder, ignore_errors=True)
    os.makedirs(config.folder)
    config.set("console.quiet", True)
    config.set("modules", MODULES)
    config.set("model", model)
    config._import(model)
    config.set("dataset.name", "toy")
    config.set("job.device", "cuda")
    config.set("train.type", "negative_sampling")
    config.set("train.max_epochs", 1)
    config.set("train.batch_size", 64)
    config.set("train.num_workers", 0)
    config.set("negative_sampling.num_samples.s", 4)
    config.set("negative_sampling.num_samples.o", 4)
    config.set("lookup_embedder.dim", D)
    config.set("valid.every", 0)
    for k in ("default", "torch", "numpy", "python"):
        config.set(f"random_seed.{k}", 17)
    for k, v in (opts or {}).items():
        config.set(k, v, create=True)
    return config


def _model(root, folder, tag, model, opts=None, state=None):
    rh.import_reference()
    from kge import Dataset
    from kge.model import KgeModel
    config = _config(root, tag, model, opts)
    dataset = Dataset.create(config, folder=folder)
    torch.manual_seed(17)
    m = KgeModel.create(config, dataset)
    if state is not None:
        m.load_state_dict(state)
    return config, dataset, m.eval()


def _close(got, want):
    # the tolerance of the TransE plugin cases (test_gpu_libkge_plugin.py: _rel(a, b) <= 1e-4), per score
    assert got.shape == want.shape
    assert bool(((got - want).abs() <= 1e-4 * want.abs().clamp_min(1.0)).all()), float((got - want).abs().max())


@pytest.mark.parametrize("lp", [1.0, 2.0])
def test_scores_match_the_reference_model_on_the_same_weights(data, lp):
    root, folder = data
    _, _, ref = _model(root, folder, f"ref{lp}", "transh", {"transh.l_norm": lp})
    _, _, hip = _model(root, folder, f"hip{lp}", "hip_transh", {"hip_transh.l_norm": lp}, ref.state_dict())
    assert tuple(hip.get_p_embedder()._embeddings.weight.shape) == (R, 2 * D)
    g = torch.Generator().manual_seed(1)
    s, p, o = (torch.randint(hi, (9,), generator=g).cuda() for hi in (E, R, E))
    sub = torch.tensor([5, 0, 5, 41], device="cuda")
    with torch.no_grad():
        _close(hip.score_spo(s, p, o, "o"), ref.score_spo(s, p, o, "o"))
        _close(hip.score_sp(s, p), ref.score_sp(s, p))
        _close(hip.score_po(p, o), ref.score_po(p, o))
        _close(hip.score_sp(s, p, sub), ref.score_sp(s, p, sub))
        _close(hip.score_sp_po(s, p, o, None), ref.score_sp_po(s, p, o, None))
        _close(hip.score_sp_po(s, p, o, sub), ref.score_sp_po(s, p, o, sub))
        val, idx = hip.predict_o(s, p, 3)
        from kge_amd.model import topk_composed
        v2, i2 = topk_composed(hip.score_sp(s, p), 3)
        assert torch.equal(val, v2) and torch.equal(idx, i2)


def test_penalty_is_the_reference_models(data):
    root, folder = data
    _, _, ref = _model(root, folder, "pref", "transh", {"transh.C": 0.5})
    _, _, hip = _model(root, folder, "phip", "hip_transh", {"hip_transh.C": 0.5}, ref.state_dict())
    kw = dict(batch={"triples": torch.zeros(2, 3, dtype=torch.long)}, num_batches=1)
    a, b = ref.penalty(**kw), hip.penalty(**kw)
    assert [k for k, _ in a] == [k for k, _ in b] == ["transh.soft_constraints_ent", "transh.soft_constraints_rel"]
    for (_, x), (_, y) in zip(a, b):
        assert torch.allclose(x, y, rtol=1e-6, atol=0) and float(x) > 0
    _, _, hip0 = _model(root, folder, "phip0", "hip_transh")
    assert hip0.penalty(**kw) == []


def test_negative_sampling_then_entity_ranking_through_the_unmodified_jobs(data):
    rh.import_reference()
    from kge.job import EvaluationJob, TrainingJob
    root, folder = data
    runs = {}
    for model in ("transh", "hip_transh"):
        from kge import Dataset
        config = _config(root, "job_" + model, model)
        dataset = Dataset.create(config, folder=folder)
        torch.manual_seed(17)
        job = TrainingJob.create(config, dataset)
        if runs:
            job.model.load_state_dict(runs["transh"][2])
        state0 = {k: v.detach().clone() for k, v in job.model.state_dict().items()}
        torch.manual_seed(23)
        job._prepare()
        job._is_prepared = True
        trace = job.run_epoch()
        config.set("eval.type", "entity_ranking")
        config.set("eval.batch_size", 32)
        result = EvaluationJob.create(config, dataset, parent_job=None, model=job.model).run()
        runs[model] = (trace, {k: v for k, v in result.items() if k.startswith(("mean_", "hits_at_"))}, state0)
    (t_ref, m_ref, _), (t_hip, m_hip, _) = runs["transh"], runs["hip_transh"]
    assert all(torch.isfinite(torch.tensor(float(t[k]))) for t in (t_ref, t_hip) for k in ("avg_loss", "avg_cost"))
    assert abs(t_hip["avg_loss"] - t_ref["avg_loss"]) <= 1e-4 * max(1.0, abs(t_ref["avg_loss"]))
    assert set(m_hip.keys()) == set(m_ref.keys())
    assert "mean_reciprocal_rank_filtered" in m_hip and 0.0 < m_hip["mean_reciprocal_rank_filtered"] <= 1.0


def test_options_without_a_transh_kernel_are_refused_by_name(data):
    root, folder = data
    _, _, hip = _model(root, folder, "opt", "hip_transh")
    with pytest.raises(ValueError, match="fused_dist_loss"):
        hip._fused_dist_loss = True
    with pytest.raises(ValueError, match="fused_f32_loss"):
        hip._fused_f32_loss = True
    hip._fused_dist_loss = False
    with pytest.raises(ValueError, match="touched_rows"):
        hip.set_touched_rows((torch.zeros(E, D, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")))
    s = torch.zeros(2, dtype=torch.long, device="cuda")
    assert hip.score_neg_shared(s, s, s, 2, s) is None and hip._rank_tables() is None
