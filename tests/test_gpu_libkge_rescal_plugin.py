"""`model: hip_rescal` inside an unmodified LibKGE on the GPU, against the reference's `rescal` on the same weights: the
pattern (and the way to find the reference package) of tests/test_gpu_libkge_transh_plugin.py, on a toy dataset."""
import os
import shutil

import numpy as np
import pytest
import torch

import _rescal_ref as rr
import ref_harness as rh

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]

E, R, D = 60, 5, 12
MODULES = ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from kge_amd.synthetic import make_splits, write_libkge_dataset
    root = tmp_path_factory.mktemp("libkge_rescal")
    splits = make_splits(E, R, 400, 60, 60, seed=3)
    return str(root), write_libkge_dataset(str(root / "toy"), "toy", E, R, splits)


def _config(root, tag, model, train_type="negative_sampling", opts=None):
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
    config.set("train.type", train_type)
    if train_type.startswith("hip_"):
        config._import(train_type)
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


def _model(root, folder, tag, model, state=None):
    rh.import_reference()
    from kge import Dataset
    from kge.model import KgeModel
    config = _config(root, tag, model)
    dataset = Dataset.create(config, folder=folder)
    torch.manual_seed(17)
    m = KgeModel.create(config, dataset)
    if state is not None:
        m.load_state_dict(state)
    return config, dataset, m.eval()


def _within(got, ref):
    want, e = ref
    got = got.detach().cpu().numpy().astype(np.float64).reshape(want.shape)
    err, b = np.abs(got - want), rr.bound(e)
    assert np.isfinite(got).all() and (err <= b).all(), float((err / b).max())


def _refuse_reference_scorer(m):
    def boom(*a, **k):
        raise AssertionError("the reference scorer's score_emb was reached on cuda")
    m.get_scorer().score_emb = boom


def test_scores_match_the_reference_weights_inside_the_bound(data):
    root, folder = data
    _, _, ref = _model(root, folder, "ref", "rescal")
    _, _, hip = _model(root, folder, "hip", "hip_rescal", ref.state_dict())
    assert tuple(hip.get_p_embedder()._embeddings.weight.shape) == (R, D * D)
    _refuse_reference_scorer(hip)
    ent = ref.get_s_embedder()._embeddings.weight.detach().cpu().numpy()
    rel = ref.get_p_embedder()._embeddings.weight.detach().cpu().numpy()
    g = torch.Generator().manual_seed(1)
    s, p, o = (torch.randint(hi, (9,), generator=g) for hi in (E, R, E))
    sn, pn, on = s.numpy(), p.numpy(), o.numpy()
    s, p, o = s.cuda(), p.cuda(), o.cuda()
    sub = torch.tensor([5, 0, 5, 41], device="cuda")
    subn = sub.cpu().numpy()
    with torch.no_grad():
        _within(hip.score_spo(s, p, o, "o"), rr.score_spo(ent, rel, sn, pn, on))
        _within(hip.score_sp(s, p), rr.score_pairs("sp_", ent, rel, sn, pn))
        _within(hip.score_po(p, o), rr.score_pairs("_po", ent, rel, on, pn))
        _within(hip.score_sp(s, p, sub), rr.score_pairs("sp_", ent, rel, sn, pn, subn))
        both = hip.score_sp_po(s, p, o, sub)
        _within(both[:, :4], rr.score_pairs("sp_", ent, rel, sn, pn, subn))
        _within(both[:, 4:], rr.score_pairs("_po", ent, rel, on, pn, subn))
        # and the reference model itself (float32 torch: its own rounding and ours -- twice the bound)
        want = ref.score_sp(s, p).double().cpu().numpy()
        val, e = rr.score_pairs("sp_", ent, rel, sn, pn)
        assert (np.abs(hip.score_sp(s, p).double().cpu().numpy() - want) <= 2 * rr.bound(e)).all()
        val, idx = hip.predict_o(s, p, 3)
        from kge_amd.model import topk_composed
        v2, i2 = topk_composed(hip.score_sp(s, p), 3)
        assert torch.equal(val, v2) and torch.equal(idx, i2)


@pytest.mark.parametrize("ref_type,hip_type", [("1vsAll", "hip_1vsAll"), ("KvsAll", "hip_KvsAll"),
                                               ("negative_sampling", "hip_negative_sampling")])
def test_the_hip_training_jobs_run_with_this_model(data, ref_type, hip_type):
    """one epoch (7 batches) of the reference job on `rescal` and of the hip job on `hip_rescal`, same initial weights and
    seeds: the loss tolerance of the TransH plugin test; then the unmodified entity_ranking and hip_entity_ranking."""
    rh.import_reference()
    from kge import Dataset
    from kge.job import EvaluationJob, TrainingJob
    root, folder = data
    runs = {}
    for model, ttype in (("rescal", ref_type), ("hip_rescal", hip_type)):
        config = _config(root, f"job_{model}_{ttype}", model, ttype)
        dataset = Dataset.create(config, folder=folder)
        torch.manual_seed(17)
        job = TrainingJob.create(config, dataset)
        if runs:
            job.model.load_state_dict(runs["rescal"][2])
            _refuse_reference_scorer(job.model)
        state0 = {k: v.detach().clone() for k, v in job.model.state_dict().items()}
        torch.manual_seed(23)
        job._prepare()
        job._is_prepared = True
        trace = job.run_epoch()
        metrics = {}
        for etype in (("entity_ranking",) if model == "rescal" else ("entity_ranking", "hip_entity_ranking")):
            config.set("eval.type", etype)
            if etype.startswith("hip_"):
                config._import(etype)
            config.set("eval.batch_size", 32)
            result = EvaluationJob.create(config, dataset, parent_job=None, model=job.model).run()
            metrics[etype] = {k: v for k, v in result.items() if k.startswith(("mean_", "hits_at_"))}
        runs[model] = (trace, metrics, state0)
    (t_ref, m_ref, _), (t_hip, m_hip, _) = runs["rescal"], runs["hip_rescal"]
    assert all(torch.isfinite(torch.tensor(float(t[k]))) for t in (t_ref, t_hip) for k in ("avg_loss", "avg_cost"))
    assert abs(t_hip["avg_loss"] - t_ref["avg_loss"]) <= 1e-4 * max(1.0, abs(t_ref["avg_loss"]))
    a, b = m_hip["entity_ranking"], m_hip["hip_entity_ranking"]
    assert set(a.keys()) == set(b.keys()) == set(m_ref["entity_ranking"].keys())
    assert 0.0 < a["mean_reciprocal_rank_filtered"] <= 1.0
    assert abs(a["mean_reciprocal_rank_filtered"] - b["mean_reciprocal_rank_filtered"]) <= 1e-6


def test_reciprocal_relations_model_over_hip_rescal_on_the_fused_path(data):
    """hip_reciprocal_relations_model over hip_rescal (no special case, as over hip_transh): score_po(p, o) is the base
    model's fused score_sp(o, p + R)."""
    root, folder = data
    rec = {"reciprocal_relations_model.base_model.type": "rescal"}
    hrec = {"hip_reciprocal_relations_model.base_model.type": "hip_rescal"}
    rh.import_reference()
    from kge import Dataset
    from kge.model import KgeModel
    models = []
    for tag, model, opts, base in (("rref", "reciprocal_relations_model", rec, "rescal"),
                                   ("rhip", "hip_reciprocal_relations_model", hrec, "hip_rescal")):
        config = _config(root, tag, model, opts=opts)
        config._import(base)
        dataset = Dataset.create(config, folder=folder)
        torch.manual_seed(17)
        m = KgeModel.create(config, dataset)
        if models:
            m.load_state_dict(models[0].state_dict())
        models.append(m.eval())
    ref, hip = models
    _refuse_reference_scorer(hip._base_model)
    ent = ref._base_model.get_s_embedder()._embeddings.weight.detach().cpu().numpy()
    rel = ref._base_model.get_p_embedder()._embeddings.weight.detach().cpu().numpy()
    assert rel.shape == (2 * R, D * D)
    g = torch.Generator().manual_seed(2)
    s, p, o = (torch.randint(hi, (7,), generator=g) for hi in (E, R, E))
    sn, pn, on = s.numpy(), p.numpy(), o.numpy()
    s, p, o = s.cuda(), p.cuda(), o.cuda()
    with torch.no_grad():
        _within(hip.score_sp(s, p), rr.score_pairs("sp_", ent, rel, sn, pn))
        _within(hip.score_po(p, o), rr.score_pairs("sp_", ent, rel, on, pn + R))
        both = hip.score_sp_po(s, p, o, None)
        _within(both[:, :E], rr.score_pairs("sp_", ent, rel, sn, pn))
        _within(both[:, E:], rr.score_pairs("sp_", ent, rel, on, pn + R))
        want = ref.score_po(p, o).double().cpu().numpy()
        _, e = rr.score_pairs("sp_", ent, rel, on, pn + R)
        assert (np.abs(hip.score_po(p, o).double().cpu().numpy() - want) <= 2 * rr.bound(e)).all()


def test_options_without_a_rescal_kernel_are_refused_by_name(data):
    root, folder = data
    _, _, hip = _model(root, folder, "opt", "hip_rescal")
    with pytest.raises(ValueError, match="fused_dist_loss"):
        hip._fused_dist_loss = True
    with pytest.raises(ValueError, match="fused_f32_loss"):
        hip._fused_f32_loss = True
    hip._fused_dist_loss = False
    with pytest.raises(ValueError, match="touched_rows"):
        hip.set_touched_rows((torch.zeros(E, D, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")))
    s = torch.zeros(2, dtype=torch.long, device="cuda")
    assert hip.score_neg_shared(s, s, s, 2, s) is None and hip._rank_tables() is None
    assert hip._fused()
