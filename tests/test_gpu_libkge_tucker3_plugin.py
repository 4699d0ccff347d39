"""`model: hip_relational_tucker3` inside an unmodified LibKGE on the GPU, against the reference's `relational_tucker3` on
the same weights: the pattern of tests/test_gpu_libkge_rescal_plugin.py, on a toy dataset."""
import os
import shutil

import numpy as np
import pytest
import torch

import _tucker3_ref as tr
import ref_harness as rh

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]

E, R, D, DR = 60, 5, 12, 7
MODULES = ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"]
NAMES = ("_entity_embedder._embeddings.weight", "_relation_embedder.base_embedder._embeddings.weight",
         "_relation_embedder.projection.weight")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from kge_amd.synthetic import make_splits, write_libkge_dataset
    root = tmp_path_factory.mktemp("libkge_tucker3")
    splits = make_splits(E, R, 400, 60, 60, seed=3)
    return str(root), write_libkge_dataset(str(root / "toy"), "toy", E, R, splits)


def _config(root, tag, model, train_type="negative_sampling", opts=None, base=None):
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
    if base is not None:
        config._import(base)
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
    if model.endswith("relational_tucker3"):  # (under the reciprocal wrapper the base table keeps lookup_embedder.dim)
        config.set(model + ".relation_embedder.base_embedder.dim", DR, create=True)
    config.set("valid.every", 0)
    for k in ("default", "torch", "numpy", "python"):
        config.set(f"random_seed.{k}", 17)
    for k, v in (opts or {}).items():
        config.set(k, v, create=True)
    return config


def _model(root, folder, tag, model, state=None, opts=None, base=None):
    rh.import_reference()
    from kge import Dataset
    from kge.model import KgeModel
    config = _config(root, tag, model, opts=opts, base=base)
    dataset = Dataset.create(config, folder=folder)
    torch.manual_seed(17)
    m = KgeModel.create(config, dataset)
    if state is not None:
        m.load_state_dict(state)
    return config, dataset, m.eval()


def _within(got, ref, factor=1.0):
    want, e = ref
    got = got.detach().cpu().numpy().astype(np.float64).reshape(want.shape)
    err, b = np.abs(got - want), factor * tr.bound(e)
    assert np.isfinite(got).all() and (err <= b).all(), float((err / b).max())


def _refuse_reference_scorer(m):
    def boom(*a, **k):
        raise AssertionError("the reference scorer's score_emb was reached on cuda")
    m.get_scorer().score_emb = boom


def _np(m):
    sd = m.state_dict()
    return tuple(sd[k].detach().cpu().numpy() for k in NAMES)


def _batch(seed, n, Rn=R):
    g = torch.Generator().manual_seed(seed)
    s, p, o = (torch.randint(hi, (n,), generator=g) for hi in (E, Rn, E))
    return (s.numpy(), p.numpy(), o.numpy()), (s.cuda(), p.cuda(), o.cuda())


def test_scores_match_the_reference_weights_inside_the_bound(data):
    root, folder = data
    _, _, ref = _model(root, folder, "ref", "relational_tucker3")
    assert set(ref.state_dict().keys()) == set(NAMES)
    _, _, hip = _model(root, folder, "hip", "hip_relational_tucker3", ref.state_dict())
    assert hip._fused()
    _refuse_reference_scorer(hip)
    ent, B, W = _np(ref)
    assert B.shape == (R, DR) and W.shape == (D * D, DR)
    (sn, pn, on), (s, p, o) = _batch(1, 9)
    M, eM = tr.project(B, W, pn)
    sub = torch.tensor([5, 0, 5, 41], device="cuda")
    subn = sub.cpu().numpy()
    with torch.no_grad():
        _within(hip.score_spo(s, p, o, "o"), tr.score_spo(ent, M, eM, sn, on))
        _within(hip.score_sp(s, p), tr.score_pairs("sp_", ent, M, eM, sn))
        _within(hip.score_po(p, o), tr.score_pairs("_po", ent, M, eM, on))
        _within(hip.score_sp(s, p, sub), tr.score_pairs("sp_", ent, M, eM, sn, subn))
        both = hip.score_sp_po(s, p, o, sub)
        _within(both[:, :4], tr.score_pairs("sp_", ent, M, eM, sn, subn))
        _within(both[:, 4:], tr.score_pairs("_po", ent, M, eM, on, subn))
        assert hip.projections == 1, "one projection for the whole evaluation"
        # and the reference model itself (float32 torch: its own rounding and ours -- twice the bound)
        _within(hip.score_sp(s, p), (ref.score_sp(s, p).double().cpu().numpy(), tr.score_pairs("sp_", ent, M, eM, sn)[1]), 2.0)
        val, idx = hip.predict_o(s, p, 3)
        from kge_amd.model import topk_composed
        v2, i2 = topk_composed(hip.score_sp(s, p), 3)
        assert torch.equal(val, v2) and torch.equal(idx, i2)


@pytest.mark.parametrize("n", [3, 9])  # R > n: the "batch" route; R <= n: "all"
def test_parameter_gradients_match_the_reference_model(data, n):
    """d/d(parameters) of sum(g * score_sp) + sum(h * score_spo) through the reference model (torch autograd, float32) and
    through the plugin: both within the restatement's bound of the float64 value, so within twice of each other"""
    root, folder = data
    _, _, ref = _model(root, folder, "gref", "relational_tucker3")
    _, _, hip = _model(root, folder, "ghip", "hip_relational_tucker3", ref.state_dict())
    _refuse_reference_scorer(hip)
    ent, B, W = _np(ref)
    (sn, pn, on), (s, p, o) = _batch(5 + n, n)
    rng = np.random.default_rng(n)
    g, h = rng.standard_normal((n, E)).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    M, eM = tr.project(B, W, pn)
    ga, gm, gt = tr.pairs_bwd("sp_", ent, M, eM, sn, None, g)
    ga2, gm2, gx2 = tr.rows_bwd("sp_", ent, M, eM, sn, on[:, None], h[:, None])
    route = hip.route(n)
    assert route == ("all" if R <= n else "batch")

    def add(x, y):  # autograd adds the two nodes' gradients: one more rounded sum
        return x[0] + y[0], x[1] + y[1] + tr.U * (np.abs(x[0]) + x[1] + np.abs(y[0]) + y[1])

    def param_grads(gm_rows):  # one score call's relation-row gradients through its own projection backward
        if route == "all":
            GM, eGM = tr.table_grad(R, pn, *gm_rows)
            return tr.project_bwd(B, W, None, GM, eGM)
        rows, g_w_ = tr.project_bwd(B, W, pn, *gm_rows)
        return tr.base_grad(R, pn, *rows), g_w_

    g_ent = add(tr.accum([(np.arange(E), *gt), (sn, *ga)], (E, D)),
                tr.accum([(sn, *ga2), (on, gx2[0].reshape(n, D), gx2[1].reshape(n, D))], (E, D)))
    (b1, w1), (b2, w2) = param_grads(gm), param_grads(gm2)
    g_b, g_w = add(b1, b2), add(w1, w2)
    gt_, ht_ = torch.from_numpy(g).cuda(), torch.from_numpy(h).cuda()
    for m in (ref, hip):
        m.zero_grad()
        ((m.score_sp(s, p) * gt_).sum() + (m.score_spo(s, p, o, "o") * ht_).sum()).backward()
    for name, want in zip(NAMES, (g_ent, g_b, g_w)):
        got = dict(hip.named_parameters())[name].grad
        _within(got, want)
        _within(got, (dict(ref.named_parameters())[name].grad.double().cpu().numpy(), want[1]), 2.0)


class _Recorder:
    """Wraps the index-level score calls of a hip model: every call is recorded with its indexes, its float32 scores and
    -- through a tensor hook -- the gradient the job's loss hands back for them."""

    def __init__(self, model):
        self.nodes = []  # one list of [kind, s, p, o, neg, scores, gout] per autograd node
        self.model = model
        for name in ("score_sp", "score_po", "score_spo", "score_neg", "score_neg_blocks"):
            setattr(model, name, self._wrap(name, getattr(model, name)))

    def _rec(self, node, kind, s, p, o, neg, out):
        if out is None:
            return
        rec = [kind, s, p, o, neg, out.detach(), None]
        if out.requires_grad:
            out.register_hook(lambda g, rec=rec: rec.__setitem__(6, g.detach().clone() if rec[6] is None else rec[6] + g))
        node.append(rec)

    def _wrap(self, name, fn):
        def call(*a, **k):
            out = fn(*a, **k)
            assert not k or (name == "score_spo" and set(k) == {"direction"}), k
            node = []
            if name == "score_sp":
                assert len(a) == 2 or a[2] is None
                self._rec(node, "sp", a[0], a[1], None, None, out)
            elif name == "score_po":
                assert len(a) == 2 or a[2] is None
                self._rec(node, "po", None, a[0], a[1], None, out)
            elif name == "score_spo":
                self._rec(node, "spo", a[0], a[1], a[2], None, out)
            elif name == "score_neg":
                assert out is not None
                self._rec(node, "neg0" if a[3] == 0 else "neg2", a[0], a[1], a[2], a[4], out)
            else:
                assert out is not None
                s, p, o = a[:3]
                neg_s, neg_o = (list(a[3:]) + [None, None])[:2]
                self._rec(node, "spo", s, p, o, None, out[0])
                self._rec(node, "neg0", s, p, o, neg_s, out[1])
                self._rec(node, "neg2", s, p, o, neg_o, out[2])
            self.nodes.append(node)
            return out
        return call


def _cpu(x):
    return None if x is None else x.detach().cpu().numpy()


@pytest.mark.parametrize("ref_type,hip_type", [("1vsAll", "hip_1vsAll"), ("KvsAll", "hip_KvsAll"),
                                               ("negative_sampling", "hip_negative_sampling")])
def test_batch_losses_and_gradients_of_the_jobs_within_bound(data, ref_type, hip_type):
    """Three batches of each job, processed (forward + backward, no optimizer step) by the reference job on
    `relational_tucker3` and by the hip job on `hip_relational_tucker3` with the same weights.

    * every score the hip job's loss saw: within the restatement's bound;
    * the three parameter gradients the hip job leaves: within the restatement's bound of the float64 gradients for the
      float32 d loss / d score the job's loss handed back (recorded by hooks; taken as exact inputs, as the rules say);
    * the batch loss against the reference job's: both are the same float32 loss code on scores that are within e of
      the float64 scores, so each is within  sum |d loss / d score| e + sum e^2  (first order with the recorded gradient;
      the losses' second derivatives are at most 1 per score, scaled like the gradient) of the loss of the float64
      scores, plus its own rounding: a sum of T terms and a log-sum-exp over at most C scores per row, (T + C + 16) u
      (1 + |loss|) with T, C counted from the recorded calls.  The two evaluations: twice that."""
    rh.import_reference()
    from kge import Dataset
    from kge.job import TrainingJob
    root, folder = data
    jobs = {}
    for model, ttype in (("relational_tucker3", ref_type), ("hip_relational_tucker3", hip_type)):
        config = _config(root, f"b_{model}_{ttype}", model, ttype)
        dataset = Dataset.create(config, folder=folder)
        torch.manual_seed(17)
        job = TrainingJob.create(config, dataset)
        if jobs:
            job.model.load_state_dict(jobs["relational_tucker3"].model.state_dict())
            _refuse_reference_scorer(job.model)
        torch.manual_seed(23)
        job._prepare()
        job._is_prepared = True
        job.model.train()
        jobs[model] = job
    ref_job, hip_job = jobs["relational_tucker3"], jobs["hip_relational_tucker3"]
    hip = hip_job.model
    ent, B, W = _np(hip)
    rec = _Recorder(hip)
    out = {}
    for name, job in jobs.items():
        torch.manual_seed(29)
        batches = []
        for i, batch in enumerate(job.loader):
            if i == 3:
                break
            batches.append(batch)
        res = []
        for i, batch in enumerate(batches):
            torch.manual_seed(31 + i)
            job.model.zero_grad()
            del rec.nodes[:]
            r = job._process_batch(i, batch)
            grads = {k: v.grad.detach().clone() for k, v in job.model.named_parameters()}
            res.append((float(r.avg_loss), grads, [list(n) for n in rec.nodes] if job is hip_job else None))
        out[name] = res
    for (l_ref, g_ref, _), (l_hip, g_hip, nodes) in zip(out["relational_tucker3"], out["hip_relational_tucker3"]):
        assert nodes and np.isfinite(l_hip)
        per_node, first, second, T, C = [], 0.0, 0.0, 0, 0
        for node in nodes:
            p = _cpu(node[0][2])
            calls = []
            for kind, s, _, o, neg, scores, gout in node:
                s, o, neg = _cpu(s), _cpu(o), _cpu(neg)
                want = tr.call_scores(ent, B, W, p, kind, s, o, neg)
                _within(scores, want)
                assert gout is not None, "every recorded score is part of the loss"
                g = gout.double().cpu().numpy().reshape(want[0].shape)
                calls.append((kind, s, o, neg, g))
                e = tr.bound(want[1])
                first += float((np.abs(g) * e).sum())
                second += float((e * e).sum())
                T += g.size
                C = max(C, g.shape[-1] if g.ndim > 1 else 1)
            per_node.append(tr.node_grads(ent, B, W, p, hip.route(len(p)), calls))
        for k, name in enumerate(NAMES):
            _within(g_hip[name], tr.add_nodes([n[k] for n in per_node]))
        one = first + second + (T + C + 16) * tr.U * (1.0 + abs(l_hip))
        assert abs(l_hip - l_ref) <= 2.0 * one, (l_hip, l_ref, one)


@pytest.mark.parametrize("ref_type,hip_type", [("1vsAll", "hip_1vsAll"), ("KvsAll", "hip_KvsAll"),
                                               ("negative_sampling", "hip_negative_sampling")])
@pytest.mark.parametrize("optimizer", ["Adagrad", "HipAdagrad"])
def test_the_hip_training_jobs_run_with_this_model(data, ref_type, hip_type, optimizer):
    """one epoch (7 batches, the reference's Adagrad) of the reference job on `relational_tucker3` and of the hip job on
    `hip_relational_tucker3`, same initial weights and seeds: the loss tolerance of the RESCAL plugin test; then the
    unmodified entity_ranking and hip_entity_ranking: identical ranks"""
    rh.import_reference()
    from kge import Dataset
    from kge.job import EvaluationJob, TrainingJob
    root, folder = data
    runs = {}
    for model, ttype in (("relational_tucker3", ref_type), ("hip_relational_tucker3", hip_type)):
        opts = {"train.optimizer.default.type": optimizer} if model.startswith("hip_") else None
        config = _config(root, f"job_{model}_{ttype}_{optimizer}", model, ttype, opts=opts)
        dataset = Dataset.create(config, folder=folder)
        torch.manual_seed(17)
        job = TrainingJob.create(config, dataset)
        if runs:
            job.model.load_state_dict(runs["relational_tucker3"][2])
            _refuse_reference_scorer(job.model)
        state0 = {k: v.detach().clone() for k, v in job.model.state_dict().items()}
        torch.manual_seed(23)
        job._prepare()
        job._is_prepared = True
        trace = job.run_epoch()
        assert any(not torch.equal(v, state0[k]) for k, v in job.model.state_dict().items()), "the optimizer stepped"
        metrics = {}
        for etype in (("entity_ranking",) if model == "relational_tucker3" else ("entity_ranking", "hip_entity_ranking")):
            config.set("eval.type", etype)
            if etype.startswith("hip_"):
                config._import(etype)
            config.set("eval.batch_size", 32)
            result = EvaluationJob.create(config, dataset, parent_job=None, model=job.model).run()
            metrics[etype] = {k: v for k, v in result.items() if k.startswith(("mean_", "hits_at_"))}
        runs[model] = (trace, metrics, state0)
    (t_ref, m_ref, _), (t_hip, m_hip, _) = runs["relational_tucker3"], runs["hip_relational_tucker3"]
    assert all(torch.isfinite(torch.tensor(float(t[k]))) for t in (t_ref, t_hip) for k in ("avg_loss", "avg_cost"))
    # (an addition to test_batch_losses_and_gradients_of_the_jobs_within_bound, which holds the bounds: seven optimizer
    # steps apart, the loose epoch tolerance of the RESCAL plugin test)
    assert abs(t_hip["avg_loss"] - t_ref["avg_loss"]) <= 1e-4 * max(1.0, abs(t_ref["avg_loss"]))
    a, b = m_hip["entity_ranking"], m_hip["hip_entity_ranking"]
    assert set(a.keys()) == set(b.keys()) == set(m_ref["entity_ranking"].keys())
    assert 0.0 < a["mean_reciprocal_rank_filtered"] <= 1.0
    assert a == b, "entity_ranking and hip_entity_ranking: identical ranks"


def test_dropout_takes_the_reference_path(data):
    root, folder = data
    for key in ("hip_relational_tucker3.relation_embedder.dropout", "hip_relational_tucker3.entity_embedder.dropout",
                "hip_relational_tucker3.relation_embedder.base_embedder.dropout"):
        _, _, hip = _model(root, folder, "drop", "hip_relational_tucker3", opts={key: 0.5})
        assert hip._fused(), "evaluation mode: no dropout is active"
        hip.train()
        assert not hip._fused(), key
        (_, _, _), (s, p, o) = _batch(3, 5)
        out = hip.score_sp(s, p)  # the reference's score_sp: embedders + the scorer's bmm / mm
        assert out.shape == (5, E) and out.requires_grad and bool(torch.isfinite(out).all())


def test_reciprocal_relations_model_over_hip_relational_tucker3(data):
    """hip_reciprocal_relations_model over it with no special case: the base table gets 2 R rows and score_po(p, o) is
    the base model's fused score_sp(o, p + R)"""
    root, folder = data
    _, _, ref = _model(root, folder, "rref", "reciprocal_relations_model",
                       opts={"reciprocal_relations_model.base_model.type": "relational_tucker3"}, base="relational_tucker3")
    _, _, hip = _model(root, folder, "rhip", "hip_reciprocal_relations_model", ref.state_dict(),
                       opts={"hip_reciprocal_relations_model.base_model.type": "hip_relational_tucker3"},
                       base="hip_relational_tucker3")
    _refuse_reference_scorer(hip._base_model)
    ent, B, W = _np(ref._base_model)
    assert B.shape[0] == 2 * R and W.shape == (D * D, B.shape[1])
    (sn, pn, on), (s, p, o) = _batch(2, 7)
    M, eM = tr.project(B, W, pn)
    M2, eM2 = tr.project(B, W, pn + R)
    with torch.no_grad():
        _within(hip.score_sp(s, p), tr.score_pairs("sp_", ent, M, eM, sn))
        _within(hip.score_po(p, o), tr.score_pairs("sp_", ent, M2, eM2, on))
        both = hip.score_sp_po(s, p, o, None)
        _within(both[:, :E], tr.score_pairs("sp_", ent, M, eM, sn))
        _within(both[:, E:], tr.score_pairs("sp_", ent, M2, eM2, on))
        _within(hip.score_po(p, o), (ref.score_po(p, o).double().cpu().numpy(),
                                     tr.score_pairs("sp_", ent, M2, eM2, on)[1]), 2.0)


def test_checkpoint_interchange_and_refusals(data):
    root, folder = data
    _, _, ref = _model(root, folder, "cref", "relational_tucker3")
    _, _, hip = _model(root, folder, "chip", "hip_relational_tucker3")
    path = os.path.join(root, "t3.pt")
    torch.save(hip.state_dict(), path)
    ref.load_state_dict(torch.load(path))   # into the reference model ...
    torch.save(ref.state_dict(), path)
    _, _, hip2 = _model(root, folder, "chip2", "hip_relational_tucker3", torch.load(path))  # ... and back
    (_, _, _), (s, p, o) = _batch(4, 6)
    with torch.no_grad():
        assert torch.equal(hip2.score_sp(s, p), hip.score_sp(s, p))
    with pytest.raises(ValueError, match="fused_dist_loss"):
        hip._fused_dist_loss = True
    with pytest.raises(ValueError, match="fused_f32_loss"):
        hip._fused_f32_loss = True
    with pytest.raises(ValueError, match="touched_rows"):
        hip.set_touched_rows((torch.zeros(E, D, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")))
    z = torch.zeros(2, dtype=torch.long, device="cuda")
    assert hip.score_neg_shared(z, z, z, 2, z) is None and hip._rank_tables() is None
    # a penalty on the projection weight and the base embedder: the reference's own code
    _, _, pen = _model(root, folder, "pen", "hip_relational_tucker3",
                       opts={"hip_relational_tucker3.relation_embedder.regularize_weight": 0.1,
                             "hip_relational_tucker3.relation_embedder.base_embedder.regularize_weight": 0.1})
    terms = pen.penalty(batch={"triples": torch.zeros(2, 3, dtype=torch.long)}, num_batches=1)
    assert len(terms) == 2


def test_projected_table_cap_under_no_grad(data):
    """`projected_table_max_bytes` (hip_relational_tucker3.yaml): a table above it is not built without a recorded gradient
    -- the batch's rows are projected per call, with the same bits"""
    root, folder = data
    _, _, hip = _model(root, folder, "cap", "hip_relational_tucker3")
    assert hip.projected_table_max_bytes == 1 << 30
    (_, _, _), (s, p, o) = _batch(6, 8)
    with torch.no_grad():
        want = (hip.score_sp(s, p), hip.score_po(p, o), hip.score_sp_po(s, p, o), hip.score_spo(s, p, o, "o"))
        assert hip.projections == 1
        _, _, small = _model(root, folder, "cap2", "hip_relational_tucker3", hip.state_dict(),
                             opts={"hip_relational_tucker3.projected_table_max_bytes": R * D * D * 4 - 1})
        got = (small.score_sp(s, p), small.score_po(p, o), small.score_sp_po(s, p, o), small.score_spo(s, p, o, "o"))
        assert small.projections == 0 and small.route(8) == "batch"
        for a, b in zip(got, want):
            assert torch.equal(a, b)
