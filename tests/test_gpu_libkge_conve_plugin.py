"""`hip_reciprocal_relations_model` over `hip_conve` inside an unmodified LibKGE on the GPU, against the reference's
`reciprocal_relations_model` over `conve` from one checkpoint: the pattern of tests/test_gpu_libkge_rescal_plugin.py on a
toy dataset.  Evaluation scores within the bound of tests/_conve_ref.py, the wrapper's delegations, an unmodified
entity_ranking pass, ranks identical at eval.batch_size 7 and 64, one KvsAll and one 1vsAll epoch (dropouts 0) under
Adagrad and HipAdagrad, and the declined options."""
import os
import shutil

import numpy as np
import pytest
import torch

import _conve_ref as cr
import ref_harness as rh

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]

E, R, D = 60, 5, 8   # d = 8: h = 2, w = 4
MODULES = ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"]
NO_DROPOUT = {"entity_embedder.dropout": 0.0, "relation_embedder.dropout": 0.0, "feature_map_dropout": 0.0,
              "projection_dropout": 0.0}


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from kge_amd.synthetic import make_splits, write_libkge_dataset
    root = tmp_path_factory.mktemp("libkge_conve")
    splits = make_splits(E, R, 400, 60, 60, seed=3)
    return str(root), write_libkge_dataset(str(root / "toy"), "toy", E, R, splits)


def _config(root, tag, hip, train_type="KvsAll", opts=None):
    rh.import_reference()
    from kge import Config
    model, base = ("hip_reciprocal_relations_model", "hip_conve") if hip else ("reciprocal_relations_model", "conve")
    config = Config()
    config.folder = os.path.join(root, tag)
    shutil.rmtree(config.folder, ignore_errors=True)
    os.makedirs(config.folder)
    config.set("console.quiet", True)
    config.set("modules", MODULES)
    config.set("model", model)
    config._import(model)
    config.set(model + ".base_model.type", base)
    config._import(base)
    config.set("dataset.name", "toy")
    config.set("job.device", "cuda")
    config.set("train.type", train_type)
    config.set("train.max_epochs", 1)
    config.set("train.batch_size", 64)
    config.set("train.num_workers", 0)
    config.set("lookup_embedder.dim", D)
    config.set("valid.every", 0)
    for k, v in NO_DROPOUT.items():
        config.set(base + "." + k, v)
    for k in ("default", "torch", "numpy", "python"):
        config.set(f"random_seed.{k}", 17)
    for k, v in (opts or {}).items():
        config.set(k, v, create=True)
    return config


def _pair(root, folder):
    """(reference model, hip model) on one state_dict, in eval mode, with running statistics that are not the initial
    0 / 1"""
    rh.import_reference()
    from kge import Dataset
    from kge.model import KgeModel
    models = []
    for tag, hip in (("ref", False), ("hip", True)):
        config = _config(root, tag, hip)
        dataset = Dataset.create(config, folder=folder)
        torch.manual_seed(17)
        m = KgeModel.create(config, dataset)
        if models:
            m.load_state_dict(models[0].state_dict())
        else:
            sc = m._base_model.get_scorer()
            g = torch.Generator().manual_seed(5)
            with torch.no_grad():
                for bn in (sc.bn1, sc.bn2):
                    bn.running_mean.copy_(0.2 * torch.randn(bn.running_mean.shape, generator=g))
                    bn.running_var.copy_(0.5 + torch.rand(bn.running_var.shape, generator=g))
        models.append(m.eval())
    return models


def _net_of(base):
    sc = base.get_scorer()
    c = lambda x: x.detach().cpu().numpy()  # noqa: E731
    fs = int(sc.filter_size)
    return dict(h=int(sc.emb_height), w=int(sc.emb_width), fs=fs, pad=int(sc.padding),
                conv_w=c(sc.convolution.weight).reshape(32, fs, fs),
                conv_b=None if sc.convolution.bias is None else c(sc.convolution.bias), mean1=c(sc.bn1.running_mean),
                var1=c(sc.bn1.running_var), eps1=sc.bn1.eps, proj_w=c(sc.projection.weight), proj_b=c(sc.projection.bias),
                mean2=c(sc.bn2.running_mean), var2=c(sc.bn2.running_var), eps2=sc.bn2.eps)


def _within(got, ref, what):
    want, e = ref
    got = got.detach().cpu().numpy().astype(np.float64).reshape(want.shape)
    err, b = np.abs(got - want), cr.bound(e)
    print("{}: max err / bound = {:.4f}".format(what, float((err / b).max())))
    assert np.isfinite(got).all() and (err <= b).all(), what


def test_scores_delegations_and_declined_options(data):
    root, folder = data
    ref, hip = _pair(root, folder)
    base = hip._base_model
    assert type(base).__name__ == "HipConvE" and type(base.get_scorer()).__name__ == "HipConvEScorer"
    assert list(hip.state_dict()) == list(ref.state_dict())
    assert tuple(base.get_s_embedder()._embeddings.weight.shape) == (E, D + 1)
    assert tuple(base.get_p_embedder()._embeddings.weight.shape) == (2 * R, D + 1)
    net = _net_of(base)
    ent = base.get_s_embedder()._embeddings.weight.detach().cpu().numpy()
    rel = base.get_p_embedder()._embeddings.weight.detach().cpu().numpy()
    g = torch.Generator().manual_seed(1)
    s, p, o = (torch.randint(hi, (9,), generator=g) for hi in (E, R, E))
    sn, pn, on = s.numpy(), p.numpy(), o.numpy()
    s, p, o = s.cuda(), p.cuda(), o.cuda()
    sub = torch.tensor([5, 0, 5, 41], device="cuda")
    subn = sub.cpu().numpy()
    with torch.no_grad():
        assert hip._base_fused() and base.kernel_route()
        _within(hip.score_sp(s, p), cr.score_sp(net, ent, rel, sn, pn), "score_sp")
        _within(hip.score_po(p, o), cr.score_sp(net, ent, rel, on, pn + R), "score_po = base.score_sp(o, p + R)")
        _within(hip.score_spo(s, p, o, "o"), cr.score_spo(net, ent, rel, sn, pn, on), "score_spo o")
        _within(hip.score_spo(s, p, o, "s"), cr.score_spo(net, ent, rel, on, pn + R, sn), "score_spo s")
        both = hip.score_sp_po(s, p, o, sub)
        _within(both[:, :4], cr.score_sp(net, ent, rel, sn, pn, subn), "score_sp_po, sp")
        _within(both[:, 4:], cr.score_sp(net, ent, rel, on, pn + R, subn), "score_sp_po, po")
        assert base.routes == {"kernel": 6, "torch": 0}, "every delegation landed on HipConvE's kernel route"
        # the reference model itself (float32 torch: its own rounding and ours -- twice the bound of a sum in any order)
        want = ref.score_po(p, o).double().cpu().numpy()
        _, e = cr.score_sp(net, ent, rel, on, pn + R, order="any")
        assert (np.abs(hip.score_po(p, o).double().cpu().numpy() - want) <= 2 * cr.bound(e)).all()
        from kge_amd.model import topk_composed
        for (val, idx), sc in ((hip.predict_o(s, p, 3), hip.score_sp(s, p)), (hip.predict_s(p, o, 3), hip.score_po(p, o))):
            v2, i2 = topk_composed(sc, 3)
            assert torch.equal(val, v2) and torch.equal(idx, i2)
    # a recorded gradient: the torch route, inside the bound of a sum in any order
    k0 = base.routes["kernel"]
    _within(hip.score_sp(s, p), cr.score_sp(net, ent, rel, sn, pn, order="any"), "torch route score_sp")
    assert base.routes["kernel"] == k0 and base.routes["torch"] == 1
    # what does not apply declines by name
    with pytest.raises(ValueError, match="ConvE can only score objects"):
        base.score_spo(s, p, o, "s")
    with pytest.raises(Exception, match="Combine _po not supported"):
        base.score_po(p, o)
    with pytest.raises(Exception, match="Combine _po not supported"):
        base.score_sp_po(s, p, o)
    for name in ("_fused_dist_loss", "_fused_f32_loss"):
        with pytest.raises(ValueError, match=name.lstrip("_")):
            setattr(base, name, True)
    with pytest.raises(ValueError, match="touched_rows"):
        base.set_touched_rows((torch.zeros(E, D + 1, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")))
    for call in (lambda: base.score_neg(s, p, o, 2, s.view(-1, 1)), lambda: base.score_neg_shared(s, p, o, 2, s),
                 lambda: base.score_neg_blocks(s, p, o, None, s.view(-1, 1))):
        with pytest.raises(ValueError, match="negative-sampling blocks"):
            call()
    assert base._rank_tables() is None and base._ce_tables() is None


def test_entity_ranking_and_identical_ranks_at_batch_sizes_7_and_64(data):
    """the property the feature exists for: on the hip model the ranks do not move with eval.batch_size"""
    rh.import_reference()
    from kge import Dataset
    from kge.job import EvaluationJob
    root, folder = data
    ref, hip = _pair(root, folder)
    results = {}
    for tag, model, is_hip in (("ref", ref, False), ("hip", hip, True)):
        for bs in (7, 64):
            config = _config(root, f"eval_{tag}_{bs}", is_hip)
            config.set("eval.type", "entity_ranking")
            config.set("eval.batch_size", bs)
            config.set("entity_ranking.hits_at_k_s", [1, 3, 10])
            dataset = Dataset.create(config, folder=folder)
            job = EvaluationJob.create(config, dataset, parent_job=None, model=model)
            result = job.run()
            results[tag, bs] = {k: v for k, v in result.items() if k.startswith(("mean_", "hits_at_"))}
    a, b = results["hip", 7], results["hip", 64]
    assert a.keys() == b.keys() == results["ref", 64].keys() and len(a) > 4
    assert a == b, "identical metrics (every rank identical) at eval.batch_size 7 and 64"
    assert 0.0 < a["mean_reciprocal_rank_filtered"] <= 1.0
    assert hip._base_model.routes["kernel"] > 0 and hip._base_model.routes["torch"] == 0
    # the scores themselves, bit for bit, whatever the batch the triple stands in: every rank follows from them
    triples = dataset.split("test").cuda()
    s, p, o = triples[:, 0], triples[:, 1], triples[:, 2]
    with torch.no_grad():
        whole = hip.score_sp_po(s, p, o, None)
        for bs in (7, 64):
            parts = [hip.score_sp_po(s[i:i + bs], p[i:i + bs], o[i:i + bs], None) for i in range(0, len(s), bs)]
            assert torch.equal(torch.cat(parts), whole), bs
        true = whole.gather(1, torch.stack((o, s + E), 1))
        ranks = (whole.view(len(s), 2, E) > true.unsqueeze(2)).sum(2)
        for bs in (7, 64):
            parts = [hip.score_sp_po(s[i:i + bs], p[i:i + bs], o[i:i + bs], None) for i in range(0, len(s), bs)]
            got = torch.cat(parts)
            assert torch.equal((got.view(len(s), 2, E) > got.gather(1, torch.stack((o, s + E), 1)).unsqueeze(2)).sum(2),
                               ranks), "every triple's raw rank, both directions"


@pytest.mark.parametrize("train_type", ["KvsAll", "1vsAll"])
@pytest.mark.parametrize("optimizer", ["Adagrad", "HipAdagrad"])
def test_one_training_epoch_matches_the_reference_job(data, train_type, optimizer):
    """one epoch of the unmodified reference job, dropouts 0, batch statistics on, the same initial weights and seeds: the
    reference over `conve` with Adagrad, the hip model with Adagrad / HipAdagrad (the loss tolerance of the RESCAL and
    TransH plugin tests) on the epoch's loss; every parameter moved, by the torch route"""
    rh.import_reference()
    from kge import Dataset
    from kge.job import TrainingJob
    root, folder = data
    runs = []
    for hip in (False, True):
        opts = {"train.optimizer.default.type": optimizer if hip else "Adagrad"}
        config = _config(root, f"train_{hip}_{train_type}_{optimizer}", hip, train_type, opts)
        dataset = Dataset.create(config, folder=folder)
        torch.manual_seed(17)
        job = TrainingJob.create(config, dataset)
        if runs:
            job.model.load_state_dict(runs[0][1])
        state0 = {k: v.detach().clone() for k, v in job.model.state_dict().items()}
        torch.manual_seed(23)
        job._prepare()
        job._is_prepared = True
        trace = job.run_epoch()
        runs.append((trace, state0, {k: v.detach().clone() for k, v in job.model.state_dict().items()}, job.model))
    (t_ref, s0, s_ref, _), (t_hip, _, s_hip, m_hip) = runs
    assert all(np.isfinite(float(t[k])) for t in (t_ref, t_hip) for k in ("avg_loss", "avg_cost"))
    assert abs(t_hip["avg_loss"] - t_ref["avg_loss"]) <= 1e-4 * max(1.0, abs(t_ref["avg_loss"]))
    base = m_hip._base_model
    assert base.routes["torch"] > 0 and base.routes["kernel"] == 0, "training mode: the torch route"
    for k in s0:
        if "num_batches_tracked" in k:
            continue
        assert not torch.equal(s_hip[k], s0[k]), k + " did not move"
    # (the updated parameters are NOT compared with the reference job's: Adagrad divides a gradient by its own running
    # magnitude, so a gradient that is rounding noise -- convolution.bias under batch statistics, which bn1's mean
    # subtraction cancels exactly in real arithmetic -- moves its parameter by about the learning rate in a direction no
    # rounding bound predicts; on an MI355X the two jobs' convolution.bias differ by as much as the update itself)


SUFFIXES = {"_entity_embedder._embeddings.weight": "ent", "_relation_embedder._embeddings.weight": "rel",
            "_scorer.convolution.weight": "conv_w", "_scorer.convolution.bias": "conv_b",
            "_scorer.projection.weight": "proj_w", "_scorer.projection.bias": "proj_b"}


def _names(model):
    """{parameter name of the (wrapped) model: key of tests/_conve_train_ref.py}; the wrapper shares the base model's
    modules, so named_parameters lists each once under whichever path it meets first"""
    out = {}
    for name, _ in model.named_parameters():
        hit = [v for k, v in SUFFIXES.items() if name.endswith(k)]
        assert len(hit) == 1, name
        out[name] = hit[0]
    assert sorted(out.values()) == sorted(SUFFIXES.values())
    return out


@pytest.mark.parametrize("train_type", ["KvsAll", "1vsAll"])
def test_first_batch_loss_and_gradients_of_the_jobs_within_bound(data, train_type):
    """The first batch of the unmodified job (forward + backward, no optimizer step, dropouts 0, batch statistics on) by
    the reference job over `conve` and by the same job over `hip_conve`, from identical weights -- the method of
    test_gpu_libkge_tucker3_plugin.py:

    * every score the hip job's loss saw (one base-model score_sp call per direction, each with its own batch
      statistics): within the bound of tests/_conve_train_ref.py;
    * every parameter gradient the hip job leaves: within that file's bound of the float64 gradients for the float32
      d loss / d score the job's loss handed back (recorded by hooks; taken as exact inputs), the calls' bounds added and
      one more rounded sum per extra call.  convolution.bias and projection.bias, whose true gradients are 0 under batch
      statistics, stay under their absolute floor;
    * the batch loss against the reference job's: each is the same float32 loss code on scores within e of the float64
      scores, so each is within  sum |d loss / d score| e + sum e^2 + (T + C + 16) u (1 + |loss|)  of the loss of the
      float64 scores (T scores in all, C per row); the two evaluations: twice that."""
    import _conve_train_ref as tr
    rh.import_reference()
    from kge import Dataset
    from kge.job import TrainingJob
    root, folder = data
    jobs = []
    for hip in (False, True):
        config = _config(root, f"b_{hip}_{train_type}", hip, train_type)
        dataset = Dataset.create(config, folder=folder)
        torch.manual_seed(17)
        job = TrainingJob.create(config, dataset)
        if jobs:
            job.model.load_state_dict(jobs[0].model.state_dict())
        torch.manual_seed(23)
        job._prepare()
        job._is_prepared = True
        job.model.train()
        jobs.append(job)
    ref_job, hip_job = jobs
    base = hip_job.model._base_model
    calls = []
    inner = base.score_sp

    def recorded(s, p, o=None):
        out = inner(s, p, o)
        assert o is None
        rec = [s.detach().cpu().numpy(), p.detach().cpu().numpy(), out.detach(), None]
        out.register_hook(lambda g, rec=rec: rec.__setitem__(3, g.detach().clone() if rec[3] is None else rec[3] + g))
        calls.append(rec)
        return out
    base.score_sp = recorded
    NAMES = _names(hip_job.model)
    P = {v: dict(hip_job.model.named_parameters())[k].detach().double().cpu().numpy() for k, v in NAMES.items()}
    sc = base.get_scorer()
    res = []
    for job in jobs:
        torch.manual_seed(29)
        batch = next(iter(job.loader))
        torch.manual_seed(31)
        job.model.zero_grad()
        r = job._process_batch(0, batch)
        res.append((float(r.avg_loss), {k: v.grad.detach().clone() for k, v in job.model.named_parameters()}))
    (l_ref, _), (l_hip, g_hip) = res
    assert calls and base.routes["kernel"] == 0 and base.routes["torch"] == len(calls)
    total, first, second, T, C = {}, 0.0, 0.0, 0, 0
    for s, p, scores, gout in calls:
        assert gout is not None, "every recorded score is part of the loss"
        g = gout.double().cpu().numpy()
        want, e, grads, unstable = tr.node(P, int(sc.emb_height), int(sc.emb_width), int(sc.padding), sc.bn1.eps,
                                           sc.bn2.eps, s, p, g)
        err = np.abs(scores.double().cpu().numpy() - want)
        print("{} call of {} rows: scores max err / bound = {:.4f}, {} unstable units".format(
            train_type, len(s), float((err / e).max()), unstable))
        assert (err <= e).all()
        first += float((np.abs(g) * e).sum())
        second += float((e * e).sum())
        T += g.size
        C = max(C, g.shape[1])
        for k, (val, tol) in grads.items():
            if k in total:
                v0, t0 = total[k]
                total[k] = (v0 + val, t0 + tol + tr.U * (np.abs(v0) + np.abs(val) + t0 + tol))
            else:
                total[k] = (val, tol)
    assert set(total) == set(NAMES.values())
    for name, k in NAMES.items():
        val, tol = total[k]
        err = np.abs(g_hip[name].double().cpu().numpy().reshape(val.shape) - val)
        print("{} gradient of {}: max err / bound = {:.4f}; median |gradient| / bound = {:.2f}".format(
            train_type, k, float((err / tol).max()), float(np.median(np.abs(val) / tol))))
        assert (err <= tol).all(), k
    for k in ("conv_b", "proj_b"):
        assert np.abs(total[k][0]).max() < 1e-9, "the true gradient of a bias in front of batch statistics is 0"
    one = first + second + (T + C + 16) * tr.U * (1.0 + abs(l_hip))
    print("{} batch loss: hip {:.8f} reference {:.8f}, |difference| / bound = {:.4f}".format(
        train_type, l_hip, l_ref, abs(l_hip - l_ref) / (2.0 * one)))
    assert np.isfinite(l_hip) and abs(l_hip - l_ref) <= 2.0 * one, (l_hip, l_ref, one)
