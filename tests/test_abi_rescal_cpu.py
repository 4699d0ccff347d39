"""KGE_RESCAL at the C ABI without a device: the table checks, the one gate (entries without a RESCAL kernel answer
KGE_ERR_UNSUPPORTED before anything is launched), the workspace rule, and the Python front end's model."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT

INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -5
TAKES_RESCAL = {"kge_score_spo", "kge_score_sp", "kge_score_po", "kge_score_sp_po", "kge_score_neg", "kge_score_pairs_bwd",
                "kge_score_spo_bwd", "kge_score_spo_bwd_accum", "kge_score_neg_bwd_accum", "kge_rescal_queries"}
MAX_DIM = 256  # KGE_RESCAL_MAX_DIM


@pytest.fixture(scope="module")
def lib():
    from kge_amd import _lib
    _lib.build()
    return _lib.lib()


def _tables(dtype=0, scorer=5, dim=8, rel_dim=64, l_norm=1.0):
    from kge_amd._lib import KgeTables
    # non-NULL table pointers that are never dereferenced: every call below must return before a launch
    return KgeTables(4096, 8192, dtype, scorer, 10, 3, dim, rel_dim, dim, rel_dim, l_norm, 0)


def test_table_checks(lib):
    from kge_amd._lib import KgeIndex
    ix = KgeIndex(4096, 1, 0, 1)
    call = lambda t: lib.kge_score_spo(ctypes.byref(t), ix, ix, ix, 0, None, None)
    assert call(_tables()) == 0  # n == 0: accepted, nothing to do
    assert call(_tables(l_norm=0.0)) == 0 and call(_tables(l_norm=3.0)) == 0  # l_norm is ignored
    assert call(_tables(rel_dim=8)) == INVALID            # rel_dim != dim^2
    assert call(_tables(rel_dim=16)) == INVALID
    assert call(_tables(dim=32, rel_dim=32)) == INVALID
    assert call(_tables(dtype=1)) == UNSUPPORTED          # bf16
    assert call(_tables(dim=MAX_DIM, rel_dim=MAX_DIM ** 2)) == 0
    assert call(_tables(dim=MAX_DIM + 1, rel_dim=(MAX_DIM + 1) ** 2)) == UNSUPPORTED
    assert call(_tables(scorer=7, rel_dim=8)) == INVALID  # outside 0..5
    assert call(_tables(scorer=6, rel_dim=64)) == INVALID
    assert lib.kge_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "kge_amd.h")).read()
    assert "#define KGE_RESCAL_MAX_DIM %d" % MAX_DIM in header and "KGE_RESCAL = 5" in header
    t = _tables()
    assert lib.kge_rescal_queries(ctypes.byref(t), 1, ix, ix, 0, None, 8, None) == 0
    assert lib.kge_rescal_queries(ctypes.byref(t), 0, ix, ix, 1, 4096, 8, None) == INVALID  # dir
    assert lib.kge_rescal_queries(ctypes.byref(t), 1, ix, ix, 1, 4096, 7, None) == INVALID  # q_ld < dim
    assert lib.kge_rescal_queries_bytes(ctypes.byref(t), 5) == 5 * 8 * 4
    assert lib.kge_score_workspace_bytes(ctypes.byref(t), 5) == (2 * 5 * 8 + 8) * 4
    assert lib.kge_score_bwd_workspace_bytes(ctypes.byref(t), 5, 3) == 2 * 5 * 8 * 4
    for bad in (_tables(dtype=1), _tables(dim=MAX_DIM + 1, rel_dim=(MAX_DIM + 1) ** 2)):
        assert lib.kge_rescal_queries_bytes(ctypes.byref(bad), 5) == 0
        assert lib.kge_score_workspace_bytes(ctypes.byref(bad), 5) == 0


def test_a_missing_workspace_is_an_error_before_any_launch(lib):
    from kge_amd._lib import KgeIndex
    ix, all_ = KgeIndex(4096, 1, 0, 1), KgeIndex(None, 1, 0, 1)
    t = _tables()
    need = lib.kge_score_workspace_bytes(ctypes.byref(t), 2)
    for ws, nbytes in ((None, 0), (None, need), (4096, need // 2 - 4)):
        assert lib.kge_score_sp(ctypes.byref(t), ix, ix, 2, all_, 10, 4096, 10, ws, nbytes, None) == WORKSPACE
        assert lib.kge_score_po(ctypes.byref(t), ix, ix, 2, all_, 10, 4096, 10, ws, nbytes, None) == WORKSPACE
    assert lib.kge_score_sp_po(ctypes.byref(t), ix, ix, ix, 2, all_, 10, 4096, 20, 4096, need - 4, None) == WORKSPACE
    assert lib.kge_score_sp(ctypes.byref(t), ix, ix, 0, all_, 10, None, 10, None, 0, None) == 0  # n == 0
    bneed = lib.kge_score_bwd_workspace_bytes(ctypes.byref(t), 2, 10)
    assert lib.kge_score_pairs_bwd(ctypes.byref(t), 1, ix, ix, 2, all_, 10, 4096, 10, None, 0, 4096, 4096, 4096, None, 0,
                                   None) == WORKSPACE
    assert lib.kge_score_pairs_bwd(ctypes.byref(t), 1, ix, ix, 2, all_, 10, 4096, 10, None, 0, 4096, 4096, 4096, 4096,
                                   bneed - 4, None) == WORKSPACE


def test_every_other_entry_declines_a_rescal_table(lib):
    from kge_amd import _lib
    t = _tables()
    checked = []
    for name, (res, args) in _lib.PROTOTYPES.items():
        if not args or args[0] is not _lib._PT or name in TAKES_RESCAL or res is not ctypes.c_int:
            continue
        vals = [ctypes.byref(t)]
        for a in args[1:]:
            if a is _lib.KgeIndex:
                vals.append(_lib.KgeIndex(4096, 1, 0, 1))
            elif a in (ctypes.c_int64, ctypes.c_int, ctypes.c_int32):
                vals.append(1)
            elif a in (ctypes.c_float, ctypes.c_double):
                vals.append(1.0)
            else:
                vals.append(None)
        assert getattr(lib, name)(*vals) == UNSUPPORTED, name
        checked.append(name)
    for must in ("kge_eval_batch", "kge_topk", "kge_score_rank_sp_po", "kge_ce_fwd", "kge_ce_dist_fwd", "kge_ce_f32_fwd",
                 "kge_kl_dist_fwd", "kge_bce_f32_bwd", "kge_score_neg_shared", "kge_score_neg_shared_bwd_accum",
                 "kge_score_neg_bwd_accum_sorted", "kge_score_emb", "kge_score_emb_bwd", "kge_score_emb_sp_po",
                 "kge_build_queries", "kge_score_queries", "kge_shard_gather", "kge_embed", "kge_multilabel2_bwd_accum"):
        assert must in checked, must
    assert lib.kge_topk_workspace_bytes(ctypes.byref(t), 4, 10, 3, 0) == 0
    assert lib.kge_ce_dist_workspace_bytes(ctypes.byref(t), 4, 0) == 0
    assert lib.kge_queries_bytes(ctypes.byref(t), 1, 4) == 0
    # kge_rescal_queries declines the five other scorers
    ix = _lib.KgeIndex(4096, 1, 0, 1)
    for scorer, dim, rel_dim in ((0, 8, 8), (1, 8, 8), (2, 8, 8), (3, 8, 4), (4, 8, 16)):
        other = _tables(scorer=scorer, dim=dim, rel_dim=rel_dim)
        assert lib.kge_rescal_queries(ctypes.byref(other), 1, ix, ix, 1, None, 8, None) == UNSUPPORTED, scorer
        assert lib.kge_rescal_queries_bytes(ctypes.byref(other), 4) == 0


def test_front_end_builds_the_model():
    from kge_amd import _lib, engine, model
    assert _lib.SCORERS["rescal"] == 5 and engine.SCORERS["rescal"] == 5 and engine.RESCAL_MAX_DIM == MAX_DIM
    m = model.create("rescal", 40, 5, 6)
    assert isinstance(m, model.Rescal) and isinstance(m.get_scorer(), model.RescalScorer)
    assert tuple(m.get_p_embedder().weight.shape) == (5, 36) and tuple(m.get_s_embedder().weight.shape) == (40, 6)
    g = torch.Generator().manual_seed(0)
    s, p, o = torch.randint(40, (6,), generator=g), torch.randint(5, (6,), generator=g), torch.randint(40, (6,), generator=g)
    se, pe, oe = m.get_s_embedder().embed(s), m.get_p_embedder().embed(p), m.get_o_embedder().embed(o)
    sc = m.get_scorer()  # the torch form of the scorer (dense embeddings)
    sp = sc.score_emb(se, pe, m.get_o_embedder().embed_all(), "sp_")
    po = sc.score_emb(m.get_s_embedder().embed_all(), pe, oe, "_po")
    spo = sc.score_emb(se, pe, oe, "spo").view(-1)
    assert sp.shape == (6, 40) and po.shape == (6, 40)
    assert torch.allclose(sp[torch.arange(6), o], spo, rtol=1e-5, atol=1e-6)
    assert torch.allclose(po[torch.arange(6), s], spo, rtol=1e-5, atol=1e-6)
    for bad in (dict(fused_dist_loss=True), dict(fused_f32_loss=True)):
        with pytest.raises(ValueError, match="|".join(bad)):
            model.create("rescal", 40, 5, 6, **bad)
    with pytest.raises(ValueError, match="dim"):
        model.create("rescal", 4, 1, MAX_DIM + 1)
    with pytest.raises(ValueError, match="touched_rows"):
        m.set_touched_rows((torch.zeros(40, 6), torch.zeros(2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="score_neg_shared"):
        m.score_neg_shared(s, p, o, 2, torch.arange(4))


def test_plugin_yaml_loads_through_the_reference_config():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness as rh
    if not rh.available():
        pytest.skip("reference package `kge` not on this box")
    rh.import_reference()
    from kge import Config, Dataset
    from kge.model import KgeModel
    config = Config()
    config.folder = None
    config.set("console.quiet", True)
    config.set("modules", ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"])
    config.set("model", "hip_rescal")
    config._import("hip_rescal")
    config.set("job.device", "cpu")
    config.set("lookup_embedder.dim", 5)
    config.set("dataset.num_entities", 20)
    config.set("dataset.num_relations", 3)
    assert config.get("hip_rescal.class_name") == "HipRescal"
    assert config.get("hip_rescal.relation_embedder.dim") == -1
    m = KgeModel.create(config, Dataset(config, folder=None))
    from kge_amd.libkge_plugin import HipRescal, HipRescalScorer
    assert isinstance(m, HipRescal) and isinstance(m.get_scorer(), HipRescalScorer)
    assert config.get("hip_rescal.relation_embedder.dim") == 25
    assert tuple(m.get_p_embedder()._embeddings.weight.shape) == (3, 25)
    s, p = torch.tensor([1, 2]), torch.tensor([0, 2])
    with torch.no_grad():
        assert tuple(m.score_sp(s, p).shape) == (2, 20)
    assert m.score_neg_shared(s, p, s, 0, s) is None and m._rank_tables() is None
    with pytest.raises(ValueError, match="touched_rows"):
        m.set_touched_rows((1, 2))
    with pytest.raises(ValueError, match="fused_f32_loss"):
        m._fused_f32_loss = True


def test_reciprocal_relations_model_over_hip_rescal_is_built_like_over_hip_transh(tmp_path):
    """hip_reciprocal_relations_model has no special case for its base model: over hip_rescal the relation embedder gets
    2 R rows of dim^2 (rescal_set_relation_embedder_dim under the wrapper's configuration key), and it scores."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_harness as rh
    if not rh.available():
        pytest.skip("reference package `kge` not on this box")
    rh.import_reference()
    from kge import Config, Dataset
    from kge.model import KgeModel
    from kge_amd.synthetic import make_splits, write_libkge_dataset
    folder = write_libkge_dataset(str(tmp_path / "toy"), "toy", 20, 3, make_splits(20, 3, 60, 10, 10, seed=3))
    config = Config()
    config.folder = None
    config.set("console.quiet", True)
    config.set("modules", ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"])
    config.set("model", "hip_reciprocal_relations_model")
    config._import("hip_reciprocal_relations_model")
    config.set("hip_reciprocal_relations_model.base_model.type", "hip_rescal")
    config._import("hip_rescal")
    config.set("dataset.name", "toy")
    config.set("job.device", "cpu")
    config.set("lookup_embedder.dim", 5)
    m = KgeModel.create(config, Dataset.create(config, folder=folder))
    from kge_amd.libkge_plugin import HipRescal
    assert isinstance(m._base_model, HipRescal)
    assert tuple(m._base_model.get_p_embedder()._embeddings.weight.shape) == (6, 25)
    s, p = torch.tensor([1, 2]), torch.tensor([0, 2])
    with torch.no_grad():
        sp, po, both = m.score_sp(s, p), m.score_po(p, s), m.score_sp_po(s, p, s, None)
    assert tuple(sp.shape) == (2, 20) and tuple(both.shape) == (2, 40)
    assert torch.equal(both[:, :20], sp) and torch.equal(both[:, 20:], po)
