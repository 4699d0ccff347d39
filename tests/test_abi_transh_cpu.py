"""KGE_TRANSH at the C ABI without a device: the table checks, the one gate (entries without a TransH kernel answer
KGE_ERR_UNSUPPORTED before anything is launched), and the Python front end's model."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT

INVALID, UNSUPPORTED = -1, -2
TAKES_TRANSH = {"kge_score_spo", "kge_score_sp", "kge_score_po", "kge_score_sp_po", "kge_score_neg", "kge_score_pairs_bwd",
                "kge_score_spo_bwd", "kge_score_spo_bwd_accum", "kge_score_neg_bwd_accum"}


@pytest.fixture(scope="module")
def lib():
    from kge_amd import _lib
    _lib.build()
    return _lib.lib()


def _tables(dtype=0, scorer=4, dim=32, rel_dim=64, l_norm=1.0):
    from kge_amd._lib import KgeTables
    # non-NULL table pointers that are never dereferenced: every call below must return before a launch
    return KgeTables(4096, 8192, dtype, scorer, 10, 3, dim, rel_dim, dim, rel_dim, l_norm, 0)


def test_table_checks(lib):
    from kge_amd._lib import KgeIndex
    ix = KgeIndex(4096, 1, 0, 1)
    call = lambda t: lib.kge_score_spo(ctypes.byref(t), ix, ix, ix, 0, None, None)
    assert call(_tables()) == 0  # n == 0: accepted, nothing to do
    assert call(_tables(rel_dim=32)) == INVALID          # rel_dim != 2 dim
    assert call(_tables(rel_dim=16)) == INVALID
    assert call(_tables(dtype=1)) == UNSUPPORTED         # bf16
    assert call(_tables(l_norm=3.0)) == UNSUPPORTED      # a p without a kernel
    assert call(_tables(l_norm=0.0)) == INVALID
    assert call(_tables(dim=2048, rel_dim=4096)) == UNSUPPORTED
    assert call(_tables(scorer=7, rel_dim=32)) == INVALID  # outside 0..4
    assert call(_tables(scorer=5, rel_dim=32)) == INVALID
    assert lib.kge_abi_version() == 1


def test_every_other_entry_declines_a_transh_table(lib):
    """Every entry that takes kge_tables and has no TransH kernel: KGE_ERR_UNSUPPORTED, whatever else it is given."""
    from kge_amd import _lib
    t = _tables()
    checked = []
    for name, (res, args) in _lib.PROTOTYPES.items():
        if not args or args[0] is not _lib._PT or name in TAKES_TRANSH or res is not ctypes.c_int:
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
    # the size queries of those entries: no workspace for a table they do not take
    assert lib.kge_topk_workspace_bytes(ctypes.byref(t), 4, 10, 3, 0) == 0
    assert lib.kge_ce_dist_workspace_bytes(ctypes.byref(t), 4, 0) == 0
    assert lib.kge_queries_bytes(ctypes.byref(t), 1, 4) == 0


def test_front_end_builds_the_model():
    from kge_amd import _lib, engine, model
    assert _lib.SCORERS["transh"] == 4 and engine.SCORERS["transh"] == 4
    m = model.create("transh", 40, 5, 16, l_norm=2.0)
    assert isinstance(m, model.TransH) and isinstance(m.get_scorer(), model.TransHScorer)
    assert tuple(m.get_p_embedder().weight.shape) == (5, 32) and tuple(m.get_s_embedder().weight.shape) == (40, 16)
    # the torch form of the scorer (dense embeddings): sp_ / _po columns equal the spo form on the expanded triples
    g = torch.Generator().manual_seed(0)
    s, p, o = torch.randint(40, (6,), generator=g), torch.randint(5, (6,), generator=g), torch.randint(40, (6,), generator=g)
    se, pe, oe = m.get_s_embedder().embed(s), m.get_p_embedder().embed(p), m.get_o_embedder().embed(o)
    sc = m.get_scorer()
    sp = sc.score_emb(se, pe, m.get_o_embedder().embed_all(), "sp_")
    po = sc.score_emb(m.get_s_embedder().embed_all(), pe, oe, "_po")
    spo = sc.score_emb(se, pe, oe, "spo").view(-1)
    assert sp.shape == (6, 40) and po.shape == (6, 40)
    assert torch.allclose(sp[torch.arange(6), o], spo, rtol=1e-5, atol=1e-6)
    assert torch.allclose(po[torch.arange(6), s], spo, rtol=1e-4, atol=1e-4)  # (the _po form shifts EPS: 2e-6 per coordinate)
    for bad in (dict(fused_dist_loss=True), dict(l_norm=3.0)):
        with pytest.raises(ValueError, match="|".join(bad)):
            model.create("transh", 40, 5, 16, **bad)
    with pytest.raises(ValueError, match="touched_rows"):
        m.set_touched_rows((torch.zeros(40, 16), torch.zeros(2, dtype=torch.int32)))


def test_plugin_yaml_loads_through_the_reference_config():
    """hip_transh.yaml through the reference's Config: the class, the options of transh.yaml, and the relation
    embedder's dimension doubled by the model's constructor (relation_embedder.dim: -1)."""
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
    config.set("model", "hip_transh")
    config._import("hip_transh")
    config.set("job.device", "cpu")
    config.set("lookup_embedder.dim", 12)
    config.set("dataset.num_entities", 20)
    config.set("dataset.num_relations", 3)
    assert config.get("hip_transh.class_name") == "HipTransH"
    assert config.get("hip_transh.l_norm") == 1.0 and config.get("hip_transh.C") == 0.0
    assert config.get("hip_transh.relation_embedder.dim") == -1
    m = KgeModel.create(config, Dataset(config, folder=None))
    from kge_amd.libkge_plugin import HipTransH, HipTransHScorer
    assert isinstance(m, HipTransH) and isinstance(m.get_scorer(), HipTransHScorer)
    assert config.get("hip_transh.relation_embedder.dim") == 24
    assert tuple(m.get_p_embedder()._embeddings.weight.shape) == (3, 24)
    assert tuple(m.get_s_embedder()._embeddings.weight.shape) == (20, 12)
    # on the CPU the model is the reference's: score_sp through the reference scorer's own score_emb
    s, p = torch.tensor([1, 2]), torch.tensor([0, 2])
    with torch.no_grad():
        assert tuple(m.score_sp(s, p).shape) == (2, 20)
    config.set("hip_transh.l_norm", 3.0)
    with pytest.raises(ValueError, match="l_norm"):
        KgeModel.create(config, Dataset(config, folder=None))
