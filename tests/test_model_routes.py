"""Which fused autograd node each public call of a kge_amd.model model takes -- per family and mode -- and the exact text
of every refusal.  The forward of the eleven route nodes is wrapped with a recorder (the pattern of
test_gpu_libkge_plugin_multilabel_f32.py::entered); a call's route is the list of nodes it entered, in order.  The
plugin's surface is pinned by test_libkge_plugin_cpu.py and the test_gpu_libkge_*plugin*.py files."""
import pytest
import torch

from kge_amd import model as km

NODES = ("_ScoreSPO", "_ScoreNeg", "_ScoreNegBlocks", "_ScorePairs", "_ScoreSO", "_ScoreNegShared", "_ScoreSPODropout",
         "_ScoreNegDropout", "_FusedCE2", "_FusedCE2Sum", "_FusedMultiLabel2")
SPO, NEG, BLOCKS, PAIRS, SO, SHARED, SPO_DROP, NEG_DROP, CE2, CE2_SUM, ML2 = NODES
E, R, N = 67, 5, 9  # E odd: the padded pitch differs from E
FAMILIES = ("complex", "distmult", "transe", "rotate", "transh", "rescal", "relational_tucker3", "conve")
DIM = {"rescal": 8, "relational_tucker3": 8, "conve": 32}  # (ConvE: the 4 x 8 image); the others 16
NO_CPU = "The MI355X engine has no CPU path"


@pytest.fixture
def entered(monkeypatch):
    calls = []
    for name in NODES:
        cls = getattr(km, name)

        def forward(ctx, *a, _orig=cls.forward, _name=name, **k):
            calls.append(_name)
            return _orig(ctx, *a, **k)
        monkeypatch.setattr(cls, "forward", staticmethod(forward))
    return calls


def create(family, device=None, **kw):
    torch.manual_seed(0)
    if family == "relational_tucker3":
        kw.setdefault("rel_base_dim", 4)
    return km.create(family, E, R, DIM.get(family, 16), device=device, **kw)


def batch(device=None, n=N):
    g = torch.Generator().manual_seed(1)
    s, p, o = (torch.randint(hi, (n,), generator=g).to(device) for hi in (E, R, E))
    neg = torch.randint(E, (n, 3), generator=g).to(device)
    unique = torch.randperm(E, generator=g)[:4].to(device)
    repeat = torch.randint(4, (2,), generator=g).to(device)
    rowptr = torch.arange(n + 1, dtype=torch.int64)
    return dict(s=s, p=p, o=o, neg=neg, unique=unique, repeat=repeat, rowptr=rowptr.to(device), col=o.long())


def calls(m, b):
    """the public calls, by the name the tables below use"""
    s, p, o, neg, rowptr, col = b["s"], b["p"], b["o"], b["neg"], b["rowptr"], b["col"]
    spo_kw = {"direction": "o"} if isinstance(m, km.ConvE) else {}
    return {
        "score_spo": lambda: m.score_spo(s, p, o, **spo_kw),
        "score_neg": lambda: m.score_neg(s, p, o, 0, neg),
        "score_neg_slot1": lambda: m.score_neg(s, p, o, 1, neg % R),
        "score_neg_shared": lambda: m.score_neg_shared(s, p, o, 2, b["unique"], None, b["repeat"]),
        "score_neg_blocks": lambda: m.score_neg_blocks(s, p, o, neg, neg),
        "score_sp": lambda: m.score_sp(s, p),
        "score_po": lambda: m.score_po(p, o),
        "score_so": lambda: m.score_so(s, o),
        "score_sp_po": lambda: m.score_sp_po(s, p, o),
        "predict_o": lambda: m.predict_o(s, p, 3),
        "loss_sp": lambda: m.loss_sp(s, p, o),
        "loss_sp_po": lambda: m.loss_sp_po(s, p, o),
        "loss_sp_po_sum": lambda: m.loss_sp_po_sum(s, p, o, 0.5),
        "multilabel": lambda: m.multilabel_loss_sp_po("kl", s, p, rowptr, col, o, p, rowptr, col),
        "multilabel_smoothed": lambda: m.multilabel_loss_sp_po("kl", s, p, rowptr, col, o, p, rowptr, col,
                                                               label_smoothing=0.1),
    }


def route(entered, fn):
    del entered[:]
    fn()
    return list(entered)


def check(entered, m, b, table):
    """table: call -> the nodes entered in order, or (exception type, full text)"""
    fns = calls(m, b)
    for name, want in table.items():
        if isinstance(want, tuple):
            with pytest.raises(want[0]) as err:
                fns[name]()
            assert str(err.value) == want[1], (type(m).__name__, name)
        else:
            assert route(entered, fns[name]) == want, (type(m).__name__, name)


def conve_table():
    """score_sp and score_spo(direction="o") on the routes of ConveRoutes (no node); whatever needs score_po refused"""
    no_po = (Exception, "Combine _po not supported in ConvE's score function")
    blocks = "ConvE: negative-sampling blocks ({}) are not supported"
    table = {name: [] for name in ("score_spo", "score_sp", "predict_o", "loss_sp")}
    table.update({name: no_po for name in ("score_po", "score_sp_po", "loss_sp_po", "loss_sp_po_sum", "multilabel",
                                           "multilabel_smoothed")})
    table.update(score_so=(Exception, "Combine s_o not supported in ConvE's score function"),
                 score_neg=(ValueError, blocks.format("score_neg")),
                 score_neg_slot1=(ValueError, blocks.format("score_neg")),
                 score_neg_shared=(ValueError, blocks.format("score_neg_shared")),
                 score_neg_blocks=(ValueError, blocks.format("score_neg_blocks")))
    return table


def shared_refusal(label, grouped=False):
    return (ValueError, "{}: {}shared negative samples (score_neg_shared) are not supported; use score_neg".format(
        label, "grouped: " if grouped else ""))


# ---- CPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("transh", "rescal", "relational_tucker3", "conve"))
def test_cpu_dropout_in_training_mode_composes_every_call(entered, family):
    """not `_fused()`: the scorers with a torch form compose every call, no node is entered"""
    m = create(family, entity_args={"dropout": 0.2})
    m.train()
    table = {name: [] for name in calls(m, batch())}
    if family in ("rescal", "relational_tucker3"):
        table["score_neg_shared"] = shared_refusal(type(m).__name__)
    if family == "conve":
        table = conve_table()
    check(entered, m, batch(), table)
    if family == "conve":
        assert m.routes["kernel"] == 0 and m.routes["torch"] > 0


@pytest.mark.parametrize("family", ("complex", "distmult", "transe", "rotate"))
def test_cpu_dropout_in_training_mode_reaches_no_node(entered, family):
    """not `_fused()`: every call goes the composed way, whose dense-row scorer (kge_score_emb) has no CPU path"""
    m = create(family, entity_args={"dropout": 0.2})
    m.train()
    for name, fn in calls(m, batch()).items():
        del entered[:]
        with pytest.raises(RuntimeError, match=NO_CPU):
            fn()
        assert entered == [], name


@pytest.mark.parametrize("family", FAMILIES[:7])
def test_cpu_plain_lookups_choose_the_gpu_route(entered, family):
    """`_fused()` holds in eval mode whatever the device: each call enters the node it would on a GPU, and that node's
    first step (engine.Tables) refuses the CPU tables -- except where a gate asks for the device first"""
    m = create(family)
    m.eval()
    fns = calls(m, batch())
    plain = family in ("complex", "distmult", "transe", "rotate")
    want = {"score_spo": [SPO], "score_neg": [NEG], "score_neg_slot1": [SPO], "score_sp": [PAIRS], "score_po": [PAIRS],
            "score_sp_po": [PAIRS], "loss_sp": [PAIRS], "loss_sp_po": [PAIRS], "loss_sp_po_sum": [PAIRS],
            "multilabel": [PAIRS], "multilabel_smoothed": [PAIRS],
            # neg_blocks_fusable and score_so_fusable ask for a GPU table, predict_o for a GPU device: composed
            "score_neg_blocks": [SPO], "predict_o": [PAIRS],
            "score_neg_shared": [SHARED] if plain else [NEG]}
    for name, nodes in want.items():
        if name == "score_neg_shared" and family in ("rescal", "relational_tucker3"):
            continue
        del entered[:]
        with pytest.raises(RuntimeError, match=NO_CPU):
            fns[name]()
        assert entered == nodes, (family, name)
    if plain:  # composed score_so: kge_score_emb has no CPU path
        with pytest.raises(RuntimeError, match=NO_CPU):
            fns["score_so"]()
    else:  # the torch form of the scorer
        assert route(entered, fns["score_so"]) == []
    with torch.no_grad():  # engine.score_sp_po on tables(): no node
        del entered[:]
        with pytest.raises(RuntimeError, match=NO_CPU):
            fns["score_sp_po"]()
        assert entered == []


def test_cpu_refusals_full_text():
    pair = (torch.zeros(E, 16), torch.zeros(3, dtype=torch.int32))
    losses = "{}: {} is not supported (the losses are composed from score_sp / score_po)"
    for family in ("complex", "distmult", "transe", "rotate", "transh", "conve"):
        with pytest.raises(ValueError) as err:
            create(family, grouped=True)
        assert str(err.value) == "{}: grouped is a route of the RESCAL kernels (rescal, relational_tucker3)".format(
            type(create(family)).__name__)
    with pytest.raises(ValueError) as err:
        create("rescal", grouped=True, fused_dropout=True)
    assert str(err.value) == "Rescal: grouped: fused_dropout is not supported"
    for family, label, opts in (("transh", "TransH", ("fused_dist_loss",)),
                                ("rescal", "Rescal", ("fused_dist_loss", "fused_f32_loss")),
                                ("relational_tucker3", "Rescal", ("fused_dist_loss", "fused_f32_loss"))):
        for opt in opts:
            with pytest.raises(ValueError) as err:
                create(family, **{opt: True})
            assert str(err.value) == losses.format(label, opt)
    for opt, value in (("fused_dist_loss", True), ("fused_f32_loss", True), ("score_dtype", torch.bfloat16)):
        with pytest.raises(ValueError) as err:
            create("conve", **{opt: value})
        assert str(err.value) == "ConvE: {} is not supported (the losses are composed from score_sp)".format(opt)
    for family, kw, text in (("transh", {}, "TransH: touched_rows is not supported"),
                             ("rescal", {}, "Rescal: touched_rows is not supported"),
                             ("rescal", {"grouped": True}, "Rescal: grouped: touched_rows is not supported"),
                             ("relational_tucker3", {}, "RelationalTucker3: touched_rows is not supported"),
                             ("relational_tucker3", {"grouped": True},
                              "RelationalTucker3: grouped: touched_rows is not supported"),
                             ("conve", {}, "ConvE: touched_rows is not supported")):
        m = create(family, **kw)
        with pytest.raises(ValueError) as err:
            m.set_touched_rows(pair)
        assert str(err.value) == text
        m.set_touched_rows(None)
        assert m._touched_rows is None
    m = create("complex")
    with pytest.raises(ValueError) as err:
        m.set_touched_rows(None, pair)
    assert str(err.value) == "ComplEx: the relation table's touched rows need the entity table's"
    m.set_touched_rows(pair, pair)
    assert m._touched_rows == (pair, pair)
    m.set_touched_rows(pair)
    assert m._touched_rows is pair
    b = batch()
    for family, kw, want in (("rescal", {}, shared_refusal("Rescal")),
                             ("rescal", {"grouped": True}, shared_refusal("Rescal", grouped=True)),
                             ("relational_tucker3", {}, shared_refusal("RelationalTucker3")),
                             ("relational_tucker3", {"grouped": True}, shared_refusal("RelationalTucker3"))):
        with pytest.raises(want[0]) as err:
            calls(create(family, **kw), b)["score_neg_shared"]()
        assert str(err.value) == want[1]
    m = create("conve")
    with pytest.raises(ValueError) as err:
        m.score_spo(b["s"], b["p"], b["o"])
    assert str(err.value) == "ConvE can only score objects"
    with pytest.raises(Exception) as err:
        m.predict_s(b["p"], b["o"], 3)
    assert str(err.value) == "Combine _po not supported in ConvE's score function"
    with pytest.raises(ValueError) as err:
        m.tables()
    assert str(err.value) == "ConvE: there are no kge_tables of a ConvE model (its score is not a function of three rows)"


# ---- GPU ---------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
ALL4 = ("complex", "distmult", "transe", "rotate")
# float32 tables, plain lookups, a recorded gradient: the same in train and eval mode
PLAIN = {"score_spo": [SPO], "score_neg": [NEG], "score_neg_slot1": [SPO], "score_neg_shared": [SHARED],
         "score_neg_blocks": [BLOCKS], "score_sp": [PAIRS], "score_po": [PAIRS], "score_so": [SO],
         "score_sp_po": [PAIRS, PAIRS], "predict_o": [], "loss_sp": [PAIRS], "loss_sp_po": [PAIRS, PAIRS],
         "loss_sp_po_sum": [PAIRS, PAIRS], "multilabel": [PAIRS, PAIRS], "multilabel_smoothed": [PAIRS, PAIRS]}
# no kge_topk, kge_score_so, kge_score_neg_shared kernel: composed from score_sp, the scorer's torch form, score_neg
TRIPLE_ONLY = dict(PLAIN, predict_o=[PAIRS], score_so=[], score_neg_shared=[NEG])


def gpu_table(family):
    if family in ALL4:
        return dict(PLAIN)
    table = dict(TRIPLE_ONLY)
    if family != "transh":
        table["score_neg_shared"] = shared_refusal({"rescal": "Rescal"}.get(family, "RelationalTucker3"))
    return table


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES[:7])
def test_gpu_plain_lookups(entered, family):
    m, b = create(family, DEV), batch(DEV)
    table = gpu_table(family)
    for training in (True, False):
        m.train(training)
        check(entered, m, b, table)
    with torch.no_grad():  # score_sp_po: one launch of the engine on tables(), no node; the rest as under autograd
        check(entered, m, b, dict(table, score_sp_po=[]))
    if family == "relational_tucker3":  # n < R: the "batch" route, the same nodes on the batch's projected rows
        small = batch(DEV, 3)
        assert m.route(3) == "batch" and m.route(N) == "all"
        check(entered, m, small, table)
        with torch.no_grad():
            assert m.route(3) == "all"
            check(entered, m, small, dict(table, score_sp_po=[]))
        for name in ("score_spo", "score_neg", "score_neg_blocks", "score_sp", "score_po"):
            fn = getattr(m, name)
            args = {"score_spo": (small["s"], small["p"], small["o"]),
                    "score_neg": (small["s"], small["p"], small["o"], 0, small["neg"]),
                    "score_neg_blocks": (small["s"], small["p"], small["o"], small["neg"], small["neg"]),
                    "score_sp": (small["s"], small["p"]), "score_po": (small["p"], small["o"])}[name]
            for project in ("all", "batch"):
                assert route(entered, lambda: fn(*args, project=project)) == PLAIN[name], (name, project)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ALL4)
def test_gpu_touched_rows(entered, family):
    """the pair reaches the nodes of score_spo / score_neg / score_neg_blocks / score_so: the same routes, and the
    backward leaves the entity table's .grad None"""
    m, b = create(family, DEV), batch(DEV)
    ent = m._entity_embedder.weight
    from kge_amd import engine
    pair = (torch.zeros_like(ent).detach(), engine.touched_bitmap(E, ent.device))
    for on in (True, False):
        m.set_touched_rows(pair if on else None)
        check(entered, m, b, PLAIN)
        for name in ("score_spo", "score_neg", "score_neg_blocks", "score_so"):
            m.zero_grad(set_to_none=True)
            out = calls(m, b)[name]()
            (out[0] if isinstance(out, tuple) else out).sum().backward()
            assert (ent.grad is None) == on, (name, on)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES[:7])
def test_gpu_entity_dropout(entered, family):
    """entity dropout 0.2 in training mode: composed, unless fused_dropout puts score_spo / score_neg (and what is composed
    from them) on the dropout nodes -- the four scorers with plain lookup embedders only; eval mode: the plain routes"""
    b = batch(DEV)
    composed = {name: [] for name in PLAIN}
    if family in ("rescal", "relational_tucker3"):
        composed["score_neg_shared"] = gpu_table(family)["score_neg_shared"]
    for fused_dropout in (False, True):
        m = create(family, DEV, entity_args={"dropout": 0.2}, fused_dropout=fused_dropout)
        m.train()
        table = dict(composed)
        if fused_dropout and family in ALL4:
            table.update(score_spo=[SPO_DROP], score_neg=[NEG_DROP], score_neg_slot1=[SPO_DROP],
                         score_neg_shared=[NEG_DROP], score_neg_blocks=[SPO_DROP, NEG_DROP, NEG_DROP])
        calls_before = m._dropout_clock.call
        check(entered, m, b, table)
        assert m._dropout_clock.call - calls_before == sum(len(v) for v in table.values() if isinstance(v, list))
        m.eval()
        check(entered, m, b, gpu_table(family))


@pytest.mark.gpu
@pytest.mark.parametrize("family", ("rescal", "relational_tucker3"))
def test_gpu_grouped(entered, family):
    m, b = create(family, DEV, grouped=True), batch(DEV)
    label = type(m).__name__
    table = dict(gpu_table(family), score_neg_shared=shared_refusal(label, grouped=(family == "rescal")))
    check(entered, m, b, table)
    for name in ("score_spo", "score_neg", "score_neg_blocks"):  # the grouped backward runs
        m.zero_grad(set_to_none=True)
        out = calls(m, b)[name]()
        (out[0] if isinstance(out, tuple) else out).sum().backward()
        assert m._entity_embedder.weight.grad is not None, name


@pytest.mark.gpu
def test_gpu_conve(entered):
    m, b = create("conve", DEV), batch(DEV)
    m.eval()
    with torch.no_grad():
        check(entered, m, b, conve_table())
    kernel = m.routes["kernel"]
    assert kernel > 0 and m.routes["torch"] == 0
    m.train()
    check(entered, m, b, conve_table())
    assert m.routes["kernel"] == kernel and m.routes["torch"] > 0


@pytest.mark.gpu
def test_gpu_bf16_scoring_takes_the_two_sided_loss_nodes(entered):
    """float32 ComplEx scored in bfloat16, d = 128: _ce_tables() holds"""
    torch.manual_seed(0)
    m, b = km.create("complex", E, R, 128, device=DEV, score_dtype=torch.bfloat16), batch(DEV)
    assert m._ce_tables() is not None and m._ce_dist_tables() is None and m._ce_f32_tables() is None
    fused = dict(PLAIN, loss_sp=[], loss_sp_po=[CE2], loss_sp_po_sum=[CE2_SUM], multilabel=[ML2], multilabel_smoothed=[])
    for training in (True, False):
        m.train(training)
        check(entered, m, b, fused)
    with torch.no_grad():
        check(entered, m, b, dict(fused, score_sp_po=[]))
    # entity dropout in training mode: no _ce_tables(), everything composed
    m = km.create("complex", E, R, 128, device=DEV, score_dtype=torch.bfloat16, entity_args={"dropout": 0.2})
    m.train()
    assert m._ce_tables() is None
    check(entered, m, b, {name: [] for name in PLAIN})
