"""kge_kvsall_collate on the MI355X against the numpy restatement (tests/_kvsall_collate_ref.py): every output exactly
equal, at the wave / workgroup / chunk edges of the scans, with rows of 0, 1 and 3,000 labels, at the fit boundary of
the padded form -- every output allocated between guard regions of a sentinel that must survive the call."""
import numpy as np
import pytest
import torch

import _kvsall_collate_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = -7777
GUARD = 64
MAX_VALUE = 5000
QT = ["sp_", "s_o", "_po"]
LONG = 3000  # labels of the long row: more than one workgroup's piece of the label copy (1024)


def _types(num_types, seed=0, keys_per_type=120):
    """Indexes with label counts 0..6, and in type 0 a key without labels (0), one with a single label (1) and one with
    3,000 labels (2)."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(num_types):
        deg = rng.integers(0, 7, keys_per_type)
        if t == 0:
            deg[:3] = (0, 1, LONG)
        out.append((ref.random_index(rng, keys_per_type, MAX_VALUE, deg), QT[t] if num_types == 3 else ["sp_", "_po"][t]))
    return out


def _device_types(types, dev):
    last = ref.last_examples(types)
    return [tuple(torch.from_numpy(x).to(dev) for x in ix) + (int(last[t]), ref.TARGET_COL[qt])
            for t, (ix, qt) in enumerate(types)]


def _guarded(shape, dtype, dev):
    numel = int(np.prod(shape))
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + numel].view(*shape)


class _Outputs:
    """Every output of one call between guards; check() compares with the restatement and looks at the guards."""

    def __init__(self, n, nnz_cap, num_types, caps, dev, batch=True, workspace=True):
        self.bufs, self.out = [], {}

        def g(shape, dtype=torch.int64):
            buf, view = _guarded(shape, dtype, dev)
            self.bufs.append((buf, int(np.prod(shape))))
            return view

        if batch:
            self.out.update(queries=g((n, 2)), query_type_indexes=g((n,)), label_coords=g((nnz_cap, 2), torch.int32),
                            triples=g((nnz_cap, 3)))
        if caps is not None:
            self.out["typed"] = [(g((rc, 2)), g((rc + 1,)), g((lc,)), g((rc,), torch.float32), g((rc,))) for rc, lc in caps]
        self.out["counts"] = g((num_types, 3))
        if workspace:
            self.out["workspace"] = g((2 * n + 4,))

    def guards_intact(self):
        for buf, numel in self.bufs:
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + numel:] == SENTINEL).all())


def _run_and_check(types, examples, caps=None, weight=0.25, batch=True, nnz_cap=None, typed=True):
    from kge_amd import engine
    dev = torch.device("cuda")
    dtypes = _device_types(types, dev)
    want_b = ref.batch_form(types, examples)
    nnz = len(want_b["label_coords"])
    nnz_cap = nnz if nnz_cap is None else nnz_cap
    T, n = len(types), len(examples)
    cnt = ref.counts(types, examples, caps)
    use_caps = None if not typed else caps if caps is not None else [(int(a), int(b)) for a, b in cnt[:, :2]]
    o = _Outputs(n, nnz_cap, T, use_caps, dev, batch=batch)
    out = o.out
    res = engine.kvsall_collate(dtypes, torch.from_numpy(examples).to(dev), nnz_cap, batch=batch, caps=use_caps,
                                weight=weight, out=out)
    torch.cuda.synchronize()
    o.guards_intact()
    assert np.array_equal(res["counts"].cpu().numpy(), cnt)
    if batch:
        for k in ("queries", "query_type_indexes"):
            assert np.array_equal(res[k].cpu().numpy(), want_b[k]), k
        m = min(nnz, nnz_cap)
        for k in ("label_coords", "triples"):
            got = res[k].cpu().numpy()
            assert got.dtype == want_b[k].dtype
            assert np.array_equal(got[:m], want_b[k][:m]), k
            assert np.all(got[m:] == SENTINEL), k  # cells the call leaves alone
    want_t = ref.typed_form(types, examples, use_caps, weight=weight) if typed else []
    for t in range(len(want_t)):
        if want_t[t] is None:
            assert cnt[t, 2] == 0
            continue
        for name, a, b in zip(("ids", "rowptr", "col", "weight", "rows"), want_t[t], res["typed"][t]):
            assert a.dtype == b.cpu().numpy().dtype and np.array_equal(a, b.cpu().numpy()), (t, name)
    return res, cnt


def _examples(types, n, seed):
    """n example numbers with repeats; the first and last example of every type lead when they fit."""
    rng = np.random.default_rng(seed)
    last = ref.last_examples(types)
    total = int(last[-1])
    edges = sorted({0, total - 1} | {int(x) for x in last[:-1]} | {int(x) - 1 for x in last[:-1]})
    ex = rng.integers(0, total, n)
    if n >= len(edges) + 4:
        ex[:len(edges)] = edges
        ex[-1] = ex[len(edges)]          # a repeated number
        ex[len(edges) + 1:len(edges) + 4] = (0, 1, 2)  # the rows of 0, 1 and 3,000 labels
    return ex.astype(np.int64)


@pytest.mark.parametrize("num_types", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 1025, 2500])
def test_both_forms_at_the_scan_edges(n, num_types):
    """Wave (64), copy workgroup (256) and scan chunk (1024: one chunk up to 1000, two at 1025, three at 2500) edges;
    both forms from one call, the typed form padded by a few rows and labels."""
    types = _types(num_types, seed=num_types)
    examples = _examples(types, n, seed=n)
    cnt = ref.counts(types, examples)
    caps = [(int(a) + 3, int(b) + 3 + 5) for a, b in cnt[:, :2]]
    _, got = _run_and_check(types, examples, caps)
    assert got[:, 2].all()


@pytest.mark.parametrize("batch", [True, False])
def test_exact_capacities_are_the_unpadded_csr(batch):
    types = _types(2, seed=7)
    examples = _examples(types, 300, seed=11)
    _run_and_check(types, examples, caps=None, batch=batch)


def test_a_batch_of_one_type_pads_the_other():
    types = _types(2, seed=8)
    m0 = len(types[0][0][0])
    examples = np.random.default_rng(5).integers(0, m0, 130).astype(np.int64)
    cnt = ref.counts(types, examples)
    assert cnt[1, 0] == 0
    res, _ = _run_and_check(types, examples, caps=[(int(cnt[0, 0]), int(cnt[0, 1])), (40, 64)])
    ids, rowptr, col, w, rows = res["typed"][1]
    assert torch.equal(rowptr.cpu(), torch.arange(41)) and not ids.any() and not col.any() and not w.any()
    assert bool((rows == -1).all())


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_row_longer_than_a_copy_piece(where):
    types = _types(3, seed=9)
    examples = _examples(types, 65, seed=3)
    examples = examples[examples != 2]
    k = {"first": 0, "middle": len(examples) // 2, "last": len(examples)}[where]
    examples = np.insert(examples, k, 2)
    assert ref.counts(types, examples)[0, 1] >= LONG
    _run_and_check(types, examples)


def test_the_fit_boundary():
    """rows_cap == n_t with lab_cap == nnz_t; lab_cap == nnz_t + pad exactly; one label less; one row less.  The types
    that do not fit report fits == 0, the others are exact, the guards survive in every case."""
    types = _types(2, seed=10)
    examples = _examples(types, 200, seed=13)
    cnt = ref.counts(types, examples)
    (n0, z0), (n1, z1) = (int(a) for a in cnt[0, :2]), (int(a) for a in cnt[1, :2])
    for caps, fits in (([(n0, z0), (n1, z1)], [1, 1]),
                       ([(n0 + 4, z0 + 4), (n1 + 1, z1 + 1)], [1, 1]),
                       ([(n0 + 4, z0 + 3), (n1, z1)], [0, 1]),
                       ([(n0, z0), (n1 - 1, z1 + 100)], [1, 0]),
                       ([(n0 - 1, z0 - 1), (n1 + 2, z1 + 1)], [0, 0]),
                       ([(0, 0), (n1, z1)], [0, 1])):
        _, got = _run_and_check(types, examples, caps)
        assert list(got[:, 2]) == fits, caps
    # a batch form that is too short for the batch: the head is right, nothing beyond it is touched
    _run_and_check(types, examples, nnz_cap=int(cnt[:, 1].sum()) - 9, typed=False)
    _run_and_check(types, examples, nnz_cap=int(cnt[:, 1].sum()) + 9)


def test_side_stream_and_graph_replay():
    """Twice on a non-default stream, then captured once and replayed on other example numbers of the same n: the
    outputs follow the new content (capacities and nnz_cap cover both batches)."""
    from kge_amd import engine
    dev = torch.device("cuda")
    types = _types(2, seed=12)
    dtypes = _device_types(types, dev)
    n = 257
    ex_a, ex_b = _examples(types, n, seed=21), _examples(types, n, seed=22)[::-1].copy()
    assert not np.array_equal(ex_a, ex_b)
    ca, cb = ref.counts(types, ex_a), ref.counts(types, ex_b)
    nnz_cap = int(max(ca[:, 1].sum(), cb[:, 1].sum())) + 5
    caps = [(int(max(ca[t, 0], cb[t, 0])) + 2, int(max(ca[t, 1], cb[t, 1])) + int(max(ca[t, 0], cb[t, 0])) + 2)
            for t in range(2)]
    o = _Outputs(n, nnz_cap, 2, caps, dev)
    static_ex = torch.from_numpy(ex_a).to(dev)

    def check(examples):
        torch.cuda.synchronize()
        o.guards_intact()
        want_b, want_t = ref.batch_form(types, examples), ref.typed_form(types, examples, caps, weight=0.5)
        nnz = len(want_b["label_coords"])
        assert np.array_equal(o.out["counts"].cpu().numpy(), ref.counts(types, examples, caps))
        assert np.array_equal(o.out["queries"].cpu().numpy(), want_b["queries"])
        assert np.array_equal(o.out["query_type_indexes"].cpu().numpy(), want_b["query_type_indexes"])
        assert np.array_equal(o.out["label_coords"].cpu().numpy()[:nnz], want_b["label_coords"])
        assert np.array_equal(o.out["triples"].cpu().numpy()[:nnz], want_b["triples"])
        for t in range(2):
            for a, b in zip(want_t[t], o.out["typed"][t]):
                assert np.array_equal(a, b.cpu().numpy())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            engine.kvsall_collate(dtypes, static_ex, nnz_cap, caps=caps, weight=0.5, out=o.out)
    check(ex_a)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        engine.kvsall_collate(dtypes, static_ex, nnz_cap, caps=caps, weight=0.5, out=o.out)
    static_ex.copy_(torch.from_numpy(ex_b))
    graph.replay()
    check(ex_b)
    static_ex.copy_(torch.from_numpy(ex_a))
    graph.replay()
    torch.cuda.synchronize()
    o.guards_intact()
    assert np.array_equal(o.out["queries"].cpu().numpy(), ref.batch_form(types, ex_a)["queries"])


@pytest.mark.parametrize("num_types", [1, 3])
def test_collator_class_and_the_extension_binding(num_types):
    """kge_amd.DeviceKvsAllCollator (outputs allocated by the torch extension): batch() is the dictionary in exact shape,
    typed() exact or padded, None when a type does not fit -- decided on the host."""
    from kge_amd import DeviceKvsAllCollator
    types = _types(num_types, seed=14)
    col = DeviceKvsAllCollator([ix for ix, _ in types], [qt for _, qt in types], "cuda")
    examples = _examples(types, 333, seed=15)
    got = col.batch(torch.from_numpy(examples))
    want = ref.batch_form(types, examples)
    assert set(got) == set(want)
    for k in want:
        assert got[k].is_cuda and tuple(got[k].shape) == want[k].shape and np.array_equal(got[k].cpu().numpy(), want[k]), k
    cnt = ref.counts(types, examples)
    for caps in (None, [(int(a) + 7, int(b) + 40) for a, b in cnt[:, :2]]):
        typed = col.typed(examples, caps=caps, weight=1.0 / 333, device_examples=torch.from_numpy(examples).cuda())
        want_t = ref.typed_form(types, examples, caps, weight=1.0 / 333)
        for t in range(num_types):
            for a, b in zip(want_t[t], typed[t]):
                assert a.dtype == b.cpu().numpy().dtype and np.array_equal(a, b.cpu().numpy())
    assert col.typed(examples, caps=(int(cnt[:, 0].max()) - 1, 1 << 20)) is None
    assert col.typed(examples, caps=(int(cnt[:, 0].max()), int(cnt[:, 1].max()) - 1)) is None
    with pytest.raises(RuntimeError, match="on the host"):
        col.batch(torch.from_numpy(examples).cuda())
