"""kge_kvsall_collate without a GPU: the numpy restatement (tests/_kvsall_collate_ref.py) against the reference's own
collate closure (kge/job/train_KvsAll.py:118-201) and against the plugin's per-type cut and padding helpers on CPU
tensors; the host half of kge_amd.DeviceKvsAllCollator (sizes, fit test, repeated labels); the C entry's argument
checks; hip_KvsAll.device_collate on a CPU job."""
import ctypes
import os
import shutil
import types

import numpy as np
import pytest
import torch

import _kvsall_collate_ref as ref
import ref_harness as rh

needs_reference = pytest.mark.skipif(not rh.available(), reason="reference tree not present")

E, R, N_TRIPLES = 40, 5, 300
KEY_COLS = {"sp_": ([0, 1], 2), "s_o": ([0, 2], 1), "_po": ([1, 2], 0)}
QUERY_TYPES = [["sp_"], ["sp_", "_po"], ["sp_", "s_o", "_po"]]


def _triples():
    """~300 distinct triples over 40 entities and 5 relations with a few high-degree keys."""
    rng = np.random.default_rng(5)
    tri = np.stack([rng.integers(0, E, N_TRIPLES), rng.integers(0, R, N_TRIPLES), rng.integers(0, E, N_TRIPLES)], axis=1)
    hub = np.stack([np.full(30, 3), np.full(30, 1), rng.choice(E, 30, replace=False)], axis=1)      # (3, 1, ?): 30 objects
    hub2 = np.stack([rng.choice(E, 25, replace=False), np.full(25, 2), np.full(25, 7)], axis=1)     # (?, 2, 7): 25 subjects
    return np.unique(np.concatenate([tri, hub, hub2]), axis=0).astype(np.int64)


def _numpy_types(query_types):
    """The restatement's indexes, built without the reference: keys sorted, labels sorted per key."""
    tri, out = _triples(), []
    for qt in query_types:
        kc, vc = KEY_COLS[qt]
        order = np.lexsort((tri[:, vc], tri[:, kc[1]], tri[:, kc[0]]))
        t = tri[order]
        keys, first = np.unique(t[:, kc], axis=0, return_index=True)
        out.append(((keys, np.append(first, len(t)).astype(np.int64), t[:, vc].copy()), qt))
    return out


def _boundary_batches(types, rng):
    """Batches that hold the first and the last example of every type, repeated numbers, and a single example."""
    last = ref.last_examples(types)
    edges = sorted({0, int(last[-1]) - 1} | {int(x) for x in last[:-1]} | {int(x) - 1 for x in last[:-1]})
    total = int(last[-1])
    yield np.asarray(edges, dtype=np.int64)
    yield np.concatenate([rng.integers(0, total, 29), edges, rng.integers(0, total, 7), edges[:2]]).astype(np.int64)
    yield np.asarray([edges[-1]], dtype=np.int64)
    yield rng.permutation(total)[:50].astype(np.int64)


@needs_reference
@pytest.mark.parametrize("query_types", QUERY_TYPES, ids=["sp", "sp_po", "sp_so_po"])
def test_batch_form_equals_the_reference_collate(query_types):
    rh.import_reference()
    from kge.indexing import KvsAllIndex
    from kge.job.train_KvsAll import TrainingJobKvsAll
    tri = torch.from_numpy(_triples()).int()
    indexes = [KvsAllIndex(tri, *KEY_COLS[qt], list) for qt in query_types]
    types_np = _numpy_types(query_types)
    for (ix_np, _), ix in zip(types_np, indexes):  # the restatement's indexes are the reference's
        assert np.array_equal(ix_np[0], ix._keys.numpy()) and np.array_equal(ix_np[1], ix._values_offset.numpy())
        assert np.array_equal(ix_np[2], ix._values.numpy())
    job = types.SimpleNamespace(query_types=query_types, query_indexes=indexes,
                                query_last_example=list(np.cumsum([len(ix) for ix in indexes])))
    collate = TrainingJobKvsAll._get_collate_fun(job)
    rng = np.random.default_rng(1)
    for examples in _boundary_batches(types_np, rng):
        want = collate([int(x) for x in examples])
        got = ref.batch_form(types_np, examples)
        assert set(got) == set(want)
        for k in want:
            assert got[k].dtype == want[k].numpy().dtype and got[k].shape == tuple(want[k].shape), k
            assert np.array_equal(got[k], want[k].numpy()), k


@pytest.mark.parametrize("query_types", QUERY_TYPES, ids=["sp", "sp_po", "sp_so_po"])
def test_typed_form_equals_the_plugin_helpers(query_types):
    """The per-type cut (`_kvsall_per_type_cut`) of the batch form and its padding (`_kvsall_pad_inputs`), on CPU
    tensors: exact size, padded, and the fit boundary in rows and in labels."""
    rh.available() and rh.import_reference()
    tj = pytest.importorskip("kge_amd.libkge_plugin.train_job")
    types_np = _numpy_types(query_types)
    rng = np.random.default_rng(2)
    for examples in _boundary_batches(types_np, rng):
        n = len(examples)
        b = {k: torch.from_numpy(v) for k, v in ref.batch_form(types_np, examples).items()}
        per_type, totals = tj._kvsall_per_type_cut(b["queries"], b["label_coords"], b["query_type_indexes"], query_types, n)
        cnt = ref.counts(types_np, examples)
        exact = ref.typed_form(types_np, examples, weight=1.0 / n)
        for t, qt in enumerate(query_types):
            if cnt[t, 0] == 0:
                assert qt not in per_type
                continue
            ids, rowptr, col, w, rows = exact[t]
            q0, q1, rp, cl = per_type[qt]
            assert totals[qt] == cnt[t, 1]
            assert np.array_equal(ids[:, 0], q0.numpy()) and np.array_equal(ids[:, 1], q1.numpy())
            assert np.array_equal(rowptr, rp.numpy()) and np.array_equal(col, cl.numpy())
            assert np.array_equal(rows, np.flatnonzero(b["query_type_indexes"].numpy() == t))
            assert np.all(w == np.float32(1.0 / n))
        # padded: every type to the same capacities, as the captured step holds them
        pads = [qt for qt in query_types if qt in ("sp_", "_po")]
        sel = [query_types.index(qt) for qt in pads]
        need_rows, need_lab = int(cnt[sel, 0].max()), int((cnt[sel, 1] + (cnt[sel, 0].max() - cnt[sel, 0])).max())
        for rows_cap, lab_cap, fit in ((need_rows, need_lab, True), (need_rows + 5, need_lab + 9, True),
                                       (need_rows, need_lab - 1, False), (need_rows - 1, need_lab + 50, False)):
            only = {qt: per_type[qt] for qt in pads if qt in per_type}
            got = tj._kvsall_pad_inputs(only, n, torch.device("cpu"), (rows_cap, lab_cap), query_types=pads)
            caps = [(rows_cap, lab_cap)] * len(query_types)
            c = ref.counts(types_np, examples, caps)
            assert (got is not None) == bool(c[sel, 2].all()) == fit
            if got is None:
                continue
            want = ref.typed_form(types_np, examples, caps, weight=1.0 / n)
            for k, t in enumerate(sel):
                for a, bb in zip(want[t][:4], got[4 * k:4 * k + 4]):
                    assert a.dtype == bb.numpy().dtype and np.array_equal(a, bb.numpy())
                assert np.all(want[t][4][int(c[t, 0]):] == -1)


@pytest.mark.parametrize("query_types", QUERY_TYPES, ids=["sp", "sp_po", "sp_so_po"])
def test_host_side_sizes_equal_the_restatement(query_types):
    from kge_amd import DeviceKvsAllCollator
    types_np = _numpy_types(query_types)
    host = DeviceKvsAllCollator.host_only([ix for ix, _ in types_np], query_types)
    assert np.array_equal(host.query_last_example, ref.last_examples(types_np))
    assert host.repeated_labels == [False] * len(query_types)
    rng = np.random.default_rng(3)
    for examples in _boundary_batches(types_np, rng):
        n_t, nnz_t = host.sizes(torch.from_numpy(examples))
        cnt = ref.counts(types_np, examples)
        assert np.array_equal(n_t, cnt[:, 0]) and np.array_equal(nnz_t, cnt[:, 1])
        caps = [(int(n) + 1, int(z) + 1) for n, z in zip(n_t, nnz_t)]
        for tweak in (0, -1):
            c = [(rc, lc + tweak) for rc, lc in caps]
            assert host.fits(n_t, nnz_t, c) == [bool(x) for x in ref.counts(types_np, examples, c)[:, 2]]
    with pytest.raises(ValueError, match="outside"):
        host.sizes([host.num_examples])
    with pytest.raises(RuntimeError, match="no CPU path"):
        host.batch([0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        DeviceKvsAllCollator([ix for ix, _ in types_np], query_types, device="cpu")
    # an index that holds a label twice under one key says so, once, at set-up
    keys, offsets, values = (x.copy() for x in types_np[0][0])
    k = int(np.argmax(np.diff(offsets) >= 2))
    values[offsets[k] + 1] = values[offsets[k]]
    twice = DeviceKvsAllCollator.host_only([(keys, offsets, values)] + [ix for ix, _ in types_np[1:]], query_types)
    assert twice.repeated_labels == [True] + [False] * (len(query_types) - 1)


def test_entry_is_declared_bound_and_validates_arguments_without_a_device():
    from kge_amd import _lib, engine
    from kge_amd._lib import KgeKvsallIndex, KgeKvsallTyped
    _lib.build()
    lib = _lib.lib()
    assert ctypes.sizeof(KgeKvsallIndex) == 40 and ctypes.sizeof(KgeKvsallTyped) == 56
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "kge_amd.h")).read()
    assert "train_KvsAll.py:118-201" in header[header.index("A KvsAll batch built ON THE DEVICE"):
                                                header.index("int kge_kvsall_collate(")]
    assert hasattr(_lib.ext(), "kvsall_collate")
    P = ctypes.c_void_p(256)  # never dereferenced on these paths
    ix = lambda last=10, col=2, keys=P: KgeKvsallIndex(keys, P, P, last, col, 0)
    one = (KgeKvsallIndex * 1)(ix())
    call = lambda types, T, n, nnz=4, batch=(P, P, P, P), typed=None, ws=P, ws_bytes=1 << 20, ex=P: \
        lib.kge_kvsall_collate(types, T, ex, n, nnz, *batch, typed, 1.0, None, ws, ws_bytes, None)
    assert lib.kge_kvsall_collate_workspace_bytes(512) == 8 * (2 * 512 + 4)
    assert call(one, 1, 0) == 0 and call(one, 1, 0, ex=None, ws=None) == 0        # an empty batch
    assert call(None, 1, 4) == -1 and call(one, 0, 4) == -1 and call(one, 4, 4) == -1
    assert call(one, 1, -1) == -1 and call(one, 1, 4, nnz=-1) == -1
    assert call((KgeKvsallIndex * 1)(ix(keys=None)), 1, 4) == -1
    assert call((KgeKvsallIndex * 1)(ix(col=3)), 1, 4) == -1
    assert call((KgeKvsallIndex * 2)(ix(10), ix(9)), 2, 4) == -1                     # last decreases
    assert call((KgeKvsallIndex * 1)(ix(0)), 1, 4) == -1                             # no example at all
    assert call(one, 1, 4, batch=(P, P, None, P)) == -1                              # the batch form in part
    assert call(one, 1, 4, ex=None) == -1 and call(one, 1, 4, ws=None) == -1
    assert call(one, 1, 4, typed=(KgeKvsallTyped * 1)(KgeKvsallTyped(P, None, P, None, None, 4, 4))) == -1
    assert call(one, 1, 4, typed=(KgeKvsallTyped * 1)(KgeKvsallTyped(P, P, P, None, None, -1, 4))) == -1
    assert call(one, 1, 4, ws_bytes=8 * (2 * 4 + 4) - 1) == -5
    assert call(one, 1, engine.KVSALL_COLLATE_MAX_N + 1, ws_bytes=1 << 40) == -2     # above the scan's ceiling
    assert call(one, 1, 4, nnz=1 << 31) == -2
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.kvsall_collate([], torch.zeros(4, dtype=torch.int64), 0)


@needs_reference
def test_device_collate_is_ignored_on_a_cpu_job(tmp_path):
    """hip_KvsAll.device_collate: true with job.device cpu -- the job is today's: the reference's collate function, no
    collator, the same loss and parameters as with the option off."""
    from kge_amd.synthetic import make_splits, write_libkge_dataset
    rh.import_reference()
    from kge import Config, Dataset
    from kge.job import TrainingJob
    folder = write_libkge_dataset(str(tmp_path / "toy"), "toy", 60, 4, make_splits(60, 4, 400, 20, 20, seed=3))
    out = []
    for option in (True, False):
        config = Config()
        config.folder = str(tmp_path / f"run_{option}")
        shutil.rmtree(config.folder, ignore_errors=True)
        os.makedirs(config.folder)
        config.set("console.quiet", True)
        config.set("modules", ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"])
        config.set("model", "hip_complex")
        config._import("hip_complex")
        config.set("dataset.name", "toy")
        config.set("job.device", "cpu")
        config.set("train.max_epochs", 1)
        config.set("train.batch_size", 64)
        config.set("train.num_workers", 0)
        config.set("lookup_embedder.dim", 16)
        for key in ("default", "torch", "numpy", "python"):
            config.set("random_seed." + key, 11)
        config._import("hip_KvsAll")
        config.set("train.type", "hip_KvsAll")
        config.set("hip_KvsAll.device_collate", option)
        torch.manual_seed(11)
        job = TrainingJob.create(config, Dataset.create(config, folder=folder))
        assert type(job).__name__ == "HipTrainingJobKvsAll" and job._device_collate is option
        torch.manual_seed(12)
        job._prepare()
        assert job._collator is None
        batch = next(iter(job.loader))
        assert set(batch) == {"queries", "label_coords", "query_type_indexes", "triples"}
        torch.manual_seed(12)
        loss = job.run_epoch()["avg_loss"]
        out.append((loss, {k: v.detach().clone() for k, v in job.model.state_dict().items()}))
    (l_on, st_on), (l_off, st_off) = out
    assert l_on == l_off
    for k in st_off:
        assert torch.equal(st_on[k], st_off[k]), k
