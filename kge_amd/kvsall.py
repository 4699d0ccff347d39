"""KvsAll batches collated on the GPU (kge_kvsall_collate): what TrainingJobKvsAll's collate function does on the host
per batch (kge/job/train_KvsAll.py:118-201, a Python loop over the batch's examples) and the cut of its `label_coords`
into one CSR per query type that the fused KvsAll losses read, padded for the captured step or not -- as two launches
on device-resident state built once:

  * the three arrays of every query type's KvsAllIndex (`_keys` [M, 2], `_values_offset` [M + 1], `_values`), uploaded
    as int64;
  * on the host, numpy copies of the offsets (as per-example label counts) and of `query_last_example`: the sizes a
    caller needs before the launch -- nnz of the batch, rows and labels per type -- are a searchsorted, a gather and
    two bincounts over the batch's example numbers.  Nothing is read back from the device.

Only the example numbers of a batch cross the bus.
"""
import numpy as np
import torch

from . import engine

TARGET_COL = {"sp_": 2, "s_o": 1, "_po": 0}  # (train_KvsAll.py:165-170)


def _arrays(index):
    """(keys, offsets, values) of a KvsAllIndex (kge/indexing.py) or of a triple of arrays, as int64 numpy arrays."""
    if hasattr(index, "_keys"):
        index = (index._keys, index._values_offset, index._values)
    keys, offsets, values = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in index)
    keys = np.ascontiguousarray(keys, dtype=np.int64).reshape(-1, 2)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    values = np.ascontiguousarray(values, dtype=np.int64).reshape(-1)
    if len(offsets) != len(keys) + 1 or (len(offsets) and (offsets[0] != 0 or offsets[-1] != len(values))) \
            or np.any(np.diff(offsets) < 0):
        raise ValueError("kge_amd: DeviceKvsAllCollator: an index is keys [M, 2], offsets [M + 1] ascending from 0 to "
                         "len(values), values")
    return keys, offsets, values


class DeviceKvsAllCollator:
    """batch(examples) -> the collate function's dictionary as device tensors; typed(examples, caps, weight) -> per query
    type (ids, rowptr, col, weight, rows), exact-size or padded to capacities.

    indexes      per query type a KvsAllIndex of the reference or a (keys, offsets, values) triple
    query_types  the job's `query_types`, e.g. ["sp_", "_po"]: the order of the example numbering
    `examples` are the batch's example numbers ON THE HOST (a tensor, an array or a sequence), in the concatenated
    numbering of `query_last_example`; `device_examples` may name a copy that already is on the device."""

    def __init__(self, indexes, query_types, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"kge_amd: DeviceKvsAllCollator collates on a GPU, not on '{self.device}' (no CPU path)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        arrays = self._init_host(indexes, query_types)
        self._types = []
        for (keys, offsets, values), last, qt in zip(arrays, self.query_last_example, self.query_types):
            if len(values) == 0:  # an empty value array still needs an address
                values = np.zeros(1, dtype=np.int64)
            dev = [torch.from_numpy(x).to(self.device) for x in (keys, offsets, values)]
            self._types.append((dev[0], dev[1], dev[2], int(last), TARGET_COL[qt]))

    @classmethod
    def host_only(cls, indexes, query_types):
        """The host half alone (sizes, fit test, repeated labels): no device, batch() / typed() are not available."""
        self = cls.__new__(cls)
        self.device, self._types = None, None
        self._init_host(indexes, query_types)
        return self

    def _init_host(self, indexes, query_types):
        self.query_types = list(query_types)
        if not 1 <= len(self.query_types) <= 3 or len(indexes) != len(self.query_types) \
                or any(qt not in TARGET_COL for qt in self.query_types):
            raise ValueError(f"kge_amd: DeviceKvsAllCollator: query types {self.query_types!r} (1 to 3 of sp_, s_o, _po, "
                             "one index each)")
        arrays = [_arrays(ix) for ix in indexes]
        self.query_last_example = np.cumsum([len(a[0]) for a in arrays]).astype(np.int64)
        self.num_examples = int(self.query_last_example[-1])
        if any(len(a[0]) == 0 for a in arrays):
            raise ValueError("kge_amd: DeviceKvsAllCollator: an index without a key")
        self._degree = np.concatenate([np.diff(a[1]) for a in arrays]).astype(np.int64)  # labels per example number
        # does any key of an index hold the same label twice (a split that repeats a triple)?  A property of the index,
        # decided once; a batch of such an index is treated as one that may repeat a (query, label) pair
        self.repeated_labels = []
        for keys, offsets, values in arrays:
            row = np.repeat(np.arange(len(keys), dtype=np.int64), np.diff(offsets))
            pair = row * (int(values.max()) + 1 if len(values) else 1) + values
            self.repeated_labels.append(bool(len(np.unique(pair)) != len(pair)))
        return arrays

    # ---- host side: sizes of a batch
    def _host_examples(self, examples):
        if torch.is_tensor(examples):
            if examples.is_cuda:
                raise RuntimeError("kge_amd: DeviceKvsAllCollator: the example numbers are given on the host (the batch's "
                                   "sizes are computed there; pass device_examples= for a copy already on the GPU)")
            examples = examples.numpy()
        ex = np.ascontiguousarray(examples, dtype=np.int64).reshape(-1)
        if len(ex) and (ex.min() < 0 or ex.max() >= self.num_examples):
            raise ValueError(f"kge_amd: DeviceKvsAllCollator: example numbers outside [0, {self.num_examples})")
        return ex

    def sizes(self, examples):
        """-> (n_t int64 [T], nnz_t int64 [T]) of a batch of example numbers: rows and labels per query type."""
        ex = self._host_examples(examples)
        T = len(self.query_types)
        t = np.searchsorted(self.query_last_example, ex, side="right")
        deg = self._degree[ex]
        n_t = np.bincount(t, minlength=T).astype(np.int64)
        nnz_t = np.zeros(T, dtype=np.int64)
        np.add.at(nnz_t, t, deg)
        return n_t, nnz_t

    @staticmethod
    def fits(n_t, nnz_t, caps):
        """The fit test of the padded form, per type: n_t <= rows_cap and nnz_t + (rows_cap - n_t) <= lab_cap."""
        return [bool(n <= rc and z + (rc - n) <= lc) for n, z, (rc, lc) in zip(n_t, nnz_t, caps)]

    # ---- device side
    def _upload(self, ex, device_examples):
        if self._types is None:
            raise RuntimeError("kge_amd: DeviceKvsAllCollator.host_only() has no device half (no CPU path)")
        if device_examples is None:
            return torch.from_numpy(ex).to(self.device, non_blocking=True)
        if not (device_examples.is_cuda and device_examples.dtype == torch.int64 and device_examples.numel() == len(ex)):
            raise ValueError("kge_amd: DeviceKvsAllCollator: device_examples is the int64 copy of examples on the GPU")
        return device_examples.contiguous().view(-1)

    def batch(self, examples, device_examples=None):
        """-> {"queries" [n, 2], "query_type_indexes" [n], "label_coords" int32 [nnz, 2], "triples" [nnz, 3]} on the
        device: element for element what the reference's collate function returns for these example numbers."""
        ex = self._host_examples(examples)
        dev_ex = self._upload(ex, device_examples)
        if len(ex) == 0:
            z = lambda *shape, dtype=torch.int64: torch.zeros(*shape, dtype=dtype, device=self.device)
            return {"queries": z(0, 2), "query_type_indexes": z(0), "label_coords": z(0, 2, dtype=torch.int32),
                    "triples": z(0, 3)}
        nnz = int(self._degree[ex].sum())
        res = engine.kvsall_collate(self._types, dev_ex, nnz, batch=True)
        res.pop("counts")
        return res

    def typed(self, examples, caps=None, weight: float = 1.0, device_examples=None):
        """-> per query type (ids [rows, 2], rowptr [rows + 1], col [labels], weight float32 [rows], rows [rows]).
        caps None: exact size (rows = n_t, labels = nnz_t).  caps = (rows_cap, lab_cap) for every type, or one pair per
        type: padded -- padding rows are query (0, 0) with the single label 0, weight 0, rows -1 -- or None for the
        whole call if a type does not fit (decided on the host, nothing is launched)."""
        ex = self._host_examples(examples)
        T = len(self.query_types)
        n_t, nnz_t = self.sizes(ex)
        if caps is None:
            caps = [(int(n), int(z)) for n, z in zip(n_t, nnz_t)]
        else:
            caps = list(caps)
            if len(caps) == 2 and not isinstance(caps[0], (tuple, list)):
                caps = [tuple(caps)] * T
            caps = [(int(rc), int(lc)) for rc, lc in caps]
            if not all(self.fits(n_t, nnz_t, caps)):
                return None
        dev_ex = self._upload(ex, device_examples)
        if len(ex) == 0:  # padding only
            out = []
            for rc, lc in caps:
                z = lambda *shape, dtype=torch.int64: torch.zeros(*shape, dtype=dtype, device=self.device)
                out.append((z(rc, 2), torch.arange(rc + 1, device=self.device), z(lc), z(rc, dtype=torch.float32),
                            torch.full((rc,), -1, dtype=torch.int64, device=self.device)))
            return out
        return engine.kvsall_collate(self._types, dev_ex, int(nnz_t.sum()), batch=False, caps=caps,
                                     weight=float(weight))["typed"]
