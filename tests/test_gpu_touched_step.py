"""kge_touched_mark and kge_adagrad_step_touched (kge_amd/csrc/touched.hip) on the MI355X, through kge_amd.engine.

Mark: the bitmap must equal the numpy restatement's (tests/_touched_ref.py) for int32 / int64 ids, a stride-3 vector and
an [n, k] block inside a wider matrix, duplicates, ids outside the table, and the edge sets (none, all, row 0, row E - 1,
bits 0 and 31 of one word); the words behind ceil(E / 32) and the guards around the allocation keep their sentinel.

Step: parameter, accumulator and bf16 copy must carry the BITS kge_adagrad_step_multi leaves on clones of the same
arrays with the same dense gradient (random on the marked rows, zero elsewhere) -- every row, the untouched ones
included: with weight_decay == 0 the dense step leaves a row whose gradient is zero bit for bit as it was (DESIGN.md
section 25).  Afterwards the gradient is all zero bytes, the bitmap all zero, and pitch padding and guard rows are
byte-equal to before.  Table sizes sit on both sides of a bitmap word (32 rows) and of the 256- and 2048-row chunk
boundaries; the row widths take every launch shape: four floats per lane with 16, 32 and 64 lanes per row (dim 4 / 20 /
64, 128, 260 contiguous), one float per lane (dim 1, 5, 130, and every width on the pitch dim + 3), rows longer than
one trip of their lanes (130, 260)."""
import numpy as np
import pytest
import torch

import _touched_ref as tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ES = [1, 31, 32, 33, 2047, 2048, 2049, 4100]
DIMS = [1, 4, 5, 20, 64, 128, 130, 260]
GUARD = 8                       # words in front of and behind the bitmap (32 bytes: the bitmap stays 16-byte aligned)
SENT_WORD = np.uint32(0xDEADBEEF)
SENT_F32 = float(np.array([0xDEADBEEF], dtype=np.uint32).view(np.float32)[0])
SENT_I16 = int(np.array([0xBEEF], dtype=np.uint16).view(np.int16)[0])


def _guarded_bitmap(E):
    """(whole allocation, the bitmap slice handed to the library, the number of words that may ever change)"""
    words = tr.bitmap_bytes(E) // 4
    whole = torch.from_numpy(np.full(words + 2 * GUARD, SENT_WORD, dtype=np.uint32).view(np.int32).copy()).to(DEV)
    live = (E + 31) // 32
    whole[GUARD:GUARD + live] = 0
    return whole, whole[GUARD:GUARD + words], live


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _id_sets(E, rng):
    w = (E - 1) // 32
    sets = {"none": np.zeros(0, np.int64), "all": np.arange(E), "row0": np.array([0]), "last": np.array([E - 1]),
            "bits_0_31": np.array([x for x in (32 * w, 32 * w + 31, 0, 31) if x < E]),
            "duplicates": rng.integers(0, E, 3 * min(E, 700) + 7),
            "outside": np.array([-1, E, E + 31, E // 2, -E - 1, 2 ** 31 - 1, -2 ** 31])}
    return sets


@pytest.mark.parametrize("itype", [torch.int32, torch.int64])
@pytest.mark.parametrize("E", ES)
def test_mark_sets_the_restatements_bits_and_nothing_else(E, itype):
    from kge_amd import engine
    rng = np.random.default_rng(E)
    for name, ids in _id_sets(E, rng).items():
        whole, bitmap, live = _guarded_bitmap(E)
        before = _words(whole).copy()
        want = tr.mark(ids, E)
        n = ids.size
        # (a) a stride-3 vector: column 1 of an [n, 3] matrix;  (b) the same ids as an [n2, k] block with ld > k
        tri = torch.full((max(n, 1), 3), E + 5, dtype=itype, device=DEV)   # (the other columns: ids outside the table)
        tri[:n, 1] = torch.from_numpy(ids).to(DEV).to(itype)
        engine.touched_mark(tri[:n, 1], bitmap, E)
        got = _words(whole)
        assert np.array_equal(got[GUARD:GUARD + want.size][:live], want[:live]), (name, "vector")
        assert np.array_equal(got[:GUARD], before[:GUARD]) and np.array_equal(got[GUARD + live:], before[GUARD + live:]), name
        whole2, bitmap2, _ = _guarded_bitmap(E)
        k = 5
        n2 = (n + k - 1) // k
        wide = torch.full((max(n2, 1), k + 3), -7, dtype=itype, device=DEV)
        flat = np.concatenate([ids, np.full(n2 * k - n, ids[0] if n else 0)])  # (padding: a duplicate)
        wide[:n2, 1:1 + k] = torch.from_numpy(flat.reshape(n2, k)).to(DEV).to(itype)
        if n2:
            engine.touched_mark(wide[:n2, 1:1 + k], bitmap2, E)
        got2 = _words(whole2)
        assert np.array_equal(got2[GUARD:GUARD + live], want[:live]), (name, "block")
        assert np.array_equal(got2[:GUARD], before[:GUARD]) and np.array_equal(got2[GUARD + live:], before[GUARD + live:]), name
    # marks accumulate over calls (what the backward nodes do: s, o, then the blocks)
    whole, bitmap, live = _guarded_bitmap(E)
    engine.touched_mark(torch.tensor([0], dtype=itype, device=DEV), bitmap, E)
    engine.touched_mark(torch.tensor([E - 1, E // 2], dtype=itype, device=DEV), bitmap, E)
    assert np.array_equal(_words(whole)[GUARD:GUARD + live], tr.mark([0, E - 1, E // 2], E)[:live])


def _dense_multi(P, G, S, with_copy, minus_clr, eps):
    """kge_adagrad_step_multi on contiguous clones -> (param, sum, copy or None)"""
    from kge_amd import _lib, engine
    P, G, S = P.clone().contiguous(), G.clone().contiguous(), S.clone().contiguous()
    C = torch.full(P.shape, SENT_I16, dtype=torch.int16, device=DEV) if with_copy else None
    seg = _lib.KgeAdagradSeg(P.data_ptr(), G.data_ptr(), S.data_ptr(), None if C is None else C.data_ptr(), P.numel(),
                             minus_clr, 0.0, eps)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().kge_adagrad_step_multi((_lib.KgeAdagradSeg * 1)(seg), 1, engine._stream(DEV)),
                   "kge_adagrad_step_multi")
    return P, S, C


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a.contiguous(),
                       b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b.contiguous())


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("E", ES)
def test_step_over_the_marked_rows_carries_the_dense_kernels_bits(E, dim):
    from kge_amd import engine
    rng = np.random.default_rng(1000 * E + dim)
    rows = np.unique(np.concatenate([rng.integers(0, E, max(1, E // 3)), [0, E - 1]]))
    zero_row = int(rows[rng.integers(0, rows.size)])          # a marked row whose gradient is all zero
    p0 = rng.standard_normal((E, dim)).astype(np.float32)
    p0[rng.random((E, dim)) < 0.03] = -0.0
    s0 = (rng.random((E, dim)) * 2).astype(np.float32)
    s0[rng.random((E, dim)) < 0.1] = 0.0
    g0 = np.zeros((E, dim), dtype=np.float32)
    g0[rows] = rng.standard_normal((rows.size, dim)).astype(np.float32)
    g0[zero_row] = 0.0
    minus_clr, eps = -0.05, 1e-10
    rp, _, rs, _, _ = tr.step_touched(p0, g0, s0, tr.mark(rows, E), minus_clr, eps)
    for ld in (dim, dim + 3):
        for with_copy in (True, False):
            def table(src, dtype=torch.float32, sent=SENT_F32):
                buf = torch.full((E + 2, ld), sent, dtype=dtype, device=DEV)   # guard rows around, pitch padding inside
                buf[1:E + 1, :dim] = src
                return buf, buf[1:E + 1, :dim]
            Pb, P = table(torch.from_numpy(p0).to(DEV))
            Sb, S = table(torch.from_numpy(s0).to(DEV))
            Gb, G = table(torch.from_numpy(g0).to(DEV))
            # the copy must be FRESH before a partial rewrite (Adagrad._step_touched sees to it): bf16(param) everywhere
            Cb, C = table(P.to(torch.bfloat16).view(torch.int16), torch.int16, SENT_I16) if with_copy else (None, None)
            wantP, wantS, wantC = _dense_multi(P, G, S, with_copy, minus_clr, eps)
            whole, bitmap, live = _guarded_bitmap(E)
            engine.touched_mark(torch.from_numpy(rows).to(DEV), bitmap, E)
            assert np.array_equal(_words(whole)[GUARD:GUARD + live], tr.mark(rows, E)[:live])
            before = [b.clone() if b is not None else None for b in (Pb, Sb, Gb, Cb)]
            engine.adagrad_step_touched(P, G, S, bitmap, minus_clr, eps, C)
            torch.cuda.synchronize()
            what = f"E={E} dim={dim} ld={ld} copy={with_copy}"
            # every row: the dense kernel's bits (its result on an untouched row IS the row as it was)
            assert _same_bits(P, wantP), what + ": param"
            assert _same_bits(S, wantS), what + ": sum"
            if with_copy:
                assert torch.equal(C, wantC), what + ": bf16 copy"
            # the numpy restatement agrees on the marked rows (and on which rows moved)
            assert np.array_equal(P.cpu().numpy().view(np.uint32), rp.view(np.uint32)), what + ": restatement"
            assert np.array_equal(S.cpu().numpy().view(np.uint32), rs.view(np.uint32)), what + ": restatement (sum)"
            # post-conditions: gradient all zero bytes, bitmap all zero, padding and guards as before
            assert not G.contiguous().view(torch.int32).any(), what + ": gradient not zero"
            got = _words(whole)
            assert not got[GUARD:GUARD + live].any(), what + ": bitmap not zero"
            assert (got[:GUARD] == SENT_WORD).all() and (got[GUARD + live:] == SENT_WORD).all(), what + ": bitmap guards"
            for buf, was in zip((Pb, Sb, Gb, Cb), before):
                if buf is None:
                    continue
                assert torch.equal(buf[0], was[0]) and torch.equal(buf[E + 1], was[E + 1]), what + ": guard rows"
                assert torch.equal(buf[1:E + 1, dim:], was[1:E + 1, dim:]), what + ": pitch padding"


def test_unmarked_rows_are_neither_read_nor_written():
    """NaN-poisoned rows without a bit stay as they are in all four arrays; a second call on the cleared bitmap moves
    nothing; bits behind the table's last row are ignored but cleared."""
    from kge_amd import engine
    E, dim = 300, 64
    rng = np.random.default_rng(5)
    rows = np.unique(rng.integers(0, E, 40))
    off = np.setdiff1d(np.arange(E), rows)
    mk = lambda: torch.from_numpy(rng.standard_normal((E, dim)).astype(np.float32)).to(DEV)
    P, G, S = mk(), mk(), mk().abs()
    C = P.to(torch.bfloat16)
    for t in (P, G, S, C):
        t[torch.from_numpy(off).to(DEV)] = float("nan")
    bitmap = engine.touched_bitmap(E, DEV)
    assert bitmap.numel() * 4 == tr.bitmap_bytes(E) and not bitmap.any()
    engine.touched_mark(torch.from_numpy(rows).to(DEV), bitmap, E)
    bitmap[(E - 1) // 32] |= 1 << 20                         # row 308 of a 300-row table: no such row
    before = [t.clone() for t in (P, G, S, C)]
    engine.adagrad_step_touched(P, G, S, bitmap, -0.1, 1e-10, C)
    o = torch.from_numpy(off).to(DEV)
    for t, was in zip((P, G, S, C), before):
        assert torch.equal(t[o].view(torch.int32 if t.dtype == torch.float32 else torch.int16),
                           was[o].view(torch.int32 if t.dtype == torch.float32 else torch.int16))
    r = torch.from_numpy(rows).to(DEV)
    assert not G[r].any() and not torch.isnan(P[r]).any() and not bitmap.any()
    after = [t.clone() for t in (P, S, C)]
    engine.adagrad_step_touched(P, G, S, bitmap, -0.1, 1e-10, C)    # nothing marked: nothing moves
    for t, was in zip((P, S, C), after):
        assert torch.equal(t[r], was[r])
