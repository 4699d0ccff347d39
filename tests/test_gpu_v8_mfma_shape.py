"""The split-query store chains of pairs_bf16_v8_kernel (d = 512) on v_mfma_f32_16x16x32_bf16.

The shape of the matrix instruction changes how a unit's 32 operand rows x 32 targets are cut into tiles, which lane
holds which score and how a unit is stored (four buffer_store_dwordx2 per wave instead of eight dword stores) -- not a
single bit of a score.  Bars:
  * BIT FOR BIT the 32x32x16 instantiation (switch V8_MFMA32 = 1) and one launch per batch on the staged split kernel
    (engine.score_queries with FLAG_SPLIT_QUERY, V8 = 0), at every edge of the tiling: fewer targets than a unit, exactly
    one, a ragged and an odd last unit, several units per XCD slice; rows >= n inside a wave, waves without rows, chunks
    with an odd number of fragment groups; a work list that crosses pair boundaries;
  * nothing written outside the score blocks (pad columns of the 256-byte pitch, rows >= n, behind the last batch);
  * the MFMA bar of DESIGN section 4 against float32 arithmetic on the bf16 table values;
  * the next group's fragments built inside the launch = build_queries_group's, bit for bit.
"""
import numpy as np
import pytest
import torch

import oracle as ko

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, R = 512, 7


@pytest.fixture(scope="module")
def eng():
    from kge_amd import engine
    return engine


_TABLES = {}


def _tables(eng, scorer, E):
    """One pair of tables per (scorer, E), shared by every test that needs it and never written."""
    key = (scorer, E)
    if key not in _TABLES:
        g = torch.Generator().manual_seed(1000 + E + (7 if scorer == "distmult" else 0))
        ent = (torch.randn(E, D, generator=g) * 0.3).bfloat16()
        rel = (torch.randn(R, D, generator=g) * 0.3).bfloat16()
        _TABLES[key] = (eng.Tables(scorer, ent.to(DEV), rel.to(DEV), flags=eng.FLAG_SPLIT_QUERY), ent, rel)
    return _TABLES[key]


def _triples(E, rows, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(hi, (rows,), generator=g) for hi in (E, R, E)], dim=1).to(DEV).contiguous()


def _same(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), f"{what}: {int(bad.sum())}/{a.size} differ, first at {np.argwhere(bad)[:3].tolist()}"


def _one_by_one(eng, T, combine, trip, n, L):
    """One launch per batch on the staged split kernel (the caller has V8 = 0 set)."""
    fl = eng.FLAG_SPLIT_QUERY
    want = []
    for l in range(L):
        t = trip[l * n:(l + 1) * n]
        q = eng.build_queries(T, combine, t[:, 0] if combine != "_po" else None, t[:, 1],
                              t[:, 2] if combine != "sp_" else None, flags=fl)
        want.append(eng.score_queries(T, q))
    return want


def _group_into_canaries(eng, T, combine, trip, n, L, E):
    """The group launch into a buffer on the 256-byte pitch with NaN canaries in the pad columns, in `guard` rows behind
    every batch and in a whole block behind the last batch -> (scores [L, n, sides * E], the whole buffer)."""
    sides = 2 if combine == "sp_po" else 1
    P = eng.score_pitch(E)
    guard = 2
    big = torch.full((L + 1, n + guard, sides * P), float("nan"), device=DEV)
    out = big[:L, :n].view(L, n, sides, P)[:, :, :, :E] if sides == 2 else big[:L, :n, :E]
    q = eng.build_queries_group(T, combine, trip, n, L, flags=eng.FLAG_SPLIT_QUERY)
    eng.score_queries_group(T, q, out)
    torch.cuda.synchronize()
    return out.reshape(L, n, sides * E).clone(), big


def _check_shapes(eng, kge_switch, scorer, combine, E, shapes, seed):
    T, _, _ = _tables(eng, scorer, E)
    sides = 2 if combine == "sp_po" else 1
    for n, L in shapes:
        trip = _triples(E, n * L, seed + 13 * n + L)
        kge_switch.set("V8", 0)
        want = _one_by_one(eng, T, combine, trip, n, L)
        kge_switch.set("V8", 1)            # (a group of one takes the persistent kernel too)
        kge_switch.set("V8_MFMA32", 1)
        old, big_old = _group_into_canaries(eng, T, combine, trip, n, L, E)
        kge_switch.unset("V8_MFMA32")
        new, big_new = _group_into_canaries(eng, T, combine, trip, n, L, E)
        what = f"{scorer} {combine} E={E} n={n} L={L}"
        for l in range(L):
            _same(new[l], old[l], f"{what} batch {l}: 16x16x32 against 32x32x16")
            _same(new[l], want[l], f"{what} batch {l}: 16x16x32 against one launch per batch")
        for big, tag in ((big_new, "16x16x32"), (big_old, "32x32x16")):
            assert int((~torch.isnan(big)).sum()) == L * n * sides * E, f"{what}: {tag} wrote outside the score blocks"
        # contiguous rows (4-byte alignment only: an 8-byte store may start on any dword)
        flat = torch.full((L, n + 1, sides * E), float("nan"), device=DEV)
        q = eng.build_queries_group(T, combine, trip, n, L, flags=eng.FLAG_SPLIT_QUERY)
        eng.score_queries_group(T, q, flat[:, :n])
        torch.cuda.synchronize()
        for l in range(L):
            _same(flat[l, :n], want[l], f"{what} batch {l}: contiguous rows")
        assert int((~torch.isnan(flat)).sum()) == L * n * sides * E, f"{what}: contiguous rows, stray writes"


# E: fewer targets than a unit / exactly one / a ragged last unit of one column / odd m / several units per XCD slice
# n: a single row / rows >= n inside a wave / a whole wave / one row of the next / a chunk / an odd number of groups
@pytest.mark.parametrize("E", [31, 32, 33, 97, 300])
@pytest.mark.parametrize("combine", ["sp_po", "_po"])
@pytest.mark.parametrize("scorer", ["complex", "distmult"])
def test_bit_for_bit_against_the_32x32x16_instantiation(eng, scorer, combine, E, kge_switch):
    shapes = [(n, L) for n in (1, 15, 16, 17, 128, 130) for L in (1, 3)]
    _check_shapes(eng, kge_switch, scorer, combine, E, shapes, seed=E)


def test_work_list_crossing_pair_boundaries(eng, kge_switch):
    """32 pairs (4 batches x 2 sides x 4 chunks): pairs >= workgroups per XCD, the list of a workgroup is walked and
    streams units across a pair boundary."""
    _check_shapes(eng, kge_switch, "complex", "sp_po", 300, [(512, 4)], seed=5)


@pytest.mark.parametrize("E", [33, 97])
def test_no_stray_writes_on_the_pitched_buffer(eng, E, kge_switch):
    """`out` as pitched views (rows on the 256-byte pitch, the po block on a column of its own, as
    test_row_pitch_and_second_block_offset writes it): canaries in the pad columns, in the rows >= n and behind the last
    batch stay what they were -- also with a finite canary, which a comparison with NaN could not tell from a score."""
    n, L = 17, 3
    T, _, _ = _tables(eng, "complex", E)
    trip = _triples(E, n * L, 77)
    kge_switch.set("V8", 1)
    P = eng.score_pitch(E)
    canary = -12345.5
    big = torch.full((L + 1, n + 3, 2 * P), canary, device=DEV)
    out = big[:L, :n].view(L, n, 2, P)[:, :, :, :E]
    q = eng.build_queries_group(T, "sp_po", trip, n, L, flags=eng.FLAG_SPLIT_QUERY)
    eng.score_queries_group(T, q, out)
    torch.cuda.synchronize()
    mask = torch.zeros_like(big, dtype=torch.bool)
    mask[:L, :n].view(L, n, 2, P)[:, :, :, :E] = True
    assert bool((big[~mask] == canary).all()), "a canary outside the score blocks was overwritten"
    assert bool((big[mask] != canary).all()), "a score was not written"
    kge_switch.set("V8", 0)
    want = _one_by_one(eng, T, "sp_po", trip, n, L)
    for l in range(L):
        _same(out[l].reshape(n, -1), want[l], f"pitched E={E} batch {l}")


@pytest.mark.parametrize("scorer", ["complex", "distmult"])
def test_against_f32_arithmetic_at_the_mfma_bar(eng, scorer, kge_switch):
    """DESIGN section 4's bar for the matrix-core kernels, |d| <= 1e-5 scale + 1e-4 |ref|, against float32 arithmetic
    on the bf16 table values."""
    E, n, L = 300, 130, 3
    T, ent, rel = _tables(eng, scorer, E)
    trip = _triples(E, n * L, 91)
    kge_switch.set("V8", 1)
    got, _ = _group_into_canaries(eng, T, "sp_po", trip, n, L, E)
    e16, r16 = ko.f32_to_bf16(ent.float().numpy()), ko.f32_to_bf16(rel.float().numpy())
    O = ko.Tables(scorer, ko.bf16_to_f32(e16), ko.bf16_to_f32(r16))
    tn = trip.cpu().numpy()
    for l in range(L):
        t = tn[l * n:(l + 1) * n]
        ref = ko.score_sp_po(O, t[:, 0], t[:, 1], t[:, 2]).astype(np.float64)
        scale = max(1.0, float(np.sqrt(np.mean(ref ** 2))))
        err = np.abs(got[l].cpu().numpy().astype(np.float64) - ref)
        assert (err <= 1e-5 * scale + 1e-4 * np.abs(ref)).all(), (scorer, l, float(err.max()), scale)


def test_next_group_built_inside_the_launch(eng, kge_switch):
    """The fragments of the NEXT group that the 16x16x32 launch builds behind its last unit = build_queries_group's."""
    E, n, L = 300, 130, 3
    fl = eng.FLAG_SPLIT_QUERY
    T, _, _ = _tables(eng, "complex", E)
    g0, g1 = _triples(E, n * L, 101), _triples(E, n * L, 102)
    qs = [eng.QueriesGroup(T, "sp_po", n, L, flags=fl) for _ in range(3)]
    for q in qs:
        q.buf.zero_()   # (the padding between two batches' fragments is nobody's)
    eng.build_queries_group(T, "sp_po", g0, n, L, out=qs[0])
    eng.build_queries_group(T, "sp_po", g1, n, L, out=qs[2])
    out = torch.empty(L, n, 2 * E, device=DEV)
    eng.score_queries_group(T, qs[0], out, next_batch=g1, next_queries=qs[1])
    torch.cuda.synchronize()
    assert torch.equal(qs[1].buf, qs[2].buf), "in-launch build differs from build_queries_group"
    kge_switch.set("V8", 0)
    want = _one_by_one(eng, T, "sp_po", g0, n, L)
    for l in range(L):
        _same(out[l], want[l], f"scores of the launch that built the next group, batch {l}")
