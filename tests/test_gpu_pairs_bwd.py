"""kge_score_pairs_bwd on float32 tables against the float64 closed forms of tests/_pairs_bwd_ref.py, inside the
derived rounding bound (K + C) u A of that module -- elementwise, on g_a, g_p and g_tgt, in both directions.

A fixed case list, each shape chosen for a branch of gemm32_kernel / run_gemm32 (ComplEx, DistMult) or of
bwd_pairs_kernel / launch_bwd_pairs (TransE, RotatE); DESIGN.md ("Pair-score backward against float64") names the
branch of every case.  tests/test_pairs_bwd_ref_cpu.py holds the reference to float64 autograd and shows, on these very
inputs, that a dropped reduction index, block or split part, a flipped cross term, a neighbour's relation row, a
coordinate read as zero or a misplaced epsilon exceeds the bound 8 times over.  This is where the error of the
composed float32 path -- the yardstick of test_gpu_ce_f32.py, test_gpu_multilabel_f32.py, test_gpu_ce_dist.py and
test_gpu_multilabel_dist.py -- is itself asserted.

Every case prints its largest err / bound per output (profiles/pairs_bwd_bound.txt is one such run)."""
import ctypes

import numpy as np
import pytest
import torch

import _pairs_bwd_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 1024      # floats of NaN in front of and between the outputs of the guard tests (outputs stay 16-byte aligned)
TAIL = 1 << 18  # and behind the last one, g_tgt: 1 MiB, more than every split-K partial of dQ laid end to end
NAN_BITS = 0x7FC00000


def _t(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else torch.from_numpy(
        np.ascontiguousarray(x)).to(DEV, dtype)


def _device_inputs(k):
    """Tables (the row pitch of the case), index tensors and gout (its pitch) on the device"""
    from kge_amd import engine as eng
    n, m, d = k["n"], k["m"], k["d"]
    ent = _t(k["ent"])
    if k.get("ent_ld"):
        buf = torch.zeros(k["E"], k["ent_ld"], device=DEV)
        buf[:, :d] = ent
        ent = buf[:, :d]
    T = eng.Tables(k["name"], ent, _t(k["rel"]), l_norm=k["l_norm"])
    a, p = _t(k["a"]), _t(k["p"])
    if k.get("triples32"):  # int32 index columns of one [n, 3] triple tensor: stride 3
        tr = torch.stack([a, p, a], dim=1).to(torch.int32).contiguous()
        a, p = tr[:, 0], tr[:, 1]
    targets = None if k["targets"] is None else _t(k["targets"])
    gout = _t(k["gout"])
    if k.get("gout_ld"):  # a column slice of a wider buffer
        buf = torch.full((n, k["gout_ld"]), float("nan"), device=DEV)
        buf[:, :m] = gout
        gout = buf[:, :m]
    return T, a, p, targets, gout


def _scores(T, k, a, p, targets):
    """the forward's float32 scores: the distance models with l_norm != 1 take the distance from them"""
    from kge_amd import engine as eng
    if k["name"] in ("complex", "distmult") or k["l_norm"] == 1.0:
        return None
    return eng.score_sp(T, a, p, targets) if k["direction"] == "sp" else eng.score_po(T, p, a, targets)


def _check(case, direction, got, want, bound, what=""):
    worst = []
    for g, w, b in zip(got, want, bound):
        g = g.double().cpu().numpy().reshape(w.shape)
        assert np.isfinite(g).all()
        err = np.abs(g - w)
        worst.append(float((err / np.maximum(b, 1e-300)).max()) if err.size and err.max() > 0 else 0.0)
    print(f"pairs_bwd {R.case_id(case)}{what} {direction}: max err / bound  g_a {worst[0]:.4f}  g_p {worst[1]:.4f}  "
          f"g_tgt {worst[2]:.4f}")
    for g, w, b, nm in zip(got, want, bound, ("g_a", "g_p", "g_tgt")):
        g = g.double().cpu().numpy().reshape(w.shape)
        bad = np.abs(g - w) > b
        assert not bad.any(), (R.case_id(case), direction, nm, int(bad.sum()), np.argwhere(bad)[:4].tolist(), worst)


@pytest.mark.parametrize("case", R.ALL_CASES, ids=R.case_id)
def test_pairs_bwd_within_bound(case):
    from kge_amd import engine as eng
    for direction in ("sp", "po"):
        k = R.make_case(case, direction)
        args = R.ref_args(k)
        want, bound = R.pairs_bwd(*args), R.pairs_bwd_bound(*args)
        T, a, p, targets, gout = _device_inputs(k)
        got = eng.score_pairs_bwd(T, direction, a, p, targets, gout, _scores(T, k, a, p, targets))
        torch.cuda.synchronize()
        _check(case, direction, got, want, bound)


GUARD_CASES = [c for c in R.ALL_CASES if (c["name"], c["n"], c["E"], c["d"]) in
               (("complex", 37, 150, 40), ("transe", 65, 150, 33)) and not c.get("triples32")]


def _abi_call(T, direction, a, p, n, targets, m, gout, ldg, scores, outs):
    """kge_score_pairs_bwd through ctypes on raw output pointers -> return code"""
    from kge_amd import _lib
    from kge_amd import engine as eng
    keep = []
    ai, pi, ti = eng._index(a, DEV, keep), eng._index(p, DEV, keep), eng._index(targets, DEV, keep)
    tc = T.c()
    return _lib.lib().kge_score_pairs_bwd(
        ctypes.byref(tc), _lib.SP_ if direction == "sp" else _lib.PO_, ai, pi, n, ti, m, gout.data_ptr(), ldg,
        None if scores is None else scores.data_ptr(), 0 if scores is None else scores.stride(0), outs[0], outs[1], outs[2],
        None, 0, eng._stream_handle(DEV))


def _nan_arena(sizes):
    """The three outputs (g_a, g_p, g_tgt) inside ONE NaN-filled allocation -> (arena, offsets, pointers)"""
    offs, off = [], PAD
    for s in sizes:
        offs.append(off)
        off += (s + 3) // 4 * 4 + PAD
    arena = torch.full((off - PAD + TAIL,), float("nan"), device=DEV)
    return arena, offs, [arena.data_ptr() + 4 * o for o in offs]


def _guards_intact(arena, offs, sizes):
    """every float of the arena outside [offs[i], offs[i] + sizes[i]) still carries the NaN's bits"""
    outside = torch.ones(arena.numel(), dtype=torch.bool, device=DEV)
    for o, s in zip(offs, sizes):
        outside[o:o + s] = False
    assert bool((arena.view(torch.int32)[outside] == NAN_BITS).all())


def _outputs(arena, offs, sizes):
    return [arena[o:o + s] for o, s in zip(offs, sizes)]


@pytest.mark.parametrize("case", GUARD_CASES, ids=R.case_id)
def test_outputs_and_nothing_else_are_written(case):
    """One direct ABI call per scorer family with the three outputs inside NaN-filled buffers: every output element
    finite and within the bound (the split-K partials and gathered rows kept in g_tgt, the pre-zeroed atomics targets:
    all overwritten), no byte outside them changed."""
    assert len(GUARD_CASES) == 2
    for direction in ("sp", "po"):
        k = R.make_case(case, direction)
        args = R.ref_args(k)
        want, bound = R.pairs_bwd(*args), R.pairs_bwd_bound(*args)
        T, a, p, targets, gout = _device_inputs(k)
        sc = _scores(T, k, a, p, targets)
        sizes = [w.size for w in want]
        arena, offs, ptrs = _nan_arena(sizes)
        assert _abi_call(T, direction, a, p, k["n"], targets, k["m"], gout, gout.stride(0), sc, ptrs) == 0
        torch.cuda.synchronize()
        _guards_intact(arena, offs, sizes)
        _check(case, direction, _outputs(arena, offs, sizes), want, bound, " (guards)")


@pytest.mark.parametrize("name,dtype,l_norm", [("complex", torch.float32, 1.0), ("transe", torch.float32, 2.0),
                                               ("complex", torch.bfloat16, 1.0)],
                         ids=["complex-f32", "transe-L2-f32", "complex-bf16"])
def test_empty_sides_zero_the_other_side(name, dtype, l_norm):
    """include/kge_amd.h: the gradients are OVERWRITTEN.  No queries: g_tgt = 0; no targets: g_a = g_p = 0 -- and
    nothing outside them is touched."""
    from kge_amd import engine as eng
    E, Rn, d = 9, 3, 8
    rng = np.random.default_rng(3)
    T = eng.Tables(name, _t(rng.standard_normal((E, d)).astype(np.float32), dtype),
                   _t(rng.standard_normal((Rn, d)).astype(np.float32), dtype), l_norm=l_norm)
    ix = torch.zeros(4, dtype=torch.int64, device=DEV)
    gout = torch.ones(4, E, device=DEV)
    for direction in ("sp", "po"):
        # n = 0 queries against all E entities
        sizes = [4, 4, E * d]  # (g_a, g_p: no element belongs to the call)
        arena, offs, ptrs = _nan_arena(sizes)
        assert _abi_call(T, direction, ix, ix, 0, None, E, gout, E, None, ptrs) == 0
        torch.cuda.synchronize()
        _guards_intact(arena, offs, [0, 0, E * d])
        assert bool((_outputs(arena, offs, sizes)[2] == 0).all())
        # n = 4 queries against an empty target list
        sizes = [4 * d, 4 * d, 4]
        arena, offs, ptrs = _nan_arena(sizes)
        assert _abi_call(T, direction, ix, ix, 4, ix, 0, gout, E, None, ptrs) == 0
        torch.cuda.synchronize()
        _guards_intact(arena, offs, [4 * d, 4 * d, 0])
        out = _outputs(arena, offs, sizes)
        assert bool((out[0] == 0).all()) and bool((out[1] == 0).all())
