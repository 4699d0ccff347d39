"""kge_score_pairs_bwd on bf16 ComplEx / DistMult tables (bwdg_run16: the backward of mixed-precision training) against
the float64 reference of tests/_pairs_bwd16_ref.py, inside its derived bound (C_ACC K + C) u A -- elementwise, on g_a,
g_p and g_tgt, in both directions.  Both operand roundings (G16 = RNE(gout), Q16 = RNE(fl32(q))) are restated exactly
there, so the bound covers float32 accumulation alone: a dropped query row or split part, a truncating cast, a pad
column left unwritten or dT taken from the unrounded query all exceed it (tests/test_pairs_bwd16_ref_cpu.py shows that on
these very inputs, 8 times over).

A fixed case list, each shape chosen for a branch of the five stages around the two products and of the choice between
gemm16_kernel and gemm32_kernel<unsigned short>; DESIGN.md ("Mixed-precision pair backward against float64") names the
branch of every case.  This is where the yardstick of test_gpu_ce.py::test_ce_bwd and of the composed path of
test_gpu_fuzz_shapes.py is itself asserted.

C_ACC = 2 is an assumption about the additions inside v_mfma_f32_32x32x16_bf16, not a measurement: every case prints its
largest err / bound per output (profiles/pairs_bwd16_bound.txt is one such run)."""
import ctypes

import numpy as np
import pytest
import torch

import _pairs_bwd16_ref as R16

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 1024      # floats of NaN in front of and between the regions of the guard test (4 KiB: 256-byte alignment is kept)
TAIL = 1 << 18  # and behind the last one: 1 MiB
NAN_BITS = 0x7FC00000
KGE_ERR_INVALID_ARG, KGE_ERR_UNSUPPORTED, KGE_ERR_WORKSPACE = -1, -2, -5  # include/kge_amd.h

_REF = {}


def _ref(case, direction):
    """inputs, reference and bound of one case and direction: computed once, shared, never modified"""
    key = (R16.case_id(case), direction)
    if key not in _REF:
        k = R16.make_case16(case, direction)
        args = R16.ref_args16(k)
        want, bound = R16.pairs_bwd16(*args), R16.pairs_bwd16_bound(*args)
        for x in (k["ent"], k["rel"], k["gout"]) + tuple(want) + tuple(bound):
            x.setflags(write=False)
        _REF[key] = (k, want, bound)
    return _REF[key]


def _t(x, dtype=None):
    x = torch.from_numpy(np.array(x))
    return x.to(DEV) if dtype is None else x.to(DEV, dtype)


def _device_inputs(k):
    """bf16 tables (the entity row pitch of the case), index tensors and float32 gout (its pitch) on the device"""
    from kge_amd import engine as eng
    n, m, d = k["n"], k["m"], k["d"]
    ent = _t(k["ent"], torch.bfloat16)  # bf16-valued: the conversion is exact
    assert torch.equal(ent.float().cpu(), torch.from_numpy(np.array(k["ent"])))
    if k.get("ent_ld"):
        buf = torch.zeros(k["E"], k["ent_ld"], device=DEV, dtype=torch.bfloat16)
        buf[:, :d] = ent
        ent = buf[:, :d]
    T = eng.Tables(k["name"], ent, _t(k["rel"], torch.bfloat16))
    a, p = _t(k["a"]), _t(k["p"])
    if k.get("triples32"):  # int32 index columns of one [n, 3] triple tensor: stride 3
        tr = torch.stack([a, p, a], dim=1).to(torch.int32).contiguous()
        a, p = tr[:, 0], tr[:, 1]
    targets = None if k["targets"] is None else _t(k["targets"])
    gout = _t(k["gout"])
    if k.get("gout_ld"):  # a column slice of a wider NaN-filled buffer
        buf = torch.full((n, k["gout_ld"]), float("nan"), device=DEV)
        buf[:, :m] = gout
        gout = buf[:, :m]
    return T, a, p, targets, gout


def _worst(got, want, bound):
    out = []
    for g, w, b in zip(got, want, bound):
        g = g.double().cpu().numpy().reshape(w.shape)
        assert np.isfinite(g).all()
        out.append(float((np.abs(g - w) / b).max()))
    return out


def _check(case, direction, got, want, bound, what="", factor=1.0):
    worst = _worst(got, want, bound)
    print(f"pairs_bwd16 {R16.case_id(case)}{what} {direction}: max err / bound  g_a {worst[0]:.4f}  g_p {worst[1]:.4f}  "
          f"g_tgt {worst[2]:.4f}")
    for g, w, b, nm in zip(got, want, bound, ("g_a", "g_p", "g_tgt")):
        g = g.double().cpu().numpy().reshape(w.shape)
        bad = np.abs(g - w) > factor * b
        assert not bad.any(), (R16.case_id(case), direction, nm, int(bad.sum()), np.argwhere(bad)[:4].tolist(), worst)


@pytest.mark.parametrize("case", R16.CASES16, ids=R16.case_id)
def test_pairs_bwd16_within_bound(case):
    from kge_amd import engine as eng
    for direction in ("sp", "po"):
        k, want, bound = _ref(case, direction)
        T, a, p, targets, gout = _device_inputs(k)
        got = eng.score_pairs_bwd(T, direction, a, p, targets, gout)
        torch.cuda.synchronize()
        _check(case, direction, got, want, bound)


MFMA16_CASES = [c for c in R16.CASES16 if c["d"] % 256 == 0]


@pytest.mark.parametrize("case", MFMA16_CASES, ids=R16.case_id)
def test_both_product_kernels_within_the_same_bound(case, kge_switch):
    """The d = 256 / 512 cases once more with BWD_GEMM_LIB = 1 (bwd_gemm16_enabled() false: both products on
    gemm32_kernel<unsigned short>, the float32 matrix cores on the widened operands).  Both runs are inside the bound and
    within twice the bound of each other: a ratio above 1 on gemm16_kernel alone is that kernel's or its instruction's, one
    on both is the reference's or the elementwise stages'."""
    from kge_amd import engine as eng
    assert len(MFMA16_CASES) == 14
    for direction in ("sp", "po"):
        k, want, bound = _ref(case, direction)
        T, a, p, targets, gout = _device_inputs(k)
        got16 = eng.score_pairs_bwd(T, direction, a, p, targets, gout)
        kge_switch.set("BWD_GEMM_LIB", 1)
        got32 = eng.score_pairs_bwd(T, direction, a, p, targets, gout)
        kge_switch.unset("BWD_GEMM_LIB")
        torch.cuda.synchronize()
        _check(case, direction, got16, want, bound, " (gemm16)")
        _check(case, direction, got32, want, bound, " (gemm32)")
        for x, y, b, nm in zip(got16, got32, bound, ("g_a", "g_p", "g_tgt")):
            diff = (x.double() - y.double()).abs().cpu().numpy().reshape(b.shape)
            assert (diff <= 2.0 * b).all(), (R16.case_id(case), direction, nm, float((diff / b).max()))


# ---- the ABI: a direct call with a caller's workspace ------------------------------------------------------------------
def _abi_call(T, direction, a, p, n, targets, m, gout, ldg, outs, ws, ws_bytes):
    """kge_score_pairs_bwd through ctypes on raw output and workspace pointers -> return code"""
    from kge_amd import _lib
    from kge_amd import engine as eng
    keep = []
    ai, pi, ti = eng._index(a, DEV, keep), eng._index(p, DEV, keep), eng._index(targets, DEV, keep)
    tc = T.c()
    return _lib.lib().kge_score_pairs_bwd(
        ctypes.byref(tc), _lib.SP_ if direction == "sp" else _lib.PO_, ai, pi, n, ti, m, gout.data_ptr(), ldg,
        None, 0, outs[0], outs[1], outs[2], ws, ws_bytes, eng._stream_handle(DEV))


def _workspace_bytes(T, n, m):
    from kge_amd import _lib
    tc = T.c()
    return int(_lib.lib().kge_score_bwd_workspace_bytes(ctypes.byref(tc), n, m))


def _nan_arena(sizes):
    """Regions of `sizes` floats inside ONE NaN-filled allocation, each starting on a 256-byte boundary, PAD floats of
    NaN between them and TAIL behind -> (arena, offsets in floats, pointers)"""
    total = 64 + sum((s + 63) // 64 * 64 + PAD for s in sizes) + TAIL
    arena = torch.full((total,), float("nan"), device=DEV)
    off = PAD + (-(arena.data_ptr() // 4 + PAD)) % 64  # 64 floats = 256 bytes
    offs = []
    for s in sizes:
        offs.append(off)
        off += (s + 63) // 64 * 64 + PAD
    assert off - PAD + TAIL <= total
    return arena, offs, [arena.data_ptr() + 4 * o for o in offs]


def _guards_intact(arena, offs, sizes):
    """every word of the arena outside [offs[i], offs[i] + sizes[i]) still carries the NaN's bits"""
    outside = torch.ones(arena.numel(), dtype=torch.bool, device=DEV)
    for o, s in zip(offs, sizes):
        outside[o:o + s] = False
    assert bool((arena.view(torch.int32)[outside] == NAN_BITS).all())


GUARD_CASES = [c for c in R16.CASES16 if R16.case_id(c) in ("complex-n37-E150-d256", "complex-n16-E1000-d256-listed300")]


@pytest.mark.parametrize("case", GUARD_CASES, ids=R16.case_id)
def test_outputs_workspace_and_nothing_else_are_written(case):
    """One direct ABI call with the three outputs AND a workspace of exactly kge_score_bwd_workspace_bytes (256-byte
    aligned) inside one NaN-filled arena: every word outside them keeps the NaN's bits, every output element is finite and
    inside the bound -- the split-K partials kept in g_tgt, the bf16 rows parked there, G16 (pad columns included) and Q16
    all stay inside their extents, and whatever NaN the outputs and the workspace held is overwritten or never read."""
    assert len(GUARD_CASES) == 2
    for direction in ("sp", "po"):
        k, want, bound = _ref(case, direction)
        T, a, p, targets, gout = _device_inputs(k)
        need = _workspace_bytes(T, k["n"], k["m"])
        mp = (k["m"] + 7) // 8 * 8
        assert need == (k["n"] * mp * 2 + 255) // 256 * 256 + (k["n"] * k["d"] * 2 + 255) // 256 * 256
        sizes = [w.size for w in want] + [need // 4]
        arena, offs, ptrs = _nan_arena(sizes)
        assert ptrs[3] % 256 == 0 and all(q % 16 == 0 for q in ptrs)
        assert _abi_call(T, direction, a, p, k["n"], targets, k["m"], gout, gout.stride(0), ptrs[:3], ptrs[3], need) == 0
        torch.cuda.synchronize()
        _guards_intact(arena, offs, sizes)
        _check(case, direction, [arena[o:o + s] for o, s in zip(offs[:3], sizes[:3])], want, bound, " (guards)")


def test_workspace_and_shape_contract():
    """What bwdg_run16, run_pairs_bwd_gemm16 and the bf16 branch of kge_score_pairs_bwd reject, with the code each of
    them returns -- and a rejected call leaves NaN-prefilled outputs untouched."""
    from kge_amd import engine as eng
    k, want, _ = _ref(R16.CASES16[2], "sp")  # complex 37 / 150 / 256
    n, m, d = k["n"], k["m"], k["d"]
    T, a, p, targets, gout = _device_inputs(k)
    need = _workspace_bytes(T, n, m)
    g16_bytes = (n * ((m + 7) // 8 * 8) * 2 + 255) // 256 * 256
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256

    def rejected(Tb, nn, mm, dd, ldg, wsp, wsb, code):
        outs = [torch.full((nn, dd), float("nan"), device=DEV), torch.full((nn, dd), float("nan"), device=DEV),
                torch.full((mm, dd), float("nan"), device=DEV)]
        rc = _abi_call(Tb, "sp", a, p, nn, None, mm, gout, ldg, [o.data_ptr() for o in outs], wsp, wsb)
        torch.cuda.synchronize()
        assert rc == code, (rc, code)
        for o in outs:
            assert bool((o.view(torch.int32) == NAN_BITS).all())

    rejected(T, n, m, d, m, None, need, KGE_ERR_WORKSPACE)                        # no workspace
    rejected(T, n, m, d, m, base + 128, need - 128, KGE_ERR_WORKSPACE)            # misaligned by 128 bytes
    rejected(T, n, m, d, m, base, g16_bytes + n * d * 2 - 1, KGE_ERR_WORKSPACE)   # one byte short
    rejected(T, n, m, d, m - 1, base, need, KGE_ERR_INVALID_ARG)                  # ldg < m
    # TransE on bf16 tables: no mixed-precision backward
    Tt = eng.Tables("transe", T.ent, T.rel)
    rejected(Tt, n, m, d, m, base, need, KGE_ERR_UNSUPPORTED)
    # odd d (DistMult; ComplEx needs an even d as a table already): the query pairs of the bf16 kernels do not exist
    ent33 = torch.ones(m, 33, device=DEV, dtype=torch.bfloat16)
    rel33 = torch.ones(7, 33, device=DEV, dtype=torch.bfloat16)
    T33 = eng.Tables("distmult", ent33, rel33)
    assert _workspace_bytes(T33, n, m) <= need
    rejected(T33, n, m, 33, m, base, need, KGE_ERR_UNSUPPORTED)
    # ... and the smallest accepted workspace is accepted: the same call as above, one byte more
    outs = [torch.full(w.shape, float("nan"), device=DEV) for w in want]
    assert _abi_call(T, "sp", a, p, n, None, m, gout, m, [o.data_ptr() for o in outs], base, g16_bytes + n * d * 2) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(o).all()) for o in outs)


DET_CASES = [c for c in R16.CASES16 if R16.case_id(c) in ("complex-n37-E150-d256", "complex-n37-E150-d40")]


@pytest.mark.parametrize("case", DET_CASES, ids=R16.case_id)
def test_repeated_calls_give_identical_bits(case):
    """Split-K on either kernel is a sum of partials in a fixed order (bwdg_reduce_kernel: gemm16_kernel's through
    bwdg_dq16, gemm32_kernel's through the P > 1 tail of run_gemm32), no float atomics anywhere on this entry's path
    (bwdg_chain16_kernel's atomics belong to the accumulating entries, acc_ent != NULL): three calls, the same bits."""
    from kge_amd import engine as eng
    assert len(DET_CASES) == 2
    k, _, _ = _ref(case, "sp")
    T, a, p, targets, gout = _device_inputs(k)
    first = eng.score_pairs_bwd(T, "sp", a, p, targets, gout)
    for _ in range(2):
        again = eng.score_pairs_bwd(T, "sp", a, p, targets, gout)
        for x, y in zip(first, again):
            assert torch.equal(x, y)
