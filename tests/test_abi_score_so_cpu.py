"""kge_score_so / kge_score_so_bwd_accum at the drop-in boundary, without a GPU: the symbols exist in libkge_amd.so and in
kge_amd._C, every return code of the header's gate comes back before anything is launched, the ABI version is
unchanged, and the new source file reads no environment variable."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -5
P = ctypes.c_void_p(16)  # never dereferenced on these paths


@pytest.fixture(scope="module")
def lib():
    from kge_amd import _lib
    _lib.build()
    return _lib.lib()


def _tables(scorer=0, dtype=0, dim=32, rel_dim=None, l_norm=1.0, R=3):
    from kge_amd._lib import KgeTables
    rel_dim = dim if rel_dim is None else rel_dim
    return KgeTables(P, P, dtype, scorer, 10, R, dim, rel_dim, dim, rel_dim, l_norm, 0)


def _ix(ptr=P, stride=1):
    from kge_amd._lib import KgeIndex
    return KgeIndex(ptr, 1, 0, stride)


def test_symbols_exist_and_the_abi_version_is_unchanged(lib):
    from kge_amd import _lib
    for name in ("kge_score_so", "kge_score_so_bwd_accum", "kge_score_so_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "kge_amd.h")).read()
    for name in ("kge_score_so", "kge_score_so_bwd_accum"):
        decl = header[:header.index("int " + name + "(")]
        comment = decl[decl.rindex("/*"):]
        assert "kge_model.py:727-747" in comment and ":202-209" in comment, name
    assert lib.kge_abi_version() == 1
    ext = _lib.ext()
    assert ext.abi_version() == 1
    assert callable(ext.score_so) and callable(ext.score_so_bwd_accum)
    ent, rel, ix = torch.randn(10, 8), torch.randn(3, 8), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ext.score_so(ent, rel, 1, 1.0, 0, ix, ix, None)
    from kge_amd import engine
    assert callable(engine.score_so) and callable(engine.score_so_bwd)


def test_forward_return_codes_without_a_launch(lib):
    t = _tables()
    fwd = lambda tb, n=4, rels=None, m=3, out=P, ldo=None, wsb=0, s=None: lib.kge_score_so(
        ctypes.byref(tb) if tb is not None else None, s or _ix(), _ix(), n, rels or _ix(None), m, out,
        m if ldo is None else ldo, None, wsb, None)
    assert fwd(None) == INVALID
    assert fwd(t, m=2) == INVALID                      # NULL rels: m must be num_rel
    assert fwd(t, n=-1) == INVALID and fwd(t, rels=_ix(), m=-1) == INVALID
    assert fwd(t, ldo=2) == INVALID                    # ldo < m
    assert fwd(t, wsb=-1) == INVALID
    assert fwd(t, out=None) == INVALID
    assert fwd(t, s=_ix(None)) == INVALID              # no subject ids
    assert fwd(t, rels=_ix(P, 0), m=2) == INVALID      # a stride below 1
    assert fwd(t, n=0, out=None) == OK                 # empty: nothing is launched
    assert fwd(t, rels=_ix(), m=0, out=None) == OK
    # rows too wide for the LDS tile, and scorers outside the four
    assert fwd(_tables(dim=1032)) == UNSUPPORTED and fwd(_tables(dtype=1, dim=2056)) == UNSUPPORTED
    assert fwd(_tables(scorer=4, dim=8, rel_dim=16)) == UNSUPPORTED    # TransH
    assert fwd(_tables(scorer=5, dim=8, rel_dim=64)) == UNSUPPORTED    # RESCAL
    assert fwd(_tables(scorer=3, dim=32, rel_dim=32)) == INVALID       # RotatE with rel_dim != dim / 2
    # the workspace: no shape needs one today, so KGE_ERR_WORKSPACE cannot be provoked -- the query says 0
    for tb in (t, _tables(scorer=3, dim=32, rel_dim=16), _tables(dtype=1, dim=2048)):
        assert lib.kge_score_so_workspace_bytes(ctypes.byref(tb), 512, 237) == 0
    assert lib.kge_status_string(WORKSPACE) == b"workspace too small"


def test_backward_return_codes_without_a_launch(lib):
    t = _tables()
    bwd = lambda tb, n=4, rels=None, m=3, gout=P, ldg=None, scores=None, lds=0, ge=P, ge_ld=None, gr=P, gr_ld=None, wsb=0: \
        lib.kge_score_so_bwd_accum(ctypes.byref(tb) if tb is not None else None, _ix(), _ix(), n, rels or _ix(None), m,
                                   gout, m if ldg is None else ldg, scores, lds, ge, tb.dim if ge_ld is None else ge_ld,
                                   gr, tb.rel_dim if gr_ld is None else gr_ld, None, wsb, None)
    assert bwd(t, m=2) == INVALID and bwd(t, n=-1) == INVALID and bwd(t, wsb=-1) == INVALID
    assert bwd(t, ldg=2) == INVALID and bwd(t, scores=P, lds=2) == INVALID
    assert bwd(t, gout=None) == INVALID and bwd(t, ge=None) == INVALID and bwd(t, gr=None) == INVALID
    assert bwd(t, ge_ld=31) == INVALID and bwd(t, gr_ld=31) == INVALID
    assert bwd(t, n=0) == OK and bwd(t, rels=_ix(), m=0) == OK
    assert bwd(_tables(dtype=1)) == UNSUPPORTED                        # bf16 tables
    assert bwd(_tables(dim=1032)) == UNSUPPORTED and bwd(_tables(dtype=1, dim=1032)) == UNSUPPORTED
    assert bwd(_tables(scorer=5, dim=8, rel_dim=64)) == UNSUPPORTED
    # TransE / RotatE with l_norm != 1 need the forward scores
    for scorer, rel_dim in ((2, 32), (3, 16)):
        for lp in (2.0, 3.0):
            assert bwd(_tables(scorer=scorer, rel_dim=rel_dim, l_norm=lp)) == INVALID, (scorer, lp)


def test_front_end_declines_what_the_kernel_does_not_take():
    from kge_amd import engine, model
    assert engine.score_so_supported("complex", torch.float32, 1024, 512)
    assert not engine.score_so_supported("complex", torch.float32, 1032, 512)
    assert engine.score_so_supported("rotate", torch.bfloat16, 2048, 512)
    assert not engine.score_so_supported("transh", torch.float32, 64, 512)
    assert not engine.score_so_supported("rescal", torch.float32, 8, 512)
    assert not engine.score_so_supported("distmult", torch.float16, 64, 512)
    # CPU parameters: the composed path, as before
    m = model.create("distmult", 20, 4, 8)
    s, o = torch.tensor([1, 2, 3]), torch.tensor([4, 5, 6])
    assert not model.score_so_fusable("distmult", m.get_s_embedder().weight, m.get_p_embedder().weight, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):  # (RelationalScorer.score_emb's kernels, as before)
        m.score_so(s, o)


def test_the_new_source_reads_no_environment_variable():
    src = open(os.path.join(ROOT, "kge_amd", "csrc", "score_so.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"getenv|environ", code)
    assert "score_so.hip" in open(os.path.join(ROOT, "kge_amd", "csrc", "Makefile")).read()
