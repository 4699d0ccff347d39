"""The embedder-dropout entries at the drop-in boundary, without a GPU: the symbols exist and are bound, the header
cites the reference, every decline of include/kge_amd.h ("Embedder dropout") comes back as KGE_ERR_UNSUPPORTED before
anything is launched, the ABI version is unchanged and the generator has ONE device definition."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

OK, INVALID, UNSUPPORTED = 0, -1, -2
P = ctypes.c_void_p(16)  # never dereferenced on these paths
NAMES = ("kge_embed_dropout", "kge_score_spo_dropout", "kge_score_neg_dropout", "kge_score_spo_dropout_bwd_accum",
         "kge_score_neg_dropout_bwd_accum")


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


def _drop(p_ent=0.1, p_rel=0.2, seed=1, call=1):
    from kge_amd._lib import KgeDropout
    return KgeDropout(p_ent, p_rel, seed, call)


def test_symbols_prototypes_and_citations(lib):
    from kge_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "kge_amd.h")).read()
    for name in NAMES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
        decl = header[:header.index("int " + name + "(")]
        comment = decl[decl.rindex("/*"):]
        assert "lookup_embedder.py:96-105" in comment, name
        if "score" in name:
            assert "sampler.py:263-306" in comment or "kge_model.py:663-680" in comment, name
    assert "typedef struct kge_dropout" in header and "0x44524F50" in header
    assert ctypes.sizeof(_lib.KgeDropout) == 24
    assert lib.kge_abi_version() == 1
    for fn in ("embed_dropout", "score_spo_dropout", "score_neg_dropout", "score_spo_dropout_bwd_accum",
               "score_neg_dropout_bwd_accum", "Dropout"):
        assert callable(getattr(engine, fn)), fn
    assert engine.Dropout(0.1, 0.2, 3, 4)._fields == ("p_ent", "p_rel", "seed", "call")


def _calls(lib, t, d, n=4, K=3, occ0=0):
    tb = ctypes.byref(t)
    db = ctypes.byref(d) if d is not None else None
    ix = _ix()
    return {
        "embed": lambda: lib.kge_embed_dropout(tb, 0, ix, n, 0, occ0, db, P, t.dim, None),
        "spo": lambda: lib.kge_score_spo_dropout(tb, ix, ix, ix, n, P, db, None),
        "neg": lambda: lib.kge_score_neg_dropout(tb, ix, ix, ix, n, 2, P, 1, K, K, P, K, db, None),
        "spo_bwd": lambda: lib.kge_score_spo_dropout_bwd_accum(tb, ix, ix, ix, n, P, P, P, t.dim, P, t.rel_dim, db, None),
        "neg_bwd": lambda: lib.kge_score_neg_dropout_bwd_accum(tb, ix, ix, ix, n, 0, P, 1, K, K, P, K, P, K, P, t.dim, P,
                                                               t.rel_dim, db, None),
    }


def test_every_decline_is_unsupported_before_a_launch(lib):
    t = _tables()
    # probabilities outside [0, 1), NaN, or both 0
    for bad in (_drop(1.0, 0.1), _drop(0.1, 1.0), _drop(-0.1, 0.1), _drop(0.1, -0.5), _drop(float("nan"), 0.1),
                _drop(0.0, 0.0), _drop(1.5, 0.0)):
        for name, call in _calls(lib, t, bad).items():
            assert call() == UNSUPPORTED, (name, bad.p_ent, bad.p_rel)
    # bf16 tables, TransH and RESCAL tables
    for tb in (_tables(dtype=1), _tables(scorer=4, dim=8, rel_dim=16), _tables(scorer=5, dim=8, rel_dim=64)):
        for name, call in _calls(lib, tb, _drop()).items():
            assert call() == UNSUPPORTED, (name, tb.scorer, tb.dtype)
    # ... in front of every other check, as every entry without a TransH / RESCAL kernel declines them: NULL arguments too
    for tb in (_tables(scorer=4, dim=8, rel_dim=16), _tables(scorer=5, dim=8, rel_dim=64)):
        for name, call in _calls(lib, tb, None).items():
            assert call() == UNSUPPORTED, (name, tb.scorer)
    # rows wider than 1024 in the scoring and backward entries
    for name, call in _calls(lib, _tables(dim=1032), _drop()).items():
        if name != "embed":
            assert call() == UNSUPPORTED, name
    # an occurrence number, or n * num_neg, at or above 2^32
    c = _calls(lib, t, _drop(), n=2, occ0=2 ** 32 - 1)
    assert c["embed"]() == UNSUPPORTED
    assert _calls(lib, t, _drop(), n=1, occ0=2 ** 32)["embed"]() == UNSUPPORTED
    big = _calls(lib, t, _drop(), n=2 ** 16, K=2 ** 16)
    assert big["neg"]() == UNSUPPORTED and big["neg_bwd"]() == UNSUPPORTED
    big = _calls(lib, t, _drop(), n=2 ** 32 + 1)
    assert big["spo"]() == UNSUPPORTED and big["spo_bwd"]() == UNSUPPORTED
    # the undropped entries' own argument errors come first; a missing record is one
    for name, call in _calls(lib, t, None).items():
        assert call() == INVALID, name
    for name, call in _calls(lib, t, _drop(), n=-1).items():
        assert call() == INVALID, name
    assert _calls(lib, _tables(scorer=3, dim=32, rel_dim=32), _drop())["spo"]() == INVALID  # RotatE, rel_dim != dim / 2
    # empty calls launch nothing
    for name, call in _calls(lib, t, _drop(), n=0).items():
        assert call() == OK, name


def test_one_generator_one_mask_definition():
    csrc = os.path.join(ROOT, "kge_amd", "csrc")
    defs = [f for f in os.listdir(csrc) if f.endswith((".hip", ".hpp"))
            and re.search(r"Philox4 philox4x32_10\(", open(os.path.join(csrc, f)).read())]
    assert defs == ["philox.hpp"], defs
    for f in ("neg_sample.hip", "score_spo.hip", "bwd.hip", "embed.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '"philox.hpp"' in src or '"spo_device.hpp"' in src, f
    code = "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, "philox.hpp")).read().splitlines())
    assert not re.search(r"getenv|environ", code)
    assert "philox.hpp" in open(os.path.join(csrc, "Makefile")).read()
