"""Generate tests/golden/transh_scores_l{1,2}_d{32,33}.npz from the LIVE reference (kge/model/transh.py), in the style of
make_golden.py (not named scores_*.npz: tests/test_oracle_golden.py runs every file of that pattern through the C
oracle, which has no TransH): seeded inputs, the reference's own KgeModel.score_spo / score_sp / score_po /
score_sp_po on them, inputs and outputs committed.  Run inside the build container only (needs the reference tree):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_transh.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.dont_write_bytecode = True

import ref_harness as rh  # noqa: E402

rh.import_reference()
import torch  # noqa: E402

CASES = [
    # name, l_norm, E, R, d, n
    ("transh_l1_d32", 1.0, 37, 5, 32, 11),
    ("transh_l2_d32", 2.0, 37, 5, 32, 11),
    ("transh_l1_d33", 1.0, 29, 4, 33, 9),
    ("transh_l2_d33", 2.0, 29, 4, 33, 9),
]


def main():
    for name, lp, E, R, d, n in CASES:
        torch.manual_seed(1234)
        m = rh.make_model("transh", E, R, d, options={"transh.l_norm": lp})
        ent, rel = rh.get_tables(m)
        assert rel.shape[1] == 2 * d
        with torch.no_grad():  # a relation whose hyperplane normal is zero: w^ = 0, no NaN
            m.get_p_embedder()._embeddings.weight[0, d:] = 0.0
        ent, rel = rh.get_tables(m)
        g = torch.Generator().manual_seed(99)
        s = torch.randint(E, (n,), generator=g)
        p = torch.randint(R, (n,), generator=g)
        p[0] = 0
        o = torch.randint(E, (n,), generator=g)
        sub = torch.randperm(E, generator=g)[: max(3, E // 3)]
        with torch.no_grad():
            out = {
                "spo": m.score_spo(s, p, o, "o"),
                "sp": m.score_sp(s, p),
                "po": m.score_po(p, o),
                "sp_sub": m.score_sp(s, p, sub),
                "po_sub": m.score_po(p, o, sub),
                "sp_po_sub": m.score_sp_po(s, p, o, sub),
            }
        np.savez_compressed(
            os.path.join(HERE, name.replace("transh_", "transh_scores_") + ".npz"), ent=ent.numpy(), rel=rel.numpy(),
            s=s.numpy(), p=p.numpy(), o=o.numpy(), sub=sub.numpy(), l_norm=np.float32(lp), **{k: v.numpy() for k, v in out.items()})
        print(name, {k: tuple(v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main()
