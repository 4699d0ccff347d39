"""Generate tests/golden/rescal_scores_d{8,13}.npz from the LIVE reference (kge/model/rescal.py), in the style of
make_golden_transh.py: seeded inputs, the reference's own KgeModel.score_spo / score_sp / score_po / score_sp_po on them,
inputs and outputs committed.  Needs the reference tree under `oracle/_ref` (or wherever ref_harness finds it):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rescal.py
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
    # name, E, R, d, n
    ("rescal_scores_d8", 37, 5, 8, 11),
    ("rescal_scores_d13", 29, 4, 13, 9),
]


def main():
    for name, E, R, d, n in CASES:
        torch.manual_seed(1234)
        m = rh.make_model("rescal", E, R, d)
        ent, rel = rh.get_tables(m)
        assert rel.shape[1] == d * d
        g = torch.Generator().manual_seed(99)
        s = torch.randint(E, (n,), generator=g)
        p = torch.randint(R, (n,), generator=g)
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
        np.savez_compressed(os.path.join(HERE, name + ".npz"), ent=ent.numpy(), rel=rel.numpy(), s=s.numpy(), p=p.numpy(),
                            o=o.numpy(), sub=sub.numpy(), **{k: v.numpy() for k, v in out.items()})
        print(name, {k: tuple(v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main()
