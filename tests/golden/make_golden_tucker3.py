"""Generate tests/golden/tucker3_scores_d{8,13}.npz from the LIVE reference (kge/model/relational_tucker3.py), in the style
of make_golden_rescal.py: seeded inputs, the reference's own KgeModel.score_spo / score_sp / score_po / score_sp_po on them,
inputs and outputs committed.  Needs the reference tree under `oracle/_ref` (or wherever ref_harness finds it):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tucker3.py

(the `tucker3_` prefix keeps the files out of the `scores_*.npz` glob of the older tests)
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
    # name, E, R, d, d_r, n
    ("tucker3_scores_d8", 37, 5, 8, 5, 11),
    ("tucker3_scores_d13", 29, 4, 13, 7, 9),
]


def main():
    for name, E, R, d, dr, n in CASES:
        torch.manual_seed(1234)
        m = rh.make_model("relational_tucker3", E, R, d,
                          options={"relational_tucker3.entity_embedder.dim": d,
                                   "relational_tucker3.relation_embedder.base_embedder.dim": dr})
        sd = m.state_dict()
        ent = sd["_entity_embedder._embeddings.weight"]
        base = sd["_relation_embedder.base_embedder._embeddings.weight"]
        proj = sd["_relation_embedder.projection.weight"]
        assert tuple(base.shape) == (R, dr) and tuple(proj.shape) == (d * d, dr)
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
        np.savez_compressed(os.path.join(HERE, name + ".npz"), ent=ent.numpy(), base=base.numpy(), proj=proj.numpy(),
                            s=s.numpy(), p=p.numpy(), o=o.numpy(), sub=sub.numpy(), **{k: v.numpy() for k, v in out.items()})
        print(name, {k: tuple(v.shape) for k, v in out.items()})


if __name__ == "__main__":
    main()
