"""The surface of the dense-row losses that the rest of the repository and outside callers use by position, without a GPU:
the twelve dist / f32 engine functions, the three `*_supported` queries and the `forward` of the nine one-sided loss
nodes.  The functions are bindings of shared bodies and the nodes subclasses of one base; their signatures are what the
separate implementations before them had (the literals below were printed by inspect.signature on those)."""
import inspect

import pytest

T = "t: kge_amd.engine.Tables, direction: str, a, p"
ENGINE = {
    "ce_dist_supported": "(t: kge_amd.engine.Tables) -> bool",
    "ce_f32_supported": "(t: kge_amd.engine.Tables) -> bool",
    "multilabel_f32_supported": "(t: kge_amd.engine.Tables) -> bool",
    "ce_dist_fwd": f"({T}, label, chunk_cols: int = 0)",
    "ce_dist_bwd": f"({T}, label, lse, g_rows=None, g_scalar: float = 1.0, chunk_cols: int = 0)",
    "kl_dist_fwd": f"({T}, lbl_rowptr, lbl_col, label_weight=None, chunk_cols: int = 0)",
    "kl_dist_bwd": f"({T}, lbl_rowptr, lbl_col, lse, g_rows=None, g_scalar: float = 1.0, label_weight=None, "
                   "chunk_cols: int = 0)",
    "bce_dist_fwd": f"({T}, lbl_rowptr, lbl_col, offset: float = 0.0, chunk_cols: int = 0)",
    "bce_dist_bwd": f"({T}, lbl_rowptr, lbl_col, offset: float = 0.0, g_rows=None, g_scalar: float = 1.0, "
                    "chunk_cols: int = 0)",
    "ce_f32_fwd": f"({T}, label, chunk_cols: int = 0)",
    "ce_f32_bwd": f"({T}, label, lse, g_rows=None, g_scalar: float = 1.0, chunk_cols: int = 0)",
    "kl_f32_fwd": f"({T}, lbl_rowptr, lbl_col, label_weight=None, chunk_cols: int = 0)",
    "kl_f32_bwd": f"({T}, lbl_rowptr, lbl_col, lse, g_rows=None, g_scalar: float = 1.0, label_weight=None, "
                  "label_bias=None, chunk_cols: int = 0)",
    "bce_f32_fwd": f"({T}, lbl_rowptr, lbl_col, offset: float = 0.0, chunk_cols: int = 0)",
    "bce_f32_bwd": f"({T}, lbl_rowptr, lbl_col, offset: float = 0.0, g_rows=None, g_scalar: float = 1.0, "
                   "chunk_cols: int = 0)",
}

N = "ctx, direction, ent, rel, a, p"
NODES = {
    "_FusedCE": f"({N}, label, tables16)",
    "_FusedCEDist": f"({N}, label, tables, chunk_cols=0)",
    "_FusedCEF32": f"({N}, label, tables, chunk_cols=0)",
    "_FusedKL": f"({N}, rowptr, col, label_weight, label_bias, tables16)",
    "_FusedKLDist": f"({N}, rowptr, col, label_weight, tables, chunk_cols=0)",
    "_FusedKLF32": f"({N}, rowptr, col, label_weight, label_bias, tables, chunk_cols=0)",
    "_FusedBCE": f"({N}, rowptr, col, offset, tables16)",
    "_FusedBCEDist": f"({N}, rowptr, col, offset, tables, chunk_cols=0)",
    "_FusedBCEF32": f"({N}, rowptr, col, offset, tables, chunk_cols=0)",
}


@pytest.mark.parametrize("name", sorted(ENGINE))
def test_engine_function_keeps_its_signature(name):
    from kge_amd import engine
    assert str(inspect.signature(getattr(engine, name))) == ENGINE[name]


@pytest.mark.parametrize("name", sorted(NODES))
def test_loss_node_keeps_its_forward_signature(name):
    import torch
    from kge_amd import model
    node = getattr(model, name)
    assert issubclass(node, torch.autograd.Function)
    assert str(inspect.signature(node.forward)) == NODES[name]
