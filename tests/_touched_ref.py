"""kge_touched_mark and kge_adagrad_step_touched (include/kge_amd.h; kge_amd/csrc/touched.hip) restated in plain numpy
for the tests (no torch, no GPU).

  bitmap_bytes   kge_touched_bitmap_bytes: 4 * ceil(num_rows / 32), rounded up to 16
  mark           kge_touched_mark: bit r % 32 of the uint32 word r // 32 for every id r in [0, num_rows); anything else
                 sets nothing; duplicates are fine
  step_touched   kge_adagrad_step_touched: for every set bit r < num_rows, in float32, every operation rounded on its own
                 and in the order the kernel writes them (the library is built with -ffp-contract=off, IEEE division and
                 square root):
                     s = s + g * g;   p = p + (minus_clr * g) / (sqrt(s) + eps);   copy = bf16 bits of p (RNE)
                 then grad[r] = 0, and the whole bitmap zero.  Rows whose bit is clear are not looked at.
The scalars are rounded to float32 the way ctypes hands a Python float to a `float` parameter of the C ABI."""
import numpy as np

_QUIET = dict(over="ignore", under="ignore", invalid="ignore", divide="ignore")


def bitmap_bytes(num_rows: int) -> int:
    if num_rows <= 0:
        return 0
    return ((num_rows + 31) // 32 * 4 + 15) // 16 * 16


def mark(ids, num_rows: int, bitmap=None):
    """-> uint32 [bitmap_bytes(num_rows) / 4] (or `bitmap`'s length): `bitmap` (or zeros) with the ids' bits set."""
    words = np.zeros(bitmap_bytes(num_rows) // 4, dtype=np.uint32) if bitmap is None else np.array(bitmap, dtype=np.uint32)
    for r in np.asarray(ids, dtype=np.int64).reshape(-1):
        r = int(r)
        if 0 <= r < num_rows:
            words[r >> 5] |= np.uint32(1 << (r & 31))
    return words


def marked_rows(bitmap, num_rows: int):
    """The rows < num_rows whose bit is set, ascending."""
    words = np.asarray(bitmap, dtype=np.uint32)
    return [r for r in range(num_rows) if (int(words[r >> 5]) >> (r & 31)) & 1]


def bf16_rne_bits(x):
    """float32 array -> uint16 bf16 bits, round to nearest even; NaN -> a quiet NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    r = (u + (np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x0040), r).astype(np.uint16)


def step_touched(param, grad, state_sum, bitmap, minus_clr, eps, copy=None):
    """param, grad, state_sum: float32 [E, dim]; bitmap: uint32 words; copy: uint16 [E, dim] or None.
    -> (param, grad, state_sum, bitmap, copy) after the call (new arrays)."""
    p, g, s = (np.array(x, dtype=np.float32) for x in (param, grad, state_sum))
    c = None if copy is None else np.array(copy, dtype=np.uint16)
    E = p.shape[0]
    minus_clr, eps = np.float32(minus_clr), np.float32(eps)
    with np.errstate(**_QUIET):
        for r in marked_rows(bitmap, E):
            ge = g[r]
            se = s[r] + ge * ge
            pe = p[r] + (minus_clr * ge) / (np.sqrt(se) + eps)
            s[r], p[r] = se, pe
            g[r] = np.float32(0)
            if c is not None:
                c[r] = bf16_rne_bits(pe)
    return p, g, s, np.zeros_like(np.asarray(bitmap, dtype=np.uint32)), c


def dense_adagrad(param, grad, state_sum, minus_clr, eps):
    """The dense step with weight_decay == 0 over EVERY element (kge_adagrad_step_multi's arithmetic) -> (param, sum)."""
    p, g, s = (np.array(x, dtype=np.float32) for x in (param, grad, state_sum))
    minus_clr, eps = np.float32(minus_clr), np.float32(eps)
    with np.errstate(**_QUIET):
        s = s + g * g
        p = p + (minus_clr * g) / (np.sqrt(s) + eps)
    return p, s
