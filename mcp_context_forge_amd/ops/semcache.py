"""Plain numpy oracles (float64 / int64) of the semantic cache's top-k lookup
kernels (csrc/semcache.hip): hip.sketch_topk and hip.verify_topk.

Slot c is *eligible* for row r when c < active, valid[c] != 0,
ident[c] == q_ident[r] and stamp[c] >= min_stamp, the stamps read as unsigned
ticks of 1 / STAMP_HZ s since the cache was created. NaN scores are out of
scope, as for rows_argmax_merge.
"""

from __future__ import annotations

import math
from typing import Tuple

import numpy as np

NONE_VAL = np.float32(-1e30)   # the "no candidate" pair is (NONE_VAL, -1)
STAMP_HZ = 16                  # stamp ticks per second


def stamp_of(t: float, t0: float) -> int:
    """floor((t - t0) * STAMP_HZ), not below 0."""
    return max(0, math.floor((t - t0) * STAMP_HZ))


def _f64(a) -> np.ndarray:
    """bf16 / fp32 torch tensor or numpy array → float64 numpy."""
    return a.double().cpu().numpy() if hasattr(a, "double") else np.asarray(a, dtype=np.float64)


def _ints(a, dtype) -> np.ndarray:
    return (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)).astype(dtype)


def sketch_topk_reference(q_sk, keys_sk, ident, stamp, valid, q_ident, min_stamp: int, active: int,
                          k: int) -> Tuple[np.ndarray, np.ndarray]:
    """→ (val f32[B, k], idx i32[B, k]): each row's eligible slots in the total
    order (score descending, slot ascending), padded with (NONE_VAL, -1). The
    score is the float64 dot of the two rows."""
    q, keys = _f64(q_sk), _f64(keys_sk)
    ident, q_ident = _ints(ident, np.int64), _ints(q_ident, np.int64)
    stamp = _ints(stamp, np.int32).view(np.uint32).astype(np.int64)
    valid = _ints(valid, np.uint8)
    slots = np.arange(keys.shape[0])
    common = (slots < active) & (valid != 0) & (stamp >= int(min_stamp))
    scores = q @ keys.T
    val = np.full((q.shape[0], k), NONE_VAL, dtype=np.float32)
    idx = np.full((q.shape[0], k), -1, dtype=np.int32)
    for r in range(q.shape[0]):
        elig = slots[common & (ident == q_ident[r])]
        order = elig[np.lexsort((elig, -scores[r, elig]))][:k]
        val[r, :order.size] = scores[r, order]
        idx[r, :order.size] = order
    return val, idx


def verify_topk_reference(feats, keys, cand) -> Tuple[np.ndarray, np.ndarray]:
    """→ (best_val f32[M], best_idx i32[M]): the greatest float64 dot of
    feats[r] with keys[cand[r, j]] over cand[r, j] >= 0, the candidate listed
    first on a tie, (NONE_VAL, -1) for a row without a candidate."""
    f, kk = _f64(feats), _f64(keys)
    cand = _ints(cand, np.int64)
    best_val = np.full(f.shape[0], NONE_VAL, dtype=np.float32)
    best_idx = np.full(f.shape[0], -1, dtype=np.int32)
    for r in range(f.shape[0]):
        best = None
        for c in cand[r]:
            if c < 0:
                continue
            d = float(f[r] @ kk[c])
            if best is None or d > best:
                best, best_idx[r] = d, c
        if best is not None:
            best_val[r] = best
    return best_val, best_idx
