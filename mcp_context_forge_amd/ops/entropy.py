"""Token entropy: symbol tables and the CPU reference of `ops/csrc/entropy.hip`.

A *run* is a maximal stretch of in-alphabet bytes; it *qualifies* when its
length n is at least `min_len`. For bin counts c_k its Shannon entropy is

    H = log2(n) - (sum_k c_k * log2(c_k)) / n      (bits per symbol)

`token_entropy_reference` is plain Python in float64, like
`dfa.match_mask_reference`: the oracle for the HIP kernel in tests AND the
code the secrets_detection plugin runs per request, so the CPU chain and the
oracle are one code path.

A symbol table is uint8[256]: byte → symbol 0..63, or NOT_MEMBER.
"""

from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np

NOT_MEMBER = 0xFF

# |H_f32 - H_f64| cap the GPU prefilter subtracts from a threshold before it
# compares the kernel's max_h (docs/kernels.md has the measured error).
TOL = 1e-3

_B64 = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"


def base64_table() -> np.ndarray:
    """64 symbols; URL-safe '-' and '_' share bins with '+' and '/'; '=' is
    not a member (padding ends a run)."""
    t = np.full(256, NOT_MEMBER, dtype=np.uint8)
    for i, b in enumerate(_B64):
        t[b] = i
    t[ord("-")] = t[ord("+")]
    t[ord("_")] = t[ord("/")]
    return t


def hex_table() -> np.ndarray:
    """16 symbols; upper- and lower-case digits share bins."""
    t = np.full(256, NOT_MEMBER, dtype=np.uint8)
    for i, b in enumerate(b"0123456789abcdef"):
        t[b] = i
    for i, b in enumerate(b"ABCDEF"):
        t[b] = 10 + i
    return t


TABLES = {"base64": base64_table, "hex": hex_table}


def run_entropy(counts: Sequence[int], n: int) -> float:
    """H of one run from its bin counts (float64)."""
    acc = 0.0
    for c in counts:
        if c > 1:
            acc += c * math.log2(c)
    return max(math.log2(n) - acc / n, 0.0)


def token_entropy_reference(data: bytes, sym_table, min_len: int
                            ) -> Tuple[List[Tuple[int, int, float]], float, Tuple[int, int], int, int]:
    """→ (runs, max_h, span, n_runs, flags) over the whole buffer.

    runs: every qualifying run as (beg, len, H), in order. The last four are
    what the kernel reports per request: the largest H (0.0 if none), that
    run's (beg, len) — the first one on ties, (-1, 0) if none — the number
    of qualifying runs, and bit 0 set when the buffer holds a backslash or
    any byte >= 0x80."""
    sym = sym_table.tolist() if hasattr(sym_table, "tolist") else list(sym_table)
    min_len = max(int(min_len), 1)
    runs: List[Tuple[int, int, float]] = []
    flags = 0
    counts = [0] * 64
    run_beg, run_len = 0, 0

    def close() -> None:
        nonlocal run_len, counts
        if run_len >= min_len:
            runs.append((run_beg, run_len, run_entropy(counts, run_len)))
        if run_len:
            counts = [0] * 64
        run_len = 0

    for pos, b in enumerate(data):
        if b == 0x5C or b >= 0x80:
            flags = 1
        s = sym[b]
        if s == NOT_MEMBER:
            if run_len:
                close()
            continue
        if run_len == 0:
            run_beg = pos
        counts[s] += 1
        run_len += 1
    if run_len:
        close()

    max_h, span = 0.0, (-1, 0)
    for (rb, rl, h) in runs:
        if span[0] < 0 or h > max_h:
            max_h, span = h, (rb, rl)
    return runs, max_h, span, len(runs), flags
