"""Time hip.json_unescape next to hip.token_entropy on the same input, and the pre-pass with gpu_unescape off and on.

    python loadtest/unescape_bench.py [--requests 8192] [--span 200] [--share 0.1] [--iters 50]

Builds the spans of loadtest/entropy_bench.py (`--requests` argument-like
JSON objects of about `--span` bytes), gives a `--share` of them a value that
needs JSON escapes, serialised with ensure_ascii as most clients do — a
multi-line query, a prompt with line breaks and tabs, accented text, an emoji;
one in eight a Windows path or a quoted word, whose decoded backslash or quote
has to route, one in eight a hidden bidi override — then times each kernel with
HIP events after warm-up and prints the median per launch, plus the pipeline's
`gp0_sql` wall time per batch with sql_sanitizer and unicode_guard on, for
gpu_unescape off and on, and the rows each plugin routed. token_entropy is a
yardstick, not a bound. docs/kernels.md records the figures.
"""

from __future__ import annotations

import argparse
import asyncio
import json
import random

import torch

from entropy_bench import make_spans, median_ms, pack_spans, prepass_ms   # same directory: sets up sys.path for the package too

STAY = ["SELECT id, name\nFROM users\nWHERE id = 7\n\tAND active = 1", "Summarise this:\n\n- first point\n- second point\n",
        "col_a\tcol_b\tcol_c\r\n1\t2\t3\r\n", "line one\nline two\nline three", "UPDATE t\nSET a = 1\nWHERE id = 2",
        "step 1:\tfetch\nstep 2:\tparse"]
NON_ASCII = ["café crème\nbrûlée", "ship it \U0001F600\n"]
ROUTE = ["C:\\Users\\dev\\notes.txt", 'say "hello"\n']
FINDING = ["invoice\u202efdp.exe\n"]


def add_escapes(spans, share: float, seed: int = 5):
    """Give `share` of the spans a "note" value that needs escapes: six in eight stay on the lane under
    unicode_guard (two of them non-ASCII once decoded), one routes by its decoded bytes, one holds a finding."""
    rng = random.Random(seed)
    out, k = [], 0
    for s in spans:
        if rng.random() < share:
            obj = json.loads(s)
            obj["note"] = rng.choice((STAY, STAY, STAY, STAY, NON_ASCII, NON_ASCII, ROUTE, FINDING)[k & 7])
            k += 1
            s = json.dumps(obj, separators=(",", ":")).encode()
        out.append(s)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=8192)
    ap.add_argument("--span", type=int, default=200)
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", type=int, default=5)
    a = ap.parse_args()

    from mcp_context_forge_amd.ops import hip
    from mcp_context_forge_amd.ops import unescape as X
    from mcp_context_forge_amd.plugins.builtin import SecretsDetectionPlugin

    spans = add_escapes(make_spans(a.requests, a.span), a.share)
    data_t, beg_t, end_t, lens = pack_spans(spans)
    b64 = hip.entropy_table(hip.ENTROPY_BASE64())
    ent_min_len = SecretsDetectionPlugin().min_len

    une_out = hip.json_unescape(data_t, beg_t, end_t)
    ent_out = hip.token_entropy(data_t, beg_t, end_t, b64, ent_min_len)
    torch.cuda.synchronize()
    flags = une_out[2].cpu().numpy()
    res = {
        "requests": a.requests, "mean_span_bytes": round(float(lens.mean()), 1), "share": a.share,
        "rows_with_escape": int(((flags & X.HAD_ESCAPE) != 0).sum()),
        "rows_route_mask": int(((flags & X.ROUTE_MASK) != 0).sum()),
        "rows_decoded_non_ascii": int(((flags & X.NON_ASCII) != 0).sum()),
        "bytes_in": int(lens.sum()), "bytes_out": int((une_out[1] - beg_t).sum()),
        "token_entropy_ms": round(median_ms(
            lambda: hip.token_entropy(data_t, beg_t, end_t, b64, ent_min_len, out=ent_out), a.iters), 4),
        "json_unescape_ms": round(median_ms(lambda: hip.json_unescape(data_t, beg_t, end_t, out=une_out), a.iters), 4),
    }
    for name, on in (("off", False), ("on", True)):
        ms, delta = asyncio.run(prepass_ms([{"name": "sql_sanitizer"}, {"name": "unicode_guard"}], "sql", spans, a.batches,
                                           gpu_unescape=on))
        res[f"gp0_sql_ms_per_batch_{name}"] = round(ms, 3)
        res[f"per_batch_{name}"] = {k: delta[k] for k in ("sql_routed", "unicode_routed", "unescape_rows")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
