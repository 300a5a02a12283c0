"""Time hip.unicode_scan next to hip.token_entropy and hip.account_scan on the same input.

    python loadtest/unicode_bench.py [--requests 8192] [--span 200] [--share 0.1] [--iters 50]

Builds the spans of loadtest/entropy_bench.py (`--requests` argument-like
JSON objects of about `--span` bytes), puts non-ASCII text into a `--share` of
them as raw UTF-8 — half of it benign (accented Latin, a Cyrillic sentence,
CJK), half with a finding — then times each kernel with HIP events after
warm-up and prints the median per launch, plus the pipeline's `gp0_unicode`
wall time per batch for the same requests (the pre-pass: uploads, one
unicode_scan launch, sync, D2H). token_entropy and account_scan are
yardsticks, not bounds. docs/kernels.md records the figures.
"""

from __future__ import annotations

import argparse
import asyncio
import json
import random

import torch

from entropy_bench import make_spans, median_ms, pack_spans, prepass_ms   # same directory: sets up sys.path for the package too

BENIGN = ["café crème brûlée à la carte", "привет мир, как дела сегодня",
          "東京都渋谷区 会議室", "Ελληνικά και λατινικά"]
FINDINGS = ["run\U000E0072\U000E006D -rf", "invoice\u202efdp.exe", "zero\u200bwidth", "log in at p\u0430ypal.com",
            "private \ue000 use", "\u0391pple \u0399D"]


def add_unicode(spans, share: float, seed: int = 5):
    """Give `share` of the spans a "note" value of raw UTF-8: benign and finding texts in turn."""
    rng = random.Random(seed)
    out, k = [], 0
    for s in spans:
        if rng.random() < share:
            obj = json.loads(s)
            obj["note"] = rng.choice(FINDINGS if k & 1 else BENIGN)
            k += 1
            s = json.dumps(obj, separators=(",", ":"), ensure_ascii=False).encode()
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

    from mcp_context_forge_amd.ops import account as A
    from mcp_context_forge_amd.ops import hip
    from mcp_context_forge_amd.ops import unicode as U
    from mcp_context_forge_amd.plugins.builtin import SecretsDetectionPlugin, UnicodeGuardPlugin

    spans = add_unicode(make_spans(a.requests, a.span), a.share)
    data_t, beg_t, end_t, lens = pack_spans(spans)
    b64 = hip.entropy_table(hip.ENTROPY_BASE64())
    ent_min_len = SecretsDetectionPlugin().min_len
    iban_table = hip.DeviceIbanTable(A.compile_iban_lengths())
    table = hip.DeviceUnicodeTable(U.compile_classes())
    mask = UnicodeGuardPlugin().report_mask()

    uni_out = hip.unicode_scan(data_t, beg_t, end_t, table, mask)
    acct_out = hip.account_scan(data_t, beg_t, end_t, iban_table, A.ALL_KINDS)
    ent_out = hip.token_entropy(data_t, beg_t, end_t, b64, ent_min_len)
    torch.cuda.synchronize()
    counts, flags = uni_out[0].cpu().numpy(), uni_out[3].cpu().numpy()
    reported = [k for k in range(U.N_KINDS) if mask >> k & 1]
    res = {
        "requests": a.requests, "mean_span_bytes": round(float(lens.mean()), 1), "share": a.share,
        "rows_non_ascii": int(((flags & 2) != 0).sum()),
        "rows_with_finding": int((counts[:, reported].sum(axis=1) > 0).sum()),
        "counts_by_kind": {U.KIND_NAMES[1 << k]: int(counts[:, k].sum()) for k in range(U.N_KINDS)},
        "token_entropy_ms": round(median_ms(
            lambda: hip.token_entropy(data_t, beg_t, end_t, b64, ent_min_len, out=ent_out), a.iters), 4),
        "account_scan_ms": round(median_ms(
            lambda: hip.account_scan(data_t, beg_t, end_t, iban_table, A.ALL_KINDS, out=acct_out), a.iters), 4),
        "unicode_scan_ms": round(median_ms(
            lambda: hip.unicode_scan(data_t, beg_t, end_t, table, mask, out=uni_out), a.iters), 4),
    }
    ms, delta = asyncio.run(prepass_ms([{"name": "unicode_guard"}], "unicode", spans, a.batches))
    res["gp0_unicode_ms_per_batch"] = round(ms, 3)
    res["unicode_routed_per_batch"] = delta["unicode_routed"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
