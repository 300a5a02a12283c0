"""Time hip.account_scan next to hip.token_entropy and hip.url_scan on the same input.

    python loadtest/account_bench.py [--requests 8192] [--span 200] [--share 0.1] [--iters 50]

Builds the spans of loadtest/entropy_bench.py (`--requests` argument-like
JSON objects of about `--span` bytes), puts a card or an IBAN into a `--share`
of them, then times each kernel with HIP events after warm-up and prints the
median per launch, plus the pipeline's `gp0_account` wall time per batch for
the same requests (the pre-pass: uploads, one account_scan launch, sync,
D2H). token_entropy and url_scan are yardsticks, not bounds. docs/kernels.md
records the figures.
"""

from __future__ import annotations

import argparse
import asyncio
import json
import random

import torch

from entropy_bench import make_spans, median_ms, pack_spans, prepass_ms   # same directory: sets up sys.path for the package too


def add_accounts(spans, share: float, seed: int = 5):
    """Give `share` of the spans an "account" value: a card or an IBAN, two in three of them valid."""
    rng = random.Random(seed)
    texts = ["card 4111 1111 1111 1111 exp 12/29", "5555-5555-5555-4444", "amex 378282246310005", "ref 4111111111111112",
             "order 1234-5678-9012-3456 of 2026-11-26", "DE89 3704 0044 0532 0130 00", "pay to GB82WEST12345698765432 today",
             "IBAN FR14 2004 1010 0505 0001 3M02 606", "DE89 3704 0044 0532 0130 01"]
    out = []
    for s in spans:
        if rng.random() < share:
            obj = json.loads(s)
            obj["account"] = rng.choice(texts)
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

    from mcp_context_forge_amd.ops import account as A
    from mcp_context_forge_amd.ops import hip
    from mcp_context_forge_amd.ops import url as U
    from mcp_context_forge_amd.plugins.builtin import SecretsDetectionPlugin

    spans = add_accounts(make_spans(a.requests, a.span), a.share)
    data_t, beg_t, end_t, lens = pack_spans(spans)
    b64 = hip.entropy_table(hip.ENTROPY_BASE64())
    ent_min_len = SecretsDetectionPlugin().min_len
    url_table = hip.DeviceUrlTable(U.compile_domains(["d%d.blocked.test" % i for i in range(256)]))
    url_mask = U.ALL_BITS & ~U.EMPTY_HOST
    table = hip.DeviceIbanTable(A.compile_iban_lengths())

    acct_out = hip.account_scan(data_t, beg_t, end_t, table, A.ALL_KINDS)
    url_out = hip.url_scan(data_t, beg_t, end_t, url_table, url_mask)
    ent_out = hip.token_entropy(data_t, beg_t, end_t, b64, ent_min_len)
    torch.cuda.synchronize()
    counts = acct_out[0].cpu().numpy()
    res = {
        "requests": a.requests, "mean_span_bytes": round(float(lens.mean()), 1), "share": a.share,
        "card_candidates": int(counts[:, 0].sum()), "valid_cards": int(counts[:, 1].sum()),
        "iban_candidates": int(counts[:, 2].sum()), "valid_ibans": int(counts[:, 3].sum()),
        "rows_with_finding": int(((counts[:, 1] + counts[:, 3]) > 0).sum()),
        "token_entropy_ms": round(median_ms(
            lambda: hip.token_entropy(data_t, beg_t, end_t, b64, ent_min_len, out=ent_out), a.iters), 4),
        "url_scan_ms": round(median_ms(
            lambda: hip.url_scan(data_t, beg_t, end_t, url_table, url_mask, out=url_out), a.iters), 4),
        "account_scan_ms": round(median_ms(
            lambda: hip.account_scan(data_t, beg_t, end_t, table, A.ALL_KINDS, out=acct_out), a.iters), 4),
    }
    ms, delta = asyncio.run(prepass_ms([{"name": "account_number_detection"}], "account", spans, a.batches))
    res["gp0_account_ms_per_batch"] = round(ms, 3)
    res["account_routed_per_batch"] = delta["account_routed"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
