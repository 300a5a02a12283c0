"""Time hip.url_scan next to hip.token_entropy and hip.sql_scan on the same input.

    python loadtest/url_bench.py [--requests 8192] [--span 200] [--share 0.1] [--iters 50]

Builds the spans of loadtest/entropy_bench.py (`--requests` argument-like
JSON objects of about `--span` bytes), puts a URL into a `--share` of them,
then times each kernel with HIP events after warm-up and prints the median
per launch for two domain tables, one on each side of
hip.URL_SCAN_LDS_SLOTS (256 domains probed in LDS, 4096 in global memory),
plus the pipeline's `gp0_url` wall time per batch for the same requests (the
pre-pass: uploads, one url_scan launch, sync, D2H). token_entropy and
sql_scan are yardsticks, not bounds. docs/kernels.md records the figures.
"""

from __future__ import annotations

import argparse
import asyncio
import json
import random

import torch

from entropy_bench import make_spans, median_ms, pack_spans, prepass_ms   # same directory: sets up sys.path for the package too

TABLE_SIZES = {"lds": 256, "global": 4096}


def domains(n: int):
    return ["d%d.blocked.test" % i for i in range(n)]


def add_urls(spans, share: float, seed: int = 3):
    """Give `share` of the spans a "link" value: a URL, half of them with a finding."""
    rng = random.Random(seed)
    texts = ["https://docs.example.org/guide/install?lang=en#step-2", "https://api.partner.example.net:8443/v2/items/17",
             "see https://status.example.org and https://www.example.org/a/b", "https://cdn.d3.allowed.test/asset.js",
             "http://intranet.example.org/wiki", "https://files.d7.blocked.test/payload.bin",
             "https://login.example.org@198.51.100.7/reset", "https://t.example.org/r?u=http://x.d200.blocked.test/"]
    out = []
    for s in spans:
        if rng.random() < share:
            obj = json.loads(s)
            obj["link"] = rng.choice(texts)
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
    from mcp_context_forge_amd.ops import url as U
    from mcp_context_forge_amd.plugins.builtin import SecretsDetectionPlugin, SqlSanitizerPlugin

    spans = add_urls(make_spans(a.requests, a.span), a.share)
    data_t, beg_t, end_t, lens = pack_spans(spans)
    sqlp = SqlSanitizerPlugin()
    kw = hip.DeviceScanTables(sqlp.keyword_tables())
    kw_len = torch.tensor(sqlp.keyword_lengths(), dtype=torch.int32, device="cuda")
    b64 = hip.entropy_table(hip.ENTROPY_BASE64())
    ent_min_len = SecretsDetectionPlugin().min_len
    mask = U.ALL_BITS & ~U.EMPTY_HOST
    tables = {k: hip.DeviceUrlTable(U.compile_domains(domains(n), ["d3.allowed.test"])) for k, n in TABLE_SIZES.items()}
    assert tables["lds"].in_lds and not tables["global"].in_lds

    url_out = {k: hip.url_scan(data_t, beg_t, end_t, t, mask) for k, t in tables.items()}
    sql_out = hip.sql_scan(data_t, beg_t, end_t, kw, kw_len, True)
    ent_out = hip.token_entropy(data_t, beg_t, end_t, b64, ent_min_len)
    torch.cuda.synchronize()
    counts = url_out["global"][0].cpu().numpy()
    res = {
        "requests": a.requests, "mean_span_bytes": round(float(lens.mean()), 1), "share": a.share,
        "urls": int(counts[:, 0].sum()), "rows_with_finding": int((counts[:, 3] > 0).sum()),
        "token_entropy_ms": round(median_ms(
            lambda: hip.token_entropy(data_t, beg_t, end_t, b64, ent_min_len, out=ent_out), a.iters), 4),
        "sql_scan_boundary_ms": round(median_ms(
            lambda: hip.sql_scan(data_t, beg_t, end_t, kw, kw_len, True, out=sql_out), a.iters), 4),
    }
    for k, t in tables.items():
        res[f"url_scan_{k}_slots"] = t.n_slots
        res[f"url_scan_{k}_ms"] = round(median_ms(
            lambda: hip.url_scan(data_t, beg_t, end_t, t, mask, out=url_out[k]), a.iters), 4)
    for k, n in TABLE_SIZES.items():
        spec = {"name": "url_reputation", "config": {"blocked_domains": domains(n), "whitelist_domains": ["d3.allowed.test"]}}
        ms, delta = asyncio.run(prepass_ms([spec], "url", spans, a.batches))
        res[f"gp0_url_{k}_ms_per_batch"] = round(ms, 3)
        res[f"url_routed_{k}_per_batch"] = delta["url_routed"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
