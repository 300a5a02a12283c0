"""Time hip.sql_scan next to hip.token_entropy and hip.decode_scan on the same input.

    python loadtest/sql_bench.py [--requests 8192] [--span 200] [--share 0.1] [--iters 50]

Builds the spans of loadtest/entropy_bench.py (`--requests` argument-like
JSON objects of about `--span` bytes), puts a SQL statement into a `--share`
of them, then times each kernel with HIP events after warm-up and prints the
median per launch, plus the pipeline's `gp0_sql` wall time per batch for the
same requests (the pre-pass: uploads, one sql_scan launch in boundary mode,
sync, D2H). token_entropy and decode_scan are yardsticks, not bounds.
docs/kernels.md records the figures.
"""

from __future__ import annotations

import argparse
import asyncio
import json
import os
import random

import numpy as np
import torch

from entropy_bench import make_spans, median_ms   # same directory: sets up sys.path for the package too


def add_sql(spans, share: float, seed: int = 3):
    """Give `share` of the spans a "query" value: a SQL statement, half of them with a finding."""
    rng = random.Random(seed)
    texts = ["select id, name from users where id = 42 -- by key",
             "INSERT INTO notes (body) VALUES ('please drop by; delete nothing from here')",
             "update accounts set balance = balance - 10 where id = 7 /* debit */",
             "DELETE FROM sessions", "DROP TABLE users; --", "update accounts set balance = 0",
             "select 1; TRUNCATE audit_log", "delete from t where 1 = 1; GRANT ALL ON t TO public"]
    out = []
    for s in spans:
        if rng.random() < share:
            obj = json.loads(s)
            obj["query"] = rng.choice(texts)
            s = json.dumps(obj, separators=(",", ":")).encode()
        out.append(s)
    return out


async def prepass_ms(spans, batches: int):
    os.environ["FORGE_PIPELINE_TIMING"] = "1"
    from mcp_context_forge_amd.config import Settings
    from mcp_context_forge_amd.engine import GatewayEngine
    from mcp_context_forge_amd.plugins.loader import default_chain_specs, load_plugin_manager
    from mcp_context_forge_amd.services.upstream import NativeInProcUpstream

    specs = default_chain_specs() + [{"name": "sql_sanitizer"}]
    e = GatewayEngine(Settings(database_url="sqlite://", federation_enabled=False, auth_required=False,
                               gpu_enabled=True), plugin_manager=load_plugin_manager(specs=specs))
    await e.gateway_service.register_gateway(name="native-time", url="inproc://n", client=NativeInProcUpstream())
    assert e.enable_gpu()
    raws = [b'{"jsonrpc":"2.0","id":%d,"method":"tools/call","params":{"name":"native-time-echo","arguments":%s}}'
            % (i, s) for i, s in enumerate(spans)]
    await e.process_rpc_batch(list(raws))   # warm-up
    pipe = e.gpu_pipeline
    pipe.timing.clear()
    routed0 = pipe.stats()["sql_routed"]
    for _ in range(batches):
        await e.process_rpc_batch(list(raws))
    ms = pipe.timing["gp0_sql"] / batches * 1e3
    routed = (pipe.stats()["sql_routed"] - routed0) // batches
    await e.shutdown()
    return ms, routed


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=8192)
    ap.add_argument("--span", type=int, default=200)
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", type=int, default=5)
    a = ap.parse_args()

    from mcp_context_forge_amd.ops import hip
    from mcp_context_forge_amd.plugins.builtin import (EncodedExfilDetectionPlugin, SecretsDetectionPlugin,
                                                       SqlSanitizerPlugin)

    spans = add_sql(make_spans(a.requests, a.span), a.share)
    lens = np.asarray([len(s) for s in spans], dtype=np.int32)
    end = np.cumsum(lens).astype(np.int32)
    beg = (end - lens).astype(np.int32)
    data_t = torch.from_numpy(np.frombuffer(b"".join(spans), dtype=np.uint8).copy()).cuda()
    beg_t, end_t = torch.from_numpy(beg).cuda(), torch.from_numpy(end).cuda()
    plugin, exfil = SqlSanitizerPlugin(), EncodedExfilDetectionPlugin()
    kw = hip.DeviceScanTables(plugin.keyword_tables())
    kw_len = torch.tensor(plugin.keyword_lengths(), dtype=torch.int32, device="cuda")
    exfil_kw = hip.DeviceScanTables(exfil.keyword_tables())
    b64 = hip.entropy_table(hip.ENTROPY_BASE64())
    ent_min_len = SecretsDetectionPlugin().min_len

    def sql(boundary, out=None):
        return hip.sql_scan(data_t, beg_t, end_t, kw, kw_len, boundary, out=out)

    def decode(out=None):
        return hip.decode_scan(data_t, beg_t, end_t, b64, 6, exfil.min_len, exfil.min_printable_permille,
                               exfil_kw, out=out)

    sql_out = {bd: sql(bd) for bd in (True, False)}
    dec_out = decode()
    ent_out = hip.token_entropy(data_t, beg_t, end_t, b64, ent_min_len)
    torch.cuda.synchronize()
    counts = sql_out[True][0].cpu().numpy()
    res = {
        "requests": a.requests, "mean_span_bytes": round(float(lens.mean()), 1), "share": a.share,
        "rows_with_finding": int(((counts[:, 1] > 0) | (counts[:, 2] > 0)
                                  | (sql_out[True][1].cpu().numpy() != 0)).sum()),
        "token_entropy_ms": round(median_ms(
            lambda: hip.token_entropy(data_t, beg_t, end_t, b64, ent_min_len, out=ent_out), a.iters), 4),
        "decode_scan_base64_ms": round(median_ms(lambda: decode(dec_out), a.iters), 4),
        "sql_scan_boundary_ms": round(median_ms(lambda: sql(True, sql_out[True]), a.iters), 4),
        "sql_scan_text_ms": round(median_ms(lambda: sql(False, sql_out[False]), a.iters), 4),
    }
    ms, routed = asyncio.run(prepass_ms(spans, a.batches))
    res["gp0_sql_ms_per_batch"] = round(ms, 3)
    res["sql_routed_per_batch"] = routed
    print(json.dumps(res))


if __name__ == "__main__":
    main()
