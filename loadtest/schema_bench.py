"""Time hip.schema_check next to hip.token_entropy on the same input, the host loop it replaces, and the pipeline's gp_schema section.

    python loadtest/schema_bench.py [--requests 8192] [--span 200] [--share 0.1] [--iters 50] [--rows 64,128,256,450,1024,8192]

Builds the spans of loadtest/entropy_bench.py (`--requests` argument-like
JSON objects of about `--span` bytes), gives each a `mode` and a `limit` and
spreads them over a dozen tools whose schemas hold an enum, integer bounds,
string lengths, a type list and `required` — "host" schemas for the byte
patterns. A `--share` of the rows fails or punts: a limit out of bounds, an
unknown mode, a missing token, a float limit, a line break (a backslash), an
accented word. Prints the median per launch of both kernels (HIP events after
warm-up), the wall time of `json.loads` plus `validate` over the same rows —
what `_host_schema_rows` costs without the kernel, per batch size of `--rows`
— and, per batch size, the pipeline's `gp_schema` wall time with the verdict
counts. token_entropy is a yardstick, not a bound. docs/kernels.md records the
figures.
"""

from __future__ import annotations

import argparse
import asyncio
import json
import os
import random
import statistics
import time

import numpy as np
import torch

from entropy_bench import make_spans, median_ms, pack_spans   # same directory: sets up sys.path for the package too

N_TOOLS = 12
MODES = ["fast", "exact", "cached", "dry-run"]


def tool_schema(t: int) -> dict:
    return {"type": "object", "required": ["id", "time", "tok"], "properties": {
        "id": {"type": "integer", "minimum": 0}, "time": {"type": "string", "minLength": 20, "maxLength": 20},
        "tok": {"type": "string", "minLength": 16, "maxLength": 32}, "mode": {"type": "string", "enum": MODES},
        "limit": {"type": "integer", "minimum": 1, "maximum": 100 + t}, "note": {"type": ["string", "null"]}}}


def make_rows(n: int, span: int, share: float, seed: int = 7):
    """→ [(tool index, argument bytes)]; a `share` of them fails or punts, six ways in turn."""
    rng = random.Random(seed)
    rows, k = [], 0
    for i, s in enumerate(make_spans(n, span)):
        obj = json.loads(s)
        obj["mode"], obj["limit"], t = rng.choice(MODES), rng.randint(1, 100), i % N_TOOLS
        if rng.random() < share:
            how, k = k % 6, k + 1
            if how == 0:
                obj["limit"] = 500
            elif how == 1:
                obj["mode"] = "turbo"
            elif how == 2:
                del obj["tok"]
            elif how == 3:
                obj["limit"] = 2.5
            else:
                obj["note"] = "line one\nline two" if how == 4 else "café"
        rows.append((t, json.dumps(obj, separators=(",", ":"), ensure_ascii=False).encode()))
    return rows


def host_loop_ms(rows, schemas, repeat: int = 5, decode_only: bool = False) -> float:
    """Median wall ms of json.loads + validate over the rows: the host-schema loop without the kernel.
    decode_only: json.loads alone, which a row the kernel passes still pays."""
    from mcp_context_forge_amd.utils.jsonschema import validate

    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        for t, s in rows:
            args = json.loads(s)
            if not decode_only:
                validate(args or {}, schemas[t])
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


async def gp_schema_ms(rows, schemas, batches: int):
    """`batches` batches of one tools/call per row through an engine with schema_guard alone and
    gpu_schema_kernel on, after one warm-up batch → (gp_schema wall ms per batch, verdict counts per batch)."""
    os.environ["FORGE_PIPELINE_TIMING"] = "1"
    from mcp_context_forge_amd.config import Settings
    from mcp_context_forge_amd.engine import GatewayEngine
    from mcp_context_forge_amd.plugins.loader import load_plugin_manager

    async def ok(args):
        return {"content": [{"type": "text", "text": "ok"}], "isError": False}

    e = GatewayEngine(Settings(database_url="sqlite://", federation_enabled=False, auth_required=False,
                               gpu_enabled=True, gpu_schema_kernel=True),
                      plugin_manager=load_plugin_manager(specs=[{"name": "schema_guard"}]))
    for t, schema in enumerate(schemas):
        e.tool_service.register_local_tool("tool%02d" % t, ok, input_schema=schema)
    assert e.enable_gpu()
    raws = [b'{"jsonrpc":"2.0","id":%d,"method":"tools/call","params":{"name":"tool%02d","arguments":%s}}' % (i, t, s)
            for i, (t, s) in enumerate(rows)]
    await e.process_rpc_batch(list(raws))   # warm-up
    pipe = e.gpu_pipeline
    pipe.timing.clear()
    before = pipe.stats()
    for _ in range(batches):
        await e.process_rpc_batch(list(raws))
    after = pipe.stats()
    ms = pipe.timing["gp_schema"] / batches * 1e3
    await e.shutdown()
    return ms, {k: (after[k] - before[k]) // batches for k in ("schema_kernel_pass", "schema_kernel_fail", "schema_kernel_punt")}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=8192)
    ap.add_argument("--span", type=int, default=200)
    ap.add_argument("--share", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--rows", default="64,128,256,450,1024,8192")
    a = ap.parse_args()

    from mcp_context_forge_amd.ops import hip, schema
    from mcp_context_forge_amd.plugins.builtin import SecretsDetectionPlugin

    schemas = [tool_schema(t) for t in range(N_TOOLS)]
    rows = make_rows(a.requests, a.span, a.share)
    table = schema.compile_schemas(schemas)
    assert all(table.compiled)
    dev = hip.DeviceSchemaTable(table)
    data_t, beg_t, end_t, lens = pack_spans([s for _t, s in rows])
    tool_t = torch.from_numpy(np.asarray([t for t, _s in rows], dtype=np.int32)).cuda()
    b64 = hip.entropy_table(hip.ENTROPY_BASE64())
    ent_min_len = SecretsDetectionPlugin().min_len

    out = hip.schema_check(data_t, beg_t, end_t, tool_t, dev)
    ent_out = hip.token_entropy(data_t, beg_t, end_t, b64, ent_min_len)
    torch.cuda.synchronize()
    verdict = out[0].cpu().numpy()
    res = {
        "requests": a.requests, "mean_span_bytes": round(float(lens.mean()), 1), "share": a.share, "table_in_lds": table.in_lds,
        "pass": int((verdict == schema.PASS).sum()), "fail": int((verdict == schema.FAIL).sum()),
        "punt": int((verdict == schema.PUNT).sum()),
        "token_entropy_ms": round(median_ms(
            lambda: hip.token_entropy(data_t, beg_t, end_t, b64, ent_min_len, out=ent_out), a.iters), 4),
        "schema_check_ms": round(median_ms(lambda: hip.schema_check(data_t, beg_t, end_t, tool_t, dev, out=out), a.iters), 4),
    }
    for n in (int(x) for x in a.rows.split(",")):
        ms, counts = asyncio.run(gp_schema_ms(rows[:n], schemas, a.batches))
        res[f"rows_{n}"] = {"host_loop_ms": round(host_loop_ms(rows[:n], schemas), 3),
                            "decode_only_ms": round(host_loop_ms(rows[:n], schemas, decode_only=True), 3),
                            "gp_schema_ms": round(ms, 3), **counts}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
