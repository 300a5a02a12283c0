"""Time hip.token_entropy next to hip.scan with the secrets bank.

    python loadtest/entropy_bench.py [--requests 8192] [--span 200] [--iters 50]

Builds `--requests` argument-like spans of about `--span` bytes (JSON with a
few identifiers, numbers and one token each), then times each kernel with HIP
events after warm-up and prints the median per launch, plus the pipeline's
`gp0_secrets` wall time per batch for the same requests (the pre-pass:
uploads, both kernels, sync, D2H). docs/kernels.md records the figures.
"""

from __future__ import annotations

import argparse
import asyncio
import json
import os
import random
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch


def make_spans(n: int, span: int, seed: int = 1):
    rng = random.Random(seed)
    b64 = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
    words = ["timezone", "source", "target", "convert", "message", "UTC", "Asia/Tokyo", "value"]
    out = []
    for i in range(n):
        obj = {"id": i, "time": "2026-01-01T10:00:%02dZ" % (i % 60)}
        while len(json.dumps(obj, separators=(",", ":"))) < span - 40:
            obj[rng.choice(words) + str(rng.randint(0, 9))] = " ".join(rng.choice(words) for _ in range(3))
        obj["tok"] = "".join(rng.choice(b64) for _ in range(rng.choice([16, 24, 32])))
        out.append(json.dumps(obj, separators=(",", ":")).encode())
    return out


def median_ms(fn, iters: int, warmup: int = 10) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


async def prepass_ms(spans, batches: int) -> float:
    os.environ["FORGE_PIPELINE_TIMING"] = "1"
    from mcp_context_forge_amd.config import Settings
    from mcp_context_forge_amd.engine import GatewayEngine
    from mcp_context_forge_amd.plugins.loader import default_chain_specs, load_plugin_manager
    from mcp_context_forge_amd.services.upstream import NativeInProcUpstream

    specs = default_chain_specs() + [{"name": "secrets_detection"}]
    e = GatewayEngine(Settings(database_url="sqlite://", federation_enabled=False, auth_required=False,
                               gpu_enabled=True), plugin_manager=load_plugin_manager(specs=specs))
    await e.gateway_service.register_gateway(name="native-time", url="inproc://n", client=NativeInProcUpstream())
    assert e.enable_gpu()
    raws = [b'{"jsonrpc":"2.0","id":%d,"method":"tools/call","params":{"name":"native-time-echo","arguments":%s}}'
            % (i, s) for i, s in enumerate(spans)]
    await e.process_rpc_batch(list(raws))   # warm-up
    pipe = e.gpu_pipeline
    pipe.timing.clear()
    for _ in range(batches):
        await e.process_rpc_batch(list(raws))
    ms = pipe.timing["gp0_secrets"] / batches * 1e3
    routed = pipe.stats()["secrets_routed"]
    await e.shutdown()
    return ms, routed


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=8192)
    ap.add_argument("--span", type=int, default=200)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", type=int, default=5)
    a = ap.parse_args()

    from mcp_context_forge_amd.ops import hip
    from mcp_context_forge_amd.plugins.builtin import SecretsDetectionPlugin

    spans = make_spans(a.requests, a.span)
    lens = np.asarray([len(s) for s in spans], dtype=np.int32)
    end = np.cumsum(lens).astype(np.int32)
    beg = (end - lens).astype(np.int32)
    data_t = torch.from_numpy(np.frombuffer(b"".join(spans), dtype=np.uint8).copy()).cuda()
    beg_t, end_t = torch.from_numpy(beg).cuda(), torch.from_numpy(end).cuda()
    plugin = SecretsDetectionPlugin()
    bank = hip.DeviceScanTables(plugin.scan_tables())
    sym = hip.entropy_table(hip.ENTROPY_BASE64())
    out = hip.token_entropy(data_t, beg_t, end_t, sym, plugin.min_len)

    res = {
        "requests": a.requests, "mean_span_bytes": round(float(lens.mean()), 1),
        "token_entropy_ms": round(median_ms(
            lambda: hip.token_entropy(data_t, beg_t, end_t, sym, plugin.min_len, out=out), a.iters), 4),
        "scan_secrets_bank_ms": round(median_ms(lambda: hip.scan(data_t, beg_t, end_t, bank), a.iters), 4),
        "bank_states": bank.n_states,
    }
    ms, routed = asyncio.run(prepass_ms(spans, a.batches))
    res["gp0_secrets_ms_per_batch"] = round(ms, 3)
    res["secrets_routed"] = routed
    print(json.dumps(res))


if __name__ == "__main__":
    main()
