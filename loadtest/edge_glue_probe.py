#!/usr/bin/env python
"""Edge glue probe: what one batch costs the asyncio thread OUTSIDE the
engine, per-row edge.poll/complete vs edge.poll_packed/complete_list.

Real sockets and the real NativeEdge batch handlers, but a stub engine that
answers from a prebuilt list, so the figure is poll + handler + completion
only. CPU-only; run it on the box whose number you want.

  python loadtest/edge_glue_probe.py --rows 1000 --rounds 30
"""

import argparse
import asyncio
import json
import os
import socket
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mcp_context_forge_amd.services.metrics import TokenUsageTracker  # noqa: E402
from mcp_context_forge_amd.transports.native_edge import NativeEdge  # noqa: E402


class StubEngine:
    def __init__(self, answers):
        self.settings = SimpleNamespace(max_request_body_bytes=1 << 20, auth_required=False,
                                        gpu_batch_window_us=0, gpu_batch_max_requests=1 << 16)
        self.token_usage = TokenUsageTracker()
        self.answers = answers

    async def process_rpc_batch(self, raws, users=None):
        return self.answers[:len(raws)]

    async def process_rpc_packed(self, blob, offs, uidx, users):
        return self.answers[:len(uidx) // 4]


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


async def measure(packed: bool, rows: int, rounds: int) -> float:
    answers = [json.dumps({"jsonrpc": "2.0", "id": i, "result": {"content": [
        {"type": "text", "text": "2026-01-01T00:00:00+00:00 " + "x" * 200}]}}).encode() for i in range(rows)]
    os.environ["FORGE_EDGE_PACKED"] = "1" if packed else "0"
    edge = NativeEdge(StubEngine(answers), port=free_port(), threads=4)
    mod = edge.edge
    edge.handle = mod.start(edge.port, edge.threads, 1 << 20, False)
    mod.auth_put(edge.handle, b"Bearer probe", "admin@example.com")
    socks = [socket.create_connection(("127.0.0.1", edge.port)) for _ in range(rows)]
    reqs = []
    for i in range(rows):
        body = json.dumps({"jsonrpc": "2.0", "id": i, "method": "tools/call", "params": {
            "name": "up0-17-convert_time", "arguments": {"time": "2026-01-17T11:22:33Z",
                                                         "source_timezone": "America/New_York",
                                                         "target_timezone": "Asia/Kolkata"}}}).encode()
        reqs.append(b"POST /rpc HTTP/1.1\r\nHost: x\r\nAuthorization: Bearer probe\r\n"
                    b"Content-Length: " + str(len(body)).encode() + b"\r\n\r\n" + body)
    poll = mod.poll_packed if packed else mod.poll
    handler = edge._handle_packed if packed else edge._handle_batch
    times = []
    for r in range(rounds):
        for c, q in zip(socks, reqs):
            c.sendall(q)
        while mod.stats(edge.handle)["hot"] < rows * (r + 1):
            await asyncio.sleep(0.001)
        await asyncio.sleep(0.01)   # let the last enqueue land
        t0 = time.perf_counter()
        batch = poll(edge.handle, 0, 0, 1 << 16)
        await handler(*batch)
        times.append(time.perf_counter() - t0)
        for c in socks:   # answers go out in queue order, so read by Content-Length
            buf = b""
            while b"\r\n\r\n" not in buf:
                buf += c.recv(65536)
            head, _, rest = buf.partition(b"\r\n\r\n")
            need = int(head.lower().split(b"content-length:")[1].split(b"\r\n")[0])
            while len(rest) < need:
                rest += c.recv(65536)
    for c in socks:
        c.close()
    mod.stop(edge.handle)
    return statistics.median(times[2:]) * 1000.0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=30)
    args = ap.parse_args()
    per_row = asyncio.run(measure(False, args.rows, args.rounds))
    packed = asyncio.run(measure(True, args.rows, args.rounds))
    print(json.dumps({"rows": args.rows, "rounds": args.rounds,
                      "per_row_ms_per_batch": round(per_row, 3),
                      "packed_ms_per_batch": round(packed, 3),
                      "per_row_us_per_row": round(per_row * 1000 / args.rows, 3),
                      "packed_us_per_row": round(packed * 1000 / args.rows, 3)}))


if __name__ == "__main__":
    main()
