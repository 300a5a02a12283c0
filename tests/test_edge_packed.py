"""Packed hot lane of the native edge: edge.poll_packed / edge.complete_list
(ops/csrc/edge.cpp + edge_pack.hpp) against the per-row edge.poll /
edge.complete, first on the extension module alone (raw sockets, no engine),
then through NativeEdge end to end (packed vs FORGE_EDGE_PACKED=0), then
GatewayEngine.process_rpc_packed vs process_rpc_batch on the GPU pipeline."""

import asyncio
import base64
import importlib.util
import json
import random
import socket
import struct
import time
from pathlib import Path

import pytest

from mcp_context_forge_amd.config import Settings
from mcp_context_forge_amd.engine import GatewayEngine
from mcp_context_forge_amd.transports.native_edge import get_edge_module

BASIC = "Basic " + base64.b64encode(b"admin:changeme").decode()
USERS = {b"Bearer tok-alice": "alice@example.com", b"Bearer tok-bob": "bob@example.com",
         b"Bearer tok-carol": "carol@example.com"}
A, B, C = sorted(USERS)


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---------------------------------------------------------------------------
# edge module directly: raw sockets, no engine
# ---------------------------------------------------------------------------


class RawEdge:
    """The extension module with auth not required (so header-less requests
    reach the queue) and three credentials pre-resolved in the C++ memo."""

    def __init__(self):
        self.mod = get_edge_module()
        self.port = free_port()
        # ONE epoll thread: requests are then handled strictly one after
        # another, which is what lets barrier() below order things
        self.h = self.mod.start(self.port, 1, 256 * 1024, False)
        for authz, user in USERS.items():
            self.mod.auth_put(self.h, authz, user)
        self.socks = []

    def queued(self) -> int:
        st = self.mod.stats(self.h)
        return st["hot"] + st["cold"]

    def send(self, body: bytes, authz=None, method="POST", target="/rpc") -> socket.socket:
        """One request on its own connection; returns once the edge has
        queued it, so requests sent one after another queue in that order."""
        before = self.queued()
        c = socket.create_connection(("127.0.0.1", self.port), timeout=5.0)
        head = f"{method} {target} HTTP/1.1\r\nHost: x\r\nContent-Length: {len(body)}\r\n"
        if authz is not None:
            head += f"Authorization: {authz.decode()}\r\n"
        c.sendall(head.encode() + b"\r\n" + body)
        deadline = time.monotonic() + 5.0
        while self.queued() == before:
            assert time.monotonic() < deadline, "request never reached the queue"
            time.sleep(0.001)
        self.barrier()
        self.socks.append(c)
        return c

    def barrier(self):
        """The counter above moves just before the request is pushed onto
        the queue. A health check answered by the same (only) epoll thread
        afterwards proves the push has happened."""
        with socket.create_connection(("127.0.0.1", self.port), timeout=5.0) as c:
            c.sendall(b"GET /healthz HTTP/1.1\r\nHost: x\r\n\r\n")
            assert b"200 OK" in read_response(c)

    def close(self):
        for c in self.socks:
            c.close()
        self.mod.stop(self.h)


@pytest.fixture()
def raw_edge():
    e = RawEdge()
    yield e
    e.close()


def read_response(c: socket.socket) -> bytes:
    """Exactly one HTTP response, raw."""
    data = b""
    while b"\r\n\r\n" not in data:
        part = c.recv(65536)
        assert part, "connection closed before a response"
        data += part
    head, _, rest = data.partition(b"\r\n\r\n")
    n = [int(ln.split(b":")[1]) for ln in head.split(b"\r\n") if ln.lower().startswith(b"content-length")][0]
    while len(rest) < n:
        part = c.recv(65536)
        assert part
        rest += part
    assert len(rest) == n
    return head + b"\r\n\r\n" + rest


def rows_of_poll(res):
    """poll's result as rows (id, kind, body, user, authz, meta)."""
    ids, kinds, bodies, users, authzs, meta = res
    assert len(ids) == 8 * len(bodies) and len(kinds) == len(bodies)
    idv = struct.unpack(f"<{len(bodies)}Q", ids)
    return [(idv[i], kinds[i], bodies[i], users[i], authzs[i], meta[i]) for i in range(len(bodies))]


def hot_rows_of_packed(res):
    """poll_packed's hot lane as rows (id, body, user), checking its layout."""
    ids, blob, offs, uidx, users, ucount, _slow = res
    h = len(ids) // 8
    assert len(ids) == 8 * h and len(offs) == 8 * (h + 1) and len(uidx) == 4 * h
    idv = struct.unpack(f"<{h}Q", ids)
    o = struct.unpack(f"<{h + 1}q", offs)
    ui = struct.unpack(f"<{h}i", uidx)
    assert o[0] == 0 and o[-1] == len(blob)
    assert all(o[i] <= o[i + 1] for i in range(h))
    assert len(users) == len(ucount) and len(set(users)) == len(users)   # distinct
    assert sum(ucount) == h
    for k, cnt in enumerate(ucount):
        assert cnt == sum(1 for x in ui if x == k) and cnt > 0
    return [(idv[i], blob[o[i]:o[i + 1]], users[ui[i]]) for i in range(h)]


def is_hot(row) -> bool:
    _id, kind, _body, user, authz, _meta = row
    return kind == 0 and (user is not None or authz is None)


def body(i: int) -> bytes:
    return json.dumps({"jsonrpc": "2.0", "id": i, "method": "ping", "pad": "p" * (i * 7 % 50)}).encode()


# (body, authz, method, target) sequences
SEQUENCES = {
    "one_row": [(body(1), A, "POST", "/rpc")],
    "zero_length_body": [(body(1), A, "POST", "/rpc"), (b"", A, "POST", "/rpc"), (body(3), B, "POST", "/rpc")],
    "three_users_interleaved": [(body(i), (A, B, C)[i % 3], "POST", "/rpc") for i in range(9)]
                               + [(body(9), A, "POST", "/rpc"), (body(10), A, "POST", "/rpc")],
    "anonymous_and_users": [(body(0), None, "POST", "/rpc"), (body(1), A, "POST", "/rpc"),
                            (body(2), None, "POST", "/rpc")],
    "mixed_lanes": [(body(0), A, "POST", "/rpc"), (body(1), b"Bearer unknown-1", "POST", "/rpc"),
                    (b"", A, "GET", "/version"), (body(3), B, "POST", "/rpc"),
                    (body(4), b"Bearer unknown-2", "POST", "/rpc"), (body(5), A, "POST", "/tools"),
                    (body(6), A, "POST", "/rpc")],
    "all_slow": [(body(0), b"Bearer unknown-1", "POST", "/rpc"), (b"", None, "GET", "/version"),
                 (body(2), b"Bearer unknown-2", "POST", "/rpc")],
}


def test_poll_packed_empty_queue(raw_edge):
    res = raw_edge.mod.poll_packed(raw_edge.h, 1000, 0, 16)
    ids, blob, offs, uidx, users, ucount, slow = res
    assert (ids, blob, uidx, users, ucount) == (b"", b"", b"", [], [])
    assert offs == struct.pack("<q", 0)
    assert slow == (b"", b"", [], [], [], [])
    assert rows_of_poll(raw_edge.mod.poll(raw_edge.h, 1000, 0, 16)) == []


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_poll_packed_agrees_with_poll(raw_edge, name):
    seq = SEQUENCES[name]
    e = raw_edge
    for b, authz, method, target in seq:
        e.send(b, authz, method, target)
    ref = rows_of_poll(e.mod.poll(e.h, 1000, 0, 64))
    assert [r[2] for r in ref] == [s[0] for s in seq]          # queue order = send order
    for b, authz, method, target in seq:
        e.send(b, authz, method, target)
    res = e.mod.poll_packed(e.h, 1000, 0, 64)
    hot = hot_rows_of_packed(res)
    slow = rows_of_poll(res[6])

    ref_hot = [r for r in ref if is_hot(r)]
    ref_slow = [r for r in ref if not is_hot(r)]
    # same rows in the same order per lane (ids name fresh connections, so
    # they are compared through the completion round trip below)
    assert [(r[1], r[2]) for r in hot] == [(r[2], r[3]) for r in ref_hot]
    assert [r[1:] for r in slow] == [r[1:] for r in ref_slow]
    assert not any(is_hot(r) for r in slow)
    if name == "all_slow":
        assert hot == [] and len(slow) == len(seq)
    if name == "three_users_interleaved":
        assert dict(zip(res[4], res[5])) == {USERS[A]: 5, USERS[B]: 3, USERS[C]: 3}
    if name == "mixed_lanes":
        assert [r[2] for r in slow] == [body(1), b"", body(4), body(5)]
        assert [r[1] for r in slow] == [0, 1, 0, 1]
        assert slow[1][5][:2] == ("GET", "/version")

    # ids: answering id k with its own request body must reach the
    # connection that sent that request
    st0 = e.mod.stats(e.h)
    assert st0["hot_rows"] == 2 * len(ref_hot) and st0["slow_rows"] == 2 * len(ref_slow)
    socks = e.socks[len(seq):]
    hot_ids = res[0]
    done = e.mod.complete_list(e.h, hot_ids, [r[1] for r in hot])
    assert done == len(hot)
    if slow:
        done = e.mod.complete(e.h, res[6][0], struct.pack(f"<{len(slow)}H", *[200] * len(slow)),
                              [r[2] for r in slow])
        assert done == len(slow)
    for c, (b, _authz, _method, _target) in zip(socks, seq):
        assert read_response(c).partition(b"\r\n\r\n")[2] == b


def test_poll_packed_max_n_keeps_the_rest_queued_in_order(raw_edge):
    e = raw_edge
    for i in range(7):
        e.send(body(i), (A, B)[i % 2])
    got = []
    for want in (3, 3, 1, 0):
        res = e.mod.poll_packed(e.h, 1000, 0, 3)
        hot = hot_rows_of_packed(res)
        assert len(hot) == want and rows_of_poll(res[6]) == []
        got += hot
    assert [r[1] for r in got] == [body(i) for i in range(7)]
    assert [r[2] for r in got] == [USERS[(A, B)[i % 2]] for i in range(7)]


def test_complete_list_matches_complete_on_the_wire(raw_edge):
    e = raw_edge
    answers = [b'{"jsonrpc":"2.0","id":1,"result":{}}', None, b"", b"x" * 70000, b'{"a":"\xc3\xa9"}']

    def round_trip(packed: bool):
        socks = [e.send(body(i), A) for i in range(len(answers))]
        if packed:
            res = e.mod.poll_packed(e.h, 1000, 0, 64)
            assert e.mod.complete_list(e.h, res[0], list(answers)) == len(answers)
        else:
            res = e.mod.poll(e.h, 1000, 0, 64)
            sts = struct.pack(f"<{len(answers)}H", *[202 if a is None else 200 for a in answers])
            assert e.mod.complete(e.h, res[0], sts, [a or b"" for a in answers]) == len(answers)
        return [read_response(c) for c in socks]

    wire_list = round_trip(True)
    wire_rows = round_trip(False)
    assert wire_list == wire_rows
    assert wire_list[1].startswith(b"HTTP/1.1 202 Accepted\r\n") and wire_list[1].endswith(b"\r\n\r\n")
    assert wire_list[0].startswith(b"HTTP/1.1 200 OK\r\n")
    with pytest.raises(TypeError):
        e.mod.complete_list(e.h, struct.pack("<Q", 1), ["not bytes"])
    with pytest.raises(ValueError):
        e.mod.complete_list(e.h, struct.pack("<Q", 1), [])


def test_complete_list_skips_a_connection_closed_after_poll(raw_edge):
    e = raw_edge
    socks = [e.send(body(i), A) for i in range(4)]
    res = e.mod.poll_packed(e.h, 1000, 0, 64)
    assert len(res[0]) == 32
    closed0 = e.mod.stats(e.h)["closed"]
    # the edge holds a connection's slot while a request of it is in flight,
    # so the slot only closes once that request is answered: answer row 2 on
    # its own, let the client hang up, and its id in the batch is now stale
    assert e.mod.complete(e.h, res[0][16:24], struct.pack("<H", 200), [b"early"]) == 1
    assert read_response(socks[2]).endswith(b"early")
    responses0 = e.mod.stats(e.h)["responses"]
    socks[2].close()
    deadline = time.monotonic() + 5.0
    while e.mod.stats(e.h)["closed"] == closed0:
        assert time.monotonic() < deadline, "edge never saw the reset"
        time.sleep(0.001)
    answers = [body(10 + i) for i in range(4)]
    assert e.mod.complete_list(e.h, res[0], answers) == 3
    assert e.mod.stats(e.h)["responses"] == responses0 + 3
    for i in (0, 1, 3):
        assert read_response(socks[i]).partition(b"\r\n\r\n")[2] == answers[i]
    e.socks.remove(socks[2])
    st = e.mod.stats(e.h)
    assert st["complete_us"] >= 0 and st["poll_pack_us"] >= 0


# ---------------------------------------------------------------------------
# NativeEdge end to end: packed vs FORGE_EDGE_PACKED=0
# ---------------------------------------------------------------------------


def _bench_make_request():
    spec = importlib.util.spec_from_file_location("_forge_bench", Path(__file__).resolve().parents[1] / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.make_request


def _corpus():
    make_request = _bench_make_request()
    rng = random.Random(20260101)
    names = ["up0-0-convert_time", "up0-0-get_system_time", "up0-0-echo"]
    reqs = [make_request(rng, names, i, 0.2) for i in range(200)]
    reqs.append(json.dumps({"jsonrpc": "2.0", "id": 900, "method": "tools/call",
                            "params": {"name": "no-such-tool", "arguments": {}}}).encode())
    reqs.append(b"{broken json")
    reqs.append(json.dumps({"jsonrpc": "2.0", "method": "notifications/initialized"}).encode())
    reqs.append(json.dumps({"jsonrpc": "2.0", "id": 901, "method": "ping"}).encode())
    return reqs


async def _serve_corpus(reqs):
    """Fresh engine + native edge; send the corpus (plus a bad-token and a
    scoped-token request) concurrently; returns [(status, body)] per request
    and the edge's stats."""
    from mcp_context_forge_amd.transports.http_app import build_app

    port = free_port()
    s = Settings(database_url="sqlite://", federation_enabled=False, auth_required=True,
                 plugins_enabled=True, gpu_enabled=False, native_edge_port=port,
                 native_edge_threads=2, max_request_body_bytes=64 * 1024)
    engine = GatewayEngine(s)

    async def echo(args):
        return args

    for name in ("up0-0-convert_time", "up0-0-get_system_time", "up0-0-echo"):
        engine.tool_service.register_local_tool(name, echo, "Echo tool")
    app = build_app(engine)
    async with app.router.lifespan_context(app):
        auth = app.state.auth
        plain = "Bearer " + auth.create_api_token("admin@example.com", "plain")
        scoped = "Bearer " + auth.create_api_token("admin@example.com", "scoped", server_id="srv-1")
        plan = [(r, (BASIC, plain)[i % 2]) for i, r in enumerate(reqs)]
        plan.append((reqs[0], "Bearer mcpg_not-a-token"))
        plan.append((reqs[1], scoped))
        plan.append((reqs[-1], scoped))
        out = [None] * len(plan)
        lanes = 24   # keep-alive connections, each sending its share in order

        async def client(k: int):
            reader, writer = await asyncio.open_connection("127.0.0.1", port)
            for i in range(k, len(plan), lanes):
                raw, authz = plan[i]
                writer.write((f"POST /rpc HTTP/1.1\r\nHost: x\r\nAuthorization: {authz}\r\n"
                              f"Content-Type: application/json\r\nContent-Length: {len(raw)}\r\n\r\n"
                              ).encode() + raw)
                await writer.drain()
                head = await reader.readuntil(b"\r\n\r\n")
                n = [int(ln.split(b":")[1]) for ln in head.split(b"\r\n")
                     if ln.lower().startswith(b"content-length")][0]
                out[i] = (int(head.split(b" ", 2)[1]), await reader.readexactly(n))
            writer.close()

        await asyncio.wait_for(asyncio.gather(*(client(k) for k in range(lanes))), timeout=60.0)
        stats = app.state.native_edge.stats()
        usage = dict(engine.token_usage._counts)
    return out, stats, usage


def test_native_edge_packed_matches_per_row(run, monkeypatch):
    reqs = _corpus()
    monkeypatch.setenv("FORGE_EDGE_PACKED", "0")
    ref, ref_stats, ref_usage = run(_serve_corpus(reqs))
    monkeypatch.delenv("FORGE_EDGE_PACKED")
    got, got_stats, got_usage = run(_serve_corpus(reqs))

    assert ref_stats["packed"] is False and got_stats["packed"] is True
    assert len(got) == len(ref) == len(reqs) + 3
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g == r, (i, g, r)
    statuses = [g[0] for g in got]
    assert statuses[202] == 202 and got[202][1] == b""       # id-less notification
    assert statuses[-3] == 401                                # bad token
    assert statuses[-2] == 200 and statuses[-1] == 200        # scoped token
    assert statuses.count(200) == len(got) - 2
    assert json.loads(got[200][1])["error"]                   # unknown tool
    assert json.loads(got[201][1])["error"]                   # invalid JSON
    # the packed run really took the packed lane, and accounted the same usage
    assert got_stats["hot_rows"] > len(reqs) // 2
    assert got_stats["hot_rows"] + got_stats["slow_rows"] == got_stats["requests"]
    assert got_stats["glue_ms"] > 0 and ref_stats["glue_ms"] > 0
    assert got_usage == ref_usage and sum(got_usage.values()) == len(reqs)


# ---------------------------------------------------------------------------
# GPU: process_rpc_packed == process_rpc_batch
# ---------------------------------------------------------------------------


def _mixed_rows(n: int):
    make_request = _bench_make_request()
    rng = random.Random(7 + n)
    names = ["nt-convert_time", "nt-get_system_time", "nt-echo"]
    raws, users = [], []
    for i in range(n):
        if i % 13 == 5:
            raws.append(json.dumps({"jsonrpc": "2.0", "id": i, "method": "ping"}).encode())
        elif i % 29 == 7:
            raws.append(json.dumps({"jsonrpc": "2.0", "id": i, "method": "tools/list"}).encode())
        elif i % 31 == 11:
            raws.append(b"{broken")
        elif i % 37 == 3:
            raws.append(json.dumps({"jsonrpc": "2.0", "method": "notifications/initialized"}).encode())
        else:
            # convert_time/echo only: get_system_time answers with the wall clock
            raws.append(make_request(rng, names[::2], i, 0.3, unknown_frac=0.05, nonascii_frac=0.05))
        users.append(("alice@example.com", "bob@example.com")[(i // 3) % 2])
    return raws, users


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 300])
def test_process_rpc_packed_matches_batch_on_gpu(run, n):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    from mcp_context_forge_amd.services.upstream import NativeInProcUpstream

    raws, users = _mixed_rows(n)
    distinct = ["alice@example.com", "bob@example.com"]
    offs = [0]
    for r in raws:
        offs.append(offs[-1] + len(r))
    blob = b"".join(raws)
    offs_b = struct.pack(f"<{n + 1}q", *offs)
    uidx_b = struct.pack(f"<{n}i", *[distinct.index(u) for u in users])

    async def go():
        s = Settings(database_url="sqlite://", federation_enabled=False, auth_required=False,
                     plugins_enabled=True, gpu_enabled=True)
        e = GatewayEngine(s)
        await e.gateway_service.register_gateway(name="nt", url="inproc://nt",
                                                 client=NativeInProcUpstream(), owner_rank=0)
        assert e.enable_gpu() and e.gpu_pipeline is not None
        ref = await e.process_rpc_batch(list(raws), users=list(users))
        got = await e.process_rpc_packed(blob, offs_b, uidx_b, distinct)
        st = e.gpu_pipeline.stats()
        await e.shutdown()
        return ref, got, st

    ref, got, st = run(go())
    assert len(got) == len(ref) == n
    for i, (g, r) in enumerate(zip(got, ref)):
        assert (g is None) == (r is None), (i, g, r)
        assert g is None or bytes(g) == bytes(r), (i, g, r)
    assert st["py_fallback"] >= 2 * (n // 13)      # non-tools/call rows rode both entries
    assert sum(1 for g in got if g is not None) > n // 2
