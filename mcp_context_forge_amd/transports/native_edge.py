"""NativeEdge — Python side of the C++ epoll HTTP edge (ops/csrc/edge.cpp).

Reference analog: the Rust mcp_runtime sidecar's role split (README.md:15-16
"Python stays authoritative for auth/RBAC"): the C++ threads own sockets,
HTTP parsing, response framing and the hot auth memo; THIS loop is the
Python authority — it authenticates cache misses, runs the engine's batched
GPU pipeline over each drained batch, and serves control-plane (non-/rpc)
requests through the regular ASGI app.

One asyncio task pulls batches with edge.poll_packed (GIL released while
waiting), processes them, and completes them back to C++. The hot lane of a
batch (requests the C++ auth memo already resolved) crosses into Python as a
handful of flat buffers and leaves through edge.complete_list, so this loop
does no per-request work for it; only the slow lane (auth misses, scoped
tokens, control-plane requests) is walked row by row. FORGE_EDGE_PACKED=0
selects the per-row edge.poll / edge.complete path instead. While Python is
busy with batch N the C++ side accumulates batch N+1 — the micro-batch
window emerges from load instead of a timer, same serial-consumer shape as
gpu/collector.py.
"""

from __future__ import annotations

import asyncio
import importlib.util
import logging
import os
import struct
import time
from typing import Dict, List, Optional, Tuple

logger = logging.getLogger(__name__)

_mod = None


def get_edge_module():
    global _mod
    if _mod is None:
        from ..ops.build import EDGE, build_edge

        build_edge(verbose=False)
        spec = importlib.util.spec_from_file_location("forge_edge", EDGE)
        _mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_mod)
    return _mod


# streaming endpoints cannot ride the buffered cold path — clients get a
# redirect to the control-plane port (uvicorn) which streams natively
_STREAM_GET_SUFFIXES = ("/mcp", "/sse", "/events")


class NativeEdge:
    def __init__(self, engine, app=None, auth=None, port: int = 4446,
                 threads: int = 4, control_url: Optional[str] = None,
                 depth: int = 2):
        self.engine = engine
        self.app = app            # FastAPI app for the cold path (optional)
        self.auth = auth          # AuthService; falls back to app.state.auth
        self.port = port
        self.threads = threads
        self.control_url = control_url
        # batches processed concurrently: with 2 in flight, batch B's C++
        # envelope/decide host stages overlap batch A's GPU sync (the
        # pipeline's _gpu_lock serializes only the device sections)
        self.depth = max(1, depth)
        self.edge = get_edge_module()
        self.handle = 0
        self._task: Optional[asyncio.Task] = None
        self._running = False
        self._auth_epoch = -1
        # python-side auth memo for server-scoped tokens (not C++-cacheable:
        # their requests must carry server_id through a per-request path)
        self._scoped_memo: Dict[bytes, Tuple[object, float]] = {}
        self.batches = 0
        self.requests = 0
        self.max_batch = 0
        self.packed = os.environ.get("FORGE_EDGE_PACKED", "1") != "0"
        # wall seconds spent in the batch handlers outside the awaited engine
        # calls: what this loop itself costs per batch
        self.glue_s = 0.0

    # ------------------------------------------------------------------
    async def start(self) -> None:
        s = self.engine.settings
        if self.auth is None and self.app is not None:
            self.auth = self.app.state.auth
        self.handle = self.edge.start(self.port, self.threads,
                                      s.max_request_body_bytes,
                                      bool(s.auth_required))
        self._running = True
        self._task = asyncio.create_task(self._loop())
        logger.info("native edge listening on :%d (%d threads)", self.port, self.threads)

    async def stop(self) -> None:
        self._running = False
        if self._task is not None:
            self._task.cancel()
            try:
                await self._task
            except (asyncio.CancelledError, Exception):
                pass
            self._task = None
        if self.handle:
            await asyncio.to_thread(self.edge.stop, self.handle)
            self.handle = 0

    def stats(self) -> dict:
        out = {"batches": self.batches, "requests": self.requests, "max_batch": self.max_batch,
               "packed": self.packed, "glue_ms": round(self.glue_s * 1000.0, 3)}
        if self.handle:
            out.update(self.edge.stats(self.handle))
        return out

    # ------------------------------------------------------------------
    def _check_revocations(self) -> None:
        if self.auth is None:
            return
        epoch = self.auth.revocation_epoch
        if epoch != self._auth_epoch:
            self._auth_epoch = epoch
            self._scoped_memo.clear()
            if self.handle:
                self.edge.auth_clear(self.handle)

    def _authenticate(self, authz: Optional[bytes]):
        """Resolve an Authorization header; returns AuthContext or None.
        Positive unscoped results are pushed into the C++ cache so the next
        request from this credential never reaches Python."""
        from ..auth.service import AuthError

        if self.auth is None:
            return None
        ent = self._scoped_memo.get(authz or b"")
        if ent is not None and ent[1] > time.monotonic():
            return ent[0]
        try:
            ctx = self.auth.authenticate(authz.decode() if authz else None)
        except AuthError:
            if authz and self.handle:
                self.edge.auth_put(self.handle, authz, None)  # negative (TTL'd)
            return None
        if authz and self.handle and ctx.server_id is None:
            self.edge.auth_put(self.handle, authz, ctx.user)
        else:
            if len(self._scoped_memo) > 2048:
                self._scoped_memo.clear()
            self._scoped_memo[authz or b""] = (ctx, time.monotonic() + 30.0)
        return ctx

    # ------------------------------------------------------------------
    async def _loop(self) -> None:
        s = self.engine.settings
        wait_us = 50_000
        linger_us = s.gpu_batch_window_us
        max_n = s.gpu_batch_max_requests
        sem = asyncio.Semaphore(self.depth)
        poll = self.edge.poll_packed if self.packed else self.edge.poll
        handle = self._handle_packed if self.packed else self._handle_batch

        async def run_one(batch):
            try:
                await handle(*batch)
            except Exception:
                logger.exception("native edge batch error")
            finally:
                sem.release()

        while self._running:
            try:
                await sem.acquire()
                batch = await asyncio.to_thread(poll, self.handle, wait_us, linger_us, max_n)
                # packed: hot ids are 8 bytes a row, batch[6] is the slow lane
                n = len(batch[0]) // 8 + len(batch[6][2]) if self.packed else len(batch[2])
                if n == 0:
                    sem.release()
                    continue
                self._check_revocations()
                self.batches += 1
                self.requests += n
                self.max_batch = max(self.max_batch, n)
                asyncio.ensure_future(run_one(batch))
            except asyncio.CancelledError:
                return
            except Exception:
                logger.exception("native edge loop error")
                sem.release()
                await asyncio.sleep(0.05)

    async def _handle_batch(self, ids: bytes, kinds: bytes, bodies, users, authzs, meta) -> None:
        t_in = time.perf_counter()
        eng = 0.0   # seconds inside awaited engine calls
        try:
            eng = await self._handle_rows(ids, kinds, bodies, users, authzs, meta)
        finally:
            self.glue_s += time.perf_counter() - t_in - eng

    async def _handle_rows(self, ids: bytes, kinds: bytes, bodies, users, authzs, meta) -> float:
        """The per-row path (FORGE_EDGE_PACKED=0). Returns the seconds spent
        inside awaited engine calls."""
        eng = 0.0
        n = len(bodies)
        statuses = bytearray(n * 2)
        outs: List[Optional[bytes]] = [None] * n

        hot_idx: List[int] = []
        hot_users: List[Optional[str]] = []
        scoped: List[Tuple[int, object]] = []   # (idx, ctx) server-scoped tokens
        cold: List[int] = []
        for i in range(n):
            if kinds[i] == 0:
                u = users[i]
                if u is None and authzs[i] is not None:
                    ctx = self._authenticate(authzs[i])
                    if ctx is None:
                        struct.pack_into("<H", statuses, i * 2, 401)
                        outs[i] = b'{"detail":"Not authenticated"}'
                        continue
                    if ctx.server_id is not None:
                        scoped.append((i, ctx))
                        continue
                    u = ctx.user
                hot_idx.append(i)
                hot_users.append(u)
            else:
                cold.append(i)

        if hot_idx:
            # usage accounting for the C++-authenticated hot lane (one
            # increment per request; credential granularity is the user —
            # the native cache intentionally does not carry token ids)
            for u in hot_users:
                self.engine.token_usage.record(f"user:{u}" if u else "anonymous", u)
            raws = [bodies[i] for i in hot_idx]
            t_e = time.perf_counter()
            results = await self.engine.process_rpc_batch(raws, users=hot_users)
            eng += time.perf_counter() - t_e
            for i, r in zip(hot_idx, results):
                if r is None:
                    struct.pack_into("<H", statuses, i * 2, 202)
                    outs[i] = b""
                else:
                    struct.pack_into("<H", statuses, i * 2, 200)
                    outs[i] = r if isinstance(r, bytes) else bytes(r)

        for i, ctx in scoped:
            t_e = time.perf_counter()
            r = await self.engine.handle_rpc_bytes(bodies[i], user=ctx.user, server_id=ctx.server_id)
            eng += time.perf_counter() - t_e
            struct.pack_into("<H", statuses, i * 2, 200 if r is not None else 202)
            outs[i] = r or b""

        # complete the hot lane first — cold requests may take arbitrary time
        if hot_idx or scoped or any(outs[i] is not None for i in range(n)):
            hot_ids = b"".join(ids[i * 8:(i + 1) * 8] for i in range(n) if outs[i] is not None)
            hot_sts = b"".join(statuses[i * 2:(i + 1) * 2] for i in range(n) if outs[i] is not None)
            hot_bodies = [outs[i] for i in range(n) if outs[i] is not None]
            await asyncio.to_thread(self.edge.complete, self.handle, hot_ids, bytes(hot_sts), hot_bodies)

        for i in cold:
            (rid,) = struct.unpack_from("<Q", ids, i * 8)
            asyncio.ensure_future(self._cold_one(rid, meta[i], bodies[i], authzs[i]))
        return eng

    # ------------------------------------------------------------------
    async def _handle_packed(self, ids: bytes, blob: bytes, offs: bytes, uidx: bytes,
                             users, ucount, slow) -> None:
        t_in = time.perf_counter()
        box = [0.0]   # seconds inside awaited engine calls
        try:
            await self._handle_lanes(ids, blob, offs, uidx, users, ucount, slow, box)
        finally:
            self.glue_s += time.perf_counter() - t_in - box[0]

    async def _handle_lanes(self, ids: bytes, blob: bytes, offs: bytes, uidx: bytes,
                            users, ucount, slow, box) -> None:
        """One poll_packed batch. The hot lane (ids/blob/offs/uidx/users/
        ucount) goes to the engine as it came; the slow lane keeps the
        per-row logic of _handle_rows."""
        s_ids, s_kinds, s_bodies, s_users, s_authzs, s_meta = slow
        denied: List[int] = []
        scoped: List[Tuple[int, object]] = []       # (idx, ctx) server-scoped tokens
        promoted: List[Tuple[int, Optional[str]]] = []  # authenticated here, unscoped
        cold: List[int] = []
        for i in range(len(s_bodies)):
            if s_kinds[i] == 0:
                u = s_users[i]
                if u is None and s_authzs[i] is not None:
                    ctx = self._authenticate(s_authzs[i])
                    if ctx is None:
                        denied.append(i)
                        continue
                    if ctx.server_id is not None:
                        scoped.append((i, ctx))
                        continue
                    u = ctx.user
                promoted.append((i, u))
            else:
                cold.append(i)

        if promoted:
            # rare (first request of a credential): append to the hot batch
            h = len(ids) // 8
            users, ucount = list(users), list(ucount)
            (last,) = struct.unpack_from("<q", offs, h * 8)
            add_ids, add_bodies, add_offs, add_uidx = [], [], [], []
            for i, u in promoted:
                if u in users:
                    k = users.index(u)
                else:
                    k = len(users)
                    users.append(u)
                    ucount.append(0)
                ucount[k] += 1
                last += len(s_bodies[i])
                add_ids.append(s_ids[i * 8:(i + 1) * 8])
                add_bodies.append(s_bodies[i])
                add_offs.append(last)
                add_uidx.append(k)
            ids += b"".join(add_ids)
            blob += b"".join(add_bodies)
            offs += struct.pack(f"<{len(add_offs)}q", *add_offs)
            uidx += struct.pack(f"<{len(add_uidx)}i", *add_uidx)

        if ids:
            # usage accounting for the C++-authenticated hot lane (credential
            # granularity is the user — the native cache intentionally does
            # not carry token ids): one increment of n per distinct user
            for u, c in zip(users, ucount):
                self.engine.token_usage.record(f"user:{u}" if u else "anonymous", u, n=c)
            t_e = time.perf_counter()
            results = await self.engine.process_rpc_packed(blob, offs, uidx, users)
            box[0] += time.perf_counter() - t_e
            # complete the hot lane first — scoped and cold requests may take
            # arbitrary time. complete_list reads `results` without the GIL:
            # nothing may touch the list until the call returns
            await asyncio.to_thread(self.edge.complete_list, self.handle, ids, results)

        if denied or scoped:
            d_ids, d_sts, d_bodies = [], [], []
            for i in denied:
                d_ids.append(s_ids[i * 8:(i + 1) * 8])
                d_sts.append(401)
                d_bodies.append(b'{"detail":"Not authenticated"}')
            for i, ctx in scoped:
                t_e = time.perf_counter()
                r = await self.engine.handle_rpc_bytes(s_bodies[i], user=ctx.user, server_id=ctx.server_id)
                box[0] += time.perf_counter() - t_e
                d_ids.append(s_ids[i * 8:(i + 1) * 8])
                d_sts.append(200 if r is not None else 202)
                d_bodies.append(r or b"")
            await asyncio.to_thread(self.edge.complete, self.handle, b"".join(d_ids),
                                    struct.pack(f"<{len(d_sts)}H", *d_sts), d_bodies)

        for i in cold:
            (rid,) = struct.unpack_from("<Q", s_ids, i * 8)
            asyncio.ensure_future(self._cold_one(rid, s_meta[i], s_bodies[i], s_authzs[i]))

    # ------------------------------------------------------------------
    async def _cold_one(self, rid: int, m, body: bytes, authz: Optional[bytes]) -> None:
        """Serve a control-plane request through the ASGI app and write the
        raw HTTP response back on the native connection."""
        try:
            raw = await self._run_asgi(m, body, authz)
        except Exception:
            logger.exception("cold path error")
            payload = b'{"detail":"internal error"}'
            raw = (b"HTTP/1.1 500 Internal Server Error\r\nContent-Type: application/json\r\n"
                   + b"Content-Length: " + str(len(payload)).encode() + b"\r\n\r\n" + payload)
        await asyncio.to_thread(self.edge.complete_raw, self.handle, rid, raw)

    async def _run_asgi(self, m, body: bytes, authz: Optional[bytes]) -> bytes:
        method, target, headers_blob = m
        path, _, query = target.partition("?")
        if self.app is None:
            payload = b'{"detail":"control plane not mounted on the native edge"}'
            return (b"HTTP/1.1 404 Not Found\r\nContent-Type: application/json\r\nContent-Length: "
                    + str(len(payload)).encode() + b"\r\n\r\n" + payload)
        if method == "GET" and (path.endswith(_STREAM_GET_SUFFIXES) or "/sse" in path):
            # streaming endpoints live on the control-plane port
            loc = (self.control_url or "") + target
            if self.control_url:
                return (b"HTTP/1.1 307 Temporary Redirect\r\nLocation: " + loc.encode()
                        + b"\r\nContent-Length: 0\r\n\r\n")
            payload = b'{"detail":"streaming endpoints are served by the control-plane port"}'
            return (b"HTTP/1.1 501 Not Implemented\r\nContent-Type: application/json\r\nContent-Length: "
                    + str(len(payload)).encode() + b"\r\n\r\n" + payload)
        # parse header lines (skip request line) into ASGI header pairs
        headers: List[Tuple[bytes, bytes]] = []
        for line in headers_blob.split(b"\r\n")[1:]:
            k, sep, v = line.partition(b":")
            if sep:
                headers.append((k.strip().lower(), v.strip()))
        scope = {
            "type": "http", "asgi": {"version": "3.0"}, "http_version": "1.1",
            "method": method, "scheme": "http", "path": path, "raw_path": path.encode(),
            "query_string": query.encode(), "headers": headers,
            "client": ("127.0.0.1", 0), "server": ("127.0.0.1", self.port),
        }
        sent = [False]

        async def receive():
            if not sent[0]:
                sent[0] = True
                return {"type": "http.request", "body": body, "more_body": False}
            return {"type": "http.disconnect"}

        status = [500]
        resp_headers: List[Tuple[bytes, bytes]] = []
        chunks: List[bytes] = []

        async def send(msg):
            if msg["type"] == "http.response.start":
                status[0] = msg["status"]
                resp_headers.extend(msg.get("headers") or [])
            elif msg["type"] == "http.response.body":
                chunks.append(msg.get("body", b""))

        await asyncio.wait_for(self.app(scope, receive, send), timeout=60.0)
        payload = b"".join(chunks)
        head = [b"HTTP/1.1 " + str(status[0]).encode() + b" X"]
        has_len = False
        for k, v in resp_headers:
            if k.lower() == b"content-length":
                has_len = True
            if k.lower() in (b"transfer-encoding", b"connection"):
                continue
            head.append(k + b": " + v)
        if not has_len:
            head.append(b"Content-Length: " + str(len(payload)).encode())
        return b"\r\n".join(head) + b"\r\n\r\n" + payload
