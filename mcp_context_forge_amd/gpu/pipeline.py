"""The batched GPU plugin pipeline — the MI355X-native hot path.

Reference analog: the per-request chain tool_service.invoke_tool (:5067)
with plugin hooks (:5530), plus the Rust edge runtime's native fast path
(crates/mcp_runtime). Here a whole micro-batch is staged to HBM and the
plugin chain's data-parallel stages run as HIP kernels (BASELINE.json),
with a C++ host fast path around them:

  C++ envelope scan   → JSON-RPC spans, no Python parse (ops/csrc/envelope.cpp)
  scan banks (GPU)    → deny / harm / pii / regex / normalizer-trigger DFAs
                        + schema-shape presence patterns, over RAW arg bytes
  featurize (GPU)     → hashed count vectors (LDS histograms)
  classifier (GPU)    → content_moderation bf16 MFMA MLP
  semcache (GPU)      → response_cache_by_prompt cosine sweep in HBM
  C++ native upstream → fast_time_server analog (ops/csrc/upstream.cpp)
  result scan (GPU)   → pii/regex/harm over serialized results

Decisions are numpy-vectorized; Python touches a request only when a kernel
flags it (rewrites, schema fallbacks, unusual envelopes) — those take the
exact per-request semantics (the plugins' own functions), so the parity
gate (tests/test_gpu_parity.py, reference analog
tests/live_gateway/mcp/test_mcp_plugin_parity.py) holds by construction.

Raw-bytes-vs-decoded-text containment (tested invariant —
tests/test_parity_fuzz.py runs adversarial generators against the CPU
chain):

  * literal deny/harm words: a RAW match implies a DECODED match (words
    are alphanumeric; no word can span JSON structural separators), so
    raw-scan blocks are sound;
  * content that can decode DIFFERENTLY from its raw bytes (JSON escapes,
    non-ASCII) always trips the escape-trigger bank, which routes the row
    to the exact host path where deny (pre-rewrite, CPU order), rewrites,
    harm, moderation and schema run over decoded text;
  * schema-shape fast patterns cannot false-positive from key lookalikes
    inside string values (embedded quotes are escaped, which breaks the
    byte pattern) and any nesting defers to exact host validation;
  * the one intentional approximation: the moderation classifier featurizes
    raw bytes for rows with NO escape triggers — wire forms that differ
    from canonical text only by whitespace/key order can score differently
    near the threshold. Rows with triggers are re-scored over canonical
    text on the host path;
  * secrets_detection is an exact prefilter over raw bytes: a span with no
    backslash and no non-ASCII byte holds every decoded string value
    verbatim between quotes, and '"' is in no entropy alphabet, so every
    run and every pattern match the CPU plugin can see is present
    byte-for-byte in the raw span. The bank's DFA patterns are supersets
    of the plugin's regexes and the entropy compare subtracts TOL (f32 vs
    f64 rounding), so the prefilter may over-flag (keys, long integers)
    but never under-flags. Flagged rows, and every span with a backslash
    or a non-ASCII byte, run the exact CPU plugin
    (tests/test_secrets_plugin.py checks the containment on the CPU);
  * encoded_exfil_detection is an exact prefilter in the same way. A span
    with no backslash and no non-ASCII byte holds every string value
    verbatim between quotes, and '"' is in neither the base64 nor the hex
    alphabet, so every run the plugin can see is present byte for byte in
    the raw span, with the same length, decoded bytes, printable count and
    keyword mask — all integers, computed by exfil.hip exactly as by
    ops/exfil.py, so nothing is subtracted. The prefilter over-flags only
    where the raw span has runs the plugin never scans (keys, long
    integers); it never under-flags. Flagged rows, and every span with a
    backslash or a non-ASCII byte, run the exact CPU plugin
    (tests/test_exfil_plugin.py checks the containment on the CPU);
  * sql_sanitizer is an exact prefilter in the same way. A span with no
    backslash and no non-ASCII byte holds every string value verbatim
    between quotes, and no such value contains '"'. sql.hip scans the raw
    span in boundary mode, where every '"' resets the lexer to CODE and
    closes the statement, so each value is lexed, matched and folded from
    a fresh state exactly as the plugin scans it alone in text mode, and
    the per-span counts are sums (the blocked mask an OR) over the values
    plus whatever keys and bare literals add: they can only add findings.
    All outputs are integers, computed by sql.hip exactly as by ops/sql.py.
    Rows with a delete / update without where the plugin blocks, a blocked
    word, a comment when strip_comments is on, and every span with a
    backslash or a non-ASCII byte, run the exact CPU plugin
    (tests/test_sql_plugin.py checks the containment on the CPU).
"""

from __future__ import annotations

import asyncio
import json
import os
import time
import uuid
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from ..models.classifier import category_names
from ..ops import dfa, hip
from ..ops.entropy import TOL as ENTROPY_TOL
from ..ops.pybridge import get as _pb_get
from ..plugins.builtin import PII_PATTERNS, _text_of, _walk_strings
from ..plugins.framework import PluginMode
from ..protocol import jsonrpc
from ..services.upstream import InProcUpstream
from ..utils.jsonschema import validate as _validate
from .batch import pack_texts
from .classifier import GpuClassifier
from .graphs import Pass1Graphs, Pass3Graphs
from .rowset import (BAD_ARGS, INVALID_ARGS, RowSet, msg_deny, msg_harm, msg_moderation, msg_pii,
                     msg_pii_bits, msg_schema)
from .semcache import GpuSemanticCache, tool_hash
from .tooltable import (PluginHandles, ToolTable, _ToolMeta, active, applies, build_tool_table,
                        enforcing, pack_strtable, pii_mode)

# normalizer-trigger prefilter (conservative superset over raw JSON bytes):
# JSON escapes for whitespace/unicode, literal multi-space, space adjacent to
# a quote, and raw non-ASCII bytes (clients that don't ensure_ascii).
_NORMALIZE_TRIGGERS = ["\\t", "\\n", "\\r", "\\f", "\\u", "  ", '" ', ' "',
                       "[" + chr(0x80) + "-" + chr(0xFF) + "]"]


def _sorted_json(obj: Any) -> str:
    """The sorted-keys scan form (_text_of's serialization)."""
    return json.dumps(obj, separators=(",", ":"), sort_keys=True, default=str)


def _wire_json(obj: Any) -> bytes:
    return json.dumps(obj, separators=(",", ":"), default=str).encode()


def _now_iso() -> str:
    return time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())


class _PackedRows:
    """raws[i] over a joined blob + offsets: a row's bytes exist only once a
    per-request path (non-tools/call, host-bound, cross-rank forward) asks."""

    __slots__ = ("blob", "offs")

    def __init__(self, blob: bytes, offs: np.ndarray):
        self.blob = blob
        self.offs = offs

    def __len__(self) -> int:
        return max(int(self.offs.shape[0]) - 1, 0)

    def __getitem__(self, i: int) -> bytes:
        return self.blob[int(self.offs[i]):int(self.offs[i + 1])]


class _IndexedUsers:
    """users[i] over the batch's distinct users + a per-row index."""

    __slots__ = ("users", "uidx")

    def __init__(self, users: List[Optional[str]], uidx: np.ndarray):
        self.users = users
        self.uidx = uidx

    def __len__(self) -> int:
        return int(self.uidx.shape[0])

    def __getitem__(self, i: int) -> Optional[str]:
        return self.users[int(self.uidx[i])]


class GpuPluginPipeline:
    def __init__(self, engine, device: str = "cuda"):
        self.engine = engine
        self.device = device
        s = engine.settings

        h = self._handles = PluginHandles(engine.plugins)
        self.deny, self.harm, self.pii, self.regex = h.deny, h.harm, h.pii, h.regex
        self.normalizer, self.moderation, self.schema_guard = h.normalizer, h.moderation, h.schema_guard
        self.semcache_plugin, self.exact_cache, self.breaker = h.semcache_plugin, h.exact_cache, h.breaker
        self.toon, self.out_guard, self.secrets, self.exfil = h.toon, h.out_guard, h.secrets, h.exfil
        self.sql = h.sql

        self.banks: Dict[str, hip.DeviceScanTables] = {}
        for name, p in (("deny", self.deny), ("harm", self.harm), ("pii", self.pii), ("regex", self.regex)):
            tables = p.scan_tables() if p is not None and hasattr(p, "scan_tables") else None
            if tables is not None:
                self.banks[name] = hip.DeviceScanTables(tables, device)
        # the escape/normalize trigger bank routes rows whose RAW bytes may
        # decode to different text (JSON escapes, non-ASCII) onto the exact
        # host path. It must exist whenever ANY content bank scans raw bytes
        # — not only when the normalizer plugin is enabled — otherwise an
        # escape-hidden deny/harm word (e.g. "forbidden") would slip
        # past the raw-byte scans with no host recheck (parity-fuzz finding)
        if any(p is not None for p in (self.normalizer, self.deny, self.harm,
                                       self.pii, self.regex, self.moderation)):
            self.banks["normalize"] = hip.DeviceScanTables(
                dfa.compile_patterns(
                    ["".join(ch if ch.isalnum() else "\\" + ch for ch in t) if not t.startswith("[") else t
                     for t in _NORMALIZE_TRIGGERS], case_insensitive=False), device)

        # secrets_detection: its format bank plus one symbol table and
        # threshold per configured entropy alphabet (entropy.hip)
        self._secret_tabs: List[Tuple[torch.Tensor, float]] = []
        if self.secrets is not None:
            tables = self.secrets.scan_tables()
            if tables is not None:
                self.banks["secrets"] = hip.DeviceScanTables(tables, device)
            self._secret_tabs = [(hip.entropy_table(tab, device), thr)
                                 for (_a, _c, tab, thr) in self.secrets.entropy_detectors]
            if not self._secret_tabs:
                # formats only: an empty alphabet still reports the
                # backslash / non-ASCII bit, which the prefilter needs
                self._secret_tabs = [(hip.entropy_table(np.full(256, 0xFF, dtype=np.uint8), device),
                                      float("inf"))]

        # encoded_exfil_detection: its keyword tables plus one symbol table
        # and symbol width per configured encoding (exfil.hip)
        self._exfil_kw: Optional[hip.DeviceScanTables] = None
        self._exfil_tabs: List[Tuple[torch.Tensor, int]] = []
        if self.exfil is not None:
            self._exfil_kw = hip.DeviceScanTables(self.exfil.keyword_tables(), device)
            self._exfil_tabs = [(hip.entropy_table(tab, device), bits)
                                for (_e, _c, tab, bits) in self.exfil.detectors]

        # sql_sanitizer: its keyword tables and the keyword lengths (sql.hip)
        self._sql_kw: Optional[hip.DeviceScanTables] = None
        self._sql_kw_len: Optional[torch.Tensor] = None
        if self.sql is not None:
            self._sql_kw = hip.DeviceScanTables(self.sql.keyword_tables(), device)
            self._sql_kw_len = torch.tensor(self.sql.keyword_lengths(), dtype=torch.int32, device=device)

        self.classifier: Optional[GpuClassifier] = None
        self.feat_dim = s.gpu_feature_dim
        if self.moderation is not None:
            self.classifier = GpuClassifier(self.moderation.model, device)
            self.feat_dim = self.moderation.dim
        # native rescoring session (rescore.hip): the moderation rescan of a
        # batch's rewritten rows as ONE call into session-owned buffers.
        # Owned by the asyncio thread; FORGE_RESCORE_NATIVE=0 (read per
        # batch) or any submit error takes the eager path instead
        self._rescore: Optional[hip.RescoreSession] = None
        if self.classifier is not None:
            c = self.classifier
            self._rescore = hip.RescoreSession(c.w1t, c.b1, c.w2t, c.b2)
        self.rescore_native = self.rescore_eager = 0

        self.semcache: Optional[GpuSemanticCache] = None
        # the HBM cache only exists when the plugin has an EXPLICIT per-tool
        # allowlist (empty by default, like the reference's cacheable_tools):
        # with no allowlisted tool the cosine sweep would be pure overhead
        # and a hit could never legally substitute a result anyway
        if self.semcache_plugin is not None and self.semcache_plugin.cacheable_tools:
            self.semcache = GpuSemanticCache(
                capacity=max(128, (s.gpu_semcache_capacity // 128) * 128),
                dim=self.feat_dim,
                threshold=self.semcache_plugin.threshold,
                ttl_s=self.semcache_plugin.ttl,
                device=device,
                sketch_dim=s.gpu_semcache_sketch_dim,
            )

        # native rewrite lane (rewrite.cpp): fixed-index PII maps for the
        # C matchers (the plugin's active list may be a config subset)
        self._pii_fixed: List[int] = []
        self._pii_active_mask = 0
        if self.pii is not None:
            fixed_index = {n: k for k, (n, _, _) in enumerate(PII_PATTERNS)}
            self._pii_fixed = [fixed_index[a[0]] for a in self.pii.active]
            self._pii_active_mask = sum(1 << i for i in self._pii_fixed)
        # deny word table for the native lane's pre-rewrite recheck
        # (lowercased when case-insensitive; non-ASCII words disable the
        # lane for deny-active tools — those rows stay on the Python path)
        words = [w.lower() if self.deny.case_insensitive else w for w in self.deny.words] if self.deny else []
        self._deny_lane_ok = bool(words) and all(w.isascii() for w in words)
        self._deny_lane_blob, self._deny_lane_off = pack_strtable(words) if self._deny_lane_ok else (None, None)
        # harm phrase table for the native POST lane (_host_post's C path):
        # pre-lowercased, plugin order; non-ASCII phrases disable the lane
        # for harm-active tools (those rows stay on the Python path)
        ph = [p.lower() for p in (getattr(self.harm, "phrases", None) or [])]
        self._harm_lane_ok = all(p.isascii() for p in ph)
        self._harm_lane_blob, self._harm_lane_off = pack_strtable(ph) if ph and self._harm_lane_ok else (None, None)

        self._pb = _pb_get()  # C response-assembly loops (fails loudly if missing)
        # two batches may be in flight (engine splits big batches): GPU
        # sections (shared pinned arena + stream) serialize on this lock,
        # host/C++ sections interleave. A short GIL switch interval keeps
        # to_thread C calls from stalling behind long Python stretches.
        self._gpu_lock = asyncio.Lock()
        # pinned-host staging arena (bump-allocated per pass; reset after each sync)
        self._pin = torch.empty(16 << 20, dtype=torch.uint8, pin_memory=True)
        self._pin_off = 0

        # post-pass metadata bank: structuredContent presence → toon candidate
        self.banks["postmeta"] = hip.DeviceScanTables(
            dfa.compile_literals(['"structuredContent"'], case_insensitive=False), device)

        # fused multi-bank scans: pass 3's bank set is static; pass 1's holds
        # the per-registry schema bank and lives in the ToolTable. With secrets
        # or exfil on, pass 3 stays eager: token_entropy / decode_scan run on
        # the same uploaded tensors
        self._bankset3 = hip.ScanBankSet(
            [(n, self.banks[n]) for n in ("pii", "regex", "harm", "postmeta", "secrets")
             if n in self.banks],
            device)
        self._graphs3 = Pass3Graphs(self) if self.secrets is None and self.exfil is None else None

        # native decision-plane stores + string tables (fastpath.cpp)
        self._slot_store = hip.store_new(self.semcache.capacity) if self.semcache is not None else 0
        self._exact_native = hip.cache_new(self.exact_cache.ttl) if self.exact_cache is not None else 0
        self._deny_tab = pack_strtable(self.deny.words if self.deny else [])
        self._harm_tab = pack_strtable(self.harm.cats if self.harm else [])
        self._mod_tab = pack_strtable(category_names(self.moderation.model.classes) if self.moderation else [])

        # per-tool tables + schema-shape bank: one ToolTable per registry /
        # plugin generation, replaced (never edited) by _meta(). A batch in
        # flight keeps its snapshot and with it the toolmap handle, so a
        # replaced table's handle is freed only a few rebuilds later
        self._tools: Optional[ToolTable] = None
        self._toolmap_graveyard: List[int] = []

        # stats
        self.batches = self.requests = self.fast_path = self.slow_path = 0
        self.blocked = self.cache_hits = self.post_rewrites = self.py_fallback = 0
        self.post_c = 0       # flagged results fully handled by forge_post_rows
        self.post_c_punt = 0  # rows the C post lane punted back to Python
        self.host_bound = 0   # requests routed to the CPU chain by plugin bindings
        self.secrets_routed = 0  # requests the secrets prefilter sent to the CPU chain
        self.exfil_routed = 0    # requests the encoded-exfil prefilter sent to the CPU chain
        self.sql_routed = 0      # requests the sql prefilter sent to the CPU chain
        # optional per-stage wall-clock accounting (FORGE_PIPELINE_TIMING=1)
        self.timing_enabled = bool(os.environ.get("FORGE_PIPELINE_TIMING"))
        self.timing: Dict[str, float] = {}

    # ------------------------------------------------------------------
    def _meta(self) -> ToolTable:
        """The current ToolTable, rebuilt when the registry generation or the
        plugins version moved. Callers read it ONCE per batch."""
        t = self._tools
        if t is None or t.generation != self.engine.registry.generation or \
           t.plugins_ver != getattr(self.engine.plugins, "version", 0):
            if t is not None and t.toolmap:
                g = self._toolmap_graveyard
                g.append(t.toolmap)
                while len(g) > 8:
                    hip.toolmap_free(g.pop(0))
            t = build_tool_table(self.engine, self._handles, self.banks, self.device,
                                 semcache_on=self.semcache is not None,
                                 harm_lane_ok=self._harm_lane_ok)
            # hipGraph fast path (gpu/graphs.py): with the semcache on, pass 1
            # stays eager (the cache probe is not captured)
            t.graphs = Pass1Graphs(self, t.bankset1) if self.semcache is None else None
            self._tools = t
        return t

    def _active(self, plugin, tool_name: str, block_class: bool) -> bool:
        return active(self.engine.plugins, plugin, tool_name, block_class)

    # ------------------------------------------------------------------
    def _tic(self):
        return time.monotonic() if self.timing_enabled else 0.0

    def _toc(self, key: str, t0: float) -> None:
        if self.timing_enabled:
            self.timing[key] = self.timing.get(key, 0.0) + (time.monotonic() - t0)

    async def process_batch(self, raws: List[bytes], user: Optional[str] = None,
                            server_id: Optional[str] = None,
                            users: Optional[List[Optional[str]]] = None) -> List[Optional[bytes]]:
        t0 = self._tic()
        joined, offs_raw = self._pb.concat_with_offsets(raws)
        return await self._process_joined(joined, offs_raw, raws, user, server_id, users, None, t0)

    async def process_packed(self, blob: bytes, offs: bytes, uidx: bytes,
                             users: List[Optional[str]],
                             server_id: Optional[str] = None) -> List[Optional[bytes]]:
        """process_batch for a batch that arrives already joined (the native
        edge's hot lane): `blob` holds every body back to back, `offs` the
        int64 offsets (n + 1, concat_with_offsets layout), `uidx` an int32
        per row into `users`, the batch's distinct users. A row's bytes are
        materialised only where a per-request path needs them, and tenant
        hashes cost one tool_hash per distinct user."""
        t0 = self._tic()
        ui = np.frombuffer(uidx, dtype=np.int32)
        table = np.array([tool_hash(u or "") for u in users], dtype=np.int64)
        uh_all = table[ui] if ui.size else np.empty(0, dtype=np.int64)
        rows = _PackedRows(blob, np.frombuffer(offs, dtype=np.int64))
        return await self._process_joined(blob, offs, rows, None, server_id,
                                          _IndexedUsers(users, ui), uh_all, t0)

    async def _process_joined(self, joined: bytes, offs_raw: bytes, raws, user: Optional[str],
                              server_id: Optional[str], users, uh_all: Optional[np.ndarray],
                              t0: float) -> List[Optional[bytes]]:
        """Shared body of process_batch / process_packed. `raws` and `users`
        are only indexed (`raws[i]`, `users[i]`), so lazy views work."""
        self.batches += 1
        n = len(raws)
        self.requests += n
        responses: List[Optional[bytes]] = [None] * n

        def row_user(i: int) -> Optional[str]:
            return users[i] if users is not None else user

        offsets = np.frombuffer(offs_raw, dtype=np.int64)
        blob = np.frombuffer(joined, dtype=np.uint8) if joined else np.zeros(1, dtype=np.uint8)
        env = hip.parse_envelopes(blob, offsets)
        self._toc("pack_envelope", t0)
        kind = env["kind"]

        other_rows = np.nonzero(kind != hip.ENV_TOOLS_CALL)[0]
        if other_rows.size:
            self.py_fallback += int(other_rows.size)
            await self._host_chain_rows(other_rows, raws, row_user, server_id, responses)

        fast_rows = np.nonzero(kind == hip.ENV_TOOLS_CALL)[0]
        if fast_rows.size:
            await self._fast_toolcalls(raws, blob, env, fast_rows, responses, user, server_id, users,
                                       row_user, uh_all)
        return responses

    async def _host_chain_rows(self, batch_rows, raws, row_user, server_id, responses) -> None:
        """Batch rows that take the exact per-request CPU chain."""
        outs = await asyncio.gather(
            *(self.engine.handle_rpc_bytes(raws[int(i)], user=row_user(int(i)), server_id=server_id)
              for i in batch_rows))
        for i, out in zip(batch_rows, outs):
            responses[int(i)] = out

    # ---- the tools/call rows of a batch ----
    async def _fast_toolcalls(self, raws, blob: np.ndarray, env: dict, rows: np.ndarray,
                              responses: List[Optional[bytes]], user: Optional[str],
                              server_id: Optional[str], users, row_user: Callable,
                              uh_all: Optional[np.ndarray]) -> None:
        # the batch's snapshot of the tool tables: every later stage reads
        # per-tool data from rs.tools, never from self
        tools = self._meta()
        m = rows.shape[0]
        # per-row tenant hash: cache identities (semantic + exact) are
        # (tool, user)-scoped so results never cross users (63-bit so the
        # XOR with tool_hash stays in int64 domain). The packed entry passes
        # them in already gathered (one tool_hash per distinct user).
        if uh_all is None and users is not None:
            memo: Dict[Optional[str], int] = {u: tool_hash(u or "") for u in set(users)}
            uh_all = np.fromiter((memo[u] for u in users), dtype=np.int64, count=len(users))
        uh = uh_all[rows] if uh_all is not None else np.full(m, tool_hash(user or ""), dtype=np.int64)
        nb = np.ascontiguousarray(env["name_beg"][rows])
        ne = np.ascontiguousarray(env["name_end"][rows])
        ab, ae = env["args_beg"], env["args_end"]
        args_b = np.ascontiguousarray(np.where(ab[rows] >= 0, ab[rows], 0).astype(np.int32))
        args_e = np.ascontiguousarray(np.where(ab[rows] >= 0, ae[rows], 0).astype(np.int32))

        t_r = self._tic()
        tool_idx = hip.toolmap_resolve(tools.toolmap, blob, nb, ne) if tools.toolmap \
            else np.full(m, -1, dtype=np.int32)
        self._toc("toolmap", t_r)
        rs = RowSet(rows, uh, tool_idx, nb, ne,
                    np.ascontiguousarray(env["id_beg"][rows]), np.ascontiguousarray(env["id_end"][rows]),
                    args_b, args_e, blob, env, responses, tools, self)

        fw_state = self._forward_foreign(rs, raws, user, users)
        if len(rs) and (tools.hostbound is not None or tools.secrets is not None
                        or tools.exfil is not None or tools.sql is not None):
            await self._route_host_rows(rs, raws, row_user, server_id)
        if len(rs):
            await self._gpu_rows(rs)
        await self._finish_forward(fw_state, responses)

    def _forward_foreign(self, rs: RowSet, raws, user, users):
        """Cross-rank routing: rows whose tool is owned by a peer rank ride
        the RCCL bus as per-destination batches (BASELINE config 3:
        federation shard fan-out); they overlap the local GPU pass and are
        spliced into `responses` at the end. → the pending forwards or None;
        forwarded rows leave the row set."""
        eng = self.engine
        if not (eng.foreign_tools and eng.forward_rpc_batch is not None and (rs.tool_idx < 0).any()):
            return None
        rows = rs.rows
        groups: Dict[int, List[int]] = {}
        for j in np.nonzero(rs.tool_idx < 0)[0]:
            j = int(j)
            name = rs.blob[rs.nb[j]:rs.ne[j]].tobytes().decode("utf-8", "replace")
            dest = eng.foreign_tools.get(name)
            if dest is not None and dest != eng.rank:
                groups.setdefault(dest, []).append(j)
        if not groups:
            return None
        tasks, fw_rows = [], []
        fw_mask = np.zeros(len(rs), dtype=bool)
        for dest, js in groups.items():
            rws = [raws[int(rows[j])] for j in js]
            if users is not None:
                us = [users[int(rows[j])] for j in js]
            else:
                us = [user] * len(js) if user is not None else None
            tasks.append(eng.forward_rpc_batch(dest, rws, us))
            fw_rows.append([int(rows[j]) for j in js])
            fw_mask[js] = True
        rs.keep(~fw_mask)
        return (asyncio.gather(*tasks), fw_rows)

    async def _finish_forward(self, fw_state, responses: List[Optional[bytes]]) -> None:
        """Splice cross-rank (bus-forwarded) responses into the batch output."""
        if fw_state is None:
            return
        gathered, fw_rows = fw_state
        outs_groups = await gathered
        for grp_rows, outs in zip(fw_rows, outs_groups):
            for r, o in zip(grp_rows, outs):
                responses[r] = o if (o is None or isinstance(o, bytes)) else bytes(o)

    async def _route_host_rows(self, rs: RowSet, raws, row_user, server_id) -> None:
        """Tools with semantics-altering plugin bindings run the full CPU
        chain (the binding-aware invoke_hook path); everything else stays on
        the GPU fast path. Routed rows are answered and leave the row set."""
        tools, tool_idx, m = rs.tools, rs.tool_idx, len(rs)
        hb_mask = np.zeros(m, dtype=bool)
        valid = tool_idx >= 0
        if tools.hostbound is not None:
            hb_mask[valid] = tools.hostbound[tool_idx[valid]]
        n_bound = int(hb_mask.sum())
        # secrets_detection / encoded_exfil_detection / sql_sanitizer pre-pass:
        # rows of tools one of them is active for, whose raw argument bytes MAY
        # hold a finding, leave with the host-bound rows and run the exact
        # CPU chain, plugins included
        def plugin_rows(per_tool: Optional[np.ndarray]) -> Optional[np.ndarray]:
            if per_tool is None:
                return None
            rows = np.zeros(m, dtype=bool)
            rows[valid] = per_tool[tool_idx[valid]]
            rows &= ~hb_mask
            return rows if rows.any() else None

        sec_rows, exf_rows = plugin_rows(tools.secrets), plugin_rows(tools.exfil)
        sql_rows = plugin_rows(tools.sql)
        if sec_rows is not None or exf_rows is not None or sql_rows is not None:
            sec_flagged, exf_flagged, sql_flagged = await self._raw_prepass(
                rs.blob, rs.args_b, rs.args_e, sec_rows, exf_rows, sql_rows)
            if sec_flagged is not None:
                self.secrets_routed += int(sec_flagged.sum())
                hb_mask |= sec_flagged
            if exf_flagged is not None:
                self.exfil_routed += int(exf_flagged.sum())
                hb_mask |= exf_flagged
            if sql_flagged is not None:
                self.sql_routed += int(sql_flagged.sum())
                hb_mask |= sql_flagged
        if hb_mask.any():
            self.host_bound += n_bound
            await self._host_chain_rows(rs.rows[hb_mask], raws, row_user, server_id, rs.responses)
            rs.keep(~hb_mask)

    async def _gpu_rows(self, rs: RowSet) -> None:
        """Pass 1 → native decide → answers, rewrites and dispatch."""
        tools, blob, tool_idx, m = rs.tools, rs.blob, rs.tool_idx, len(rs)

        # --- GPU pass 1 over raw argument spans ---
        def pass1_extra(data_gpu, beg_t, end_t):
            # eager only: the captured graph holds featurize + classifier itself
            feats = scores_t = cache_val_t = cache_idx_t = feats_sk = None
            if self.classifier is not None or self.semcache is not None:
                feats, _ = hip.featurize(data_gpu, beg_t, end_t, self.feat_dim, pad_to=128)
            if self.classifier is not None:
                scores_t = self.classifier.forward(feats)[:m]
            if self.semcache is not None:
                bv, bi, feats_sk = self.semcache.lookup(feats)
                cache_val_t, cache_idx_t = bv[:m], bi[:m]
            return feats, scores_t, cache_val_t, cache_idx_t, feats_sk

        mm, sc_np, ext = await self._scan_pass(tools.graphs, tools.bankset1, blob, rs.args_b, rs.args_e,
                                               m, extra=pass1_extra, timed=True)
        t_d = self._tic()
        feats, scores_t, cache_val_t, cache_idx_t, feats_sk = ext or (None,) * 5
        if scores_t is not None:
            sc_np = scores_t.cpu().numpy()

        def mask(name):
            i = tools.bankset1.index.get(name)
            return mm[i] if i is not None else np.zeros(m, dtype=np.uint32)

        deny_m, harm_m, pii_m = mask("deny"), mask("harm"), mask("pii")
        regex_m, norm_m, schema_m = mask("regex"), mask("normalize"), mask("schema")

        # deny/harm raw-byte hits are VERDICT CANDIDATES, not verdicts:
        # duplicate JSON keys can place the word in a value json.loads
        # discards (last-key-wins), so a raw match is NOT ⊆ decoded match.
        # Candidates route to the host lane, whose pre-rewrite deny recheck
        # and post-rewrite harm rescan run over decoded text — exact CPU
        # semantics. Benign traffic never pays this (no hits, no routing).
        cand = (deny_m != 0) | (harm_m != 0)
        if cand.any():
            norm_m = norm_m.copy()
            norm_m[cand] |= 1
            deny_m = np.where(cand, 0, deny_m).astype(np.uint32)
            harm_m = np.where(cand, 0, harm_m).astype(np.uint32)

        mod_block = np.zeros(m, dtype=np.uint8)
        mod_cat = np.zeros(m, dtype=np.int32)
        mod_score = np.zeros(m, dtype=np.float32)
        if sc_np is not None:
            mod_score = np.ascontiguousarray(sc_np.max(axis=1).astype(np.float32))
            mod_cat = np.ascontiguousarray(sc_np.argmax(axis=1).astype(np.int32))
            mod_block = (mod_score >= self.moderation.threshold).astype(np.uint8)

        # semcache identity = tool_hash XOR user_hash (tenant-scoped)
        th_arr = np.where(tool_idx >= 0, tools.thash[np.clip(tool_idx, 0, None)] ^ rs.uh, 0)
        hit = np.zeros(m, dtype=np.uint8)
        hit_slot = np.full(m, -1, dtype=np.int32)
        if cache_val_t is not None:
            cache_val = cache_val_t.cpu().numpy()
            hit_slot = np.ascontiguousarray(cache_idx_t.cpu().numpy().astype(np.int32))
            hit = self.semcache.resolve_hits_np(cache_val, hit_slot, th_arr).astype(np.uint8)

        # breaker overlay: flip TF_BREAKER_OPEN for tools with open circuits
        flags = tools.flags
        if self.breaker is not None and self.breaker.state:
            now0 = time.monotonic()
            open_tis = [tools.index[nm] for nm, st in self.breaker.state.items()
                        if now0 < st["open_until"] and nm in tools.index]
            if open_tis:
                flags = flags.copy()
                flags[open_tis] |= hip.TF_BREAKER_OPEN

        t0 = time.monotonic()
        state, nk, reason, arena, rb, re_, _n_arena = hip.decide(
            blob, rs.id_b, rs.id_e, rs.args_b, rs.args_e, tool_idx, rs.nb, rs.ne,
            deny_m, harm_m, pii_m, regex_m, norm_m, schema_m,
            mod_block, mod_cat, mod_score, hit, hit_slot, rs.uh,
            flags, tools.required, tools.typed,
            tools.name_beg, tools.name_end, tools.name_blob, tools.native_kind,
            tools.nest_bits,
            self._deny_tab[0], self._deny_tab[1], self._harm_tab[0], self._harm_tab[1],
            self._mod_tab[0], self._mod_tab[1],
            self._slot_store, self._exact_native, time.monotonic())

        self._toc("decide", t_d)
        t_a = self._tic()
        answered = np.nonzero(state == hip.ST_ANSWERED)[0]
        if answered.size:
            # C-loop scatter (ops/csrc/pybridge.c): no arena copy, no
            # per-row Python slicing
            self._pb.scatter_slices(arena, np.ascontiguousarray(rb[answered]),
                                    np.ascontiguousarray(re_[answered]),
                                    np.ascontiguousarray(rs.rows[answered].astype(np.int64)),
                                    rs.responses)
        rc = np.bincount(reason[answered].astype(np.int64), minlength=9) if answered.size else np.zeros(9, int)
        self.blocked += int(rc[3] + rc[4] + rc[5] + rc[8])
        self.cache_hits += int(rc[6] + rc[7])

        extra_py = self._host_schema_rows(rs, np.nonzero(state == hip.ST_HOST_SCHEMA)[0], hit, hit_slot)

        # (measured: running the native batch in an executor thread to
        # overlap with the rewrite pass LOSES ~10% — GIL handoff churn across
        # every host stage — so it stays synchronous inside dispatch)
        native_js = [int(j) for j in np.nonzero(state == hip.ST_DISPATCH_NATIVE)[0]]

        # --- PASS 2: rewrite-flagged subset ---
        rewrite_js = [int(j) for j in np.nonzero(state == hip.ST_REWRITE)[0]]
        rewrite_finish = None
        if rewrite_js:
            self.slow_path += len(rewrite_js)
            t_rw = self._tic()
            rewrite_finish = await self._rewrite_pass(rs, rewrite_js, hit, hit_slot, pii_m, regex_m, norm_m)
            self._toc("rewrite_pass", t_rw)

        self._toc("answer_assign", t_a)
        py_items = [(int(j), None) for j in np.nonzero(state == hip.ST_DISPATCH_PY)[0]] + extra_py
        self.fast_path += len(native_js) + len(py_items)
        if native_js or py_items or rewrite_finish is not None:
            await self._dispatch_and_post(rs, nk, feats, th_arr, native_js, py_items, t0, feats_sk,
                                          rewrite_finish)

    def _schema_errors(self, mt: _ToolMeta, args: Any) -> List[str]:
        """The exact schema_guard check of one row's decoded arguments."""
        return _validate(args or {}, mt.tool.get("input_schema") or {})

    def _host_schema_rows(self, rs: RowSet, js, hit, hit_slot) -> List[Tuple[int, Any]]:
        """Host-schema fallback rows (exact validation) → the (row, args)
        that pass and still need dispatch."""
        extra_py: List[Tuple[int, Any]] = []
        for j in js:
            j = int(j)
            args = rs.decode_args(j)
            if args is BAD_ARGS:
                continue
            errs = self._schema_errors(rs.meta(j), args)
            if errs:
                rs.block(j, msg_schema(errs))
            elif hit[j]:
                rs.answer_cached(j, self._cache_result_bytes(int(hit_slot[j])))
            else:
                # native tools land in the nat2 C++ batch inside dispatch
                extra_py.append((j, args))
        return extra_py

    async def _a2a_fast_invoke(self, mt: _ToolMeta, args: Any) -> Dict[str, Any]:
        """A2A fast lane: handler call + the exact result shape of
        tool_service A2A dispatch wrapping invoke_agent, minus the per-row
        Python hook chain (GPU banks + pass 3 + host post cover it)."""
        message = args.get("message") if isinstance(args, dict) else None
        if not isinstance(message, str):
            message = json.dumps(args or {}, default=str)
        t0 = time.monotonic()
        reply_text = await mt.handler(message, {})
        sc = {"agent": mt.original_name, "response": reply_text,
              "latency_ms": round((time.monotonic() - t0) * 1000, 2),
              "uaid": uuid.uuid4().hex}
        return {"content": [{"type": "text", "text": reply_text}],
                "structuredContent": sc, "isError": False}

    # ---- GPU sections ----
    async def _await_gpu(self) -> None:
        """Await completion of the current stream WITHOUT
        hipDeviceSynchronize: a device-wide sync holds HIP runtime locks
        that serialize the OTHER in-flight batch's kernel launches
        (measured ~1ms/batch of launch-side stalls). An event record +
        non-blocking hipEventQuery poll yields the event loop instead."""
        ev = torch.cuda.Event()
        ev.record()
        if ev.query():
            return
        for _ in range(200000):
            await asyncio.sleep(0)
            if ev.query():
                return
        await asyncio.to_thread(ev.synchronize)

    def _rescore_submit(self, texts: List[bytes]) -> int:
        """Submit the rescan of `texts` to the native session → its slot, or
        -1 when the eager path has to run: no session, FORGE_RESCORE_NATIVE=0,
        or the submit refused (too many rows or bytes, every slot busy)."""
        sess = self._rescore
        if sess is None or os.environ.get("FORGE_RESCORE_NATIVE", "1") == "0":
            return -1
        blob, offs = self._pb.concat_with_offsets(texts)
        slot = sess.submit(blob, offs, len(texts))
        return slot if slot >= 0 else -1

    async def _rescore_collect(self, slot: int, n: int) -> np.ndarray:
        """Await the slot's scores (one poll, then yielding polls with
        _await_gpu's bound, then an off-loop wait), copy them out and release
        the slot whatever happens."""
        sess = self._rescore
        try:
            if not sess.poll(slot):
                for _ in range(200000):
                    await asyncio.sleep(0)
                    if sess.poll(slot):
                        break
                else:
                    await asyncio.to_thread(sess.wait, slot)
            return sess.scores(slot, n)
        finally:
            sess.release(slot)

    def close(self) -> None:
        """Free the native rescoring session (engine shutdown). Batches after
        this take the eager rescan."""
        sess, self._rescore = self._rescore, None
        if sess is not None:
            sess.close()

    def _upload(self, arr: np.ndarray) -> torch.Tensor:
        """Stage a host array through the pinned arena → async H2D. Safe to
        call repeatedly within one pass; reset after the pass's sync."""
        raw = arr.view(np.uint8).reshape(-1)
        n = raw.nbytes
        off = (self._pin_off + 255) & ~255
        if off + n > self._pin.numel():
            grow = max(self._pin.numel() * 2, off + n)
            self._pin = torch.empty(grow, dtype=torch.uint8, pin_memory=True)
            off = 0
        self._pin_off = off + n
        view = self._pin[off:off + n]
        view.numpy()[:] = raw
        # pow2-bucketed device alloc: per-batch byte counts vary by a few
        # KB, and exact-size allocs make the caching allocator split blocks
        # and fall into real hipMalloc on the hot path (measured ~1ms/batch
        # of launch-side stalls) — pow2 buckets recycle perfectly
        cap = 1 << max(16, (n - 1).bit_length()) if n else 1
        dev = torch.empty(cap, dtype=torch.uint8, device=self.device)[:n]
        dev.copy_(view, non_blocking=True)
        tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32,
               np.dtype(np.int64): torch.int64, np.dtype(np.float32): torch.float32}[np.dtype(arr.dtype)]
        return dev.view(tdt).reshape(arr.shape)

    async def _scan_pass(self, graphs, bankset, blob: np.ndarray, beg: np.ndarray, end: np.ndarray,
                         m: int, extra: Optional[Callable] = None, timed: bool = False):
        """One GPU section over `m` spans of `blob`, under _gpu_lock: the
        pinned arena and the stream are shared by the batches in flight, and
        a leaked lock stops the server, hence the `finally`.

        With a bucket of `graphs` for the shape the whole pass — H2D stages,
        fused scan, pass 1's featurize + classifier, D2H into pinned — is ONE
        hipGraphLaunch. Otherwise it runs eager: upload, scan_multi over
        `bankset` (every DFA bank in one launch, grid.y=bank), then
        `extra(data, beg, end)`, the caller's further launches on the same
        uploaded tensors. A `bankset` of None launches `extra` alone.

        → (uint32 mask matrix [n_banks, m] or None, the graph's classifier
        scores or None, what `extra` returned or None). `timed` brackets
        the steps with pass 1's FORGE_PIPELINE_TIMING keys."""
        toc = self._toc if timed else (lambda key, t: None)
        t_g = self._tic()
        out = scores = ext = None
        await self._gpu_lock.acquire()
        try:
            toc("gp1_lockwait", t_g)
            g = graphs.get(m, int(blob.nbytes)) if graphs is not None else None
            if g is not None:
                t_st = self._tic()
                g.stage(blob, beg, end, m)
                toc("gp1_stage", t_st)
                toc("gp1_upload", t_g)
                t_l = self._tic()
                g.replay()
                graphs.replays += 1
                toc("gp1_launch", t_l)
                t_s = self._tic()
                await self._await_gpu()
                # read under the lock: the next replay overwrites the pinned outputs
                mm = g.read_multi(m)
                scores = g.read_scores(m)
            else:
                self._pin_off = 0
                data_t = self._upload(blob)
                beg_t = self._upload(beg)
                end_t = self._upload(end)
                toc("gp1_upload", t_g)
                t_l = self._tic()
                if bankset is not None:
                    out = hip.scan_multi(data_t, beg_t, end_t, bankset)
                if extra is not None:
                    ext = extra(data_t, beg_t, end_t)
                toc("gp1_launch", t_l)
                t_s = self._tic()
                # off-loop sync: a blocking synchronize would stall the event loop
                # and starve the micro-batch collector under live HTTP load
                await self._await_gpu()
        finally:
            self._gpu_lock.release()
        toc("gp1_sync", t_s)
        if g is None:
            mm = out.cpu().numpy().view(np.uint32) if out is not None else None  # one D2H for every bank
        toc("gpu_pass1", t_g)
        return mm, scores, ext

    def _entropy_launch(self, data_t, beg_t, end_t):
        """One token_entropy launch per configured alphabet → [(outputs, threshold)]."""
        return [(hip.token_entropy(data_t, beg_t, end_t, tab, self.secrets.min_len), thr)
                for tab, thr in self._secret_tabs]

    def _entropy_flags(self, ent, n: int) -> np.ndarray:
        """Secrets prefilter over hip.token_entropy outputs, one entry per
        alphabet as ((max_h, span, n_runs, flags), threshold): a row is
        flagged when max_h >= threshold - TOL, or when its span holds a
        backslash or a non-ASCII byte (raw bytes may differ from the
        decoded strings, so only the host check is exact)."""
        out = np.zeros(n, dtype=bool)
        for (max_h, _span, _runs, flags), thr in ent:
            out |= max_h.cpu().numpy() >= np.float32(thr - ENTROPY_TOL)
            out |= (flags.cpu().numpy() & 1) != 0
        return out

    def _exfil_launch(self, data_t, beg_t, end_t):
        """One decode_scan launch per configured encoding → [(counts, kw, span, flags)]."""
        p = self.exfil
        return [hip.decode_scan(data_t, beg_t, end_t, tab, bits, p.min_len,
                                p.min_printable_permille, self._exfil_kw)
                for tab, bits in self._exfil_tabs]

    def _exfil_flags(self, dec, n: int) -> np.ndarray:
        """Encoded-exfil prefilter over hip.decode_scan outputs, one entry
        per encoding: a row is flagged when a text run holds a keyword
        (any text run when the plugin does not require one), or when its
        span holds a backslash or a non-ASCII byte. Integer outputs, equal
        to the plugin's own: nothing to round."""
        out = np.zeros(n, dtype=bool)
        for counts, _kw, _span, flags in dec:
            c = counts.cpu().numpy()
            out |= c[:, 2] > 0
            if not self.exfil.require_keyword:
                out |= c[:, 1] > 0
            out |= (flags.cpu().numpy() & 1) != 0
        return out

    def _sql_flags(self, out, n: int) -> np.ndarray:
        """SQL prefilter over hip.sql_scan outputs (boundary mode): a row is
        flagged when it holds a delete / update without where that the
        plugin blocks, a blocked word, a comment while strip_comments is on,
        or when its span holds a backslash or a non-ASCII byte. Integer
        outputs, equal to the plugin's own: nothing to round."""
        counts, blocked, _first, flags = out
        c = counts.cpu().numpy()
        res = blocked.cpu().numpy() != 0
        if self.sql.block_delete_without_where:
            res |= c[:, 1] > 0
        if self.sql.block_update_without_where:
            res |= c[:, 2] > 0
        if self.sql.strip_comments:
            res |= c[:, 3] > 0
        res |= (flags.cpu().numpy() & 1) != 0
        return res

    async def _raw_prepass(self, blob: np.ndarray, args_b: np.ndarray, args_e: np.ndarray,
                           sec_rows: Optional[np.ndarray], exf_rows: Optional[np.ndarray],
                           sql_rows: Optional[np.ndarray] = None
                           ) -> Tuple[Optional[np.ndarray], Optional[np.ndarray], Optional[np.ndarray]]:
        """secrets_detection, encoded_exfil_detection and sql_sanitizer
        prefilters over raw argument bytes → (bool[m] or None) per plugin,
        True where the row must run the exact CPU chain; `sec_rows` /
        `exf_rows` / `sql_rows` mark the rows of tools each plugin is active
        for (None: not this batch). Eager, under _gpu_lock, ONE upload for
        all: the secrets format bank (scan.hip) and one token_entropy launch
        per alphabet, one decode_scan launch per encoding, one sql_scan
        launch in boundary mode, over the union of the marked rows; every
        other row gets an empty span, and each verdict is masked with its
        own plugin's rows. The blob is uploaded here and again by pass 1 on
        purpose — folding this pre-pass into the captured pass-1 graph is a
        later change. Timed as gp0_secrets when secrets_detection takes
        part, else as gp0_exfil when encoded_exfil_detection does, as
        gp0_sql when sql_sanitizer alone does."""
        t0 = self._tic()
        m = args_b.shape[0]
        rows = np.zeros(m, dtype=bool)
        for part in (sec_rows, exf_rows, sql_rows):
            if part is not None:
                rows |= part
        sb = np.ascontiguousarray(np.where(rows, args_b, 0).astype(np.int32))
        se = np.ascontiguousarray(np.where(rows, args_e, 0).astype(np.int32))

        def launch(data_t, beg_t, end_t):
            mask_t = ent = dec = sq = None
            if sec_rows is not None:
                if "secrets" in self.banks:
                    mask_t = hip.scan(data_t, beg_t, end_t, self.banks["secrets"])[0]
                ent = self._entropy_launch(data_t, beg_t, end_t)
            if exf_rows is not None:
                dec = self._exfil_launch(data_t, beg_t, end_t)
            if sql_rows is not None:
                sq = hip.sql_scan(data_t, beg_t, end_t, self._sql_kw, self._sql_kw_len, True)
            return mask_t, ent, dec, sq

        _mm, _scores, (mask_t, ent, dec, sq) = await self._scan_pass(None, None, blob, sb, se, m, extra=launch)
        sec_flagged = exf_flagged = sql_flagged = None
        if sec_rows is not None:
            sec_flagged = self._entropy_flags(ent, m)
            if mask_t is not None:
                sec_flagged |= mask_t.cpu().numpy() != 0
            sec_flagged &= sec_rows
        if exf_rows is not None:
            exf_flagged = self._exfil_flags(dec, m) & exf_rows
        if sql_rows is not None:
            sql_flagged = self._sql_flags(sq, m) & sql_rows
        self._toc("gp0_secrets" if sec_rows is not None else "gp0_exfil" if exf_rows is not None else "gp0_sql", t0)
        return sec_flagged, exf_flagged, sql_flagged

    def _cache_result_bytes(self, slot: int) -> Optional[bytes]:
        if self._slot_store:
            res = hip.store_get(self._slot_store, slot)
            if res:
                return res
        res = self.semcache.results[slot] if self.semcache is not None else None
        if res is None:
            return None
        return res if isinstance(res, bytes) else json.dumps(res, separators=(",", ":")).encode()

    # ---- pass 2: rewrites ----
    def _apply_rewrites(self, name: str, args: Any, do_norm: bool = True,
                        do_regex: bool = True, do_pii: bool = True,
                        pii_bits: int = -1) -> Tuple[str, Any]:
        """Host rewrites in CPU-chain priority order: normalizer(15) →
        regex(20) → pii(30), using the plugins' own functions. The do_*
        flags come from the per-bank GPU masks: a bank that did not fire on
        this row means its plugin is an identity transform here (the DFA
        banks are conservative supersets of the host matchers), so it can
        be skipped without changing the outcome."""
        if do_norm and self._active(self.normalizer, name, block_class=False):
            args = _walk_strings(args, self.normalizer.norm)
        if do_regex and self._active(self.regex, name, block_class=False):
            args = _walk_strings(args, self.regex.apply_rules)
        if do_pii and self._active(self.pii, name, block_class=False):
            args, blocked_msg = self._pii_pass(args, pii_bits)
            if blocked_msg:
                return ("__block__", blocked_msg)
        return ("__ok__", args)

    def _pii_pass(self, obj: Any, pii_bits: int = -1) -> Tuple[Any, Optional[str]]:
        """pii_filter over every string of `obj` (only the patterns in
        `pii_bits` when >= 0) → (obj, masked if the action is mask; the block
        message if the action is an enforced block)."""
        found: List[str] = []

        def fn(s: str) -> str:
            masked, f = self.pii.mask_text_subset(s, pii_bits) if pii_bits >= 0 else self.pii.mask_text(s)
            found.extend(f)
            return masked

        new = _walk_strings(obj, fn)
        if found and self.pii.action == "block" and enforcing(self.pii):
            return obj, msg_pii(found)
        return (new if found and self.pii.action == "mask" else obj), None

    async def _rewrite_pass(self, rs: RowSet, rewrite_js: List[int], hit, hit_slot,
                            pii_m, regex_m, norm_m):
        """Rewrite the flagged rows (native lane, then the exact Python lane
        for the rest) and launch the moderation rescan of the rewritten texts.
        → None when every row was answered here, else `finish()`, which awaits
        the rescan and returns the surviving (row, args) dispatch items."""
        ok_items: List[Tuple[int, Any]] = []
        scan_bytes: Dict[int, bytes] = {}  # native lane: sorted-keys scan form
        harm_c: Dict[int, int] = {}        # row → harm phrase idx (post-rewrite text)
        schema_c: Dict[int, int] = {}      # row → C fast-schema verdict (1 = passed)

        py_js = self._rewrite_native(rs, rewrite_js, pii_m, regex_m, norm_m,
                                     ok_items, scan_bytes, harm_c, schema_c)
        t_sub = self._tic()
        self._rewrite_python(rs, py_js, pii_m, regex_m, norm_m, ok_items, harm_c)
        self._toc("rw_pyloop", t_sub)
        if not ok_items:
            return None
        t_sub = self._tic()

        # scan texts are the sorted-keys form (_text_of): native-lane rows
        # have it precomputed; python-lane entries serialize here
        texts2 = [scan_bytes[j] if j in scan_bytes else _sorted_json(a).encode()
                  for (j, a) in ok_items]
        # scores2_t: None, the eager path's device tensor, or the native
        # session's slot (an int)
        scores2_t = None
        if self.classifier is not None:
            slot = self._rescore_submit(texts2)
            if slot >= 0:
                scores2_t = slot
                self.rescore_native += 1
            else:
                data2, beg2, end2 = pack_texts(texts2, self.device)
                f2, _ = hip.featurize(data2, beg2, end2, self.feat_dim, pad_to=128)
                scores2_t = self.classifier.forward(f2)[: len(ok_items)]
                self.rescore_eager += 1

        self._toc("rw_launch", t_sub)
        # the rescan kernels are IN FLIGHT — the sync happens inside the
        # returned closure, which the caller awaits AFTER the big native
        # upstream batch so the GPU rescan overlaps that C++ work
        async def finish() -> List[Tuple[int, Any]]:
            return await self._finish_rewrite(rs, ok_items, harm_c, schema_c, scores2_t, hit, hit_slot)

        return finish

    def _rewrite_native(self, rs: RowSet, rewrite_js, pii_m, regex_m, norm_m,
                        ok_items, scan_bytes, harm_c, schema_c) -> List[int]:
        """Native lane (rewrite.cpp): rows with no user regexes and
        provably-equivalent content; the C side punts anything outside its
        envelope. Fills ok_items / scan_bytes / harm_c / schema_c, answers
        the rows it blocks → the rows left for the Python lane, in order."""
        tools, tool_idx = rs.tools, rs.tool_idx
        rw_regex, rw_deny, rw_harm = tools.rw_regex, tools.rw_deny, tools.rw_harm
        rw_norm, rw_pii, sk_range = tools.rw_norm, tools.rw_pii, tools.sk_range
        sg_sk = enforcing(self.schema_guard) and tools.sk_tables is not None
        t_sub = self._tic()
        nat_idx: List[int] = []
        flags_l: List[int] = []
        want_l: List[int] = []
        for j in rewrite_js:
            ti = tool_idx[j]
            if regex_m[j] and rw_regex[ti]:
                continue  # user-configured Python regexes → Python lane
            deny_needed = rw_deny[ti]
            if deny_needed and not self._deny_lane_ok:
                continue  # non-ASCII deny words → Python lane recheck
            harm_needed = rw_harm[ti]
            if harm_needed and not self._harm_lane_ok:
                continue  # non-ASCII harm phrases → Python lane
            do_norm = bool(norm_m[j]) and rw_norm[ti]
            do_pii = bool(pii_m[j]) and rw_pii[ti]
            fl = (1 if do_norm else 0) | (2 if do_pii else 0) | (4 if deny_needed else 0) | \
                (8 if harm_needed else 0)
            if sg_sk and sk_range[ti, 0] >= 0:
                fl |= 16
            if do_pii:
                bits = int(pii_m[j])
                want = 0
                for k, fixed in enumerate(self._pii_fixed):
                    if (bits >> k) & 1:
                        want |= 1 << fixed
            else:
                want = self._pii_active_mask
            nat_idx.append(j)
            flags_l.append(fl)
            want_l.append(want)
        self._toc("rw_elig", t_sub)
        t_sub = self._tic()
        py_js = rewrite_js
        if nat_idx:
            njs = np.asarray(nat_idx, dtype=np.int64)
            tis = tool_idx[njs]
            sk = tools.sk_tables
            t_call = self._tic()
            st, found, deny_hit, harm_hit, schema_ok, rw_arena, rb, re_, sb, se = hip.rewrite_rows(
                rs.blob, np.ascontiguousarray(rs.args_b[njs]), np.ascontiguousarray(rs.args_e[njs]),
                np.asarray(flags_l, dtype=np.uint8), np.asarray(want_l, dtype=np.uint32),
                self._pii_active_mask, pii_mode(self.pii),
                bool(self.normalizer and self.normalizer.collapse_ws),
                bool(self.normalizer and self.normalizer.strip),
                deny_blob=self._deny_lane_blob, deny_off=self._deny_lane_off,
                deny_ci=bool(self.deny and self.deny.case_insensitive),
                harm_blob=self._harm_lane_blob, harm_off=self._harm_lane_off,
                sk_tables=sk,
                sk_lo=np.ascontiguousarray(sk_range[tis, 0]) if sk is not None else None,
                sk_hi=np.ascontiguousarray(sk_range[tis, 1]) if sk is not None else None)
            self._toc("rw_call", t_call)
            punted: List[int] = []
            done_m = st == hip.RW_DONE
            done_ks = np.nonzero(done_m)[0]
            if done_ks.size:
                # C-loop slicing for the common path: both byte forms in
                # two bridge calls instead of 2 python slices per row
                wires = self._pb.slices_list(rw_arena, np.ascontiguousarray(rb[done_ks]),
                                             np.ascontiguousarray(re_[done_ks]))
                scans = self._pb.slices_list(rw_arena, np.ascontiguousarray(sb[done_ks]),
                                             np.ascontiguousarray(se[done_ks]))
                for q, k in enumerate(done_ks):
                    j = nat_idx[int(k)]
                    ok_items.append((j, wires[q]))
                    scan_bytes[j] = scans[q]
                    if harm_hit[k] >= 0:
                        harm_c[j] = int(harm_hit[k])
                    if schema_ok[k] != 2:
                        schema_c[j] = int(schema_ok[k])
            for k in np.nonzero(~done_m)[0]:
                j = nat_idx[int(k)]
                if st[k] == hip.RW_DENY:
                    rs.block(j, msg_deny(self.deny.words[int(deny_hit[k])]))
                elif st[k] == hip.RW_BLOCKED:
                    rs.block(j, msg_pii_bits(int(found[k])))
                else:
                    punted.append(j)
            nat_set = set(nat_idx)  # hoisted: inside the comprehension this
            # was rebuilt per element — O(n²), 31 ms/batch at 20% flagged
            py_js = [j for j in rewrite_js if j not in nat_set] + punted
            py_js.sort()
        self._toc("rw_c", t_sub)
        return py_js

    def _rewrite_python(self, rs: RowSet, py_js, pii_m, regex_m, norm_m, ok_items, harm_c) -> None:
        """Python lane: the plugins' own functions over the decoded arguments."""
        tools, tool_idx = rs.tools, rs.tool_idx
        for j in py_js:
            ti = tool_idx[j]
            args = rs.decode_args(j)
            if args is BAD_ARGS:
                continue
            # deny recheck over DECODED text, pre-rewrite (CPU chain order:
            # deny@10 before normalizer@15) — the raw-byte scan misses
            # escape-hidden words (forbidden), which is exactly what
            # routed this row here (parity-fuzz finding)
            if self.deny is not None and tools.rw_deny[ti]:
                hay = _text_of(args)
                hay = hay.lower() if self.deny.case_insensitive else hay
                word = next((w for w in self.deny.words
                             if (w.lower() if self.deny.case_insensitive else w) in hay), None)
                if word is not None:
                    rs.block(j, msg_deny(word))
                    continue
            status, payload = self._apply_rewrites(
                tools.metas[ti].name, args, do_norm=bool(norm_m[j]), do_regex=bool(regex_m[j]),
                do_pii=bool(pii_m[j]), pii_bits=int(pii_m[j]))
            if status == "__block__":
                rs.block(j, payload)
                continue
            # harmful_content@60 over the rewritten text (the CPU plugin's
            # own check; verdict ordering vs moderation happens in
            # _finish_rewrite exactly like the chain)
            if self.harm is not None and tools.rw_harm[ti]:
                hay2 = _text_of(payload).lower()
                for w, ph in enumerate(self.harm.phrases):
                    if ph.lower() in hay2:
                        harm_c[j] = w
                        break
            ok_items.append((j, payload))

    async def _finish_rewrite(self, rs: RowSet, ok_items, harm_c, schema_c, scores2_t,
                              hit, hit_slot) -> List[Tuple[int, Any]]:
        """Phase B of the rewrite pass: await the rescan verdicts of the
        rewritten texts (harm scan + moderation classifier) and emit the
        surviving (row, args) dispatch items."""
        t_sub = self._tic()
        if isinstance(scores2_t, int):
            scores2 = await self._rescore_collect(scores2_t, len(ok_items))
            self._toc("rw_sync", t_sub)
            t_sub = self._tic()
        else:
            if scores2_t is not None:
                await self._await_gpu()
            self._toc("rw_sync", t_sub)
            t_sub = self._tic()
            scores2 = scores2_t.cpu().numpy() if scores2_t is not None else None

        # hoisted gating: vectorized score reduction, per-tool applies from
        # the snapshot's arrays, id bytes only for rows that need a splice
        tools, tool_idx = rs.tools, rs.tool_idx
        mod_on = scores2 is not None and enforcing(self.moderation)
        sc_max = scores2.max(axis=1) if mod_on else None
        sc_arg = scores2.argmax(axis=1) if mod_on else None
        mod_thr = self.moderation.threshold if mod_on else 0.0
        cat_names = category_names(scores2.shape[1]) if mod_on else None
        sg_on = enforcing(self.schema_guard)
        mod_app, metas, harm_cats = tools.mod_app, tools.metas, (self.harm.cats if self.harm else [])

        out: List[Tuple[int, Any]] = []
        for jj, (j, args2) in enumerate(ok_items):
            ti = tool_idx[j]
            if mod_on and mod_app[ti] and float(sc_max[jj]) >= mod_thr:
                rs.block(j, msg_moderation(cat_names[int(sc_arg[jj])], float(sc_max[jj])))
                continue
            hj = harm_c.get(j, -1)
            if hj >= 0:   # gating applied where harm_c was computed
                rs.block(j, msg_harm(harm_cats[hj] if hj < len(harm_cats) else "?"))
                continue
            if sg_on and schema_c.get(j, 2) == 1:
                pass  # C fast-schema check passed on the rewritten tree
            elif sg_on and metas[ti].schema_mode != "trivial":
                if isinstance(args2, bytes):
                    args2 = json.loads(args2)
                errs = self._schema_errors(metas[ti], args2)
                if errs:
                    rs.block(j, msg_schema(errs))
                    continue
            if hit[j]:
                rs.answer_cached(j, self._cache_result_bytes(int(hit_slot[j])))
                continue
            out.append((j, args2))
        self._toc("rw_verdict", t_sub)
        return out

    # ---- dispatch, pass 3, finalize ----
    async def _dispatch_and_post(self, rs: RowSet, nk, feats, th_arr,
                                 native_js: List[int], py_items: List[Tuple[int, Any]],
                                 t0: float, feats_sk, rewrite_finish) -> None:
        t_u = self._tic()
        native_js, py_items, nat = self._native_upstream(rs, nk, native_js, py_items)

        # rewrite rescan verdicts: awaited here so the GPU rescan (launched
        # in _rewrite_pass) ran concurrently with the C++ native batch above
        if rewrite_finish is not None:
            t_rw2 = self._tic()
            fin_items = await rewrite_finish()
            py_items = py_items + fin_items
            self.fast_path += len(fin_items)
            self._toc("rewrite_pass", t_rw2)

        py_results, py_errors = await self._python_dispatch(rs, py_items)
        self._toc("dispatch", t_u)

        t_p = self._tic()
        all_js = list(native_js) + [j for j, _ in py_items]
        all_js_np = np.asarray(all_js, dtype=np.int64)
        n_all = len(all_js)
        res_blob, res_beg, res_end, err_rows = self._assemble(len(native_js), nat, py_results)
        needs_host, regex3 = await self._pass3(rs, all_js_np, res_blob, res_beg, res_end, err_rows)
        self._toc("post_scan", t_p)

        # --- finalize: splice every result that needs no host work (C) ---
        t_f = self._tic()
        t_fc = self._tic()
        tools = rs.tools
        arena2, rb2, re2, is_err, cacheable = hip.finalize(
            rs.blob, rs.id_b, rs.id_e, rs.args_b, rs.args_e, rs.tool_idx, rs.uh,
            np.ascontiguousarray(all_js_np.astype(np.int32)), res_blob, res_beg, res_end,
            np.ascontiguousarray(needs_host.astype(np.uint8)),
            tools.name_beg, tools.name_end, tools.name_blob, tools.flags,
            self._exact_native, time.monotonic(), self.exact_cache.ttl if self.exact_cache else 0.0)
        if n_all:
            self._pb.scatter_slices(arena2, rb2, re2,
                                    np.ascontiguousarray(rs.rows[all_js_np].astype(np.int64)),
                                    rs.responses)
        self._toc("fin_splice", t_fc)

        t_fh = self._tic()
        host_cached = self._host_post_rows(rs, all_js, all_js_np, np.nonzero(needs_host)[0], regex3,
                                           res_blob, res_beg, res_end, err_rows, py_errors,
                                           len(native_js), is_err, cacheable)
        self._toc("fin_hostpost", t_fh)
        self._bookkeeping(rs, all_js_np, res_blob, res_beg, res_end, is_err, cacheable,
                          host_cached, feats, feats_sk, th_arr, t0)
        self._toc("finalize", t_f)

    def _native_upstream(self, rs: RowSet, nk, native_js: List[int], py_items):
        """Native upstream batch (C++) → (native_js, py_items, (blob, beg,
        end)): rows the C++ side punted move from native_js to py_items."""
        nat_blob = np.zeros(0, dtype=np.uint8)
        nat_beg = nat_end = np.zeros(0, dtype=np.int64)
        if native_js:
            njs = np.asarray(native_js, dtype=np.int64)
            kinds = np.ascontiguousarray(nk[njs].astype(np.int32))
            nb_ = np.ascontiguousarray(rs.args_b[njs])
            ne_ = np.ascontiguousarray(rs.args_e[njs])
            nb_ = np.where(ne_ > nb_, nb_, -1).astype(np.int32)
            nat_blob, nat_beg, nat_end = hip.upstream_call_batch(rs.blob, nb_, ne_, kinds, _now_iso())
            # empty spans = C++ punted a non-canonical args span (escapes,
            # floats, whitespace formatting); answer those rows on the exact
            # Python path so results match the CPU reference byte-for-byte
            punted = np.nonzero((nat_end == nat_beg) & (nb_ >= 0))[0]
            if punted.size:
                pm = set(int(x) for x in punted)
                py_items = py_items + [(native_js[i], None) for i in pm]
                served = np.ones(len(native_js), dtype=bool)
                served[list(pm)] = False
                native_js = [j for i, j in enumerate(native_js) if i not in pm]
                nat_beg = np.ascontiguousarray(nat_beg[served])
                nat_end = np.ascontiguousarray(nat_end[served])
        return native_js, py_items, (nat_blob, nat_beg, nat_end)

    async def _python_dispatch(self, rs: RowSet, py_items):
        """Python dispatch (non-native upstreams / rewritten args) →
        (serialized result or None per item, {item index: exception})."""
        py_results: List[Optional[bytes]] = [None] * len(py_items)
        py_errors: Dict[int, Exception] = {}
        if not py_items:
            return py_results, py_errors
        ts = self.engine.tool_service

        async def one(idx: int, j: int, args2: Any) -> None:
            mt = rs.meta(j)
            args = args2
            if args is None:
                try:
                    args = rs.parse_args(j)
                except Exception:
                    py_errors[idx] = jsonrpc.JSONRPCError(jsonrpc.INVALID_PARAMS, INVALID_ARGS)
                    return
            elif isinstance(args, bytes):  # native rewrite-lane output
                args = json.loads(args)
            try:
                if mt.a2a_fast:
                    result = await self._a2a_fast_invoke(mt, args)
                else:
                    result = await ts.dispatch(mt.tool, args)
                py_results[idx] = _wire_json(result)
            except Exception as exc:
                py_errors[idx] = exc

        seq, conc, nat2 = [], [], []
        for idx, (j, args2) in enumerate(py_items):
            mt = rs.meta(j)
            if mt.native_kind >= 0 and args2 is not None:
                # rewritten args for a native tool: batch through the C++
                # upstream instead of per-request Python dispatch (the
                # native rewrite lane already produced canonical bytes)
                nat2.append((idx, args2 if isinstance(args2, bytes) else _wire_json(args2),
                             mt.native_kind))
            elif (mt.itype == "LOCAL" and not (mt.tool.get("annotations") or {}).get("io")) \
                    or mt.a2a_fast \
                    or isinstance(mt.client, InProcUpstream) or mt.native_kind >= 0:
                # pure in-proc handlers: sequential await beats gather
                # overhead; IO-backed LOCAL tools (annotations.io, e.g.
                # gRPC-translated methods) need real concurrency
                seq.append((idx, j, args2))
            else:
                conc.append((idx, j, args2))
        if nat2:
            blob2, offs2 = pack_strtable(a for _, a, _ in nat2)
            kinds2 = np.fromiter((k for _, _, k in nat2), dtype=np.int32, count=len(nat2))
            ob2, ob2b, ob2e = hip.upstream_call_batch(
                blob2, np.ascontiguousarray(offs2[:-1]), np.ascontiguousarray(offs2[1:]),
                kinds2, _now_iso())
            outs2 = self._pb.slices_list(ob2, ob2b, ob2e)
            for (idx, _a, _k), rbytes in zip(nat2, outs2):
                if rbytes:
                    py_results[idx] = rbytes
                else:
                    # canonical-gate punt on the redispatch too → exact path
                    seq.append((idx, py_items[idx][0], py_items[idx][1]))
        for idx, j, args2 in seq:
            await one(idx, j, args2)
        if conc:
            await asyncio.gather(*(one(idx, j, a) for idx, j, a in conc))
        return py_results, py_errors

    def _assemble(self, n_native: int, nat, py_results):
        """One result blob (native results + python results) → (blob, beg,
        end, err_rows); an item with no result has an empty span and err 1."""
        nat_blob, nat_beg, nat_end = nat
        n_all = n_native + len(py_results)
        nat_used = int(nat_end[-1]) if n_native else 0
        py_blob = b"".join(r or b"" for r in py_results)
        res_blob = np.concatenate([nat_blob[:nat_used],
                                   np.frombuffer(py_blob, dtype=np.uint8)]) if py_blob else \
            np.ascontiguousarray(nat_blob[:nat_used])
        if res_blob.size == 0:
            res_blob = np.zeros(1, dtype=np.uint8)
        res_beg = np.zeros(n_all, dtype=np.int64)
        res_end = np.zeros(n_all, dtype=np.int64)
        res_beg[:n_native] = nat_beg
        res_end[:n_native] = nat_end
        off = nat_used
        err_rows = np.zeros(n_all, dtype=np.uint8)
        for idx, r in enumerate(py_results):
            k = n_native + idx
            if r is not None:
                res_beg[k] = off
                off += len(r)
                res_end[k] = off
            else:
                err_rows[k] = 1
        return res_blob, res_beg, res_end, err_rows

    async def _pass3(self, rs: RowSet, all_js_np, res_blob, res_beg, res_end, err_rows):
        """PASS 3: GPU scans over serialized results → (needs_host, regex3):
        which results need the host post chain, and which hit the regex bank."""
        n_all = all_js_np.shape[0]
        tools = rs.tools
        post_flag = np.zeros(n_all, dtype=bool)
        toon_meta = np.zeros(n_all, dtype=bool)
        regex3 = np.zeros(n_all, dtype=bool)
        sec3 = None  # secrets prefilter verdict per result (secrets-active tools only)
        exf3 = None  # encoded-exfil prefilter verdict per result (exfil-active tools only)
        if n_all:
            def pass3_extra(data_t, beg_t, end_t):
                return (self._entropy_launch(data_t, beg_t, end_t) if self.secrets is not None else None,
                        self._exfil_launch(data_t, beg_t, end_t) if self.exfil is not None else None)

            mm3, _scores, ext3 = await self._scan_pass(
                self._graphs3, self._bankset3, res_blob,
                res_beg.astype(np.int32), res_end.astype(np.int32), n_all,
                extra=pass3_extra if self._graphs3 is None else None)
            ent3, dec3 = ext3 or (None, None)
            if self.secrets is not None and tools.secrets is not None:
                sec3 = self._entropy_flags(ent3, n_all)
                if "secrets" in self._bankset3.index:
                    sec3 |= mm3[self._bankset3.index["secrets"]] != 0
                sec3 &= tools.secrets[np.clip(rs.tool_idx[all_js_np], 0, None)]
            if self.exfil is not None and tools.exfil is not None:
                exf3 = self._exfil_flags(dec3, n_all) & tools.exfil[np.clip(rs.tool_idx[all_js_np], 0, None)]
            for b, i in self._bankset3.index.items():
                h = mm3[i] != 0
                if b == "postmeta":
                    toon_meta = h
                else:
                    if b == "regex":
                        regex3 = h
                    post_flag |= h

        res_len = res_end - res_beg
        toon_min = self.toon.min_size if self.toon is not None else 1 << 60
        guard_max = self.out_guard.max_chars if self.out_guard is not None else 1 << 60
        outschema = tools.outschema[np.clip(rs.tool_idx[all_js_np], 0, None)] if n_all else np.zeros(0, bool)
        needs_host = post_flag | outschema | (toon_meta & (res_len >= toon_min)) | \
            (res_len > guard_max) | err_rows.astype(bool)
        if sec3 is not None:
            needs_host = needs_host | sec3
        if exf3 is not None:
            needs_host = needs_host | exf3
        return needs_host, regex3

    def _host_post_rows(self, rs: RowSet, all_js, all_js_np, host_ks, regex3, res_blob, res_beg, res_end,
                        err_rows, py_errors, n_native: int, is_err, cacheable) -> List[Tuple[int, bytes]]:
        """Host post chain for flagged results; updates is_err / cacheable in
        place → [(k, result bytes)] of host-modified results, for the cache."""
        host_cached: List[Tuple[int, bytes]] = []
        if not host_ks.size:
            return host_cached
        tools, tool_idx = rs.tools, rs.tool_idx
        # native POST lane (rewrite.cpp forge_post_rows): pii → harm → toon
        # → serialize in C for eligible rows; punts fall through to the
        # exact Python _host_post below
        c_handled: set = set()
        pl = tools.postlane
        res_len = res_end - res_beg
        guard_max = self.out_guard.max_chars if self.out_guard is not None else 1 << 60
        nat_ks = [int(k) for k in host_ks
                  if not err_rows[k]
                  and pl[tool_idx[all_js[int(k)]]] >= 0
                  and not (pl[tool_idx[all_js[int(k)]]] & 8 and regex3[int(k)])
                  and res_len[int(k)] <= guard_max]
        if nat_ks:
            nk_np = np.asarray(nat_ks, dtype=np.int64)
            st_p, found_p, harm_p, iserr_p, p_arena, pb, pe = hip.post_rows(
                res_blob,
                np.ascontiguousarray(res_beg[nk_np].astype(np.int64)),
                np.ascontiguousarray(res_end[nk_np].astype(np.int64)),
                np.ascontiguousarray((pl[tool_idx[all_js_np[nk_np]]] & 7).astype(np.uint8)),
                self._pii_active_mask, pii_mode(self.pii),
                harm_blob=self._harm_lane_blob, harm_off=self._harm_lane_off,
                toon_min_size=self.toon.min_size if self.toon is not None else (1 << 60),
                toon_min_savings=self.toon.min_savings if self.toon is not None else 1.0)
            for q, k in enumerate(nat_ks):
                j = all_js[k]
                if st_p[q] == hip.RW_DONE:
                    rbytes = p_arena[pb[q]:pe[q]].tobytes()
                    rs.result(j, rbytes)
                    if iserr_p[q]:
                        is_err[k] = 1
                    else:
                        is_err[k] = 0
                        cacheable[k] = 1
                        host_cached.append((k, rbytes))
                elif st_p[q] == hip.RW_BLOCKED:
                    rs.block(j, msg_pii_bits(int(found_p[q])))
                    is_err[k] = 1
                elif st_p[q] == hip.RW_DENY:
                    rs.block(j, msg_harm(self.harm.cats[int(harm_p[q])]))
                    is_err[k] = 1
                else:
                    continue  # PUNT/BADJSON → python loop below
                self.post_rewrites += 1
                c_handled.add(k)
            self.post_c += len(c_handled)
            self.post_c_punt += len(nat_ks) - len(c_handled)

        for k in host_ks:
            k = int(k)
            if k in c_handled:
                continue
            j = all_js[k]
            if err_rows[k]:
                exc = py_errors.get(k - n_native)
                code = getattr(exc, "code", jsonrpc.SERVER_ERROR)
                rs.error(j, code if isinstance(code, int) else jsonrpc.SERVER_ERROR, str(exc))
                is_err[k] = 1
                continue
            rbytes = res_blob[res_beg[k]:res_end[k]].tobytes()
            rbytes, host_err, blocked_msg = self._host_post(rs.meta(j), rbytes)
            if blocked_msg:
                rs.block(j, blocked_msg)
                is_err[k] = 1
                continue
            is_err[k] = 1 if host_err else 0
            rs.result(j, rbytes)
            if not host_err:
                cacheable[k] = 1
                host_cached.append((k, rbytes))
        return host_cached

    def _bookkeeping(self, rs: RowSet, all_js_np, res_blob, res_beg, res_end, is_err, cacheable,
                     host_cached, feats, feats_sk, th_arr, t0: float) -> None:
        """Semcache insert, breaker, metrics for the dispatched rows."""
        tools = rs.tools
        tis = rs.tool_idx[all_js_np]
        t_fs = self._tic()
        if self.semcache is not None and tis.size:
            # only allowlisted tools are inserted (cacheable_tools gate);
            # that also gates lookups implicitly — a non-allowlisted tool's
            # (tool,user) identity never exists in the cache
            ins = np.nonzero((cacheable == 1) & tools.semallow[np.clip(tis, 0, None)])[0]
            if ins.size:
                ins_js = all_js_np[ins]
                slots = self.semcache.assign_slots(int(ins.size))
                self.semcache.insert_features(feats, ins_js, slots, th_arr[ins_js], sketch=feats_sk)
                if self._slot_store:
                    hip.store_put_batch(self._slot_store, slots, res_blob,
                                        np.ascontiguousarray(res_beg[ins]),
                                        np.ascontiguousarray(res_end[ins]))
                    for (k, rbytes) in host_cached:  # host-modified results overwrite
                        pos = np.nonzero(ins == k)[0]
                        if pos.size:
                            hip.store_put(self._slot_store, int(slots[pos[0]]), rbytes)
        self._toc("fin_seminsert", t_fs)

        t_fm = self._tic()
        if not tis.size:
            return self._toc("fin_metrics", t_fm)
        ms = (time.monotonic() - t0) * 1000.0
        nt = len(tools.metas)
        counts_all = np.bincount(tis, minlength=nt)
        errs_all = np.bincount(tis, weights=is_err.astype(np.float64), minlength=nt).astype(np.int64)
        uniq = np.nonzero(counts_all)[0]
        counts = counts_all[uniq]
        errs = errs_all[uniq]
        if self.breaker is not None:
            # breaker bookkeeping only where it can change state: tools with
            # errors this batch, or tools that already have a window/state
            for k, ti in enumerate(uniq):
                name = tools.names[int(ti)]
                if errs[k] or name in self.breaker.state:
                    self._breaker_record_bulk(name, int(counts[k]), int(errs[k]))
        self.engine.metrics.record_aggregate_many(
            [tools.tids[int(ti)] for ti in uniq], counts, errs, ms)
        self._toc("fin_metrics", t_fm)

    def _breaker_record_bulk(self, name: str, n: int, n_err: int) -> None:
        b = self.breaker
        st = b._st(name)
        st["results"].extend([True] * n_err + [False] * (n - n_err))
        if len(st["results"]) > b.window:
            st["results"] = st["results"][-b.window:]
        if len(st["results"]) >= b.window and (sum(st["results"]) / len(st["results"])) >= b.error_threshold:
            st["open_until"] = time.monotonic() + b.cooldown
            st["results"] = []

    def _host_post(self, mt: _ToolMeta, rb: bytes) -> Tuple[bytes, bool, Optional[str]]:
        """Exact host post chain for flagged results: secrets(5) → exfil(6) → regex(20) → pii(30) →
        output-schema → harm(60) → toon(900) → guard(950)."""
        self.post_rewrites += 1
        try:
            result = json.loads(rb)
        except Exception:
            return rb, True, None
        name = mt.name
        if self._active(self.secrets, name, block_class=False):
            # secrets_detection(5) first, as the plugin's hook plus the
            # manager's mode handling would: an enforce-mode block ends the
            # chain, a permissive one is only logged, redact always rewrites.
            # (Like the rewriters below it sees the upstream result; the
            # CPU chain checks an output schema before its post hooks, so a
            # result that violates one is scanned here and not there.)
            new, findings = self.secrets.scan_payload(result)
            reason = self.secrets.block_reason(findings)
            if reason is not None and self.engine.plugins.effective_mode(self.secrets, name) in (
                    PluginMode.ENFORCE, PluginMode.ENFORCE_IGNORE_ERROR):
                return rb, True, f"secrets_detection: {reason}"
            if findings and self.secrets.action == "redact":
                result = new
        if self._active(self.exfil, name, block_class=False):
            # encoded_exfil_detection(6) next, with the same mode handling
            new, findings = self.exfil.scan_payload(result)
            reason = self.exfil.block_reason(findings)
            if reason is not None and self.engine.plugins.effective_mode(self.exfil, name) in (
                    PluginMode.ENFORCE, PluginMode.ENFORCE_IGNORE_ERROR):
                return rb, True, f"encoded_exfil_detection: {reason}"
            if findings and self.exfil.action == "redact":
                result = new
        if self._active(self.regex, name, block_class=False):
            result = _walk_strings(result, self.regex.apply_rules)
        if self._active(self.pii, name, block_class=False):
            result, blocked_msg = self._pii_pass(result)
            if blocked_msg:
                return rb, True, blocked_msg
        if mt.has_output_schema and isinstance(result, dict):
            payload = result.get("structuredContent", result)
            errs = _validate(payload, mt.tool.get("output_schema") or {})
            if errs:
                result = {"content": [{"type": "text", "text": "output schema violation: " + "; ".join(errs[:3])}],
                          "isError": True}
        if enforcing(self.harm) and applies(self.harm, name):
            hay = _sorted_json(result).lower()
            for phrase, cat in zip(self.harm.phrases, self.harm.cats):
                if phrase.lower() in hay:
                    return rb, True, msg_harm(cat)
        if self.toon is not None and applies(self.toon, name) and isinstance(result, dict):
            new = self.toon.encode_result(result)
            if new is not None:
                result = new
        if self.out_guard is not None and isinstance(result, dict):
            total = sum(len(c.get("text", "")) for c in result.get("content", []) if isinstance(c, dict))
            if total > self.out_guard.max_chars and self.out_guard.action == "truncate":
                result = dict(result)
                result["content"] = [
                    {**c, "text": c["text"][: self.out_guard.max_chars]}
                    if isinstance(c, dict) and isinstance(c.get("text"), str) else c
                    for c in result.get("content", [])
                ]
        is_err = bool(isinstance(result, dict) and result.get("isError"))
        return _wire_json(result), is_err, None

    def stats(self) -> Dict[str, Any]:
        out = {
            "timing_s": {k: round(v, 4) for k, v in self.timing.items()} if self.timing_enabled else None,
            "batches": self.batches, "requests": self.requests, "fast_path": self.fast_path,
            "slow_path": self.slow_path, "blocked": self.blocked, "cache_hits": self.cache_hits,
            "host_bound": self.host_bound, "secrets_routed": self.secrets_routed,
            "exfil_routed": self.exfil_routed,
            "sql_routed": self.sql_routed,
            "post_rewrites": self.post_rewrites, "post_c": self.post_c,
            "post_c_punt": self.post_c_punt, "py_fallback": self.py_fallback,
            "rescore_native": self.rescore_native, "rescore_eager": self.rescore_eager,
            "banks": {k: {"states": v.n_states, "classes": v.n_classes} for k, v in self.banks.items()},
        }
        if self.semcache is not None:
            out["semcache"] = self.semcache.stats()
        return out
