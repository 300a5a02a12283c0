"""ToolTable: the GPU pipeline's per-tool tables, as one snapshot.

Built for one (registry generation, plugins version) and never changed
afterwards. A batch reads `GpuPluginPipeline._tools` once and hands that
object to every later stage, so a registry or plugin change that lands while
the batch is suspended (the lock, the GPU sync, upstream dispatch) gives the
NEXT batch a new table and leaves this one's `tool_idx` indexing the tables
it was resolved against. `tool_flags` needs no device
(tests/test_tooltable.py checks its rules on the CPU).
"""

from __future__ import annotations

from typing import Any, Dict, Iterable, List, Optional, Tuple

import numpy as np

from ..ops import dfa, hip
from ..plugins.framework import HookType, PluginContext, PluginMode
from .semcache import tool_hash

_SCHEMA_NEST_PATTERNS = [":\\{", ":\\["]

_TYPED_PAT = {
    "string": '"{k}":"',
    "number": '"{k}":[0-9\\-]',
    "integer": '"{k}":[0-9\\-]',
    "boolean": '"{k}":[tf]',
    "array": '"{k}":\\[',
}

_TYPE_CODE = {"string": 1, "integer": 2, "boolean": 3, "array": 4, "object": 5, "null": 6}

# plugins the fast path MODELS (as GPU banks, post-chain stages or decision
# flags). Any OTHER tool-hooked plugin in the chain (header_injector, an
# external-process plugin, a user plugin) routes its tools to the exact
# host chain — correctness by construction, never a silently skipped hook.
_HANDLES = {"deny": "deny_filter", "harm": "harmful_content_detector", "pii": "pii_filter",
            "regex": "regex_filter", "normalizer": "argument_normalizer",
            "moderation": "content_moderation", "semcache_plugin": "response_cache_by_prompt",
            "schema_guard": "schema_guard", "toon": "toon_encoder",
            "out_guard": "output_length_guard", "exact_cache": "cached_tool_result",
            "breaker": "circuit_breaker", "secrets": "secrets_detection",
            "exfil": "encoded_exfil_detection", "sql": "sql_sanitizer"}
MODELED = frozenset(_HANDLES.values())


class PluginHandles:
    """The modeled plugins of one manager, `None` where absent or disabled."""

    __slots__ = tuple(_HANDLES)

    def __init__(self, mgr):
        for attr, name in _HANDLES.items():
            p = mgr.get(name)
            setattr(self, attr, p if p is not None and p.mode != PluginMode.DISABLED else None)


def enforcing(plugin) -> bool:
    return plugin is not None and plugin.mode in (PluginMode.ENFORCE, PluginMode.ENFORCE_IGNORE_ERROR)


def applies(plugin, name: str) -> bool:
    return plugin is not None and (not plugin.conditions or plugin.applies_to(
        PluginContext(hook=HookType.TOOL_PRE_INVOKE, name=name)))


def active(mgr, plugin, tool_name: str, block_class: bool) -> bool:
    """Per-tool effective activation of a GPU bank: a plugin binding may
    flip the mode for this tool (reference: tool_plugin_bindings).
    block_class banks (deny/harm/moderation/schema) only fire in enforce
    modes; rewrite banks (pii/regex/normalize) fire unless disabled."""
    if plugin is None:
        return False
    mode = mgr.effective_mode(plugin, tool_name)
    if mode == PluginMode.DISABLED or (block_class and mode == PluginMode.PERMISSIVE):
        return False
    return applies(plugin, tool_name)


def pii_mode(pii) -> int:
    """forge_rewrite_rows / forge_post_rows pii mode: 0 mask, 1 block, 2 report only."""
    if pii is not None and pii.action == "block" and enforcing(pii):
        return 1
    if pii is not None and pii.action not in ("mask",):
        return 2
    return 0


def pack_strtable(items: Iterable[Any]) -> Tuple[np.ndarray, np.ndarray]:
    """str/bytes items → (joined uint8 blob, int32 offsets of len + 1); an
    empty blob is one zero byte so its pointer is always valid."""
    enc = [x.encode() if isinstance(x, str) else bytes(x) for x in items]
    off = np.zeros(len(enc) + 1, dtype=np.int32)
    np.cumsum(np.fromiter(map(len, enc), dtype=np.int32, count=len(enc)), out=off[1:])
    blob = b"".join(enc)
    return (np.frombuffer(blob, dtype=np.uint8).copy() if blob else np.zeros(1, dtype=np.uint8)), off


class _ToolMeta:
    __slots__ = ("tool", "name", "tid", "itype", "thash", "native_kind", "native_client",
                 "client", "handler", "schema_mode", "required_bits", "typed_pairs",
                 "has_output_schema", "original_name", "reachable", "host_chain", "a2a_fast")

    def __init__(self):
        self.schema_mode = "host"   # "trivial" | "fast" | "host"
        self.required_bits = 0
        self.typed_pairs: List[Tuple[int, int]] = []
        self.native_kind = -1
        self.native_client = self.client = self.handler = None
        self.has_output_schema = False
        self.host_chain = False     # per-tool plugin binding forces the CPU chain
        self.a2a_fast = False       # in-proc agent, hooks fully GPU-covered


class ToolTable:
    """One registry/plugin generation's tables. Arrays are indexed by the
    `tool_idx` that `toolmap` resolves; with no tools they hold one dummy
    entry. `hostbound`, `secrets`, `exfil`, `sql`, `sk_tables`, `schema_bank` and
    `graphs` are None where absent."""

    __slots__ = ("generation", "plugins_ver", "metas", "by_name", "index", "names", "tids",
                 "schema_bank", "nest_bits", "bankset1", "graphs", "toolmap",
                 "name_blob", "name_beg", "name_end", "required", "typed", "native_kind",
                 "outschema", "thash", "semallow",
                 "flags", "postlane", "hostbound", "secrets", "exfil", "sql",
                 "rw_norm", "rw_regex", "rw_deny", "rw_pii", "rw_harm", "mod_app",
                 "sk_tables", "sk_range")


# ---- per-tool meta ----
def _esc_key(k: str) -> Optional[str]:
    return k if k and all(c.isalnum() or c == "_" for c in k) else None


def _pattern_id(pat_ids: Dict[str, int], pat: str) -> int:
    return pat_ids.setdefault(pat, len(pat_ids))


def _compile_tool_schema(meta: _ToolMeta, schema: Optional[dict], schema_guard,
                         pat_ids: Dict[str, int]) -> None:
    """Flat object schemas compile to presence/type byte patterns scanned
    on-GPU; anything richer falls back to host validation (exact)."""
    schema = schema or {}
    props = schema.get("properties") or {}
    required = schema.get("required") or []
    rich = schema.get("additionalProperties") is False or schema.get("anyOf") or \
        schema.get("allOf") or schema.get("oneOf")
    if schema_guard is None or not (props or required or rich):
        meta.schema_mode = "trivial"
        return
    if rich:
        meta.schema_mode = "host"
        return
    req_bits = 0
    pairs: List[Tuple[int, int]] = []
    for k, sub in props.items():
        ek = _esc_key(k)
        ty = sub.get("type") if isinstance(sub, dict) else None
        extra = isinstance(sub, dict) and any(
            c in sub for c in ("enum", "const", "pattern", "minimum", "maximum", "minLength",
                               "maxLength", "minItems", "maxItems", "properties", "items",
                               "anyOf", "allOf", "oneOf", "exclusiveMinimum", "exclusiveMaximum"))
        if ek is None or extra or (ty is not None and not isinstance(ty, str)) or \
           (ty is not None and ty not in _TYPED_PAT and ty not in ("object", "null")):
            meta.schema_mode = "host"
            return
        present = _pattern_id(pat_ids, f'"{ek}":')
        if ty in _TYPED_PAT:
            typed = _pattern_id(pat_ids, _TYPED_PAT[ty].format(k=ek))
            pairs.append((present, typed))
        if k in required:
            req_bits |= 1 << present
    for k in required:
        if k not in props:
            ek = _esc_key(k)
            if ek is None:
                meta.schema_mode = "host"
                return
            req_bits |= 1 << _pattern_id(pat_ids, f'"{ek}":')
    if len(pat_ids) > 30 - len(_SCHEMA_NEST_PATTERNS):
        meta.schema_mode = "host"
        return
    meta.schema_mode = "fast"
    meta.required_bits = req_bits
    meta.typed_pairs = pairs


def _a2a_fast_handler(engine, h: PluginHandles, m: _ToolMeta):
    """A2A fast lane (BASELINE config 4): an in-proc agent whose agent-hook
    plugins are ALL GPU-covered banks with no conditions/bindings can skip
    the per-row Python hook chain — the decide pass applied the same
    deny/harm/moderation blocks over the same text (args dict incl. the
    message wrapper), and pass 3 + the host post chain cover the
    response-side pii/regex/harm hooks. → the agent's handler, or None."""
    a2a = getattr(engine, "a2a_service", None)
    agent = engine.registry.find("a2a_agent", m.original_name)
    handler = a2a._local_handlers.get(m.original_name) if a2a else None
    if agent is None or not agent.get("enabled", True) or handler is None \
            or not str(agent.get("endpoint_url", "")).startswith("inproc://"):
        return None
    agent_hooks = (HookType.AGENT_PRE_INVOKE, HookType.AGENT_POST_INVOKE)
    hooked = [p for p in engine.plugins.plugins
              if p.mode != PluginMode.DISABLED and any(k in p.hooks for k in agent_hooks)]
    bank_set = {p.name for p in (h.deny, h.pii, h.regex, h.normalizer, h.moderation, h.harm)
                if p is not None}
    if any(p.conditions for p in hooked) or not {p.name for p in hooked} <= bank_set \
            or engine.plugins.bindings_for_tool(m.original_name):
        return None
    return handler


def per_tool_meta(engine, h: PluginHandles) -> Tuple[List[_ToolMeta], Dict[str, int]]:
    """→ (one _ToolMeta per enabled tool in Registry.list order, the
    schema-shape pattern ids their "fast" schemas refer to)."""
    from ..services.upstream import NativeInProcUpstream

    ts = engine.tool_service
    by_name: Dict[str, _ToolMeta] = {}
    pat_ids: Dict[str, int] = {}
    for tool in engine.registry.list("tool", include_disabled=False):
        m = _ToolMeta()
        m.tool = tool
        m.name = tool["name"]
        m.tid = tool.get("id", m.name)
        m.itype = tool.get("integration_type", "MCP")
        m.thash = tool_hash(m.name)
        m.original_name = tool.get("original_name", m.name)
        m.has_output_schema = bool(tool.get("output_schema"))
        m.reachable = tool.get("reachable", True)
        if m.itype == "LOCAL":
            m.handler = ts._local_handlers.get(m.name)
        elif m.itype == "A2A":
            handler = _a2a_fast_handler(engine, h, m)
            if handler is not None:
                m.a2a_fast = True
                m.handler = handler
        elif m.itype == "MCP":
            m.client = ts._upstreams.get(tool.get("gateway_id") or "")
            if isinstance(m.client, NativeInProcUpstream):
                m.native_kind = m.client.TOOL_KINDS.get(m.original_name, -1)
                m.native_client = m.client
        _compile_tool_schema(m, tool.get("input_schema"), h.schema_guard, pat_ids)
        by_name[m.name] = m   # a repeated name keeps its first position, last entry
    return list(by_name.values()), pat_ids


# ---- schema bank ----
def schema_bank(metas: List[_ToolMeta], pat_ids: Dict[str, int], schema_guard, device):
    """→ (DeviceScanTables or None, nest_bits). Tools whose patterns do not
    fit a DFA fall back to host validation."""
    pats = list(pat_ids.keys())
    if not pats or schema_guard is None:
        return None, 0
    nest_bits = sum(1 << (len(pats) + i) for i in range(len(_SCHEMA_NEST_PATTERNS)))
    try:
        bank = hip.DeviceScanTables(
            dfa.compile_patterns(pats + _SCHEMA_NEST_PATTERNS, case_insensitive=False), device)
    except ValueError:
        bank = None
        for m in metas:
            if m.schema_mode == "fast":
                m.schema_mode = "host"
    return bank, nest_bits


# ---- flat arrays for the native decision plane (fastpath.cpp) ----
def flat_arrays(t: ToolTable, metas: List[_ToolMeta]) -> None:
    nt = len(metas)

    def arr(values, dtype):
        return np.array(values, dtype=dtype) if nt else np.zeros(1, dtype=dtype)

    t.metas = metas
    t.by_name = {m.name: m for m in metas}
    t.index = {m.name: i for i, m in enumerate(metas)}
    t.names = [m.name for m in metas]
    t.tids = [m.tid for m in metas]
    t.name_blob, off = pack_strtable(t.names)
    t.name_beg = np.ascontiguousarray(off[:-1])
    t.name_end = np.ascontiguousarray(off[1:])
    t.toolmap = hip.toolmap_new(t.name_blob, t.name_beg, t.name_end) if nt else 0
    t.required = arr([m.required_bits for m in metas], np.uint32)
    typed = np.full(max(nt, 1), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    for i, m in enumerate(metas):   # up to four (present, typed) pattern-id pairs, 0xFFFF = none
        pk = [(a << 8) | b for a, b in m.typed_pairs[:4]] + [0xFFFF] * 4
        typed[i] = sum(pk[k] << (k * 16) for k in range(4))
    t.typed = typed
    t.native_kind = arr([m.native_kind for m in metas], np.int8)
    t.outschema = arr([m.has_output_schema for m in metas], bool)
    t.thash = arr([m.thash for m in metas], np.int64)


# ---- flags and post lane ----
def tool_flags(t: ToolTable, metas: List[_ToolMeta], mgr, h: PluginHandles, bank_names,
               semcache_on: bool, harm_lane_ok: bool) -> None:
    """Per-tool plugin activation. Per-tool bindings: mode flips for the bank
    plugins map onto the flag bits; config overrides or bindings on non-bank
    plugins force the full CPU chain for that tool (correctness over speed).
    `bank_names` are the content banks that exist (only "regex" is asked)."""
    n1 = max(len(metas), 1)
    modeled_banks = {p.name for p in (h.deny, h.pii, h.regex, h.normalizer, h.moderation, h.harm,
                                      h.schema_guard, h.secrets, h.exfil, h.sql) if p is not None}
    extra_chain = [p for p in mgr.plugins
                   if p.mode != PluginMode.DISABLED and p.name not in MODELED
                   and (HookType.TOOL_PRE_INVOKE in p.hooks or HookType.TOOL_POST_INVOKE in p.hooks)]
    flags = np.zeros(n1, dtype=np.uint32)
    hostbound = np.zeros(n1, dtype=bool)
    postlane = np.full(n1, -1, dtype=np.int8)
    # rewrite/verdict lane per-tool activation (hoists the per-row
    # active/applies python calls out of the hot loops)
    (t.rw_norm, t.rw_regex, t.rw_deny, t.rw_pii, t.rw_harm, t.mod_app, sec_act, exf_act, sql_act,
     t.semallow) = (np.zeros(n1, dtype=bool) for _ in range(10))
    for i, m in enumerate(metas):
        name = m.name
        m.host_chain = any(b.get("config") or (pname not in modeled_banks)
                           for pname, b in mgr.bindings_for_tool(name).items())
        # unmodeled tool-hooked plugins (external-process, custom) that
        # apply to this tool force the exact host chain for it
        if not m.host_chain and extra_chain:
            m.host_chain = any(applies(p, name) for p in extra_chain)
        hostbound[i] = m.host_chain
        deny = t.rw_deny[i] = active(mgr, h.deny, name, block_class=True)
        pii = t.rw_pii[i] = active(mgr, h.pii, name, block_class=False)
        regex = t.rw_regex[i] = active(mgr, h.regex, name, block_class=False)
        norm = t.rw_norm[i] = active(mgr, h.normalizer, name, block_class=False)
        harm = active(mgr, h.harm, name, block_class=True)
        mod = active(mgr, h.moderation, name, block_class=True)
        harm_post = t.rw_harm[i] = bool(enforcing(h.harm) and applies(h.harm, name))
        t.mod_app[i] = applies(h.moderation, name)
        sec_act[i] = active(mgr, h.secrets, name, block_class=False)
        exf_act[i] = active(mgr, h.exfil, name, block_class=False)
        sql_act[i] = active(mgr, h.sql, name, block_class=False)
        # semcache insert allowlist (tool-level; lookups are gated by TF_CACHE)
        t.semallow[i] = bool(semcache_on and h.semcache_plugin.cacheable(name))
        # TF_NORM = "escape triggers route this tool to the host path":
        # needed when the normalizer applies OR any raw-byte content
        # bank is active (their exact semantics are over DECODED text)
        schema = m.schema_mode if active(mgr, h.schema_guard, name, block_class=True) else None
        flags[i] = sum(bit for on, bit in (
            (m.reachable, hip.TF_REACHABLE), (deny, hip.TF_DENY), (pii, hip.TF_PII),
            (regex, hip.TF_REGEX), (norm or deny or harm or pii or mod, hip.TF_NORM),
            (mod, hip.TF_MOD), (harm, hip.TF_HARM),
            (schema == "fast", hip.TF_SCHEMA_FAST), (schema == "host", hip.TF_SCHEMA_HOST),
            (t.semallow[i], hip.TF_CACHE), (h.exact_cache is not None, hip.TF_EXACT)) if on)
        # native POST lane eligibility (forge_post_rows): -1 = this
        # tool's flagged results must run the exact Python _host_post
        # (user regexes, output schemas); otherwise bit0 pii, bit1
        # harm, bit2 toon — mirroring _host_post's own gates
        pf = 0
        if m.host_chain or m.has_output_schema:
            pf = -1
        if pf >= 0 and regex:
            # regex rules run in C-lane rows ONLY when the pass-3 regex
            # bank scan proves identity (no hit): rows WITH a bank hit
            # punt (bit3). No bank at all (un-DFA-able rules) → no
            # identity proof → the whole tool stays on the Python path.
            pf = (pf | 8) if "regex" in bank_names else -1
        if pf >= 0 and pii:
            pf |= 1
        if pf >= 0 and harm_post:
            pf = (pf | 2) if harm_lane_ok else -1
        if pf >= 0 and h.toon is not None and applies(h.toon, name):
            # guard soundness: with positive min_savings the TOON text is
            # strictly shorter than the JSON it replaces, so a row under
            # the guard bound stays under it; otherwise punt to Python
            if h.out_guard is not None and h.toon.min_savings <= 0:
                pf = -1
            else:
                pf |= 4
        if sec_act[i] or exf_act[i]:
            pf = -1  # flagged results need scan_payload: Python _host_post
        postlane[i] = pf
    t.flags = flags
    t.postlane = postlane
    t.hostbound = hostbound if hostbound.any() else None
    t.secrets = sec_act if sec_act.any() else None
    t.exfil = exf_act if exf_act.any() else None
    t.sql = sql_act if sql_act.any() else None


# ---- schema-key tables ----
def schema_key_tables(t: ToolTable, metas: List[_ToolMeta]) -> None:
    """FAST-mode schema descriptors for the C rewrite lane (presence + type
    checks only — richer schemas never compile to "fast"); a C pass means
    the exact validator is skipped, a C fail reruns it for the byte-exact
    error message."""
    keys: List[bytes] = []
    sk_ty: List[int] = []
    sk_rq: List[int] = []
    sk_range = np.full((max(len(metas), 1), 2), -1, dtype=np.int32)
    for i, m in enumerate(metas):
        if m.schema_mode != "fast":
            continue
        schema = m.tool.get("input_schema") or {}
        props = schema.get("properties") or {}
        required = set(schema.get("required") or [])
        lo = len(keys)
        for k, sub in props.items():
            keys.append(k.encode())
            sk_ty.append(_TYPE_CODE.get(sub.get("type") if isinstance(sub, dict) else None, 0))
            sk_rq.append(1 if k in required else 0)
        for k in required:
            if k not in props:
                keys.append(k.encode())
                sk_ty.append(0)
                sk_rq.append(1)
        sk_range[i] = (lo, len(keys))
    t.sk_range = sk_range
    t.sk_tables = None
    if keys:
        blob, off = pack_strtable(keys)
        t.sk_tables = (blob, np.ascontiguousarray(off[:-1]), np.ascontiguousarray(off[1:]),
                       np.asarray(sk_ty, dtype=np.int8), np.asarray(sk_rq, dtype=np.uint8))


def build_tool_table(engine, h: PluginHandles, banks: Dict[str, Any], device, *,
                     semcache_on: bool, harm_lane_ok: bool) -> ToolTable:
    """The snapshot for the engine's current registry generation and plugins
    version. The owning pipeline attaches `graphs`, a new pass-1 GraphCache
    per table: captured graphs bake this table's bank pointers."""
    t = ToolTable()
    t.generation = engine.registry.generation
    t.plugins_ver = getattr(engine.plugins, "version", 0)
    metas, pat_ids = per_tool_meta(engine, h)
    t.schema_bank, t.nest_bits = schema_bank(metas, pat_ids, h.schema_guard, device)
    # pass-1 fused bank set (depends on the schema bank just built)
    b1 = [(n, banks[n]) for n in ("deny", "harm", "pii", "regex", "normalize") if n in banks]
    if t.schema_bank is not None:
        b1.append(("schema", t.schema_bank))
    t.bankset1 = hip.ScanBankSet(b1, device)
    t.graphs = None
    flat_arrays(t, metas)
    tool_flags(t, metas, engine.plugins, h, banks.keys(), semcache_on, harm_lane_ok)
    schema_key_tables(t, metas)
    return t
