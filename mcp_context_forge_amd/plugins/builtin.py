"""Builtin plugin set.

Per-plugin reference analogs (behavioral port, no code copied):
  deny_filter        → plugins/deny_filter/deny.py (deny-list word filter)
  regex_filter       → plugins/regex_filter/search_replace.py
  pii_filter         → cpex-pii-filter (detect/mask emails, SSNs, cards, phones, IPs)
  secrets_detection  → plugins/secrets_detection (provider key formats + high-entropy
                       base64/hex tokens; block / redact / audit). Opt-in: not
                       in the default chain
  encoded_exfil_detection → cpex-encoded-exfil-detection (long base64/hex runs that
                       decode to printable text naming a credential; block /
                       redact / audit). Opt-in: not in the default chain
  sql_sanitizer      → plugins/sql_sanitizer (blocked statement keywords, DELETE /
                       UPDATE without WHERE, outside strings and comments;
                       block / audit, optional comment stripping). Opt-in: not
                       in the default chain
  schema_guard      → plugins/schema_guard (JSON-Schema arg/result validation)
  toon_encoder       → plugins/toon_encoder (JSON→TOON result compression)
  content_moderation → plugins/content_moderation (category classifier)
  harmful_content    → plugins/harmful_content_detector (keyword+classifier)
  response_cache_by_prompt → semantic cosine cache (plugins/response_cache_by_prompt)
  cached_tool_result → plugins/cached_tool_result (TTL exact-match cache)
  circuit_breaker    → plugins/circuit_breaker (per-tool error-rate breaker)
  argument_normalizer→ plugins/argument_normalizer (unicode/whitespace normalize)
  output_length_guard→ plugins/output_length_guard
  header_injector / header_filter → plugins/header_injector, plugins/header_filter

Each plugin implements the per-request async hooks (the CPU/reference path
and the parity oracle). GPU-capable plugins additionally expose the data
the batched pipeline needs (`scan_tables()`, `classifier()`, `featurize
dim`), and the pipeline applies their semantics batch-wide with HIP kernels
— see gpu/pipeline.py. Detection parity between the two paths is asserted
in tests/test_gpu_parity.py.
"""

from __future__ import annotations

import hashlib
import json
import re
import time
import unicodedata
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from ..ops import dfa
from ..ops.featurize import featurize
from ..utils.jsonschema import validate as schema_validate
from . import toon as toon_codec
from .framework import HookType, Plugin, PluginContext, PluginResult


def _text_of(payload: Any) -> str:
    """Canonical text of an args/result payload for scanning/featurizing."""
    if payload is None:
        return ""
    if isinstance(payload, str):
        return payload
    try:
        return json.dumps(payload, separators=(",", ":"), sort_keys=True, default=str)
    except Exception:
        return str(payload)


def _walk_strings(payload: Any, fn) -> Any:
    if isinstance(payload, str):
        return fn(payload)
    if isinstance(payload, dict):
        return {k: _walk_strings(v, fn) for k, v in payload.items()}
    if isinstance(payload, list):
        return [_walk_strings(v, fn) for v in payload]
    return payload


# ---------------------------------------------------------------------------


class DenyFilterPlugin(Plugin):
    """Block requests containing deny-listed words (reference: deny.py:118)."""

    name = "deny_filter"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.PROMPT_PRE_FETCH, HookType.AGENT_PRE_INVOKE)
    priority = 10
    gpu_capable = True

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        self.words: List[str] = list(self.config.get("words") or ["forbidden", "blocked_word"])
        self.case_insensitive: bool = bool(self.config.get("case_insensitive", True))
        self._tables = dfa.compile_literals(self.words, self.case_insensitive)

    def scan_tables(self) -> dfa.ScanTables:
        return self._tables

    async def tool_pre_invoke(self, ctx: PluginContext) -> PluginResult:
        text = _text_of(ctx.args)
        hay = text.lower() if self.case_insensitive else text
        for w in self.words:
            needle = w.lower() if self.case_insensitive else w
            if needle in hay:
                return PluginResult.block(f"deny word {w!r} present", code="deny")
        return PluginResult.ok()

    prompt_pre_fetch = tool_pre_invoke
    agent_pre_invoke = tool_pre_invoke


class RegexFilterPlugin(Plugin):
    """Regex search/replace on args and results (reference: search_replace.py:190)."""

    name = "regex_filter"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.TOOL_POST_INVOKE, HookType.PROMPT_PRE_FETCH)
    priority = 20
    gpu_capable = True

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        rules = self.config.get("rules") or [{"search": r"crap", "replace": "crud"}]
        self.rules: List[Tuple[re.Pattern, str]] = [
            (re.compile(r["search"], re.IGNORECASE if r.get("ignorecase", True) else 0), r["replace"]) for r in rules
        ]
        # GPU prefilter tables: the DFA flags requests containing any rule match;
        # only flagged requests pay the host rewrite.
        try:
            self._tables = dfa.compile_patterns(
                [r["search"] for r in rules],
                case_insensitive=any(r.get("ignorecase", True) for r in rules),
            )
        except ValueError:
            self._tables = None

    def scan_tables(self) -> Optional[dfa.ScanTables]:
        return self._tables

    def apply_rules(self, text: str) -> str:
        for pat, repl in self.rules:
            text = pat.sub(repl, text)
        return text

    async def tool_pre_invoke(self, ctx: PluginContext) -> PluginResult:
        return PluginResult.ok(_walk_strings(ctx.args, self.apply_rules))

    async def tool_post_invoke(self, ctx: PluginContext) -> PluginResult:
        return PluginResult.ok(_walk_strings(ctx.args, self.apply_rules))

    prompt_pre_fetch = tool_pre_invoke


# PII pattern set (shared between CPU re-path and the GPU DFA bank).
PII_PATTERNS: List[Tuple[str, str, str]] = [
    # (name, dfa_pattern, python_regex)
    ("ssn", r"\d{3}-\d{2}-\d{4}", r"\b\d{3}-\d{2}-\d{4}\b"),
    ("email", r"[A-Za-z0-9._%+\-]+@[A-Za-z0-9.\-]+\.[A-Za-z][A-Za-z]+", r"[A-Za-z0-9._%+\-]+@[A-Za-z0-9.\-]+\.[A-Za-z]{2,}"),
    ("credit_card", r"\d{4}[ \-]\d{4}[ \-]\d{4}[ \-]\d{4}", r"\b\d{4}[ \-]\d{4}[ \-]\d{4}[ \-]\d{4}\b"),
    ("phone", r"\(?\d{3}\)?[ .\-]\d{3}[ .\-]\d{4}", r"\(?\b\d{3}\)?[ .\-]\d{3}[ .\-]\d{4}\b"),
    ("ipv4", r"\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3}", r"\b\d{1,3}\.\d{1,3}\.\d{1,3}\.\d{1,3}\b"),
    ("aws_key", r"AKIA[0-9A-Z]{16}", r"\bAKIA[0-9A-Z]{16}\b"),
]


class PIIFilterPlugin(Plugin):
    """Detect and mask PII in args and results (reference: cpex-pii-filter)."""

    name = "pii_filter"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.TOOL_POST_INVOKE, HookType.PROMPT_PRE_FETCH,
             HookType.AGENT_PRE_INVOKE, HookType.AGENT_POST_INVOKE)
    priority = 30
    gpu_capable = True

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        self.action: str = self.config.get("action", "mask")  # mask | block | audit
        names = set(self.config.get("categories") or [n for n, _, _ in PII_PATTERNS])
        self.active = [(n, d, re.compile(p)) for (n, d, p) in PII_PATTERNS if n in names]
        self._tables = dfa.compile_patterns([d for (_, d, _) in self.active])

    def scan_tables(self) -> dfa.ScanTables:
        return self._tables

    def mask_text(self, text: str) -> Tuple[str, List[str]]:
        found: List[str] = []
        for name, _d, rx in self.active:
            if rx.search(text):
                found.append(name)
                text = rx.sub(f"[{name.upper()}_REDACTED]", text)
        return text, found

    def mask_text_subset(self, text: str, pattern_bits: int) -> Tuple[str, List[str]]:
        """Masked-pattern fast path: bit i of `pattern_bits` is the GPU scan
        bank's accept bit for self.active[i] (same compile order) — only the
        patterns the DFA flagged need their Python regex run."""
        found: List[str] = []
        for i, (name, _d, rx) in enumerate(self.active):
            if not (pattern_bits >> i) & 1:
                continue
            if rx.search(text):
                found.append(name)
                text = rx.sub(f"[{name.upper()}_REDACTED]", text)
        return text, found

    async def _apply(self, ctx: PluginContext) -> PluginResult:
        found_all: List[str] = []

        def fn(s: str) -> str:
            masked, found = self.mask_text(s)
            found_all.extend(found)
            return masked

        new_payload = _walk_strings(ctx.args, fn)
        if found_all and self.action == "block":
            return PluginResult.block(f"PII detected: {sorted(set(found_all))}", code="pii")
        if found_all and self.action == "mask":
            return PluginResult.ok(new_payload, pii=sorted(set(found_all)))
        if found_all:  # audit mode: annotate only
            return PluginResult.ok(pii=sorted(set(found_all)))
        return PluginResult.ok()

    tool_pre_invoke = _apply
    tool_post_invoke = _apply
    prompt_pre_fetch = _apply
    agent_pre_invoke = _apply
    agent_post_invoke = _apply


# Known secret formats (shared between the CPU re-path and the GPU DFA bank).
# The DFA pattern is a SUPERSET of the Python regex: the provider prefix plus
# the first four bytes of the token body, no word boundaries, so wherever the
# regex matches, the search automaton has matched too. Full-length bodies
# would be exact but their counters multiply across patterns in the subset
# construction (the six full patterns exceed 60 000 states; this bank has
# under 1 000). A prefilter hit only routes the row to the exact host check.
SECRET_PATTERNS: List[Tuple[str, str, str]] = [
    # (name, dfa_pattern, python_regex)
    ("aws_access_key_id", r"A[KS]IA[0-9A-Z]{4}", r"\bA[KS]IA[0-9A-Z]{16}\b"),
    ("github_token", r"gh[pousr]_[A-Za-z0-9]{4}", r"\bgh[pousr]_[A-Za-z0-9]{36,}"),
    ("github_fine_grained_pat", r"github_pat_[A-Za-z0-9_]{4}", r"\bgithub_pat_[A-Za-z0-9_]{22,}"),
    ("slack_token", r"xox[abeoprs]-[A-Za-z0-9\-]{4}", r"\bxox[abeoprs]-[A-Za-z0-9\-]{10,}"),
    ("google_api_key", r"AIza[0-9A-Za-z_\-]{4}", r"\bAIza[0-9A-Za-z_\-]{35}"),
    ("pem_private_key", r"-----BEGIN [A-Z ]*PRIVATE KEY-----", r"-----BEGIN (?:[A-Z]+ )*PRIVATE KEY-----"),
    ("jwt", r"eyJ[A-Za-z0-9_\-]{4,}\.eyJ",
     r"\beyJ[A-Za-z0-9_\-]{8,}\.eyJ[A-Za-z0-9_\-]{8,}\.[A-Za-z0-9_\-]{8,}"),
]

# Well-known entropy thresholds (bits per symbol) per alphabet.
ENTROPY_THRESHOLDS = {"base64": 4.5, "hex": 3.0}


class SecretsDetectionPlugin(Plugin):
    """Stop credentials travelling in arguments or coming back in results:
    known provider formats (a DFA bank on the GPU path) plus long base64/hex
    tokens of high Shannon entropy (ops/entropy.py; entropy.hip on the GPU
    path). Priority 5: it sees the payload before any rewriter in both
    directions, which is what makes the pipeline's raw-byte prefilter sound.

    Config: action block (default, code "secrets") | redact | audit,
    redaction_text, min_findings_to_block, categories (subset of the format
    names and "high_entropy_<alphabet>"), alphabets (["base64"], "hex"
    optional), min_len (20), thresholds ({"base64": 4.5, "hex": 3.0}).
    """

    name = "secrets_detection"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.TOOL_POST_INVOKE, HookType.PROMPT_PRE_FETCH,
             HookType.RESOURCE_POST_FETCH)
    priority = 5
    gpu_capable = True

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        from ..ops import entropy as _entropy

        self._entropy = _entropy
        self.action: str = self.config.get("action", "block")  # block | redact | audit
        self.redaction_text: str = str(self.config.get("redaction_text", "[SECRET_REDACTED]"))
        self.min_findings_to_block = int(self.config.get("min_findings_to_block", 1))
        self.min_len = max(int(self.config.get("min_len", 20)), 1)
        alphabets = list(self.config.get("alphabets") or ["base64"])
        for a in alphabets:
            if a not in _entropy.TABLES:
                raise ValueError(f"unknown entropy alphabet {a!r}")
        thresholds = {**ENTROPY_THRESHOLDS, **(self.config.get("thresholds") or {})}
        all_names = [n for n, _, _ in SECRET_PATTERNS] + [f"high_entropy_{a}" for a in alphabets]
        names = set(self.config.get("categories") or all_names)
        # bytes regexes: spans are byte offsets, shared with the entropy runs
        self.active = [(n, d, re.compile(p.encode())) for (n, d, p) in SECRET_PATTERNS if n in names]
        # (alphabet, category, symbol table, threshold) per enabled entropy detector
        self.entropy_detectors = [(a, f"high_entropy_{a}", _entropy.TABLES[a](), float(thresholds[a]))
                                  for a in alphabets if f"high_entropy_{a}" in names]
        self._tables = dfa.compile_patterns([d for (_, d, _) in self.active]) if self.active else None

    def scan_tables(self) -> Optional[dfa.ScanTables]:
        return self._tables

    def find_spans(self, raw: bytes) -> List[Tuple[int, int, str]]:
        """Every finding in one string's UTF-8 bytes as (beg, end, category)."""
        out: List[Tuple[int, int, str]] = []
        for name, _d, rx in self.active:
            for mt in rx.finditer(raw):
                out.append((mt.start(), mt.end(), name))
        for _a, cat, table, thr in self.entropy_detectors:
            runs = self._entropy.token_entropy_reference(raw, table, self.min_len)[0]
            out.extend((b, b + n, cat) for (b, n, h) in runs if h >= thr)
        return out

    def _redact(self, raw: bytes, spans: List[Tuple[int, int, str]]) -> bytes:
        merged: List[List[int]] = []
        for b, e, _c in sorted(spans):
            if merged and b <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], e)
            else:
                merged.append([b, e])
        rep = self.redaction_text.encode()
        parts, pos = [], 0
        for b, e in merged:
            parts.append(raw[pos:b])
            parts.append(rep)
            pos = e
        parts.append(raw[pos:])
        return b"".join(parts)

    def scan_payload(self, payload: Any) -> Tuple[Any, List[str]]:
        """Synchronous scan of every string value, shared by the hooks and
        the GPU pipeline's host lane. → (payload, findings): the payload has
        every finding's span replaced by redaction_text when action is
        "redact" (otherwise it is returned as is); findings holds one
        category name per finding."""
        findings: List[str] = []
        redact = self.action == "redact"

        def fn(s: str) -> str:
            raw = s.encode("utf-8", "surrogatepass")
            spans = self.find_spans(raw)
            if not spans:
                return s
            findings.extend(c for _b, _e, c in spans)
            if not redact:
                return s
            return self._redact(raw, spans).decode("utf-8", "surrogatepass")

        new_payload = _walk_strings(payload, fn)
        return (new_payload if redact and findings else payload), findings

    def block_reason(self, findings: List[str]) -> Optional[str]:
        """The violation text when these findings block, else None."""
        if self.action == "block" and findings and len(findings) >= self.min_findings_to_block:
            return f"secrets detected: {sorted(set(findings))}"
        return None

    async def _apply(self, ctx: PluginContext) -> PluginResult:
        new_payload, findings = self.scan_payload(ctx.args)
        if not findings:
            return PluginResult.ok()
        reason = self.block_reason(findings)
        if reason is not None:
            return PluginResult.block(reason, code="secrets")
        if self.action == "redact":
            return PluginResult.ok(new_payload, secrets=sorted(set(findings)))
        return PluginResult.ok(secrets=sorted(set(findings)))  # audit: annotate only

    tool_pre_invoke = _apply
    tool_post_invoke = _apply
    prompt_pre_fetch = _apply
    resource_post_fetch = _apply


class EncodedExfilDetectionPlugin(Plugin):
    """Stop credentials that travel ENCODED: a long base64 or hex run whose
    decoded bytes are mostly printable text and name a credential
    (ops/exfil.py; exfil.hip on the GPU path). The encoded bytes pass every
    byte-pattern plugin and, being encoded English, the entropy detector too.
    Priority 6: directly after secrets_detection and before any rewriter in
    both directions, which is what makes the pipeline's raw-byte prefilter
    sound.

    Config: action block (default, code "exfil") | redact | audit,
    redaction_text, min_findings_to_block, encodings (["base64", "hex"]),
    min_len (24), min_printable (0.8, kept as integer per-mille), keywords
    (1 to 32 words of 2 to 16 printable ASCII bytes, matched case-
    insensitively), require_keyword (true: a finding is a text run that
    holds a keyword; false: any text run).
    """

    name = "encoded_exfil_detection"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.TOOL_POST_INVOKE, HookType.PROMPT_PRE_FETCH,
             HookType.RESOURCE_POST_FETCH)
    priority = 6
    gpu_capable = True

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        from ..ops import exfil as _exfil

        self._exfil = _exfil
        self.action: str = self.config.get("action", "block")  # block | redact | audit
        self.redaction_text: str = str(self.config.get("redaction_text", "[ENCODED_REDACTED]"))
        self.min_findings_to_block = int(self.config.get("min_findings_to_block", 1))
        self.min_len = max(int(self.config.get("min_len", 24)), 1)
        self.min_printable_permille = int(round(float(self.config.get("min_printable", 0.8)) * 1000))
        self.require_keyword = bool(self.config.get("require_keyword", True))
        encodings = list(self.config.get("encodings") or ["base64", "hex"])
        for e in encodings:
            if e not in _exfil.ENCODINGS:
                raise ValueError(f"unknown encoding {e!r}")
        self.keywords: List[str] = list(self.config.get("keywords") or _exfil.DEFAULT_KEYWORDS)
        self._kw_tables = _exfil.compile_keywords(self.keywords)   # raises over the kernel's limits
        # (encoding, category, symbol table, bits per symbol) per configured encoding
        self.detectors = [(e, f"encoded_{e}", _exfil.ENCODINGS[e][0](), _exfil.ENCODINGS[e][1])
                          for e in encodings]

    def keyword_tables(self) -> dfa.ScanTables:
        return self._kw_tables

    def find_spans(self, raw: bytes) -> List[Tuple[int, int, str]]:
        """Every finding in one string's UTF-8 bytes as (beg, end, category)."""
        out: List[Tuple[int, int, str]] = []
        for _e, cat, table, bits in self.detectors:
            runs = self._exfil.decode_scan_reference(raw, table, bits, self.min_len,
                                                     self.min_printable_permille, self._kw_tables)[0]
            out.extend((b, b + n, cat) for (b, n, _dl, _pr, text, mask) in runs
                       if text and (mask or not self.require_keyword))
        return out

    _redact = SecretsDetectionPlugin._redact   # overlapping spans collapse to one replacement

    def scan_payload(self, payload: Any) -> Tuple[Any, List[str]]:
        """Synchronous scan of every string value, shared by the hooks and
        the GPU pipeline's host lane, like SecretsDetectionPlugin.scan_payload.
        → (payload, findings): the payload has every finding's span replaced
        by redaction_text when action is "redact" (otherwise it is returned
        as is); findings holds one category name per finding."""
        findings: List[str] = []
        redact = self.action == "redact"

        def fn(s: str) -> str:
            raw = s.encode("utf-8", "surrogatepass")
            spans = self.find_spans(raw)
            if not spans:
                return s
            findings.extend(c for _b, _e, c in spans)
            if not redact:
                return s
            return self._redact(raw, spans).decode("utf-8", "surrogatepass")

        new_payload = _walk_strings(payload, fn)
        return (new_payload if redact and findings else payload), findings

    def block_reason(self, findings: List[str]) -> Optional[str]:
        """The violation text when these findings block, else None."""
        if self.action == "block" and findings and len(findings) >= self.min_findings_to_block:
            return f"encoded payloads detected: {sorted(set(findings))}"
        return None

    async def _apply(self, ctx: PluginContext) -> PluginResult:
        new_payload, findings = self.scan_payload(ctx.args)
        if not findings:
            return PluginResult.ok()
        reason = self.block_reason(findings)
        if reason is not None:
            return PluginResult.block(reason, code="exfil")
        if self.action == "redact":
            return PluginResult.ok(new_payload, encoded=sorted(set(findings)))
        return PluginResult.ok(encoded=sorted(set(findings)))  # audit: annotate only

    tool_pre_invoke = _apply
    tool_post_invoke = _apply
    prompt_pre_fetch = _apply
    resource_post_fetch = _apply


class SqlSanitizerPlugin(Plugin):
    """Stop dangerous SQL travelling in arguments: blocked statement keywords
    (DROP, TRUNCATE, ...) and DELETE / UPDATE without WHERE, found by a lexer
    that knows string literals and comments and folds per statement
    (ops/sql.py; sql.hip on the GPU path). A keyword inside a string or a
    comment is not code, `DR/**/OP` is two words, `drops` is not `drop`.
    Priority 7: after encoded_exfil_detection and before any rewriter, which
    is what makes the pipeline's raw-byte prefilter sound. Pre hooks only, as
    the reference plugin.

    Config: action block (default, code "sql") | audit, blocked_statements
    (1 to 24 words of 2 to 16 bytes over [A-Za-z0-9_], matched as whole words
    and case-insensitively; default drop, truncate, alter, grant, revoke),
    block_delete_without_where (true), block_update_without_where (true),
    min_findings_to_block (1), fields (top-level argument names to scan;
    default every string value), strip_comments (false: when true every
    comment of a scanned string becomes one space in the forwarded payload,
    unless the request is blocked).

    Dialect limits: backticks, [..] identifiers, # comments, dollar quoting
    and backslash escapes are not lexed; those bytes are plain code bytes.
    """

    name = "sql_sanitizer"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.PROMPT_PRE_FETCH)
    priority = 7
    gpu_capable = True

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        from ..ops import sql as _sql

        self._sql = _sql
        self.action: str = self.config.get("action", "block")  # block | audit
        if self.action not in ("block", "audit"):
            raise ValueError(f"unknown sql_sanitizer action {self.action!r}")
        self.min_findings_to_block = int(self.config.get("min_findings_to_block", 1))
        self.block_delete_without_where = bool(self.config.get("block_delete_without_where", True))
        self.block_update_without_where = bool(self.config.get("block_update_without_where", True))
        self.strip_comments = bool(self.config.get("strip_comments", False))
        fields = self.config.get("fields")
        self.fields: Optional[List[str]] = [str(f) for f in fields] if fields else None
        self.blocked: List[str] = list(self.config.get("blocked_statements") or _sql.DEFAULT_BLOCKED)
        self._kw_tables, self._kw_len = _sql.compile_sql_keywords(self.blocked)   # raises over the kernel's limits

    def keyword_tables(self) -> dfa.ScanTables:
        return self._kw_tables

    def keyword_lengths(self) -> List[int]:
        return list(self._kw_len)

    def _wanted(self, category: str) -> bool:
        if category == "delete_without_where":
            return self.block_delete_without_where
        if category == "update_without_where":
            return self.block_update_without_where
        return True

    def _scan(self, raw: bytes) -> Tuple[List[Tuple[int, int, str]], List[Tuple[int, int]]]:
        findings, comments = self._sql.sql_scan_reference(raw, self._kw_tables, self._kw_len, False)[:2]
        return [(b, b + n, c) for (b, n, c) in findings if self._wanted(c)], comments

    def find_spans(self, raw: bytes) -> List[Tuple[int, int, str]]:
        """Every finding in one string's UTF-8 bytes as (beg, end, category)."""
        return self._scan(raw)[0]

    def scan_payload(self, payload: Any) -> Tuple[Any, List[str]]:
        """Synchronous scan of every string value (of the `fields` arguments
        when configured). → (payload, findings): the payload has every
        comment replaced by one space when strip_comments is on and a scanned
        string held one (otherwise it is returned as is); findings holds one
        category name per finding."""
        findings: List[str] = []
        stripped = False

        def fn(s: str) -> str:
            nonlocal stripped
            raw = s.encode("utf-8", "surrogatepass")
            spans, comments = self._scan(raw)
            findings.extend(c for _b, _e, c in spans)
            if not (self.strip_comments and comments):
                return s
            stripped = True
            parts, pos = [], 0
            for b, n in comments:
                parts.append(raw[pos:b])
                parts.append(b" ")
                pos = b + n
            parts.append(raw[pos:])
            return b"".join(parts).decode("utf-8", "surrogatepass")

        if self.fields is not None and isinstance(payload, dict):
            new_payload = {k: (_walk_strings(v, fn) if k in self.fields else v) for k, v in payload.items()}
        else:
            new_payload = _walk_strings(payload, fn)
        return (new_payload if stripped else payload), findings

    def block_reason(self, findings: List[str]) -> Optional[str]:
        """The violation text when these findings block, else None."""
        if self.action == "block" and findings and len(findings) >= self.min_findings_to_block:
            return f"dangerous sql detected: {sorted(set(findings))}"
        return None

    async def _apply(self, ctx: PluginContext) -> PluginResult:
        new_payload, findings = self.scan_payload(ctx.args)
        reason = self.block_reason(findings)
        if reason is not None:
            return PluginResult.block(reason, code="sql")
        meta = {"sql": sorted(set(findings))} if findings else {}   # audit: annotate only
        if new_payload is not ctx.args:
            return PluginResult.ok(new_payload, **meta)
        return PluginResult.ok(**meta)

    tool_pre_invoke = _apply
    prompt_pre_fetch = _apply


class SchemaGuardPlugin(Plugin):
    """Validate args/results against the tool's JSON schema (reference: schema_guard.py:168)."""

    name = "schema_guard"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.TOOL_POST_INVOKE)
    priority = 40
    gpu_capable = True  # GPU does the byte-level structural guard over the batch

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        self.max_depth = int(self.config.get("max_depth", 64))
        self.max_string = int(self.config.get("max_string", 1 << 20))

    async def tool_pre_invoke(self, ctx: PluginContext) -> PluginResult:
        schema = ctx.state.get("input_schema")
        if schema:
            errs = schema_validate(ctx.args or {}, schema)
            if errs:
                return PluginResult.block("schema violation: " + "; ".join(errs[:5]), code="schema")
        return PluginResult.ok()

    async def tool_post_invoke(self, ctx: PluginContext) -> PluginResult:
        schema = ctx.state.get("output_schema")
        if schema:
            payload = ctx.args
            if isinstance(payload, dict) and "structuredContent" in payload:
                payload = payload["structuredContent"]
            errs = schema_validate(payload, schema)
            if errs:
                return PluginResult.block("output schema violation: " + "; ".join(errs[:5]), code="schema")
        return PluginResult.ok()


class ToonEncoderPlugin(Plugin):
    """Compress JSON tool results to TOON (reference: toon_encoder)."""

    name = "toon_encoder"
    hooks = (HookType.TOOL_POST_INVOKE,)
    priority = 900
    gpu_capable = True

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        self.min_savings = float(self.config.get("min_savings", 0.1))
        self.min_size = int(self.config.get("min_size", 256))

    def encode_result(self, result: Any) -> Optional[Dict[str, Any]]:
        """Returns modified tool-result dict or None if not worth encoding."""
        if not isinstance(result, dict):
            return None
        sc = result.get("structuredContent")
        if sc is None:
            return None
        j = len(json.dumps(sc, separators=(",", ":")))
        if j < self.min_size:  # cheap reject before paying for the TOON encode
            return None
        encoded = toon_codec.encode(sc)
        t = len(encoded)
        frac = 1.0 - t / j if j else 0.0
        if frac < self.min_savings:
            return None
        new = dict(result)
        new["content"] = [{"type": "text", "text": encoded}]
        meta = new.get("_meta")
        if "_meta" not in new:
            meta = new["_meta"] = {}
        if isinstance(meta, dict):  # a non-dict _meta from the upstream is left alone
            meta["toon"] = {"json_bytes": j, "toon_bytes": t, "savings": round(frac, 4)}
        return new

    async def tool_post_invoke(self, ctx: PluginContext) -> PluginResult:
        new = self.encode_result(ctx.args)
        return PluginResult.ok(new) if new is not None else PluginResult.ok()


class ContentModerationPlugin(Plugin):
    """Category-score moderation classifier (reference: content_moderation.py:846).

    The reference calls external APIs (Watson/OpenAI/patterns); per
    BASELINE.json this build runs a local bf16-MFMA classifier over hashed
    features (random-init weights). CPU path = fp32 torch forward.
    """

    name = "content_moderation"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.PROMPT_PRE_FETCH, HookType.AGENT_PRE_INVOKE)
    priority = 50
    gpu_capable = True

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        from ..models.classifier import HashedTextClassifier

        self.dim = int(self.config.get("dim", 4096))
        self.threshold = float(self.config.get("threshold", 0.95))
        self.model = HashedTextClassifier(
            dim=self.dim,
            hidden=int(self.config.get("hidden", 1024)),
            classes=int(self.config.get("classes", 8)),
            seed=int(self.config.get("seed", 1234)),
        ).eval()

    def classifier(self):
        return self.model

    def score_text(self, text: str) -> np.ndarray:
        import torch

        feats = torch.from_numpy(featurize(text, self.dim)).unsqueeze(0)
        with torch.no_grad():
            return self.model(feats)[0].numpy()

    async def tool_pre_invoke(self, ctx: PluginContext) -> PluginResult:
        scores = self.score_text(_text_of(ctx.args))
        worst = float(scores.max())
        if worst >= self.threshold:
            from ..models.classifier import category_names

            cat = category_names(len(scores))[int(scores.argmax())]
            return PluginResult.block(f"moderation: category {cat} score {worst:.3f}", code="moderation")
        return PluginResult.ok(metadata={"moderation_max": worst})

    prompt_pre_fetch = tool_pre_invoke
    agent_pre_invoke = tool_pre_invoke


class HarmfulContentPlugin(Plugin):
    """Keyword-bank harm detector (reference: harmful_content_detector.py:207)."""

    name = "harmful_content_detector"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.TOOL_POST_INVOKE, HookType.AGENT_PRE_INVOKE)
    priority = 60
    gpu_capable = True

    DEFAULT_BANK = {
        "violence": ["kill them all", "how to make a bomb"],
        "self_harm": ["ways to hurt myself"],
        "illegal": ["buy stolen credit cards"],
    }

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        self.bank: Dict[str, List[str]] = self.config.get("bank") or dict(self.DEFAULT_BANK)
        phrases, cats = [], []
        for cat, plist in self.bank.items():
            for p in plist:
                phrases.append(p)
                cats.append(cat)
        self.phrases, self.cats = phrases, cats
        self._tables = dfa.compile_literals(phrases, case_insensitive=True)

    def scan_tables(self) -> dfa.ScanTables:
        return self._tables

    async def tool_pre_invoke(self, ctx: PluginContext) -> PluginResult:
        hay = _text_of(ctx.args).lower()
        for phrase, cat in zip(self.phrases, self.cats):
            if phrase.lower() in hay:
                return PluginResult.block(f"harmful content ({cat})", code="harmful_content")
        return PluginResult.ok()

    tool_post_invoke = tool_pre_invoke
    agent_pre_invoke = tool_pre_invoke


class ResponseCacheByPromptPlugin(Plugin):
    """Semantic result cache via cosine over hashed count vectors
    (reference: response_cache_by_prompt.py `_vectorize`:55 `_cos_sim`:74 `_find_best`:163).

    CPU path keeps the matrix in numpy; the GPU pipeline keeps it resident
    in HBM and runs the similarity matmul on MFMA.
    """

    name = "response_cache_by_prompt"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.TOOL_POST_INVOKE)
    priority = 5  # before everything: a cache hit skips the chain
    gpu_capable = True

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        self.dim = int(self.config.get("dim", 4096))
        self.threshold = float(self.config.get("threshold", 0.92))
        self.capacity = int(self.config.get("capacity", 4096))
        self.ttl = float(self.config.get("ttl", 600.0))
        # result substitution is gated on an EXPLICIT per-tool allowlist
        # (reference default: empty cacheable_tools — a near-miss cosine hit
        # on an unlisted tool must never replace a live invocation), and
        # entries are tenant-scoped: the identity compared on hit is
        # (tool, user), so one user's result is never served to another.
        self.cacheable_tools = frozenset(self.config.get("cacheable_tools") or [])
        # preallocated ring (matrix never reallocates — mirrors the GPU cache)
        self.vectors = np.zeros((self.capacity, self.dim), dtype=np.float32)
        self.entries: List[Optional[Tuple[Tuple[str, str], float, Any]]] = [None] * self.capacity
        self.size = 0
        self.write_ptr = 0
        self.hits = 0
        self.misses = 0

    def cacheable(self, tool: str) -> bool:
        return tool in self.cacheable_tools

    def lookup(self, tool: str, text: str, user: Optional[str] = None) -> Optional[Any]:
        if self.size == 0:
            self.misses += 1
            return None
        v = featurize(text, self.dim)
        sims = self.vectors[: self.size] @ v
        best = int(np.argmax(sims))
        now = time.monotonic()
        ent = self.entries[best]
        if ent is not None:
            ent_key, ts, result = ent
            if sims[best] >= self.threshold and ent_key == (tool, user or "") and now - ts <= self.ttl:
                self.hits += 1
                return result
        self.misses += 1
        return None

    def insert(self, tool: str, text: str, result: Any, user: Optional[str] = None) -> None:
        slot = self.write_ptr
        self.vectors[slot] = featurize(text, self.dim)
        self.entries[slot] = ((tool, user or ""), time.monotonic(), result)
        self.write_ptr = (self.write_ptr + 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)

    async def tool_pre_invoke(self, ctx: PluginContext) -> PluginResult:
        if not self.cacheable(ctx.name):
            return PluginResult.ok()
        hit = self.lookup(ctx.name, _text_of(ctx.args), user=ctx.user)
        if hit is not None:
            ctx.state["cache_hit"] = hit
        return PluginResult.ok()

    async def tool_post_invoke(self, ctx: PluginContext) -> PluginResult:
        if self.cacheable(ctx.name) and "cache_hit" not in ctx.state and ctx.args is not None:
            req_text = ctx.state.get("request_text", "")
            if req_text:
                self.insert(ctx.name, req_text, ctx.args, user=ctx.user)
        return PluginResult.ok()


class CachedToolResultPlugin(Plugin):
    """Exact-match TTL result cache (reference: cached_tool_result)."""

    name = "cached_tool_result"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.TOOL_POST_INVOKE)
    priority = 6

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        self.ttl = float(self.config.get("ttl", 300.0))
        self.store: Dict[str, Tuple[float, Any]] = {}

    def _key(self, name: str, args: Any, user: Optional[str] = None) -> str:
        # user is part of the key: exact-match results never cross tenants
        return hashlib.sha256((name + "\x00" + (user or "") + "\x00" + _text_of(args)).encode()).hexdigest()

    async def tool_pre_invoke(self, ctx: PluginContext) -> PluginResult:
        k = self._key(ctx.name, ctx.args, user=ctx.user)
        ent = self.store.get(k)
        if ent and time.monotonic() - ent[0] <= self.ttl:
            ctx.state["cache_hit"] = ent[1]
        ctx.state["exact_cache_key"] = k
        return PluginResult.ok()

    async def tool_post_invoke(self, ctx: PluginContext) -> PluginResult:
        k = ctx.state.get("exact_cache_key")
        if k and "cache_hit" not in ctx.state:
            self.store[k] = (time.monotonic(), ctx.args)
        return PluginResult.ok()


class CircuitBreakerPlugin(Plugin):
    """Per-tool error-rate breaker (reference: plugins/circuit_breaker)."""

    name = "circuit_breaker"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.TOOL_POST_INVOKE)
    priority = 8

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        self.error_threshold = float(self.config.get("error_threshold", 0.5))
        self.window = int(self.config.get("window", 20))
        self.cooldown = float(self.config.get("cooldown", 30.0))
        self.state: Dict[str, Dict[str, Any]] = {}

    def _st(self, tool: str) -> Dict[str, Any]:
        return self.state.setdefault(tool, {"results": [], "open_until": 0.0})

    async def tool_pre_invoke(self, ctx: PluginContext) -> PluginResult:
        st = self._st(ctx.name)
        if time.monotonic() < st["open_until"]:
            return PluginResult.block(f"circuit open for tool {ctx.name}", code="circuit_open")
        return PluginResult.ok()

    async def tool_post_invoke(self, ctx: PluginContext) -> PluginResult:
        st = self._st(ctx.name)
        is_error = bool(isinstance(ctx.args, dict) and ctx.args.get("isError"))
        st["results"].append(is_error)
        if len(st["results"]) > self.window:
            st["results"] = st["results"][-self.window:]
        if len(st["results"]) >= self.window and (sum(st["results"]) / len(st["results"])) >= self.error_threshold:
            st["open_until"] = time.monotonic() + self.cooldown
            st["results"] = []
        return PluginResult.ok()


class ArgumentNormalizerPlugin(Plugin):
    """Unicode/whitespace normalization of string args (reference: argument_normalizer)."""

    name = "argument_normalizer"
    hooks = (HookType.TOOL_PRE_INVOKE, HookType.PROMPT_PRE_FETCH)
    priority = 15

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        self.form = self.config.get("unicode_form", "NFC")
        self.collapse_ws = bool(self.config.get("collapse_whitespace", True))
        self.strip = bool(self.config.get("strip", True))

    def norm(self, s: str) -> str:
        s = unicodedata.normalize(self.form, s)
        if self.collapse_ws:
            s = re.sub(r"[ \t\f\v]+", " ", s)
        if self.strip:
            s = s.strip()
        return s

    async def tool_pre_invoke(self, ctx: PluginContext) -> PluginResult:
        return PluginResult.ok(_walk_strings(ctx.args, self.norm))

    prompt_pre_fetch = tool_pre_invoke


class OutputLengthGuardPlugin(Plugin):
    """Cap result size (reference: output_length_guard)."""

    name = "output_length_guard"
    hooks = (HookType.TOOL_POST_INVOKE,)
    priority = 950

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        self.max_chars = int(self.config.get("max_chars", 1 << 20))
        self.action = self.config.get("action", "truncate")  # truncate | block

    async def tool_post_invoke(self, ctx: PluginContext) -> PluginResult:
        result = ctx.args
        if not isinstance(result, dict):
            return PluginResult.ok()
        total = 0
        for c in result.get("content", []):
            if isinstance(c, dict) and isinstance(c.get("text"), str):
                total += len(c["text"])
        if total <= self.max_chars:
            return PluginResult.ok()
        if self.action == "block":
            return PluginResult.block(f"output too large ({total} chars)", code="output_length")
        new = dict(result)
        new["content"] = [
            {**c, "text": c["text"][: self.max_chars]} if isinstance(c, dict) and isinstance(c.get("text"), str) else c
            for c in result.get("content", [])
        ]
        return PluginResult.ok(new)


class HeaderInjectorPlugin(Plugin):
    """Inject headers on outbound calls (reference: header_injector)."""

    name = "header_injector"
    hooks = (HookType.HTTP_PRE_REQUEST, HookType.TOOL_PRE_INVOKE)
    priority = 70

    def __init__(self, config: Optional[Dict[str, Any]] = None):
        super().__init__(config)
        self.headers: Dict[str, str] = dict(self.config.get("headers") or {})

    async def http_pre_request(self, ctx: PluginContext) -> PluginResult:
        ctx.headers.update(self.headers)
        return PluginResult.ok()

    async def tool_pre_invoke(self, ctx: PluginContext) -> PluginResult:
        ctx.headers.update(self.headers)
        return PluginResult.ok()


BUILTIN_PLUGINS = {
    p.name: p
    for p in (
        DenyFilterPlugin,
        RegexFilterPlugin,
        PIIFilterPlugin,
        SecretsDetectionPlugin,
        EncodedExfilDetectionPlugin,
        SqlSanitizerPlugin,
        SchemaGuardPlugin,
        ToonEncoderPlugin,
        ContentModerationPlugin,
        HarmfulContentPlugin,
        ResponseCacheByPromptPlugin,
        CachedToolResultPlugin,
        CircuitBreakerPlugin,
        ArgumentNormalizerPlugin,
        OutputLengthGuardPlugin,
        HeaderInjectorPlugin,
    )
}
