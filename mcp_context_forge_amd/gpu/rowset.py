"""RowSet: the tools/call rows of one batch that are still on the fast path.

The per-row arrays travel together and are narrowed together: `keep()` is
the only place that drops rows, so no array can fall out of step with the
others. Next to them sit the batch constants every stage needs — the joined
byte blob, the envelope spans, the response list and the ToolTable snapshot
the batch resolved its `tool_idx` against — and the few ways a stage answers
a row itself (block, JSON-RPC error, result). Each plugin's block message is
formatted here and nowhere else; the CPU plugins produce the same bytes.
"""

from __future__ import annotations

import json
from typing import Any, Iterable, List, Optional

import numpy as np

from ..plugins.builtin import PII_PATTERNS
from ..protocol import jsonrpc

PII_NAMES = [n for (n, _, _) in PII_PATTERNS]   # fixed index order of the C matchers
INVALID_ARGS = "invalid arguments"
BAD_ARGS = object()   # decode_args: the span was not JSON and the row is answered


def msg_deny(word: str) -> str:
    return f"deny_filter: deny word {word!r} present"


def msg_pii(found: Iterable[str]) -> str:
    return f"pii_filter: PII detected: {sorted(set(found))}"


def msg_pii_bits(bits: int) -> str:
    return msg_pii(n for i, n in enumerate(PII_NAMES) if (bits >> i) & 1)


def msg_harm(cat: str) -> str:
    return f"harmful_content_detector: harmful content ({cat})"


def msg_moderation(cat: str, score: float) -> str:
    return f"content_moderation: moderation: category {cat} score {score:.3f}"


def msg_schema(errs: List[str]) -> str:
    return "schema_guard: schema violation: " + "; ".join(errs[:5])


def splice_result(id_bytes: bytes, result_bytes: bytes) -> bytes:
    return b'{"jsonrpc":"2.0","id":' + id_bytes + b',"result":' + result_bytes + b"}"


def splice_error(id_bytes: Optional[bytes], code: int, message: str) -> Optional[bytes]:
    if id_bytes is None:
        return None
    return (b'{"jsonrpc":"2.0","id":' + id_bytes + b',"error":{"code":' + str(code).encode()
            + b',"message":' + json.dumps(message).encode() + b"}}")


class RowSet:
    """Row j of every PER_ROW array describes request `rows[j]` of the batch.
    `counters` is whatever owns the `blocked` / `cache_hits` counts (the
    pipeline)."""

    PER_ROW = ("rows", "uh", "tool_idx", "nb", "ne", "id_b", "id_e", "args_b", "args_e")
    __slots__ = PER_ROW + ("blob", "env", "responses", "tools", "counters")

    def __init__(self, rows, uh, tool_idx, nb, ne, id_b, id_e, args_b, args_e,
                 blob, env, responses, tools, counters):
        self.rows, self.uh, self.tool_idx = rows, uh, tool_idx
        self.nb, self.ne, self.id_b, self.id_e = nb, ne, id_b, id_e
        self.args_b, self.args_e = args_b, args_e
        self.blob, self.env, self.responses = blob, env, responses
        self.tools, self.counters = tools, counters

    def __len__(self) -> int:
        return self.rows.shape[0]

    def keep(self, mask: np.ndarray) -> None:
        """Narrow every per-row array to the rows where `mask` is true."""
        for f in self.PER_ROW:
            setattr(self, f, np.ascontiguousarray(getattr(self, f)[mask]))

    def meta(self, j: int):
        return self.tools.metas[self.tool_idx[j]]

    def id_bytes(self, j: int) -> Optional[bytes]:
        b = int(self.id_b[j])
        if b < 0:   # a notification: nothing is answered
            return None
        return self.blob[b:int(self.id_e[j])].tobytes()

    def error(self, j: int, code: int, message: str) -> None:
        self.responses[int(self.rows[j])] = splice_error(self.id_bytes(j), code, message)

    def block(self, j: int, message: str) -> None:
        """POLICY_DENIED with a plugin's message; counts as blocked."""
        self.error(j, jsonrpc.POLICY_DENIED, message)
        self.counters.blocked += 1

    def result(self, j: int, result_bytes: bytes) -> None:
        idb = self.id_bytes(j)
        if idb is not None:
            self.responses[int(self.rows[j])] = splice_result(idb, result_bytes)

    def answer_cached(self, j: int, result_bytes: Optional[bytes]) -> None:
        """A semantic-cache hit: the slot's stored result, if it still has one."""
        if result_bytes is not None:
            self.result(j, result_bytes)
        self.counters.cache_hits += 1

    def parse_args(self, j: int) -> Any:
        return json.loads(self.blob[self.args_b[j]:self.args_e[j]].tobytes() or b"{}")

    def decode_args(self, j: int) -> Any:
        """The row's argument span decoded, or BAD_ARGS after answering it."""
        try:
            return self.parse_args(j)
        except Exception:
            self.error(j, jsonrpc.INVALID_PARAMS, INVALID_ARGS)
            return BAD_ARGS
