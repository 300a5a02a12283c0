"""SQL scan: lex a buffer as SQL, match whole words, fold per statement.

CPU reference of `ops/csrc/sql.hip`, plain Python and integer-exact, like
`ops/exfil.py`: the oracle for the HIP kernel in tests AND the code the
sql_sanitizer plugin runs per string, so the CPU chain and the oracle are one
code path.

The *lexer* is a byte-level state machine over the whole buffer with the
states CODE, SQUOTE, DQUOTE, LINE and BLOCK; it starts in CODE.

  CODE, in this priority: `'` enters SQUOTE; `"` enters DQUOTE; `--` enters
    LINE and `/*` enters BLOCK (both bytes are consumed, so `/*/` does not
    close itself; the comment begins at the first byte); `;` closes the
    statement; a maximal run of [A-Za-z0-9_] is a *word*; any other byte is
    skipped.
  SQUOTE: `'` returns to CODE, so a doubled `''` closes and reopens.
  DQUOTE: `"` returns to CODE.
  LINE:   `\\n` returns to CODE; the newline is not part of the comment.
  BLOCK:  `*/` returns to CODE after both bytes. Comments do not nest.

In *boundary mode* (dquote_boundary) a `"` in ANY state is a field boundary:
it ends an open comment, returns to CODE and closes the statement; DQUOTE is
never entered. That is how the GPU pipeline scans a raw JSON span: every
string value sits between two boundaries and is lexed as the plugin lexes it
on its own in text mode.

Dialect limits: backticks, `[...]` identifiers, `#` comments, dollar quoting
and backslash escapes inside strings are not SQL syntax here — those bytes
are plain code (or plain string) bytes.

A word of length L *matches* keyword i when the search automaton, run over
the word alone, reports pattern i and kw_len[i] == L: an automaton that
accepts pattern i after exactly len(pattern i) bytes from the start state has
matched the whole word. So `xdrop`, `drops`, `_drop` and `drop1` are not
`drop`, and a word longer than the longest keyword matches nothing.

Keywords 0..4 are the structural words delete, from, update, set, where; the
configured blocked words follow from bit 5. Every match sets its bit in the
open *statement*'s mask. A statement closes at `;`, at a boundary and at the
end of the data; one whose mask is non-zero counts as a keyword statement.
On close, delete and from without where is the finding
`delete_without_where` at the statement's first delete, update and set
without where is `update_without_where` at its first update (asking for
from / set keeps `SELECT … FOR UPDATE` and `ON DUPLICATE KEY UPDATE` clean; a
WHERE inside a subquery counts). A blocked word is the finding
`blocked:<word>` wherever it stands in code.
"""

from __future__ import annotations

from typing import List, Sequence, Tuple

from . import dfa

STRUCTURAL = ["delete", "from", "update", "set", "where"]
KW_DELETE, KW_FROM, KW_UPDATE, KW_SET, KW_WHERE = (1 << i for i in range(5))
N_STRUCTURAL = len(STRUCTURAL)

DEFAULT_BLOCKED = ["drop", "truncate", "alter", "grant", "revoke"]

# Limits of a blocked-word list (the kernel stages the tables in LDS and walks
# words of up to KW_MAX_LEN + 1 bytes). KW_TABLE_LIMIT is
# hip.SQL_SCAN_TABLE_LIMIT / FORGE_SQL_SCAN_TABLE_LIMIT in csrc/forge_api.h.
KW_MAX_WORDS = 24
KW_MIN_LEN, KW_MAX_LEN = 2, 16
KW_TABLE_LIMIT = 16 * 1024

CODE, SQUOTE, DQUOTE, LINE, BLOCK = range(5)

_WORD = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_")


def table_bytes(n_states: int, n_classes: int) -> int:
    """hip.scan_table_bytes, here so that the CPU chain needs no torch."""
    return n_states * n_classes * 2 + 256 + n_states * 4


def compile_sql_keywords(blocked: Sequence[str]) -> Tuple[dfa.ScanTables, List[int]]:
    """Blocked-word list → (case-insensitive literal DFA over the structural
    keywords followed by the blocked words, length of each keyword)."""
    cfg = [str(w) for w in blocked]
    if not 1 <= len(cfg) <= KW_MAX_WORDS:
        raise ValueError(f"need 1 to {KW_MAX_WORDS} blocked words, got {len(cfg)}")
    seen = set(STRUCTURAL)
    for w in cfg:
        if not KW_MIN_LEN <= len(w) <= KW_MAX_LEN or any(ord(c) not in _WORD for c in w):
            raise ValueError(f"blocked word {w!r} must be {KW_MIN_LEN} to {KW_MAX_LEN} bytes of [A-Za-z0-9_]")
        if w.lower() in seen:
            raise ValueError(f"blocked word {w!r} is a structural keyword or listed twice")
        seen.add(w.lower())
    words = STRUCTURAL + cfg
    tables = dfa.compile_literals(words, case_insensitive=True)
    if table_bytes(tables.n_states, tables.n_classes) > KW_TABLE_LIMIT:
        raise ValueError(f"keyword tables need {table_bytes(tables.n_states, tables.n_classes)} bytes, "
                         f"limit {KW_TABLE_LIMIT}")
    kw_len = [len(w) for w in words]
    assert kw_len == list(tables.max_len)
    return tables, kw_len


def keyword_names(tables: dfa.ScanTables) -> List[str]:
    """The keywords of tables from compile_sql_keywords, lower case (the
    patterns are the words with '_' escaped)."""
    return [p.replace("\\", "").lower() for p in tables.patterns]


Finding = Tuple[int, int, str]   # (beg, len, category)


def sql_scan_reference(data: bytes, tables: dfa.ScanTables, kw_len: Sequence[int], dquote_boundary: bool
                       ) -> Tuple[List[Finding], List[Tuple[int, int]], Tuple[int, int, int, int], int,
                                  Tuple[int, int], int]:
    """→ (findings, comments, counts, blocked_mask, first, flags) over the whole buffer.

    findings: (beg, len, category) in the order they are established;
    comments: (beg, len) of every comment, one still open at the end of the
    data running to the end. The last four are what the kernel reports per
    request: counts = (keyword statements, delete_without_where,
    update_without_where, comments), blocked_mask with bit i - 5 set for
    blocked keyword i, first = (beg, len) of the finding with the smallest
    begin — (-1, 0) if none — and flags with bit 0 set when the buffer holds
    a backslash or a byte >= 0x80."""
    n = len(data)
    words = keyword_names(tables)
    max_kw = max(kw_len)
    findings: List[Finding] = []
    comments: List[Tuple[int, int]] = []
    blocked_mask = 0
    n_stmt = n_dww = n_uww = 0
    stmt = {"mask": 0, "del": -1, "upd": -1}

    def close_stmt() -> None:
        nonlocal n_stmt, n_dww, n_uww
        mask = stmt["mask"]
        if mask:
            n_stmt += 1
            if mask & KW_DELETE and mask & KW_FROM and not mask & KW_WHERE:
                n_dww += 1
                findings.append((stmt["del"], 6, "delete_without_where"))
            if mask & KW_UPDATE and mask & KW_SET and not mask & KW_WHERE:
                n_uww += 1
                findings.append((stmt["upd"], 6, "update_without_where"))
        stmt["mask"], stmt["del"], stmt["upd"] = 0, -1, -1

    state, com_beg, i = CODE, 0, 0
    while i < n:
        b = data[i]
        if dquote_boundary and b == 0x22:
            if state in (LINE, BLOCK):
                comments.append((com_beg, i - com_beg))
            state = CODE
            close_stmt()
            i += 1
        elif state == CODE:
            if b == 0x27:
                state = SQUOTE
                i += 1
            elif b == 0x22:
                state = DQUOTE
                i += 1
            elif b == 0x2D and i + 1 < n and data[i + 1] == 0x2D:
                state, com_beg = LINE, i
                i += 2
            elif b == 0x2F and i + 1 < n and data[i + 1] == 0x2A:
                state, com_beg = BLOCK, i
                i += 2
            elif b == 0x3B:
                close_stmt()
                i += 1
            elif b in _WORD:
                j = i + 1
                while j < n and data[j] in _WORD:
                    j += 1
                length = j - i
                if length <= max_kw:
                    m = dfa.match_mask_reference(tables, data[i:j])
                    for k, kl in enumerate(kw_len):
                        if m >> k & 1 and kl == length:
                            if k == 0 and not stmt["mask"] & KW_DELETE:
                                stmt["del"] = i
                            if k == 2 and not stmt["mask"] & KW_UPDATE:
                                stmt["upd"] = i
                            stmt["mask"] |= 1 << k
                            if k >= N_STRUCTURAL:
                                findings.append((i, length, f"blocked:{words[k]}"))
                                blocked_mask |= 1 << (k - N_STRUCTURAL)
                i = j
            else:
                i += 1
        elif state == SQUOTE:
            if b == 0x27:
                state = CODE
            i += 1
        elif state == DQUOTE:
            if b == 0x22:
                state = CODE
            i += 1
        elif state == LINE:
            if b == 0x0A:
                comments.append((com_beg, i - com_beg))
                state = CODE
            i += 1
        else:
            if b == 0x2A and i + 1 < n and data[i + 1] == 0x2F:
                comments.append((com_beg, i + 2 - com_beg))
                state = CODE
                i += 2
            else:
                i += 1
    if state in (LINE, BLOCK):
        comments.append((com_beg, n - com_beg))
    close_stmt()

    first = (-1, 0)
    for beg, length, _cat in findings:
        if first[0] < 0 or beg < first[0]:
            first = (beg, length)
    flags = 1 if any(b == 0x5C or b >= 0x80 for b in data) else 0
    return findings, comments, (n_stmt, n_dww, n_uww, len(comments)), blocked_mask, first, flags
