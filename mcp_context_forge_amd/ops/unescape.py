"""JSON string unescape over raw bytes: what the raw-byte prefilters scan when
`gpu_unescape` is on.

CPU reference of `ops/csrc/unescape.hip`, plain Python on bytes with no JSON
parser, like `ops/unicode.py`: the oracle for the HIP kernel in tests.

The span `blob[begin:end]` is walked left to right.

* A byte other than a backslash is copied.
* A backslash followed inside the span by one of `" \\ / b f n r t` emits the
  one decoded byte and consumes two bytes.
* `\\u` followed inside the span by four hex digits of either case is a code
  unit c. Outside D800..DFFF it emits the UTF-8 of c (1 to 3 bytes) and
  consumes 6 bytes. A high surrogate (D800..DBFF) immediately followed inside
  the span by `\\u` and four hex digits d in DC00..DFFF emits the 4-byte UTF-8
  of 0x10000 + ((c - 0xD800) << 10) + (d - 0xDC00) and consumes 12 bytes. Any
  other surrogate is LONE: it emits EF BF BD (U+FFFD) and consumes 6 bytes.
* Anything else is BAD: a backslash as the span's last byte, before any other
  byte, or before `u` with fewer than four hex digits inside the span. The
  backslash is copied as a plain byte and the walk goes on with the next byte.

Every form emits fewer bytes than it consumes, or as many, so the output is
never longer than the input.

Flags: HAD_ESCAPE an escape was decoded (a LONE one included, a BAD backslash
not); QUOTE a decoded U+0022; BACKSLASH a decoded U+005C or a BAD backslash
that was copied; BAD; LONE; NUL a decoded U+0000; NON_ASCII a decoded code
point >= 0x80, the U+FFFD of a LONE surrogate included. A span with a ROUTE_MASK
bit holds a value whose decoded bytes do not stand verbatim between its quotes
(gpu/pipeline.py), so its row runs the exact CPU chain.
"""

from __future__ import annotations

from typing import Tuple

HAD_ESCAPE, QUOTE, BACKSLASH, BAD, LONE, NUL, NON_ASCII = (1 << k for k in range(7))
ROUTE_MASK = QUOTE | BACKSLASH | BAD | LONE | NUL

_SHORT = {0x22: 0x22, 0x5C: 0x5C, 0x2F: 0x2F, ord("b"): 8, ord("f"): 12, ord("n"): 10, ord("r"): 13, ord("t"): 9}
_HEX = {ord(ch): int(ch, 16) for ch in "0123456789abcdefABCDEF"}


def _unit(blob: bytes, p: int, end: int) -> int:
    """The code unit of `\\uXXXX` at p when all six bytes lie in [p, end), else -1."""
    if p + 6 > end or blob[p] != 0x5C or blob[p + 1] != ord("u"):
        return -1
    c = 0
    for b in blob[p + 2:p + 6]:
        if b not in _HEX:
            return -1
        c = c << 4 | _HEX[b]
    return c


def json_unescape_reference(blob: bytes, begin: int, end: int) -> Tuple[bytes, int]:
    """→ (the decoded bytes of blob[begin:end], the flag bits)."""
    out = bytearray()
    flags = 0
    p = begin
    while p < end:
        b = blob[p]
        if b != 0x5C:
            out.append(b)
            p += 1
            continue
        c = _unit(blob, p, end)
        if p + 1 < end and blob[p + 1] in _SHORT:
            cp, used = _SHORT[blob[p + 1]], 2
        elif c < 0:
            flags |= BAD | BACKSLASH
            out.append(b)
            p += 1
            continue
        elif not 0xD800 <= c <= 0xDFFF:
            cp, used = c, 6
        else:
            d = _unit(blob, p + 6, end) if c <= 0xDBFF else -1
            if 0xDC00 <= d <= 0xDFFF:
                cp, used = 0x10000 + ((c - 0xD800) << 10) + (d - 0xDC00), 12
            else:
                flags |= LONE
                cp, used = 0xFFFD, 6
        flags |= HAD_ESCAPE
        flags |= QUOTE if cp == 0x22 else BACKSLASH if cp == 0x5C else NUL if cp == 0 else NON_ASCII if cp >= 0x80 else 0
        out += chr(cp).encode()
        p += used
    return bytes(out), flags
