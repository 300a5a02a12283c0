"""Tool-argument schema check: a JSON structure walk against compiled schemas.

CPU side of `ops/csrc/schema.hip`: `compile_schemas` lays the tables out,
`validate_table` checks their bytes before upload and
`schema_check_reference` is the oracle the kernel equals in every integer on
any bytes. It is NOT what schema_guard runs on the CPU chain: that stays
`utils/jsonschema.validate`. The walk is exact towards it in one direction
only: for a span `json.loads` accepts, PASS implies `validate(json.loads(span)
or {}, schema) == []` and FAIL implies a non-empty list; PUNT says nothing and
the caller runs `validate`.

*Tables.* Little-endian records, back to back:
  tool  (24 bytes) u32 prop_beg, prop_cnt, flags (1 compiled, 2 additional
                   properties forbidden), pad; u64 required (bit p: property p)
  prop  (40 bytes) u32 key_hash, key_off, key_len, tflags; i64 lo, hi;
                   u32 enum_beg, enum_cnt
  enum  (16 bytes) i64 value; u32 off, len
plus one byte pool that holds the keys and the string enum entries. `tflags`
is the 7-bit type mask (string, integer, number, boolean, null, object, array;
all seven when the property names no type) and F_BOUND, F_LENGTH, F_ENUM.
`[lo, hi]` is the inclusive value bound of a numeric property or the length
bound of a string one. An enum entry of a string property is (hash, off, len),
one of an integer property its value. `const` is an enum of one entry. A hash
is sum(c[i] * HASH_B ** (len - 1 - i)) mod 2^32; it only selects what is
byte-compared.
"""

from __future__ import annotations

import struct
from typing import Any, List, NamedTuple, Optional, Sequence, Tuple

T_STRING, T_INTEGER, T_NUMBER, T_BOOLEAN, T_NULL, T_OBJECT, T_ARRAY = (1 << k for k in range(7))
T_ANY = 0x7F
TYPE_BITS = {"string": T_STRING, "integer": T_INTEGER, "number": T_NUMBER, "boolean": T_BOOLEAN,
             "null": T_NULL, "object": T_OBJECT, "array": T_ARRAY}
F_BOUND, F_LENGTH, F_ENUM = 0x100, 0x200, 0x400
TOOL_COMPILED, TOOL_NO_ADDITIONAL = 1, 2

PASS, FAIL, PUNT = 0, 1, 2
MISSING_REQUIRED, TYPE, ENUM, BOUND, LENGTH, ADDITIONAL = (1 << k for k in range(6))
BACKSLASH, NON_ASCII, NOT_OBJECT, LONG, DUP_KEY, NUMBER_FORM, NO_TABLE = (1 << k for k in range(7))

TOOL_FMT, PROP_FMT, ENUM_FMT = "<IIIIQ", "<IIIIqqII", "<qII"
TOOL_BYTES, PROP_BYTES, ENUM_BYTES = 24, 40, 16
MAX_PROPS_PER_TOOL = 64
MAX_KEY = 64            # bytes of a key, of a string enum entry and of a number token
MAX_DIGITS = 18
INT_LIMIT = 1 << 62     # |v| of every integer in a schema stays below it; the open bounds are -+ it
MAX_TOOLS, MAX_PROPS, MAX_ENUMS, POOL_MAX = 4096, 1 << 18, 1 << 20, 1 << 24
LDS_TOOLS, LDS_PROPS = 64, 256   # tables up to both are staged into LDS
HASH_B = 0x01000193

_TOP_KEYS = {"type", "properties", "required", "additionalProperties", "description", "title", "$schema"}
_PROP_KEYS = {"type", "enum", "const", "minimum", "maximum", "exclusiveMinimum", "exclusiveMaximum", "minLength",
              "maxLength", "description", "title", "default", "examples", "format"}
_WS = b" \t\n\r"


class SchemaTable(NamedTuple):
    tools: bytes
    props: bytes
    enums: bytes
    pool: bytes
    compiled: Tuple[bool, ...]

    @property
    def n_tools(self) -> int:
        return len(self.tools) // TOOL_BYTES

    @property
    def n_props(self) -> int:
        return len(self.props) // PROP_BYTES

    @property
    def n_enums(self) -> int:
        return len(self.enums) // ENUM_BYTES

    @property
    def in_lds(self) -> bool:
        return self.n_tools <= LDS_TOOLS and self.n_props <= LDS_PROPS


def key_hash(b: bytes) -> int:
    h = 0
    for c in b:
        h = (h * HASH_B + c) & 0xFFFFFFFF
    return h


def _text(s: Any, min_len: int) -> Optional[bytes]:
    """The bytes of a key or a string enum entry the walk can compare, or None."""
    if not isinstance(s, str) or not min_len <= len(s) <= MAX_KEY:
        return None
    if not all(0x20 <= ord(c) < 0x80 and c not in '"\\' for c in s):
        return None
    return s.encode()


def _int(v: Any) -> bool:
    return isinstance(v, int) and not isinstance(v, bool) and -INT_LIMIT < v < INT_LIMIT


def _compile_prop(sub: Any) -> Optional[Tuple[int, int, int, Optional[list]]]:
    """→ (tflags, lo, hi, enum entries or None) of one property schema, or None."""
    if not isinstance(sub, dict) or not set(sub) <= _PROP_KEYS:
        return None
    ty = sub.get("type")
    names = ty if isinstance(ty, list) else [ty] if ty is not None else list(TYPE_BITS)
    if not names or not all(isinstance(t, str) and t in TYPE_BITS for t in names):
        return None
    tflags, lo, hi, entries = sum({TYPE_BITS[t] for t in names}), -INT_LIMIT, INT_LIMIT, None
    if "enum" in sub or "const" in sub:
        want = sub.get("enum", [])
        if ty not in ("string", "integer") or not isinstance(want, list):
            return None
        want = want + ([sub["const"]] if "const" in sub else [])
        entries = [_text(e, 0) for e in want] if ty == "string" else [e if _int(e) else None for e in want]
        if any(e is None for e in entries):
            return None
        if "const" in sub:   # both: the const, if the enum lists it
            entries = entries[-1:] if "enum" not in sub or entries[-1] in entries[:-1] else []
        tflags |= F_ENUM
    bounds = [k for k in ("minimum", "maximum", "exclusiveMinimum", "exclusiveMaximum") if k in sub]
    if bounds:
        if ty not in ("integer", "number") or not all(_int(sub[k]) for k in bounds):
            return None
        lo = max([lo] + [sub[k] for k in bounds if k == "minimum"] + [sub[k] + 1 for k in bounds if k == "exclusiveMinimum"])
        hi = min([hi] + [sub[k] for k in bounds if k == "maximum"] + [sub[k] - 1 for k in bounds if k == "exclusiveMaximum"])
        tflags |= F_BOUND
    lengths = [k for k in ("minLength", "maxLength") if k in sub]
    if lengths:
        if ty != "string" or not all(_int(sub[k]) for k in lengths):
            return None
        lo, hi = sub.get("minLength", lo), sub.get("maxLength", hi)
        tflags |= F_LENGTH
    return tflags, lo, hi, entries


def _compile_tool(schema: Any) -> Optional[Tuple[List[tuple], int, int]]:
    """→ ([(key, tflags, lo, hi, entries)], required mask, tool flags), or None
    when the schema is outside what the walk decides."""
    if not isinstance(schema, dict) or not set(schema) <= _TOP_KEYS or schema.get("type", "object") != "object":
        return None
    props, required, extra = schema.get("properties", {}), schema.get("required", []), schema.get("additionalProperties", True)
    if not isinstance(props, dict) or not isinstance(required, list) or not isinstance(extra, bool):
        return None
    # `validate` takes "known" from `properties` alone: where additional properties are forbidden, a key that only
    # `required` names is demanded and rejected at once, which a property record cannot say
    if not extra and not all(isinstance(k, str) and k in props for k in required):
        return None
    out, index = [], {}
    for k, sub in list(props.items()) + [(k, {}) for k in required if not (isinstance(k, str) and k in props)]:
        kb, rec = _text(k, 1), _compile_prop(sub)
        if kb is None or rec is None:
            return None
        if kb not in index:   # a key that `required` names twice
            index[kb] = len(out)
            out.append((kb,) + rec)
    if len(out) > MAX_PROPS_PER_TOOL:
        return None
    return out, sum({1 << index[k.encode()] for k in required}), TOOL_COMPILED | (0 if extra else TOOL_NO_ADDITIONAL)


def compile_schemas(schemas: Sequence[Any]) -> SchemaTable:
    """One entry per tool, in tool-table order: its input schema, or None for a
    tool the kernel is not to judge. A schema outside the compilable subset
    (the issue's list: flat properties with type, enum / const, integer
    bounds, string lengths, required, boolean additionalProperties), or one
    that forbids additional properties and requires a key `properties` does
    not name, leaves its tool uncompiled, and the walk answers NO_TABLE for it."""
    tools, props, enums, pool, compiled = [], [], [], bytearray(), []

    def put(b: bytes) -> int:
        pool.extend(b)
        return len(pool) - len(b)

    for schema in schemas:
        c = _compile_tool(schema) if schema is not None else None
        compiled.append(c is not None)
        if c is None:
            tools.append(struct.pack(TOOL_FMT, 0, 0, 0, 0, 0))
            continue
        recs, required, flags = c
        tools.append(struct.pack(TOOL_FMT, len(props), len(recs), flags, 0, required))
        for kb, tflags, lo, hi, entries in recs:
            props.append(struct.pack(PROP_FMT, key_hash(kb), put(kb), len(kb), tflags, lo, hi, len(enums), len(entries or ())))
            for e in entries or ():
                enums.append(struct.pack(ENUM_FMT, key_hash(e), put(e), len(e)) if isinstance(e, bytes)
                             else struct.pack(ENUM_FMT, e, 0, 0))
    table = SchemaTable(b"".join(tools), b"".join(props), b"".join(enums), bytes(pool), tuple(compiled))
    validate_table(table)
    return table


def validate_table(t: SchemaTable) -> None:
    """Raises ValueError unless every index the kernel forms from the table
    stays inside it: record sizes and counts, property and enum ranges, pool
    ranges, key lengths, a required mask within the property count."""
    if len(t.tools) % TOOL_BYTES or len(t.props) % PROP_BYTES or len(t.enums) % ENUM_BYTES:
        raise ValueError("schema table: a partial record")
    if t.n_tools > MAX_TOOLS or t.n_props > MAX_PROPS or t.n_enums > MAX_ENUMS or len(t.pool) > POOL_MAX:
        raise ValueError("schema table: too many tools, properties, enum entries or pool bytes")
    for i in range(t.n_tools):
        beg, cnt, flags, _pad, required = struct.unpack_from(TOOL_FMT, t.tools, i * TOOL_BYTES)
        if flags & ~(TOOL_COMPILED | TOOL_NO_ADDITIONAL) or cnt > MAX_PROPS_PER_TOOL or beg + cnt > t.n_props \
                or required >> cnt:
            raise ValueError(f"schema table: tool {i} is out of range")
    for i in range(t.n_props):
        _h, off, klen, tflags, lo, hi, ebeg, ecnt = struct.unpack_from(PROP_FMT, t.props, i * PROP_BYTES)
        if not 1 <= klen <= MAX_KEY or off + klen > len(t.pool) or ebeg + ecnt > t.n_enums \
                or tflags & ~(T_ANY | F_BOUND | F_LENGTH | F_ENUM) or not -INT_LIMIT <= lo <= INT_LIMIT \
                or not -INT_LIMIT <= hi <= INT_LIMIT:
            raise ValueError(f"schema table: property {i} is out of range")
        if tflags & F_ENUM and tflags & T_ANY == T_STRING:
            for e in range(ebeg, ebeg + ecnt):
                _v, eoff, elen = struct.unpack_from(ENUM_FMT, t.enums, e * ENUM_BYTES)
                if elen > MAX_KEY or eoff + elen > len(t.pool):
                    raise ValueError(f"schema table: enum entry {e} is out of range")


def _find(d: bytes, p: int, lim: int, stop: bytes) -> int:
    """The first index in [p, lim) whose byte is in `stop`, or lim."""
    while p < lim and d[p] not in stop:
        p += 1
    return p


def schema_check_reference(blob: bytes, beg: int, end: int, tool_idx: int, table: SchemaTable
                           ) -> Tuple[int, int, int, int]:
    """→ (verdict, fail, punt, seen) for the span blob[beg:end], n bytes d.

    verdict is PUNT if punt != 0, else FAIL if fail != 0, else PASS; with a
    punt, fail and seen are 0. seen has bit p for property p of the tool.

    1. tool_idx outside the table or an uncompiled tool: NO_TABLE alone.
    2. A backslash gives BACKSLASH; a byte >= 0x80 or a NUL byte gives
       NON_ASCII (json.loads guesses UTF-16 / 32 from NUL bytes). With either,
       punt is exactly those bits.
    3. Strings run from a '"' to the next '"'. Outside strings '{' '[' raise
       the depth and '}' ']' lower it (it may go negative). Whitespace is
       space, tab, LF, CR. The first non-whitespace byte must be '{', else
       NOT_OBJECT alone (an empty span too).
    4. The structural bytes are, outside strings: a '{' that raises the depth
       to 1, and ',' and ':' at depth 1. A string that opens at depth 1 while
       the last structural byte before it is '{' or ',' is a key. Keys are
       judged in order; the first punt of a key ends the walk.
    5. A key whose closing quote is not among the 65 bytes after its opening
       quote (the span end counts as none): LONG. The key is looked up in its
       tool's properties by hash and length, then byte-compared. Unknown:
       ADDITIONAL where the tool forbids additional properties; its value is
       not looked at. Known and met before: DUP_KEY. Then seen gains its bit.
    6. The value starts at the first non-whitespace byte after the first ':'
       (any ':', string or not) after the key's closing quote; no such byte:
       NUMBER_FORM. Its first byte gives the class: '"' string (to the next
       '"' or the span end; its length is the bytes between), '{' object, '['
       array, 't' 'f' boolean, 'n' null, a digit or '-' and a digit: number;
       anything else NUMBER_FORM.
    7. A number token ends before the next whitespace byte, ',' or '}' or at
       the span end; over 64 bytes: LONG. With '.', 'e' or 'E' in it it is a
       float. Otherwise it is an integer: a byte that is no digit after the
       optional '-': NUMBER_FORM; over 18 digits: LONG; else its exact value.
       A float on a property with a bound: NUMBER_FORM.
    8. A class outside the type mask (an integer satisfies integer and number,
       a float number, a boolean only boolean): TYPE, nothing else for this
       value. Else ENUM (string bytes or integer value among the entries),
       BOUND (lo <= value <= hi), LENGTH (lo <= byte count <= hi), each where
       the property has one.
    9. After the walk, a required property not seen: MISSING_REQUIRED.
    """
    if not 0 <= tool_idx < table.n_tools:
        return PUNT, 0, NO_TABLE, 0
    pbeg, pcnt, tflags_tool, _pad, required = struct.unpack_from(TOOL_FMT, table.tools, tool_idx * TOOL_BYTES)
    if not tflags_tool & TOOL_COMPILED:
        return PUNT, 0, NO_TABLE, 0
    d = bytes(blob[beg:end])
    n = len(d)
    punt = (BACKSLASH if 0x5C in d else 0) | (NON_ASCII if any(b >= 0x80 or b == 0 for b in d) else 0)
    first = _find(d, 0, n, bytes(set(range(256)) - set(_WS)))
    if not punt and (first == n or d[first] != 0x7B):
        punt = NOT_OBJECT
    if punt:
        return PUNT, 0, punt, 0
    props = [struct.unpack_from(PROP_FMT, table.props, (pbeg + p) * PROP_BYTES) for p in range(pcnt)]
    fail = seen = 0

    def key(q: int) -> int:
        """Judge the key whose opening quote is d[q] → its punt bit or 0."""
        nonlocal fail, seen
        ks = q + 1
        lim = min(n, ks + MAX_KEY + 1)
        ke = _find(d, ks, lim, b'"')
        if ke == lim:
            return LONG
        name = d[ks:ke]
        p = next((p for p, r in enumerate(props) if r[0] == key_hash(name) and r[2] == len(name)
                  and table.pool[r[1]:r[1] + r[2]] == name), -1)
        if p < 0:
            fail |= ADDITIONAL if tflags_tool & TOOL_NO_ADDITIONAL else 0
            return 0
        if seen >> p & 1:
            return DUP_KEY
        seen |= 1 << p
        _h, _off, _len, tflags, lo, hi, ebeg, ecnt = props[p]
        colon = _find(d, ke + 1, n, b":")
        v = _find(d, min(colon + 1, n), n, bytes(set(range(256)) - set(_WS)))
        if v == n:
            return NUMBER_FORM
        c, val, slen = d[v], None, 0
        if c == 0x22:
            cls, vs = T_STRING, v + 1
            slen = _find(d, vs, n, b'"') - vs
        elif c in b"{[tfn":
            cls = {0x7B: T_OBJECT, 0x5B: T_ARRAY, 0x74: T_BOOLEAN, 0x66: T_BOOLEAN, 0x6E: T_NULL}[c]
        elif 0x30 <= c <= 0x39 or (c == 0x2D and v + 1 < n and 0x30 <= d[v + 1] <= 0x39):
            lim = min(n, v + MAX_KEY + 1)
            te = _find(d, v, lim, _WS + b",}")
            if te - v > MAX_KEY:
                return LONG
            tok = d[v:te]
            if any(b in b".eE" for b in tok):
                cls = T_NUMBER
                if tflags & F_BOUND:
                    return NUMBER_FORM
            else:
                digits = tok[1:] if c == 0x2D else tok
                if not all(0x30 <= b <= 0x39 for b in digits):
                    return NUMBER_FORM
                if len(digits) > MAX_DIGITS:
                    return LONG
                cls, val = T_INTEGER | T_NUMBER, int(tok)
        else:
            return NUMBER_FORM
        if not cls & tflags:
            fail |= TYPE
            return 0
        if tflags & F_ENUM:
            entries = [struct.unpack_from(ENUM_FMT, table.enums, e * ENUM_BYTES) for e in range(ebeg, ebeg + ecnt)]
            if cls == T_STRING:
                s = d[vs:vs + slen]
                ok = any(el == slen and table.pool[eo:eo + el] == s for _v, eo, el in entries)
            else:
                ok = val is not None and any(ev == val for ev, _o, _l in entries)
            fail |= 0 if ok else ENUM
        if tflags & F_BOUND and val is not None and not lo <= val <= hi:
            fail |= BOUND
        if tflags & F_LENGTH and cls == T_STRING and not lo <= slen <= hi:
            fail |= LENGTH
        return 0

    in_str, depth, last_key = False, 0, False
    for i, b in enumerate(d):
        if in_str:
            in_str = b != 0x22
        elif b == 0x22:
            in_str = True
            if depth == 1 and last_key:
                punt = key(i)
                if punt:
                    return PUNT, 0, punt, 0
        elif b in b"{[":
            depth += 1
            if b == 0x7B and depth == 1:
                last_key = True
        elif b in b"}]":
            depth -= 1
        elif b in b",:" and depth == 1:
            last_key = b == 0x2C
    if required & ~seen:
        fail |= MISSING_REQUIRED
    return (FAIL if fail else PASS), fail, 0, seen
