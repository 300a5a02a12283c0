"""URL scan: find every URL of a buffer, delimit its host, judge it.

CPU reference of `ops/csrc/url.hip`, plain Python and integer-exact, like
`ops/sql.py`: the oracle for the HIP kernel in tests AND the code the
url_reputation plugin runs per string, so the CPU chain and the oracle are one
code path. It slices `bytes` and looks domains up in a `dict`; the hash table
that `compile_domains` builds for the kernel is an implementation detail that
must reproduce this exact string matching.

A *URL* is every offset p with data[p:p+3] == b"://" (all three bytes inside
the buffer) whose *scheme*, the run of [A-Za-z0-9+.-] that ends at p - 1, has
a length L >= 1; counting stops at SCHEME_MAX. The scheme is https when L == 5
and the bytes are `https` in any case, http when L == 4 likewise, anything
else is OTHER_SCHEME. The URL begins at p - L. Every candidate is judged on
its own: URLs do not consume one another, so all outputs are sums, ORs and
minima.

The *authority* runs from a = p + 3 to e, the first terminator at or after a
or the buffer end. Terminators are every byte <= 0x20, 0x7F and the bytes of
TERMINATORS. An authority longer than AUTH_MAX is OVERLONG: the URL is
reported with the length a + AUTH_MAX - begin and its host is not analysed.
Otherwise the reported length is e - begin.

*Host analysis*: the last `@` of the authority sets USERINFO and the host
begins after it; a host whose first byte is `[` is BRACKET and is not analysed
further; the first `:` ends the host; every trailing `.` is stripped; an empty
host is EMPTY_HOST. Of a non-empty host: NUMERIC when every byte is in
[0-9.], NON_ASCII when some byte is >= 0x80, PUNYCODE when some label begins
with `xn--` in any case. A *label start* is an s that is the first host byte
or follows a `.`, and is no `.` itself. For every label start the suffix
host[s:], with A-Z lower-cased, is looked up in the domain table and the tags
of all matches are ORed: with tag ALLOW the URL is *allowed* — counted, and
contributing nothing else — else with tag BLOCK it is BLOCKED.
"""

from __future__ import annotations

from typing import Dict, Iterable, List, NamedTuple, Tuple

import numpy as np

(BLOCKED, HTTP, OTHER_SCHEME, NUMERIC, BRACKET, USERINFO, PUNYCODE, NON_ASCII, OVERLONG,
 EMPTY_HOST) = (1 << i for i in range(10))
ALL_BITS = (1 << 10) - 1
CATEGORY_NAMES = {BLOCKED: "blocked_domain", HTTP: "non_https", OTHER_SCHEME: "other_scheme",
                  NUMERIC: "numeric_host", BRACKET: "bracket_host", USERINFO: "userinfo",
                  PUNYCODE: "punycode_host", NON_ASCII: "non_ascii_host", OVERLONG: "overlong_authority",
                  EMPTY_HOST: "empty_host"}
SCHEME_BITS = HTTP | OTHER_SCHEME
HEURISTIC_BITS = NUMERIC | BRACKET | USERINFO | PUNYCODE | NON_ASCII | OVERLONG

TAG_BLOCK, TAG_ALLOW = 1, 2

SCHEME_MAX = 16
AUTH_MAX = 256
TERMINATORS = b"\"'<>/?#\\`,;(){}|^"

_SCHEME = frozenset(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+.-")
_TERM = frozenset(range(0x21)) | {0x7F} | frozenset(TERMINATORS)
_NUMERIC = frozenset(b"0123456789.")
_DOMAIN = frozenset(b"abcdefghijklmnopqrstuvwxyz0123456789._-")
_UPPER = bytes(range(65, 91))
_LOWER = bytes(range(97, 123))
_FOLD = bytes.maketrans(_UPPER, _LOWER)

# Limits of a domain table. The kernel probes tables of up to LDS_SLOTS slots
# in LDS and larger ones in global memory; LDS_SLOTS is hip.URL_SCAN_LDS_SLOTS
# / FORGE_URL_SCAN_LDS_SLOTS in csrc/forge_api.h, MAX_SLOTS FORGE_URL_SCAN_MAX_SLOTS.
DOMAIN_MAX_LEN = 253
MAX_DOMAINS = 1 << 19
MAX_SLOTS = 1 << 20
LDS_SLOTS = 1024

# The table's hashes, shared with url.hip (URL_B1, URL_B2, URL_MIX): both are
# the polynomial sum(c[j] * B ** (n - 1 - j)) mod 2 ** 32 over the lower-cased
# bytes. H1 picks the first slot, H2 is the key the slot stores.
HASH_B1 = 0x01000193
HASH_B2 = 0x9E3779B1
HASH_MIX = 0x85EBCA6B
N_POWERS = AUTH_MAX
_M32 = 0xFFFFFFFF


def _poly(raw: bytes, base: int) -> int:
    h = 0
    for c in raw:
        h = (h * base + c) & _M32
    return h


def first_slot(h1: int, n_slots: int) -> int:
    return (((h1 * HASH_MIX) & _M32) >> 12) & (n_slots - 1)


class DomainTable(NamedTuple):
    """What compile_domains builds. `domains` is what the reference uses;
    `slots` u32[n_slots, 4] (key H2, tag or 0 for an empty slot, offset and
    length in the pool), `pool` u8 (every domain, lower case, back to back)
    and `powers` u32[2, N_POWERS] (B1 ** i, B2 ** i) are what the kernel uses."""
    domains: Dict[bytes, int]
    slots: np.ndarray
    pool: np.ndarray
    powers: np.ndarray

    @property
    def n_slots(self) -> int:
        return int(self.slots.shape[0])


def _domain_bytes(d) -> bytes:
    raw = (d.encode("utf-8", "surrogatepass") if isinstance(d, str) else bytes(d)).translate(_FOLD)
    if not 1 <= len(raw) <= DOMAIN_MAX_LEN or any(c not in _DOMAIN for c in raw):
        raise ValueError(f"domain {d!r} must be 1 to {DOMAIN_MAX_LEN} bytes of [a-z0-9._-]")
    if raw[0] == 0x2E or raw[-1] == 0x2E or b".." in raw:
        raise ValueError(f"domain {d!r} has a leading or trailing dot or an empty label")
    return raw


def compile_domains(blocked: Iterable, allowed: Iterable = ()) -> DomainTable:
    """Blocked and allowed domain lists → DomainTable: an open-addressed
    table with a power-of-two slot count and a load of at most one half,
    filled by linear probing from first_slot(H1), plus the byte pool."""
    domains: Dict[bytes, int] = {}
    for tag, items in ((TAG_BLOCK, blocked), (TAG_ALLOW, allowed)):
        for d in items:
            raw = _domain_bytes(d)
            if raw in domains:
                raise ValueError(f"domain {d!r} is listed twice")
            domains[raw] = tag
    if len(domains) > MAX_DOMAINS:
        raise ValueError(f"at most {MAX_DOMAINS} domains, got {len(domains)}")
    n_slots = 2
    while n_slots < 2 * len(domains):
        n_slots *= 2
    slots = np.zeros((n_slots, 4), dtype=np.uint32)
    used = bytearray(n_slots)
    off = 0
    for raw, tag in domains.items():
        i = first_slot(_poly(raw, HASH_B1), n_slots)
        while used[i]:
            i = (i + 1) & (n_slots - 1)
        used[i] = 1
        slots[i] = (_poly(raw, HASH_B2), tag, off, len(raw))
        off += len(raw)
    pool = np.frombuffer(b"".join(domains) or b"\0", dtype=np.uint8).copy()
    powers = np.empty((2, N_POWERS), dtype=np.uint32)
    for row, base in enumerate((HASH_B1, HASH_B2)):
        v = 1
        for i in range(N_POWERS):
            powers[row, i] = v
            v = (v * base) & _M32
    return DomainTable(domains, slots, pool, powers)


Url = Tuple[int, int, int, bool]   # (beg, len, bits, allowed)


def _host_bits(data: bytes, a: int, e: int, domains: Dict[bytes, int]) -> Tuple[int, bool]:
    """Host analysis of the authority data[a:e] → (bits, allowed)."""
    bits = 0
    hb = a
    at = data.rfind(b"@", a, e)
    if at >= 0:
        bits |= USERINFO
        hb = at + 1
    if hb < e and data[hb] == 0x5B:
        return bits | BRACKET, False
    he = data.find(b":", hb, e)
    if he < 0:
        he = e
    while he > hb and data[he - 1] == 0x2E:
        he -= 1
    if he == hb:
        return bits | EMPTY_HOST, False
    host = data[hb:he]
    if all(c in _NUMERIC for c in host):
        bits |= NUMERIC
    if any(c >= 0x80 for c in host):
        bits |= NON_ASCII
    folded = host.translate(_FOLD)
    tags = 0
    for s in range(len(host)):
        if host[s] != 0x2E and (s == 0 or host[s - 1] == 0x2E):
            if folded[s:s + 4] == b"xn--":
                bits |= PUNYCODE
            tags |= domains.get(folded[s:], 0)
    if tags & TAG_ALLOW:
        return bits, True
    if tags & TAG_BLOCK:
        bits |= BLOCKED
    return bits, False


def url_scan_reference(data: bytes, domains: Dict[bytes, int], report_mask: int
                       ) -> Tuple[List[Url], Tuple[int, int, int, int], int, Tuple[int, int], int]:
    """→ (urls, counts, mask, first, flags) over the whole buffer.

    urls: (beg, len, bits, allowed) by begin. The last four are what the
    kernel reports per request: counts = (urls, allowed urls, blocked-domain
    urls, reported urls), where a URL that is not allowed is *reported* when
    bits & report_mask is non-zero; mask is the OR of the bits of every URL
    that is not allowed, whatever report_mask; first = (beg, len) of the
    reported URL with the smallest begin — (-1, 0) if none — and flags has
    bit 0 set when the buffer holds a backslash or a byte >= 0x80."""
    n = len(data)
    urls: List[Url] = []
    p = data.find(b"://")
    while p >= 0:
        length = 0
        while length < SCHEME_MAX and p - 1 - length >= 0 and data[p - 1 - length] in _SCHEME:
            length += 1
        if length:
            beg, a = p - length, p + 3
            scheme = data[beg:p].translate(_FOLD)
            bits = 0 if scheme == b"https" else HTTP if scheme == b"http" else OTHER_SCHEME
            e = a
            while e < n and data[e] not in _TERM:
                e += 1
            if e - a > AUTH_MAX:
                urls.append((beg, a + AUTH_MAX - beg, bits | OVERLONG, False))
            else:
                host_bits, allowed = _host_bits(data, a, e, domains)
                urls.append((beg, e - beg, bits | host_bits, allowed))
        p = data.find(b"://", p + 1)

    mask = n_allowed = n_blocked = n_reported = 0
    first = (-1, 0)
    for beg, length, bits, allowed in urls:
        if allowed:
            n_allowed += 1
            continue
        mask |= bits
        n_blocked += 1 if bits & BLOCKED else 0
        if bits & report_mask:
            n_reported += 1
            if first[0] < 0 or beg < first[0]:
                first = (beg, length)
    flags = 1 if any(b == 0x5C or b >= 0x80 for b in data) else 0
    return urls, (len(urls), n_allowed, n_blocked, n_reported), mask, first, flags


def category_names(bits: int) -> List[str]:
    """The category names of a URL's bits, in bit order."""
    return [name for bit, name in CATEGORY_NAMES.items() if bits & bit]
