"""Account-number scan: payment cards by Luhn, IBANs by country length and mod 97.

CPU reference of `ops/csrc/account.hip`, plain Python and integer-exact, like
`ops/url.py`: the oracle for the HIP kernel in tests AND the code the
account_number_detection plugin runs per string, so the CPU chain and the
oracle are one code path.

*Cards.* A byte is a *card byte* when it is [0-9], or a space or `-` whose two
neighbours are both digits inside the buffer. A *card run* is a maximal
stretch of card bytes: it begins and ends on a digit, and two separators in a
row split it. With d its digit count the run is a *card candidate* when
13 <= d <= 19, its first digit is not `0`, the byte before it (if any) is none
of [A-Za-z_.] and the byte after it (if any) none of [A-Za-z_]. The `.` keeps
the mantissa of a JSON float out, the letters keep the digits that follow an
IBAN's country code out. A candidate is *valid* when its Luhn sum is a
multiple of 10: from the rightmost digit every second digit is doubled, and 9
is subtracted from a doubled value over 9. Longer runs are not searched for
windows. A card spans first digit to last digit.

*IBANs.* `iban_len` is a 676-byte table indexed by 26 * (c0 - 'A') + (c1 - 'A'):
0 for an unknown country, else the IBAN's length, 15..34
(`compile_iban_lengths`). Every offset p is a candidate start when bytes p,
p + 1 are [A-Z], p + 2, p + 3 are [0-9], the byte before p (if any) is not
[A-Za-z0-9] and the country's entry L is non-zero. From p, bytes are taken
while they are [A-Z0-9], or a single space whose next byte is [A-Z0-9]. It is
an *IBAN candidate* when L alphanumerics are collected before anything else
stops the walk and the byte after the L-th (if any) is not [A-Za-z0-9]. It is
*valid* when, with the first four symbols moved to the end and every letter
read as 10..35 (two decimal digits), the number is 1 mod 97. An IBAN spans
first letter to last alphanumeric. Only upper case counts.

Findings do not consume one another (the digit groups at the tail of a GB
IBAN may count as a card run too): every output is a sum, an OR or a minimum.
"""

from __future__ import annotations

from typing import Dict, List, Mapping, Optional, Tuple

CARD, IBAN = 1, 2
ALL_KINDS = CARD | IBAN
KIND_NAMES = {CARD: "card", IBAN: "iban"}

CARD_MIN_DIGITS, CARD_MAX_DIGITS = 13, 19
IBAN_MIN_LEN, IBAN_MAX_LEN = 15, 34
IBAN_TABLE_BYTES = 26 * 26
# The first four symbols stand together and no two spaces follow one another,
# so the 34th symbol stands at offset 63 at the latest: with the byte after it,
# 65 bytes decide an IBAN.
IBAN_READ_MAX = 4 + 2 * (IBAN_MAX_LEN - 4) + 1
# decimal digits to the right of a symbol after the rotation: at most 6 + 2 * 29
N_POW97 = 69

# A country is listed only with an example that passes mod 97 at that length
# (tests/test_account_plugin.py holds one per entry); config extends the list.
DEFAULT_IBAN_LENGTHS: Dict[str, int] = {
    "DE": 22, "GB": 22, "FR": 27, "ES": 24, "IT": 27, "BE": 16, "CH": 21, "AT": 20, "NO": 15, "MT": 31,
    "SE": 24, "PL": 28, "PT": 25, "IE": 22, "DK": 18, "FI": 18, "LU": 20,
}

_DIGIT = frozenset(b"0123456789")
_UPPER = frozenset(range(65, 91))
_UPNUM = _UPPER | _DIGIT
_ALNUM = _UPNUM | frozenset(range(97, 123))
_WORD = _UPPER | frozenset(range(97, 123)) | {0x5F}
_SEP = frozenset(b" -")


def compile_iban_lengths(extra: Optional[Mapping[str, int]] = None) -> bytes:
    """DEFAULT_IBAN_LENGTHS with `extra` merged over it → the 676-byte table.
    A code is two letters A-Z; a length is 15..34, or 0 to drop a country."""
    merged: Dict[str, int] = dict(DEFAULT_IBAN_LENGTHS)
    for code, length in dict(extra or {}).items():
        if not (isinstance(code, str) and len(code) == 2 and all("A" <= c <= "Z" for c in code)):
            raise ValueError(f"IBAN country code {code!r} must be two letters A-Z")
        if isinstance(length, bool) or not isinstance(length, int) or not (
                length == 0 or IBAN_MIN_LEN <= length <= IBAN_MAX_LEN):
            raise ValueError(f"IBAN length {length!r} of {code} must be 0 or {IBAN_MIN_LEN}..{IBAN_MAX_LEN}")
        merged[code] = length
    table = bytearray(IBAN_TABLE_BYTES)
    for code, length in merged.items():
        table[26 * (ord(code[0]) - 65) + ord(code[1]) - 65] = length
    return bytes(table)


def luhn_valid(digits: bytes) -> bool:
    total = 0
    for k, c in enumerate(reversed(digits)):
        v = c - 48
        if k & 1:
            v = 2 * v - 9 if v > 4 else 2 * v
        total += v
    return total % 10 == 0


def iban_valid(symbols: bytes) -> bool:
    """mod 97 of the rotated symbols [A-Z0-9], letters as 10..35."""
    rem = 0
    for c in symbols[4:] + symbols[:4]:
        rem = (rem * 10 + c - 48) % 97 if c in _DIGIT else (rem * 100 + c - 55) % 97
    return rem == 1


Finding = Tuple[int, int, int]   # (beg, len, kind), valid findings only


def _cards(data: bytes, n: int) -> Tuple[int, List[Finding]]:
    def card_byte(i: int) -> bool:
        c = data[i]
        return c in _DIGIT or (c in _SEP and 0 < i < n - 1 and data[i - 1] in _DIGIT and data[i + 1] in _DIGIT)

    candidates, found, i = 0, [], 0
    while i < n:
        if not card_byte(i):
            i += 1
            continue
        e = i
        while e < n and card_byte(e):
            e += 1
        digits = bytes(c for c in data[i:e] if c in _DIGIT)
        if (CARD_MIN_DIGITS <= len(digits) <= CARD_MAX_DIGITS and digits[0] != 0x30
                and not (i > 0 and (data[i - 1] in _WORD or data[i - 1] == 0x2E))
                and not (e < n and data[e] in _WORD)):
            candidates += 1
            if luhn_valid(digits):
                found.append((i, e - i, CARD))
        i = e
    return candidates, found


def _ibans(data: bytes, n: int, iban_len: bytes) -> Tuple[int, List[Finding]]:
    candidates, found = 0, []
    for p in range(n - 3):
        if not (data[p] in _UPPER and data[p + 1] in _UPPER and data[p + 2] in _DIGIT and data[p + 3] in _DIGIT):
            continue
        if p > 0 and data[p - 1] in _ALNUM:
            continue
        want = iban_len[26 * (data[p] - 65) + data[p + 1] - 65]
        if not want:
            continue
        symbols, i = bytearray(), p
        while len(symbols) < want and i < n:
            c = data[i]
            if c in _UPNUM:
                symbols.append(c)
            elif not (c == 0x20 and i + 1 < n and data[i + 1] in _UPNUM):
                break
            i += 1
        if len(symbols) == want and not (i < n and data[i] in _ALNUM):
            candidates += 1
            if iban_valid(bytes(symbols)):
                found.append((p, i - p, IBAN))
    return candidates, found


def account_scan_reference(data: bytes, iban_len: bytes, report_mask: int
                           ) -> Tuple[List[Finding], Tuple[int, int, int, int], int, Tuple[int, int], int]:
    """→ (findings, counts, kinds, first, flags) over the whole buffer.

    findings: every valid card and IBAN as (beg, len, kind), by begin, whatever
    report_mask. The last four are what the kernel reports per request: counts
    = (card candidates, valid cards, IBAN candidates, valid IBANs); kinds has
    CARD set with a valid card and IBAN with a valid IBAN; first = (beg, len)
    of the valid finding with the smallest begin among the kinds of
    report_mask — (-1, 0) if none — and flags has bit 0 set when the buffer
    holds a backslash or a byte >= 0x80."""
    if len(iban_len) != IBAN_TABLE_BYTES:
        raise ValueError(f"iban_len must hold {IBAN_TABLE_BYTES} bytes")
    if report_mask & ~ALL_KINDS:
        raise ValueError("report_mask has bits outside CARD | IBAN")
    n = len(data)
    card_candidates, cards = _cards(data, n)
    iban_candidates, ibans = _ibans(data, n, iban_len)
    findings = sorted(cards + ibans)
    kinds = (CARD if cards else 0) | (IBAN if ibans else 0)
    first = next(((b, length) for b, length, kind in findings if kind & report_mask), (-1, 0))
    flags = 1 if any(b == 0x5C or b >= 0x80 for b in data) else 0
    return findings, (card_candidates, len(cards), iban_candidates, len(ibans)), kinds, first, flags
