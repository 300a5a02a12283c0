"""sql_sanitizer on the GPU: the SQL lexer kernel against its CPU reference, as
exact integers, on the smallest shapes that can break it, and the pipeline's
prefilter against the CPU chain."""

import asyncio
import functools
import json
import random

import numpy as np
import pytest
import torch

from mcp_context_forge_amd.ops import dfa
from mcp_context_forge_amd.ops import sql as S

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no ROCm device")

KW16 = "drop_everything_"
# blocked-word lists: the default one, one 2-byte word, and one with a 16-byte word
KEYWORDS = {"default": S.DEFAULT_BLOCKED, "kw2": ["go"], "kw16": [KW16, "drop"]}
PRE = b" drop ;"   # the bytes before a span: a blocked word and a terminator that belong to no request
DWW, UWW = "delete_without_where", "update_without_where"


# ---------------------------------------------------------------------------
# kernel vs reference
# ---------------------------------------------------------------------------

def _requests():
    """[(name, bytes before the span, span bytes)] — the bytes before a span
    belong to no request; they spell " drop ;" so that a read outside
    [beg, end) would change a result. Chunks of 64 bytes start at the span's
    begin, so an offset in the span is an offset in a chunk."""
    assert len(KW16) == 16
    rng = random.Random(5)
    reqs = []
    for n in (0, 1, 63, 64, 65, 129):                          # span lengths around the 64-byte chunk
        reqs.append((f"len{n}", PRE, (b"delete from t; drop x -- c\n" * 8)[:n]))
    reqs.append(("unaligned_beg", b"ABC" + PRE, b"drop table t where 'drop'"))
    for off in (62, 63, 64):                                   # two-byte tokens on the chunk edge
        reqs.append((f"line_at_{off}", PRE, b" " * off + b"-- drop\ndrop"))
        reqs.append((f"open_at_{off}", PRE, b" " * off + b"/* drop */ drop"))
        reqs.append((f"close_at_{off}", PRE, b"/*" + b" " * (off - 2) + b"*/ drop /"))
        reqs.append((f"open_slash_at_{off}", PRE, b" " * off + b"/*/ drop */ truncate"))     # /*/ does not close
        reqs.append((f"close_star_at_{off}", PRE, b"/*" + b" " * (off - 2) + b"*/* drop */ alter"))   # */* does not reopen
        reqs.append((f"line_then_end_at_{off}", PRE, b"drop" + b" " * (off - 4) + b"--"))       # the token ends the span
        reqs.append((f"dashes_at_{off}", PRE, b" " * off + b"---\ndrop - -drop"))
    for off in (63, 64):
        reqs.append((f"quote_at_{off}", PRE, b" " * off + b"' drop ' drop"))
        reqs.append((f"quotes_at_{off}", PRE, b" " * (off - 1) + b"'' drop 'x'' drop' grant"))   # '' at off - 1, off
        reqs.append((f"dquote_at_{off}", PRE, b" " * off + b'" drop " drop'))
        reqs.append((f"semi_at_{off}", PRE, b"delete from t" + b" " * (off - 13) + b";where x"))
        reqs.append((f"newline_at_{off}", PRE, b"--" + b" " * (off - 2) + b"\ndrop"))
    reqs.append(("dash_at_span_end", PRE, b" " * 63 + b"-"))              # the byte after the span is '-' as well
    reqs.append(("slash_at_span_end", b"- drop ;", b" " * 63 + b"/"))     # and here '*'
    # a keyword straddling the chunk edge at every byte offset, structural and blocked
    for shift in range(1, 8):
        reqs.append((f"kw_edge_truncate_{shift}", b"* drop ;" if shift == 1 else PRE,
                     b" " * (64 - shift) + b"TRUNCATE t"))
    for shift in range(1, 6):
        reqs.append((f"kw_edge_delete_{shift}", PRE, b" " * (64 - shift) + b"delete from t"))
        reqs.append((f"kw_edge_where_{shift}", PRE, b"delete from t" + b" " * (51 - shift) + b"where x"))
    for shift in range(1, 16):
        reqs.append((f"kw_edge_16_{shift}", PRE, b" " * (64 - shift) + KW16.encode() + b";"))
        reqs.append((f"kw_edge_17_{shift}", PRE, b" " * (64 - shift) + KW16.encode() + b"x;"))
    reqs.append(("kw16_and_17", PRE, KW16.encode() + b" x " + KW16.encode() + b"x " + KW16.upper().encode()))
    reqs.append(("kw16_at_span_end", PRE, b" " * 60 + KW16.encode()))
    reqs.append(("kw_at_span_end", PRE, b"x drop"))
    reqs.append(("kw_at_span_end_on_edge", PRE, b" " * 60 + b"drop"))
    reqs.append(("kw_cut_by_span_end", PRE, b"x dr"))                     # the bytes after the span spell "op table"
    reqs.append(("kw_cut_at_edge", b"op table; drop ;", b" " * 62 + b"dr"))
    reqs.append(("word_run_on", b"op drop ;", b"dropdrop drops xdrop _drop drop1 drop_ " + b"drop" * 20 + b" dr"))
    reqs.append(("far_where", b"op drop ;", b"delete from t " + b"x " * 100 + b"where y"))               # three chunks apart
    reqs.append(("far_no_where", PRE, b"delete from t " + b"x " * 100 + b"; where y"))
    reqs.append(("far_update", PRE, b"x update " + b"(a) " * 40 + b"set " + b"b, " * 30))
    reqs.append(("closed_by_span_end", PRE, b"update t set a=1"))
    reqs.append(("semi_in_string_and_comment", PRE, b"delete from t 'a;b' /* ; */ -- ;\n where x"))
    reqs.append(("three_statements", PRE, b"delete from t;update t set a;drop x"))
    reqs.append(("both_rules_one_statement", PRE, b"x delete delete from update set update"))
    reqs.append(("finding_order", PRE, b"delete drop from t"))            # first is the smallest begin
    reqs.append(("select_for_update", PRE, b"select * from t for update"))
    reqs.append(("split_by_comment", PRE, b"DR/**/OP TABLE x"))
    reqs.append(("doubled_quotes", PRE, b"it''s drop 'it''s drop'"))
    reqs.append(("adjacent_a", PRE, b"delete from t --"))                 # no gap to the next two:
    reqs.append(("adjacent_b", b"", b"where x\ndrop 'a"))                 # neither lexer state nor statement
    reqs.append(("adjacent_c", b"", b"drop' drop"))                       # may leak into the next request
    reqs.append(("backslash", PRE, b"select 'a\\'' drop"))
    reqs.append(("non_ascii", PRE, "café drop".encode()))
    reqs.append(("json_span", PRE, b'{"q":"delete from t -- x","r":"where","drop":[1,"it\'s"],"s":"drop"}'))
    reqs.append(("kw2", PRE, b"go; GO go1 ago g o (go)"))
    reqs.append(("many_quotes", PRE, b'","' * 40 + b"drop"))
    reqs.append(("many_terminators", PRE, b"drop;" * 30))
    # a few hundred requests from a fragment generator
    frags = [b"DELETE", b"delete", b"FROM", b"from", b"WHERE", b"UPDATE", b"update", b"SET", b"set", b";", b"'", b"''",
             b"--", b"/*", b"*/", b"-", b"/", b"*", b"drop", b"DROP", b"truncate", b"go", KW16.encode(),
             KW16.encode() + b"x", b"\n", b'"', b"t1", b"_", b"(", b",", b"=", b"\\", "é".encode(), b";", b";", b";", b"FROM", b"set"]
    for i in range(300):
        parts = []
        for _ in range(rng.choice([0, 1, 3, 8, 20, 40, 60])):
            parts.append(rng.choice(frags))
            parts.append(rng.choice([b"", b" ", b" ", b"  "]))
        span = b"".join(parts)
        if rng.random() < 0.3:
            span = b" " * rng.randint(50, 70) + span
        reqs.append((f"rand{i}", b"A" * rng.randint(0, 3) + PRE, span))
    return reqs


@functools.lru_cache(maxsize=None)
def _corpus():
    """→ (names, blob u8, beg i32, end i32); computed once, never modified."""
    names, chunks, beg, end, off = [], [], [], [], 0
    for name, before, span in _requests():
        chunks.append(before + span)
        names.append(name)
        beg.append(off + len(before))
        end.append(off + len(before) + len(span))
        off += len(before) + len(span)
    blob = np.frombuffer(b"".join(chunks) + PRE, dtype=np.uint8)   # read-only view of the bytes
    return tuple(names), blob, np.asarray(beg, dtype=np.int32), np.asarray(end, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _kw(kw_name):
    return S.compile_sql_keywords(KEYWORDS[kw_name])


@functools.lru_cache(maxsize=None)
def _reference(kw_name, boundary):
    _names, blob, beg, end = _corpus()
    tables, kw_len = _kw(kw_name)
    raw = blob.tobytes()
    return tuple(S.sql_scan_reference(raw[b:e], tables, kw_len, boundary) for b, e in zip(beg, end))


def _launch(kw_name, boundary, lo, hi, out=None):
    from mcp_context_forge_amd.ops import hip

    _names, blob, beg, end = _corpus()
    tables, kw_len = _kw(kw_name)
    data_t = torch.from_numpy(blob.copy()).cuda()
    beg_t = torch.from_numpy(beg[lo:hi].copy()).cuda()
    end_t = torch.from_numpy(end[lo:hi].copy()).cuda()
    got = hip.sql_scan(data_t, beg_t, end_t, hip.DeviceScanTables(tables), kw_len, boundary, out=out)
    torch.cuda.synchronize()
    return got


def _check(kw_name, boundary, lo, hi):
    """Kernel vs reference over requests [lo, hi) of the corpus, every output an exact integer."""
    names, _blob, beg, _end = _corpus()
    ref = _reference(kw_name, boundary)
    counts, blocked, first, flags = _launch(kw_name, boundary, lo, hi)
    assert counts.dtype == torch.int32 and counts.shape == (hi - lo, 4) and first.shape == (hi - lo, 2)
    counts, first, flags = (t.cpu().numpy() for t in (counts, first, flags))
    blocked = blocked.cpu().numpy().view(np.uint32)
    for k in range(hi - lo):
        _f, _c, r_counts, r_blocked, r_first, r_flags = ref[lo + k]
        what = (kw_name, boundary, names[lo + k])
        assert tuple(int(c) for c in counts[k]) == r_counts, what
        assert int(blocked[k]) == r_blocked, what
        want = (int(beg[lo + k]) + r_first[0], r_first[1]) if r_first[0] >= 0 else (-1, 0)
        assert (int(first[k, 0]), int(first[k, 1])) == want, what
        assert int(flags[k]) == r_flags, what


def test_corpus_exercises_what_it_names():
    """CPU-side: the named cases are what their names say (checked on the reference)."""
    names, blob, beg, end = _corpus()
    raw = blob.tobytes()
    by = lambda kwn="default", bd=False: dict(zip(names, _reference(kwn, bd)))
    d, db, k2, k16 = by(), by(bd=True), by("kw2"), by("kw16")
    drop = [(0, 4, "blocked:drop")]
    assert len(names) > 400 and beg[names.index("unaligned_beg")] % 4 != 0
    assert [int(e - b) for b, e in zip(beg[:6], end[:6])] == [0, 1, 63, 64, 65, 129]
    # every span but the adjacent ones is preceded by " drop ;", and followed by bytes that are not its own
    assert all(raw[b - 7:b] == PRE for n, b in zip(names, beg) if n not in ("adjacent_b", "adjacent_c"))
    assert end[names.index("adjacent_a")] == beg[names.index("adjacent_b")]
    assert end[names.index("adjacent_b")] == beg[names.index("adjacent_c")]
    for off in (62, 63, 64):
        assert d[f"line_at_{off}"][0] == [(off + 8, 4, "blocked:drop")] and d[f"line_at_{off}"][1] == [(off, 7)]
        assert d[f"open_at_{off}"][0] == [(off + 11, 4, "blocked:drop")] and d[f"open_at_{off}"][1] == [(off, 10)]
        assert d[f"close_at_{off}"][0] == [(off + 3, 4, "blocked:drop")] and d[f"close_at_{off}"][1] == [(0, off + 2)]
        assert d[f"open_slash_at_{off}"][0] == [(off + 12, 8, "blocked:truncate")]
        assert d[f"close_star_at_{off}"][0] == [(off + 4, 4, "blocked:drop"), (off + 12, 5, "blocked:alter")]
        assert d[f"line_then_end_at_{off}"][1] == [(off, 2)] and d[f"line_then_end_at_{off}"][0] == drop
        assert d[f"dashes_at_{off}"][1] == [(off, 3)] and len(d[f"dashes_at_{off}"][0]) == 2
    for off in (63, 64):
        assert d[f"quote_at_{off}"][0] == [(off + 9, 4, "blocked:drop")]
        assert d[f"quotes_at_{off}"][0] == [(off + 2, 4, "blocked:drop"), (off + 18, 5, "blocked:grant")]
        assert d[f"dquote_at_{off}"][0] == [(off + 9, 4, "blocked:drop")] and len(db[f"dquote_at_{off}"][0]) == 2
        assert d[f"semi_at_{off}"][0] == [(0, 6, DWW)] and d[f"semi_at_{off}"][2] == (2, 1, 0, 0)
        assert d[f"newline_at_{off}"][0] == [(off + 1, 4, "blocked:drop")]
    assert d["dash_at_span_end"][2] == (0, 0, 0, 0) and raw[end[names.index("dash_at_span_end")]] == ord("-")
    assert d["slash_at_span_end"][2] == (0, 0, 0, 0) and raw[end[names.index("slash_at_span_end")]] == ord("*")
    assert all(d[f"kw_edge_truncate_{s}"][0] == [(64 - s, 8, "blocked:truncate")] for s in range(1, 8))
    assert all(d[f"kw_edge_delete_{s}"][0] == [(64 - s, 6, DWW)] for s in range(1, 6))
    assert all(d[f"kw_edge_where_{s}"][2] == (1, 0, 0, 0) for s in range(1, 6))
    assert all(k16[f"kw_edge_16_{s}"][3] == 1 and k16[f"kw_edge_17_{s}"][3] == 0 for s in range(1, 16))
    assert [f[0] for f in k16["kw16_and_17"][0]] == [0, 37] and max(_kw("kw16")[1]) == 16
    assert k16["kw16_at_span_end"][0] == [(60, 16, "blocked:" + KW16)]
    assert d["kw_at_span_end"][0] == [(2, 4, "blocked:drop")] and d["kw_at_span_end_on_edge"][4] == (60, 4)
    for name in ("kw_cut_by_span_end", "kw_cut_at_edge"):
        assert d[name][0] == [] and raw[end[names.index(name)]:][:2] == b"op"
    assert d["word_run_on"][0] == [] and raw[end[names.index("word_run_on")]:][:2] == b"op"
    assert d["far_where"][0] == [] and d["far_no_where"][0] == [(0, 6, DWW)] and d["far_update"][0] == [(2, 6, UWW)]
    assert len(raw[beg[names.index("far_where")]:end[names.index("far_where")]]) > 3 * 64
    assert d["closed_by_span_end"][2] == (1, 0, 1, 0) and d["semi_in_string_and_comment"][2] == (1, 0, 0, 2)
    assert d["three_statements"][2] == (3, 1, 1, 0) and d["three_statements"][3] == 1
    assert d["both_rules_one_statement"][2] == (1, 1, 1, 0) and d["finding_order"][4] == (0, 6)
    assert d["select_for_update"][0] == [] and d["split_by_comment"][2] == (0, 0, 0, 1)
    assert d["doubled_quotes"][0] == [(6, 4, "blocked:drop")]
    assert d["adjacent_a"][2] == (1, 1, 0, 1) and d["adjacent_b"][0] == [(8, 4, "blocked:drop")]
    assert d["adjacent_c"][0] == drop and d["backslash"][5] == 1 and d["non_ascii"][5] == 1
    assert db["json_span"][2] == (4, 1, 0, 1) and db["json_span"][3] == 1 and d["json_span"][0] == []
    assert [f[0] for f in k2["kw2"][0]] == [0, 4, 20] and d["kw2"][0] == []
    assert len(d["many_terminators"][0]) == 30 and db["many_quotes"][2] == (1, 0, 0, 0)
    # the generated part has findings of every kind, comments, clean requests, and differs between the modes
    rand = [(v, w) for (n, v), w in zip(d.items(), db.values()) if n.startswith("rand")]
    assert sum(1 for v, _w in rand if v[2][1]) > 10 and sum(1 for v, _w in rand if v[2][2]) > 10
    assert sum(1 for v, _w in rand if v[3]) > 30 and sum(1 for v, _w in rand if v[2][3]) > 30
    assert sum(1 for v, _w in rand if not v[0]) > 30 and sum(1 for v, w in rand if v[2:] != w[2:]) > 30
    assert sum(1 for n, v in k16.items() if n.startswith("rand") and v[3] & 1) > 10


@requires_gpu
@pytest.mark.parametrize("kw_name", ["default", "kw2", "kw16"])
@pytest.mark.parametrize("boundary", [False, True])
def test_sql_scan_matches_reference(kw_name, boundary):
    names, _blob, _beg, _end = _corpus()
    _check(kw_name, boundary, 0, len(names))


@requires_gpu
@pytest.mark.parametrize("batch", [1, 3, 4, 5])
def test_sql_scan_partial_blocks(batch):
    """Four waves per block: batches that leave waves of the last block idle."""
    names, _blob, _beg, _end = _corpus()
    lo = names.index("line_at_62")
    _check("default", False, lo, lo + batch)
    _check("kw16", True, names.index("kw_edge_16_1"), names.index("kw_edge_16_1") + batch)


@requires_gpu
def test_sql_scan_known_values_preallocated_and_empty_batch():
    from mcp_context_forge_amd.ops import hip

    names, blob, beg, _end = _corpus()
    lo = names.index("three_statements")
    counts, blocked, first, flags = _launch("default", False, lo, lo + 2)
    assert counts.cpu().tolist() == [[3, 1, 1, 0], [1, 1, 1, 0]] and blocked.cpu().tolist() == [1, 0]
    assert first.cpu().tolist() == [[int(beg[lo]), 6], [int(beg[lo + 1]) + 2, 6]] and flags.cpu().tolist() == [0, 0]
    # preallocated outputs are written in place
    out = (torch.full((2, 4), 7, dtype=torch.int32, device="cuda"), torch.full((2,), 7, dtype=torch.int32, device="cuda"),
           torch.full((2, 2), 7, dtype=torch.int32, device="cuda"), torch.full((2,), 7, dtype=torch.int32, device="cuda"))
    lo = names.index("backslash")
    got = _launch("default", True, lo, lo + 2, out=out)
    assert all(g is o for g, o in zip(got, out))
    assert out[0].cpu().tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]] and out[1].cpu().tolist() == [0, 1]
    assert out[2].cpu().tolist() == [[-1, 0], [int(beg[lo + 1]) + 6, 4]] and out[3].cpu().tolist() == [1, 1]
    # an empty batch launches nothing
    data_t = torch.from_numpy(blob.copy()).cuda()
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    tables, kw_len = _kw("default")
    res = hip.sql_scan(data_t, empty, empty, hip.DeviceScanTables(tables), kw_len, False)
    assert res[0].shape == (0, 4) and res[1].numel() == 0


@requires_gpu
def test_sql_scan_argument_errors():
    from mcp_context_forge_amd.ops import hip

    data_t = torch.from_numpy(np.frombuffer(b"drop" * 16, dtype=np.uint8).copy()).cuda()
    beg_t = torch.zeros(1, dtype=torch.int32, device="cuda")
    end_t = torch.full((1,), 64, dtype=torch.int32, device="cuda")
    tables, kw_len = _kw("default")
    good = hip.DeviceScanTables(tables)

    def call(dev_tables, lens):
        return hip.sql_scan(data_t, beg_t, end_t, dev_tables, lens, False)

    assert call(good, kw_len)[1].cpu().tolist() == [0]          # "dropdrop…" is one long word
    big = ["%02d" % i + "".join(chr(97 + (i * 7 + j * 3) % 26) for j in range(14)) for i in range(24)]
    big_tables = dfa.compile_literals(S.STRUCTURAL + big, case_insensitive=True)
    assert hip.scan_table_bytes(big_tables.n_states, big_tables.n_classes) > hip.SQL_SCAN_TABLE_LIMIT == 16 * 1024
    for dev_tables, lens in (
            (good, kw_len[:5]), (good, kw_len + [4] * 20),                                          # n_kw 5, 30
            (hip.DeviceScanTables(dfa.compile_literals(S.STRUCTURAL + ["a" * 17])), kw_len[:5] + [17]),    # kw_max_len 17
            (hip.DeviceScanTables(big_tables), [6, 4, 6, 3, 5] + [16] * 24)):
        with pytest.raises(hip.ForgeHipError, match="9006"):
            call(dev_tables, lens)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# pipeline parity
# ---------------------------------------------------------------------------

def _mk_raw(name, args_json, rid):
    return ('{"jsonrpc":"2.0","id":%d,"method":"tools/call","params":{"name":"%s","arguments":%s}}'
            % (rid, name, args_json)).encode()


def _j(obj):
    return json.dumps(obj, separators=(",", ":"))


B64_EXFIL = "cGFzc3dvcmQgcGFzc3dvcmQgcGFzc3dvcmQ="   # password password password: text, and low entropy
AWS_DOC_SECRET = "wJalrXUtnFEMI/K7MDENG/bPxRfiCYEXAMPLEKEY"
TIME_ARGS = {"time": "2026-01-01T10:00:00Z", "source_timezone": "UTC", "target_timezone": "Asia/Tokyo"}


def _traffic():
    """[(tool, arguments JSON)]; the request id is the index."""
    return [
        ("fast-time-echo", _j({"msg": "plain benign payload"})),
        ("fast-time-convert_time", _j(TIME_ARGS)),
        ("native-time-convert_time", _j({**TIME_ARGS, "target_timezone": "UTC"})),
        ("fast-time-echo", _j({"q": "select * from t where id = 1"})),
        ("fast-time-echo", _j({"q": "DROP TABLE users"})),                                  # 4: blocked word
        ("fast-time-echo", _j({"q": "delete from t", "n": 1})),                             # 5: delete without where
        ("fast-time-echo", _j({"a": {"b": ["x", "update t set a = 1; select 1"]}})),        # 6: nested, update
        ("fast-time-echo", _j({"q": "INSERT INTO notes VALUES ('please drop by')"})),       # 7: in a string: clean
        ("fast-time-echo", _j({"q": "select 1 /* drop */ from t -- truncate"})),            # 8: in comments: clean
        ("fast-time-echo", _j({"q": "DR/**/OP TABLE x"})),                                  # 9: two words: clean
        ("fast-time-echo", '{"q":"select 1 from a\\/b"}'),                                  # 10: a backslash routes
        ("fast-time-echo", _j({"q": "delete from t", "r": "where x"})),                     # 11: where in another value
        ("native-time-echo", _j({"q": "DROP TABLE users", "why": "plugin bound disabled here"})),   # 12
        ("fast-time-echo", _j({"drop": "a key is not scanned"})),                           # 13: over-flagged, answered
        ("fast-time-echo", _j({"q": "delete from t where id = 1"})),                        # 14
        ("fast-time-echo", _j({"k": B64_EXFIL})),                                           # 15: exfil's row
        ("fast-time-echo", _j({"k": AWS_DOC_SECRET})),                                      # 16: secrets' row
    ]


def _raws(traffic):
    return [_mk_raw(name, args, rid) for rid, (name, args) in enumerate(traffic)]


def _sql_prefilter(plugin, raw: bytes) -> bool:
    """The argument prefilter, from the reference, over one raw span."""
    _f, _c, counts, mask, _first, flags = S.sql_scan_reference(raw, plugin.keyword_tables(),
                                                               plugin.keyword_lengths(), True)
    return bool(flags & 1 or mask or (counts[1] and plugin.block_delete_without_where)
                or (counts[2] and plugin.block_update_without_where) or (counts[3] and plugin.strip_comments))


def _flagged(plugin, traffic):
    return [name != "native-time-echo" and _sql_prefilter(plugin, args.encode()) for name, args in traffic]


async def _build(gpu: bool, sql_config=None, with_others=False, bind_off=True):
    from mcp_context_forge_amd.config import Settings
    from mcp_context_forge_amd.engine import GatewayEngine
    from mcp_context_forge_amd.plugins.loader import default_chain_specs, load_plugin_manager
    from mcp_context_forge_amd.services.upstream import NativeInProcUpstream, make_fake_time_upstream

    settings = Settings(database_url="sqlite://", federation_enabled=False, auth_required=False,
                        gpu_enabled=gpu, gpu_semcache_capacity=1024)
    specs = default_chain_specs()
    if with_others:
        specs.append({"name": "secrets_detection", "config": {"alphabets": ["base64", "hex"]}})
        specs.append({"name": "encoded_exfil_detection"})
    specs.append({"name": "sql_sanitizer", "config": dict(sql_config or {})})
    e = GatewayEngine(settings, plugin_manager=load_plugin_manager(specs=specs))
    await e.gateway_service.register_gateway(name="fast-time", url="inproc://t", client=make_fake_time_upstream())
    await e.gateway_service.register_gateway(name="native-time", url="inproc://n", client=NativeInProcUpstream())
    if bind_off:
        for plugin in ["sql_sanitizer"] + (["secrets_detection", "encoded_exfil_detection"] if with_others else []):
            e.set_plugin_binding("native-time-echo", plugin, mode="disabled")
    if gpu:
        assert e.enable_gpu()
    return e


def _same_outcomes(cpu_out, gpu_out):
    assert len(cpu_out) == len(gpu_out)
    for i, (c, g) in enumerate(zip(cpu_out, gpu_out)):
        co = json.loads(c) if c else None
        go = json.loads(g) if g else None
        if co is None or go is None:
            assert co == go, (i, co, go)
        elif "error" in co or "error" in go:
            assert co.get("error", {}).get("code") == go.get("error", {}).get("code"), (i, co, go)
            assert co["error"]["message"] == go["error"]["message"], (i, co, go)
        else:
            assert co["result"] == go["result"], (i, co, go)


async def _both(sql_config=None, with_others=False):
    cpu = await _build(gpu=False, sql_config=sql_config, with_others=with_others)
    gpu = await _build(gpu=True, sql_config=sql_config, with_others=with_others)
    traffic = _traffic()
    raws = _raws(traffic)
    cpu_out = await cpu.process_rpc_batch(list(raws))
    gpu_out = await gpu.process_rpc_batch(list(raws))
    _same_outcomes(cpu_out, gpu_out)
    flagged = _flagged(cpu.plugins.get("sql_sanitizer"), traffic)
    stats = gpu.gpu_pipeline.stats()
    await cpu.shutdown()
    await gpu.shutdown()
    return traffic, [json.loads(g) for g in gpu_out], flagged, stats


@requires_gpu
def test_pipeline_sql_parity_block(monkeypatch):
    monkeypatch.setenv("FORGE_PIPELINE_TIMING", "1")

    async def run():
        from mcp_context_forge_amd.protocol import jsonrpc

        traffic, outs, flagged, st = await _both()
        assert [i for i, f in enumerate(flagged) if f] == [4, 5, 6, 10, 11, 13]
        blocked = {o["id"] for o in outs if o.get("error", {}).get("code") == jsonrpc.POLICY_DENIED}
        assert blocked == {4, 5, 6, 11}
        assert all("sql_sanitizer: dangerous sql detected" in o["error"]["message"] for o in outs if o["id"] in blocked)
        assert "blocked:drop" in outs[4]["error"]["message"] and DWW in outs[5]["error"]["message"]
        assert UWW in outs[6]["error"]["message"]
        assert all("result" in outs[i] for i in (7, 8, 9, 10, 13, 14))
        assert "DROP TABLE users" in json.dumps(outs[12]["result"])       # plugin disabled for this tool
        assert st["sql_routed"] == sum(flagged) == 6 and st["secrets_routed"] == 0 and st["exfil_routed"] == 0
        assert st["host_bound"] == 0
        # every unflagged row stayed on the fast path; an unmodelled plugin would have made every tool host-bound
        assert st["fast_path"] == len(traffic) - sum(flagged)
        assert st["timing_s"]["gp0_sql"] > 0.0
        assert "gp0_secrets" not in st["timing_s"] and "gp0_exfil" not in st["timing_s"]

    asyncio.run(run())


@requires_gpu
def test_pipeline_sql_parity_audit():
    async def run():
        traffic, outs, flagged, st = await _both({"action": "audit"})
        assert all("result" in o for o in outs)
        assert "DROP TABLE users" in json.dumps(outs[4]["result"])
        assert st["sql_routed"] == sum(flagged) == 6 and st["fast_path"] == len(traffic) - 6

    asyncio.run(run())


@requires_gpu
def test_pipeline_sql_parity_strip_comments():
    async def run():
        cfg = {"strip_comments": True, "block_delete_without_where": False}
        traffic, outs, flagged, st = await _both(cfg)
        # comments route now, a delete without where no longer does
        assert [i for i, f in enumerate(flagged) if f] == [4, 6, 8, 9, 10, 13]
        assert "error" in outs[4] and "error" in outs[6] and "result" in outs[5] and "result" in outs[11]
        text8 = json.dumps(outs[8]["result"])
        assert "select 1" in text8 and "drop" not in text8 and "truncate" not in text8 and "/*" not in text8
        assert "DR OP TABLE x" in json.dumps(outs[9]["result"])
        assert st["sql_routed"] == sum(flagged) == 6 and st["fast_path"] == len(traffic) - 6

    asyncio.run(run())


@requires_gpu
def test_pipeline_parity_with_secrets_exfil_and_sql(monkeypatch):
    monkeypatch.setenv("FORGE_PIPELINE_TIMING", "1")

    async def run():
        traffic, outs, flagged, st = await _both(with_others=True)
        assert "error" in outs[15] and "encoded_exfil_detection" in outs[15]["error"]["message"]
        assert "error" in outs[16] and "secrets_detection" in outs[16]["error"]["message"]
        assert "sql_sanitizer" in outs[4]["error"]["message"]
        assert "DROP TABLE users" in json.dumps(outs[12]["result"])
        # each prefilter has rows of its own; the backslash row (10) is flagged by all three
        assert st["sql_routed"] == sum(flagged) == 6 and st["exfil_routed"] == 2 and st["secrets_routed"] == 2
        assert not flagged[15] and not flagged[16] and st["host_bound"] == 0
        # the benign rows (0, 1, 2, 3, 7, 8, 9, 12, 14) stayed on the fast path
        assert st["fast_path"] == len(traffic) - 8 == 9
        assert st["timing_s"]["gp0_secrets"] > 0.0 and "gp0_sql" not in st["timing_s"]

    asyncio.run(run())


@requires_gpu
def test_pipeline_sql_off_launches_nothing():
    """Without the plugin the pre-pass does not run and the counter stays 0."""
    async def run():
        from mcp_context_forge_amd.config import Settings
        from mcp_context_forge_amd.engine import GatewayEngine
        from mcp_context_forge_amd.services.upstream import make_fake_time_upstream

        e = GatewayEngine(Settings(database_url="sqlite://", federation_enabled=False, auth_required=False,
                                   gpu_enabled=True, gpu_semcache_capacity=1024))
        await e.gateway_service.register_gateway(name="fast-time", url="inproc://t", client=make_fake_time_upstream())
        assert e.enable_gpu()
        out = await e.process_rpc_batch([_mk_raw("fast-time-echo", _j({"q": "DROP TABLE users"}), 1)])
        assert "result" in json.loads(out[0])
        st = e.gpu_pipeline.stats()
        assert st["sql_routed"] == 0 and st["fast_path"] == 1 and e.gpu_pipeline._tools.sql is None
        await e.shutdown()

    asyncio.run(run())
