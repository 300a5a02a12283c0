"""gpu/rowset.py and gpu/tooltable.py without a device: RowSet.keep() narrows
every per-row field, and the per-tool flag / post-lane rules of tool_flags."""

import asyncio
from types import SimpleNamespace

import numpy as np

from mcp_context_forge_amd.gpu.rowset import BAD_ARGS, RowSet
from mcp_context_forge_amd.protocol import jsonrpc

# batch constants: shared by every stage, never narrowed
_CONSTANTS = {"blob", "env", "responses", "tools", "counters"}


def _row_set(m=7):
    """Distinct values per field (field k holds 100*k + row) and a mix of dtypes."""
    dtypes = {"rows": np.int64, "uh": np.int64, "tool_idx": np.int32, "id_b": np.int64, "id_e": np.int64}
    fields = {}
    for k, name in enumerate(s for s in RowSet.__slots__ if s not in _CONSTANTS):
        fields[name] = (np.arange(m) + 100 * (k + 1)).astype(dtypes.get(name, np.int32))
    consts = dict(blob=np.zeros(3, dtype=np.uint8), env={"kind": None}, responses=[None] * 400,
                  tools=object(), counters=SimpleNamespace(blocked=0, cache_hits=0))
    return RowSet(**fields, **consts), fields, consts


def test_rowset_keep_narrows_every_per_row_field():
    rs, fields, consts = _row_set()
    assert set(fields) == set(RowSet.PER_ROW) and len(fields) == 9
    mask = np.array([True, False, True, True, False, False, True])
    rs.keep(mask)
    assert len(rs) == 4
    # by __slots__: a field added later and left out of keep() fails here
    for name in RowSet.__slots__:
        got = getattr(rs, name)
        if name in _CONSTANTS:
            assert got is consts[name], name
            continue
        assert isinstance(got, np.ndarray), name
        assert got.tolist() == fields[name][[0, 2, 3, 6]].tolist(), name
        assert got.flags["C_CONTIGUOUS"], name
        assert got.dtype == fields[name].dtype, name
    rs.keep(np.zeros(4, dtype=bool))
    assert len(rs) == 0
    for name in RowSet.__slots__:
        if name not in _CONSTANTS:
            got = getattr(rs, name)
            assert got.shape == (0,) and got.dtype == fields[name].dtype and got.flags["C_CONTIGUOUS"], name


def test_rowset_row_answers():
    rs, _fields, consts = _row_set()
    rs.blob = np.frombuffer(b'7"a"{"k":1}{bad', dtype=np.uint8)
    rs.id_b[:3], rs.id_e[:3] = [0, 1, -1], [1, 4, -1]
    rs.args_b[:2], rs.args_e[:2] = [4, 11], [11, 15]
    rs.block(0, "deny_filter: x")
    assert rs.responses[int(rs.rows[0])] == \
        b'{"jsonrpc":"2.0","id":7,"error":{"code":%d,"message":"deny_filter: x"}}' % jsonrpc.POLICY_DENIED
    assert consts["counters"].blocked == 1
    rs.answer_cached(1, b'{"ok":true}')
    assert rs.responses[int(rs.rows[1])] == b'{"jsonrpc":"2.0","id":"a","result":{"ok":true}}'
    rs.answer_cached(2, b"{}")          # a notification is never answered, still a hit
    assert rs.responses[int(rs.rows[2])] is None and consts["counters"].cache_hits == 2
    assert rs.decode_args(0) == {"k": 1}
    assert rs.decode_args(1) is BAD_ARGS and b"invalid arguments" in rs.responses[int(rs.rows[1])]


def test_tool_flags_and_post_lane_rules():
    from mcp_context_forge_amd.config import Settings
    from mcp_context_forge_amd.engine import GatewayEngine
    from mcp_context_forge_amd.gpu import tooltable as T
    from mcp_context_forge_amd.ops import hip
    from mcp_context_forge_amd.plugins.loader import default_chain_specs, load_plugin_manager

    specs = default_chain_specs() + [{"name": "secrets_detection", "config": {"alphabets": ["base64"]}}]
    e = GatewayEngine(Settings(database_url="sqlite://", federation_enabled=False, auth_required=False,
                               gpu_enabled=False), plugin_manager=load_plugin_manager(specs=specs))

    async def handler(args):
        return "ok"

    for name, out_schema in (("plain", None), ("bound", None), ("quiet", None),
                             ("shaped", {"type": "object", "properties": {"v": {"type": "string"}}})):
        e.tool_service.register_local_tool(name, handler, output_schema=out_schema)
    content = ("deny_filter", "harmful_content_detector", "pii_filter", "content_moderation",
               "argument_normalizer")
    e.set_plugin_binding("bound", "header_injector", mode="enforce")      # a plugin the fast path does not model
    for p in content + ("secrets_detection",):                            # nothing left that reads raw bytes
        e.set_plugin_binding("quiet", p, mode="disabled")
    for p in ("secrets_detection",) + tuple(c for c in content if c != "pii_filter"):
        e.set_plugin_binding("shaped", p, mode="disabled")                # pii is the only content bank left

    h = T.PluginHandles(e.plugins)
    assert h.secrets is not None and h.pii is not None
    metas, _pat_ids = T.per_tool_meta(e, h)
    assert [m.name for m in metas] == ["plain", "bound", "quiet", "shaped"]
    t = T.ToolTable()
    T.tool_flags(t, metas, e.plugins, h, {"deny", "harm", "pii", "regex", "normalize"},
                 semcache_on=False, harm_lane_ok=True)
    plain, bound, quiet, shaped = range(4)

    # a tool bound to an unmodeled plugin is host-bound and has post lane -1
    assert t.hostbound.tolist() == [False, True, False, False]
    assert metas[bound].host_chain and t.postlane[bound] == -1
    # a tool with an output schema has post lane -1, without being host-bound or secrets-active
    assert not t.secrets[shaped] and t.postlane[shaped] == -1
    # a secrets-active tool has post lane -1
    assert t.secrets.tolist() == [True, True, False, False]
    assert t.postlane[plain] == -1
    # none of the three: the native post lane is open (bit 3: regex rows punt on a bank hit)
    assert t.postlane[quiet] >= 0
    # TF_NORM whenever a raw-byte content bank is active for the tool
    norm = [(int(f) & hip.TF_NORM) != 0 for f in t.flags]
    assert norm == [True, True, False, True]
    assert int(t.flags[shaped]) & hip.TF_PII and not int(t.flags[shaped]) & hip.TF_DENY
    assert not int(t.flags[quiet]) & (hip.TF_DENY | hip.TF_PII | hip.TF_HARM | hip.TF_MOD)
    assert t.rw_pii.tolist() == [True, True, False, True] and t.rw_deny.tolist() == [True, True, False, False]
    asyncio.run(e.shutdown())


def test_pack_strtable():
    from mcp_context_forge_amd.gpu.tooltable import pack_strtable

    blob, off = pack_strtable(["ab", "", "çd", b"xyz"])
    assert blob.tobytes() == "abçdxyz".encode() and off.tolist() == [0, 2, 2, 5, 8]
    assert blob.dtype == np.uint8 and off.dtype == np.int32
    blob, off = pack_strtable([])
    assert blob.tolist() == [0] and off.tolist() == [0]
