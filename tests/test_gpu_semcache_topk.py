"""hip.sketch_topk / hip.verify_topk (semcache.hip) against ops/semcache.py, and the identity-aware lookup
through GpuSemanticCache and the pipeline. Integer cases have no tolerance (inputs in -4..4, every partial sum
below 2^24); random cases assert the bounds of tests/kernel_oracles.py."""

import asyncio
import json
import time

import numpy as np
import pytest
import torch

import kernel_oracles as ko
from mcp_context_forge_amd.ops import semcache as ref
from test_gpu_parity import _mk

pytestmark = pytest.mark.gpu

A, B, NOBODY = 0x1234567811, -77, 5   # identities: many slots, four slots (three eligible), none
MIN_STAMP = 100


@pytest.fixture(scope="module")
def hip():
    from mcp_context_forge_amd.ops import hip as _hip

    if not _hip.available():
        pytest.fail("libforge_hip must load on a GPU box (no silent fallback)")
    return _hip


def _int_case(b, s, cap=256):
    """Rows 0..4 of q against 64 integer key rows repeated over the slots (slot c ties with c + 64); every
    seventh slot invalid and holding the greatest score of any row; stamps 98..102 around MIN_STAMP."""
    q = ko.int_operand(b, s, 1).abs()
    keys = ko.int_operand(64, s, 2).repeat(cap // 64, 1)
    c = np.arange(cap)
    valid = (c % 7 != 3).astype(np.uint8)
    keys[torch.from_numpy(valid == 0)] = 4.0
    ident = np.where(np.isin(c, (5, 7, 72, 144)), B, A).astype(np.int64)   # slot 5 too old, 7 and 72 on MIN_STAMP
    stamp = (98 + c % 5).astype(np.int32)
    q_ident = np.array([A, B, NOBODY], dtype=np.int64)[np.arange(b) % 3]
    return q, keys, ident, stamp, valid, q_ident


def _topk(hip, case, active, k, splits, min_stamp=MIN_STAMP):
    q, keys, ident, stamp, valid, q_ident = case
    dev = [torch.as_tensor(x).cuda() for x in (q, keys, ident, stamp, valid, q_ident)]
    val, idx = hip.sketch_topk(*dev, min_stamp, active, k, splits=splits)
    return val.cpu(), idx.cpu()


@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("s", [64, 256])
@pytest.mark.parametrize("active", [64, 130, 192])
@pytest.mark.parametrize("b", [64, 128])
def test_sketch_topk_integer_exact(hip, b, active, s, k):
    case = _int_case(b, s)
    want_val, want_idx = ref.sketch_topk_reference(*case, MIN_STAMP, active, k)
    assert (want_idx[1] >= 0).sum() < max(k, 2) and (want_idx[2] == -1).all() and (want_idx[0] >= 0).all()
    for splits in (1, 3, 0):
        val, idx = _topk(hip, case, active, k, splits)
        assert torch.equal(idx, torch.from_numpy(want_idx)), (splits, idx[:3], want_idx[:3])
        assert torch.equal(val, torch.from_numpy(want_val)), splits


def test_sketch_topk_random_within_bound(hip):
    b, cap, s, k = 64, 256, 256, 4
    q, keys = ko.random_operands(b, cap, s, seed=91)
    case = (q, keys, np.full(cap, A), np.zeros(cap, np.int32), np.ones(cap, np.uint8), np.full(b, A))
    val, idx = _topk(hip, case, cap, k, 0, min_stamp=0)
    exact, bound = ko.gemm_ref(q, keys), s * ko.GEMM_HARD_EPS * ko.abs_dot(q, keys)
    rows = torch.arange(b)[:, None]
    assert (idx >= 0).all() and all(len(set(r)) == k for r in idx.tolist())
    err = (val.double() - exact[rows, idx.long()]).abs()
    print("max err / bound:", (err / bound[rows, idx.long()]).max().item())
    assert (err <= bound[rows, idx.long()]).all()
    left_out = exact.clone()
    left_out[rows, idx.long()] = -np.inf
    assert (left_out.max(dim=1).values <= val[:, k - 1].double() + 2 * bound.max(dim=1).values).all()


@pytest.mark.parametrize("d", [8, 512, 4096])
def test_verify_topk_integer_exact(hip, d):
    feats, keys = ko.int_operand(5, d, 3), ko.int_operand(7, d, 4)
    keys[6] = keys[2]                                   # slots 2 and 6 tie for every row
    cand = torch.tensor([[2, 6, -1, 3], [6, 2, 0, 1], [-1, 4, -1, 1], [-1, -1, -1, -1], [0, 1, 2, 3]], dtype=torch.int32)
    want_val, want_idx = ref.verify_topk_reference(feats, keys, cand)
    val, idx = hip.verify_topk(feats.cuda(), keys.cuda(), cand.cuda())
    assert torch.equal(idx.cpu(), torch.from_numpy(want_idx)) and torch.equal(val.cpu(), torch.from_numpy(want_val))


def test_verify_topk_random_within_bound_and_verify_dot_bits(hip):
    m, cap, d = 6, 9, 4096
    feats, keys = ko.random_operands(m, cap, d, seed=57)
    cand = torch.tensor([[(3 * r + j) % cap for j in range(4)] for r in range(m)], dtype=torch.int32)
    val, idx = hip.verify_topk(feats.cuda(), keys.cuda(), cand.cuda())
    want_val, want_idx = ref.verify_topk_reference(feats, keys, cand)
    assert torch.equal(idx.cpu(), torch.from_numpy(want_idx))
    bound = d * ko.DOT_EPS * ko.abs_dot(feats, keys)[torch.arange(m), idx.cpu().long()]
    assert ((val.cpu().double() - ko.gemm_ref(feats, keys)[torch.arange(m), idx.cpu().long()]).abs() <= bound).all()
    assert torch.equal(val, hip.verify_dot(feats.cuda(), keys.cuda(), idx))      # the same bits for the same pair
    with pytest.raises(hip.ForgeHipError, match="9004"):
        hip.verify_topk(feats[:, :12].contiguous().cuda(), keys[:, :12].contiguous().cuda(), cand.cuda())


@pytest.mark.parametrize("bad", [dict(k=0), dict(k=9), dict(s=96), dict(s=576), dict(b=32), dict(splits=65),
                                 dict(splits=-1), dict(null_out=True)])
def test_sketch_topk_argument_errors(hip, bad):
    b, s, k = bad.get("b", 64), bad.get("s", 64), bad.get("k", 4)
    q, keys, ident, stamp, valid, q_ident = (torch.as_tensor(x).cuda() for x in _int_case(64, 64))
    q, keys = torch.zeros((b, s), dtype=torch.bfloat16).cuda(), torch.zeros((256, s), dtype=torch.bfloat16).cuda()
    out = (torch.full((64, 8), 7.0).cuda(), torch.full((64, 8), 7, dtype=torch.int32).cuda())
    if bad.get("null_out"):
        part = torch.empty(64 * 64 * 8, dtype=torch.float32).cuda()
        rc = hip._load().forge_sketch_topk(*(t.data_ptr() for t in (q, keys, ident, stamp, valid, q_ident)), 0, 64,
                                           b, s, k, 0, part.data_ptr(), part.data_ptr(), out[0].data_ptr(), None, None)
        assert rc == hip.ERR_SEMCACHE_TOPK
    else:
        with pytest.raises(hip.ForgeHipError, match="9013"):
            hip.sketch_topk(q, keys, ident, stamp, valid, q_ident[:b], 0, 64, k, splits=bad.get("splits", 0), out=out)
    torch.cuda.synchronize()
    assert (out[0] == 7.0).all() and (out[1] == 7).all()


def test_sketch_topk_empty_inputs(hip):
    case = _int_case(64, 64)
    val, idx = _topk(hip, case, 0, 4, 0)                # active == 0: padding everywhere
    assert (val == ref.NONE_VAL).all() and (idx == -1).all()
    q, keys, ident, stamp, valid, q_ident = (torch.as_tensor(x).cuda() for x in case)
    val, idx = hip.sketch_topk(q[:0], keys, ident, stamp, valid, q_ident[:0], 0, 64, 4)
    assert val.shape == (0, 4) and idx.shape == (0, 4)


def test_cache_lookup_is_identity_and_age_aware():
    from mcp_context_forge_amd.gpu.semcache import GpuSemanticCache

    cache = GpuSemanticCache(capacity=256, dim=512, sketch_dim=128, topk=4, threshold=0.9, ttl_s=60.0)
    feats = torch.zeros((128, 512), dtype=torch.bfloat16)
    feats[0] = torch.nn.functional.normalize(ko.random_operands(1, 1, 512, seed=3)[0].float(), dim=1).bfloat16()
    feats = feats.cuda()
    for ident in (A, A, B):                             # slots 0, 1, 2: A old, A fresh, B
        cache.insert_batch(feats, [0], [ident], ["r"])
    cache.t0 -= 120.0                                   # the cache is two TTLs old and slot 0 keeps its stamp ...
    cache.stamp[1:3] = ref.stamp_of(time.monotonic(), cache.t0)   # ... while slots 1 and 2 were inserted just now
    cache.timestamps[0] -= 120.0                        # the host's exact copy of slot 0's age
    for ident, slot in ((B, 2), (A, 1)):
        val, idx, _ = cache.lookup(feats, idents=np.array([ident], dtype=np.int64))
        val, idx = val[:1].cpu().numpy(), idx[:1].cpu().numpy()
        assert idx[0] == slot and cache.resolve_hits_np(val, idx, np.array([ident]))[0]
    assert cache.stats()["topk"] == 4


async def _engine(gpu, topk=0):
    from mcp_context_forge_amd.config import Settings
    from mcp_context_forge_amd.engine import GatewayEngine
    from mcp_context_forge_amd.plugins.loader import default_chain_specs, load_plugin_manager
    from mcp_context_forge_amd.services.upstream import make_fake_time_upstream

    specs = default_chain_specs()
    for s in specs:
        if s["name"] == "response_cache_by_prompt":
            s["config"] = {"cacheable_tools": ["fast-time-convert_time"]}
    e = GatewayEngine(Settings(database_url="sqlite://", federation_enabled=False, auth_required=False, gpu_enabled=gpu,
                               gpu_semcache_capacity=1024, gpu_semcache_topk=topk),
                      plugin_manager=load_plugin_manager(specs=specs))
    await e.gateway_service.register_gateway(name="fast-time", url="inproc://t", client=make_fake_time_upstream())
    if gpu:
        assert e.enable_gpu()
    return e


def test_pipeline_two_tenants_both_hit():
    raw = _mk("fast-time-convert_time", {"time": "2026-02-02T02:02:02Z", "source_timezone": "UTC",
                                         "target_timezone": "UTC"}, 1)
    users = ["alice", "mallory", "alice", "mallory"]

    async def run(gpu, topk):
        e = await _engine(gpu, topk)
        outs = [json.loads((await e.process_rpc_batch([raw], users=[u]))[0])["result"] for u in users]
        sem = e.gpu_pipeline.semcache if gpu else None
        counts = (sem.hits, sem.size) if gpu else None
        await e.shutdown()
        return outs, counts

    cpu_outs, _ = asyncio.run(run(False, 0))
    outs, (hits, size) = asyncio.run(run(True, 4))
    assert outs == cpu_outs
    assert hits == 2 and size == 2                      # both second requests hit; no insert follows a hit
    _, (hits_off, _) = asyncio.run(run(True, 0))
    assert hits_off == 1                                # setting off: alice's slot shadows mallory's, as before
