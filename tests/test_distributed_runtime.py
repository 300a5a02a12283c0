"""Distributed gateway runtime over gloo world-2: shared-DB registry with
broadcast invalidation + cross-rank RPC forwarding (the complete Redis
replacement — reference: session_affinity + plugin invalidation pub/sub)."""

import os
import subprocess
import sys
from pathlib import Path

REPO = str(Path(__file__).resolve().parent.parent)

WORKER = r"""
import asyncio, json, os, sys
import torch.distributed as dist
from mcp_context_forge_amd.config import Settings
from mcp_context_forge_amd.engine import GatewayEngine
from mcp_context_forge_amd.parallel import collectives
from mcp_context_forge_amd.parallel.runtime import DistributedGateway

rank, world = collectives.init_from_env()
db_path = os.environ["SHARED_DB"]

async def main():
    engine = GatewayEngine(Settings(database_url=f"sqlite:///{db_path}",
                                    federation_enabled=False, auth_required=False,
                                    plugins_enabled=False),
                           rank=rank, world_size=world)
    dg = DistributedGateway(engine, cadence_us=2000)
    await dg.start()
    try:
        assert dg.is_leader == (rank == 0)
        await asyncio.to_thread(collectives.barrier)
        if rank == 0:
            # leader registers a LOCAL tool (handler exists only on rank 0)
            async def only_here(args):
                return {"served_by_rank": 0, **args}

            engine.tool_service.register_local_tool("rank0_tool", only_here)
            dg.broadcast_invalidation("registry")
        # wait for invalidation to propagate (shared sqlite + broadcast)
        for _ in range(200):
            if engine.registry.find("tool", "rank0_tool"):
                break
            await asyncio.sleep(0.02)
        assert engine.registry.find("tool", "rank0_tool") is not None, f"rank {rank} never saw the tool"

        if rank == 1:
            # rank 1 has no handler → forward to the owner rank over the bus
            raw = json.dumps({"jsonrpc": "2.0", "id": 1, "method": "tools/call",
                              "params": {"name": "rank0_tool", "arguments": {"q": 9}}}).encode()
            out = await dg.forward_rpc(0, raw)
            res = json.loads(out)
            assert res["result"]["structuredContent"] == {"served_by_rank": 0, "q": 9}, res
        # NB: dist.barrier() would block the event loop and starve the bus
        # handler on the serving rank — run it in a thread (documented in
        # parallel/runtime.py).
        await asyncio.to_thread(collectives.barrier)
    finally:
        await dg.stop()
    if rank == 0:
        print("DISTRIBUTED_OK")

asyncio.run(main())
dist.destroy_process_group()
"""


def test_distributed_runtime_world2(tmp_path):
    script = tmp_path / "dist_worker.py"
    script.write_text(WORKER)
    db = tmp_path / "shared.db"
    env = dict(os.environ, PYTHONPATH=REPO, SHARED_DB=str(db))
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", "29671", str(script)],
        capture_output=True, text=True, timeout=240, env=env, cwd=REPO)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "DISTRIBUTED_OK" in out.stdout


ROUTER_WORKER = r"""
import asyncio, json, os, sys
import torch.distributed as dist
from mcp_context_forge_amd.config import Settings
from mcp_context_forge_amd.engine import GatewayEngine
from mcp_context_forge_amd.parallel import collectives
from mcp_context_forge_amd.parallel.runtime import DistributedGateway
from mcp_context_forge_amd.services.upstream import NativeInProcUpstream

rank, world = collectives.init_from_env()

async def main():
    # each rank has its OWN registry (sharded upstreams, BASELINE config 3)
    engine = GatewayEngine(Settings(database_url="sqlite://",
                                    federation_enabled=False, auth_required=False,
                                    plugins_enabled=True),
                           rank=rank, world_size=world)
    dg = DistributedGateway(engine, cadence_us=2000)
    up = NativeInProcUpstream(name=f"up{rank}")
    await engine.gateway_service.register_gateway(
        name=f"up{rank}", url=f"inproc://up{rank}", client=up, owner_rank=rank)
    # ownership sync is a collective on the default group: run it BEFORE the
    # bus pump starts so the two never interleave
    await dg.sync_tool_ownership()
    await dg.start()
    try:
        other = 1 - rank
        assert f"up{other}-echo" in engine.foreign_tools, engine.foreign_tools
        assert engine.foreign_tools[f"up{other}-echo"] == other
        # a batch mixing local + foreign tools routes transparently
        raws = []
        for i in range(8):
            target = rank if i % 2 == 0 else other
            raws.append(json.dumps({
                "jsonrpc": "2.0", "id": i, "method": "tools/call",
                "params": {"name": f"up{target}-echo", "arguments": {"msg": f"r{rank}-i{i}"}},
            }).encode())
        outs = await engine.process_rpc_batch(raws, users=[f"user{rank}"] * len(raws))
        assert len(outs) == 8
        for i, o in enumerate(outs):
            res = json.loads(o)
            assert res["id"] == i, res
            assert "result" in res, res
            text = res["result"]["content"][0]["text"]
            assert f"r{rank}-i{i}" in text, (i, res)
        await asyncio.to_thread(collectives.barrier)
    finally:
        await dg.stop()
    if rank == 0:
        print("ROUTING_OK")

asyncio.run(main())
dist.destroy_process_group()
"""


def test_cross_rank_tool_routing_world2(tmp_path):
    """Foreign-tool rows in a batch ride the bus to their owner rank and the
    responses splice back in order (the pipeline's fw_state path on GPU; the
    per-request handle_rpc_bytes path on CPU — this exercises the latter plus
    the rpc_batch bus handler both directions)."""
    script = tmp_path / "router_worker.py"
    script.write_text(ROUTER_WORKER)
    env = dict(os.environ, PYTHONPATH=REPO)
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", "29673", str(script)],
        capture_output=True, text=True, timeout=240, env=env, cwd=REPO)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ROUTING_OK" in out.stdout
