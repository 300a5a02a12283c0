"""RCCL affinity bus over gloo world-2 (reference analog: session_affinity
forwarding over Redis — tests the exchange-pump request/response semantics)."""

import os
import subprocess
import sys
from pathlib import Path

REPO = str(Path(__file__).resolve().parent.parent)

WORKER = r"""
import asyncio, json, sys
import torch.distributed as dist
from mcp_context_forge_amd.parallel import collectives
from mcp_context_forge_amd.parallel.bus import RcclBus, stable_hash

rank, world = collectives.init_from_env()

async def main():
    loop = asyncio.get_running_loop()

    async def handler(payload):
        await asyncio.sleep(0.001)
        return {"echo": payload, "served_by": rank}

    bus = RcclBus(handler, loop=loop, cadence_us=2000)
    bus.start()
    try:
        # each rank forwards to the OTHER rank
        dest = 1 - rank
        results = await asyncio.gather(*(bus.submit(dest, {"n": i, "from": rank}) for i in range(20)))
        assert all(r["served_by"] == dest for r in results), results[:2]
        assert sorted(r["echo"]["n"] for r in results) == list(range(20))
        # local submit bypasses the pump
        r = await bus.submit(rank, {"local": True})
        assert r["served_by"] == rank
        # ownership is stable and covers both ranks
        owners = {bus.owner_of(f"session-{i}") for i in range(64)}
        assert owners == {0, 1}
        assert stable_hash("x") == stable_hash("x")
        # keep pumping until both sides drained (symmetric shutdown)
        collectives.barrier()
    finally:
        bus.stop()
    if rank == 0:
        print("BUS_OK", json.dumps(bus.stats()))

asyncio.run(main())
dist.destroy_process_group()
"""


def test_bus_gloo_world2(tmp_path):
    script = tmp_path / "bus_worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, PYTHONPATH=REPO)
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
         "--master-addr", "127.0.0.1", "--master-port", "29651", str(script)],
        capture_output=True, text=True, timeout=240, env=env, cwd=REPO)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "BUS_OK" in out.stdout
