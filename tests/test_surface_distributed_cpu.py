"""parallel.gather_surface on the CPU: gloo processes each reduce their shard of an adversarial
summary matrix on the host, all-gather the aggregates and merge them, and every rank must hold
the surface of the whole matrix, byte for byte (the transport of test_distributed_cpu.py)."""
import os
import socket

import pytest

S, P = 65, 12


def _worker(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    import dbx_amd as D
    from dbx_amd import parallel as PAR
    from surface_cases import adversarial
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        m, ids = adversarial(S, P)
        begin, count = PAR.shard(S, world, rank)
        local = D.surface_host(m[begin:begin + count], ids[begin:begin + count])
        got = PAR.gather_surface(local, dist)
        assert got.best.tobytes() == local.best.tobytes()
        q.put((rank, got.params.tobytes()))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 3])
def test_gathered_surface_equals_the_whole(world):
    import torch.multiprocessing as mp
    from surface_cases import adversarial_ref
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = adversarial_ref(S, P)[0].tobytes()
    assert sorted(r for r, _ in out) == list(range(world))
    for rank, params in out:
        assert params == want, rank
