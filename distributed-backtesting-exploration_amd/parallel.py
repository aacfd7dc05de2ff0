"""Multi-GPU layout of the hot path: one process per GPU, symbols sharded in
contiguous blocks, no data-path collective. The only exchange is at the end of a step:
an all-gather of every rank's top-k records (k x 24 B) and an all-reduce of the run counters,
over torch.distributed (backend "nccl" = RCCL over xGMI on MI355X; "gloo" in CPU tests).

The reference has one parallelism strategy — file-level job farming, each worker taking whole
files (/root/reference/src/server/main.rs:131-143) — and no collectives at all; this module is
the MI355X-native replacement for scale-out inside one node.
"""
from __future__ import annotations

import numpy as np

from .engine import TOPK_DTYPE, merge_topk


def shard(n_symbols: int, world: int, rank: int) -> tuple:
    """Contiguous block of symbols for `rank`: S_g = ceil(S / G) (the last block may be short)."""
    per = -(-n_symbols // world)
    begin = min(rank * per, n_symbols)
    return begin, max(0, min(per, n_symbols - begin))


def _device_for(dist):
    import torch
    return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" \
        else torch.device("cpu")


def gather_topk(local: np.ndarray, k: int, dist) -> np.ndarray:
    """All-gather every rank's top-k records and merge them with the engine's order
    (sharpe desc, sym asc, param asc). Ranks may hold fewer than k records."""
    import torch
    world = dist.get_world_size()
    buf = np.zeros(k, TOPK_DTYPE)
    n = min(len(local), k)
    buf[:n] = np.asarray(local, TOPK_DTYPE)[:n]
    dev = _device_for(dist)
    t = torch.from_numpy(buf.view(np.int64).reshape(k, 3).copy()).to(dev)
    cnt = torch.tensor([n], dtype=torch.int64, device=dev)
    bufs = [torch.empty_like(t) for _ in range(world)]
    cnts = [torch.empty_like(cnt) for _ in range(world)]
    dist.all_gather(bufs, t)
    dist.all_gather(cnts, cnt)
    parts = [b.cpu().numpy().reshape(-1).view(TOPK_DTYPE)[:int(c.item())] for b, c in zip(bufs, cnts)]
    return merge_topk(np.concatenate(parts) if parts else np.zeros(0, TOPK_DTYPE), k)


def gather_surface(local, dist):
    """All-gather every rank's per-parameter aggregates (Surface.params, P x 104 B) and merge
    them with bt_surface_merge: the surface of the whole symbol universe, identical on every rank
    and identical to a single engine's (docs/surface_spec.md §3). The per-symbol records are not
    exchanged: the result's `best` is this rank's own."""
    import torch
    from .engine import PARAM_AGG_DTYPE, Surface, merge_surfaces
    world = dist.get_world_size()
    mine = np.ascontiguousarray(local.params, PARAM_AGG_DTYPE)
    t = torch.from_numpy(mine.view(np.uint8).copy()).to(_device_for(dist))
    out = torch.empty(world * t.numel(), dtype=torch.uint8, device=t.device)
    dist.all_gather_into_tensor(out, t)
    blocks = out.cpu().numpy().view(PARAM_AGG_DTYPE).reshape(world, len(mine))
    return Surface(merge_surfaces([Surface(b, None) for b in blocks]).params, local.best)


def exchange(local: np.ndarray, k: int, counters, dist) -> tuple:
    """The whole per-step exchange as ONE all-gather of the byte message bt_exchange_async sends
    over RCCL (csrc/comm.cpp: [header record with the count | k records | bar-evals | trades]),
    merged by the same C function bt_exchange_wait calls (bt_exchange_merge). This is the
    torch.distributed carrier of that exchange: the fallback when the C-ABI communicator cannot
    be created, and the rehearsal with ranks sharing one GPU (gloo), so the world > 1 parse and
    merge run the product code either way. counters = [bar-evals, trades].
    Returns (merged top-k, summed counters)."""
    import torch
    from .engine import exchange_merge, exchange_message
    world = dist.get_world_size()
    evals, trades = (int(v) for v in counters)
    n = min(len(local), k)
    msg = exchange_message(np.asarray(local, TOPK_DTYPE)[:n], k, evals, trades)
    t = torch.frombuffer(bytearray(msg), dtype=torch.uint8).to(_device_for(dist))
    out = torch.empty(world * len(msg), dtype=torch.uint8, device=t.device)
    dist.all_gather_into_tensor(out, t)
    return exchange_merge(out.cpu().numpy().tobytes(), world, k, k)


class PendingExchange:
    """An exchange (see `exchange`) whose all-gather is in flight: wait() returns (merged top-k,
    summed counters). Lets a caller overlap the collective with its next step."""

    def __init__(self, work, out, world, k):
        self._work, self._out, self._world, self._k = work, out, world, k

    def wait(self) -> tuple:
        from .engine import exchange_merge
        self._work.wait()
        return exchange_merge(self._out.cpu().numpy().tobytes(), self._world, self._k, self._k)


def exchange_async(local: np.ndarray, k: int, counters, dist) -> PendingExchange:
    """`exchange` with the all-gather issued asynchronously (async_op): the same byte message
    and merge, completed by PendingExchange.wait()."""
    import torch
    from .engine import exchange_message
    world = dist.get_world_size()
    evals, trades = (int(v) for v in counters)
    n = min(len(local), k)
    msg = exchange_message(np.asarray(local, TOPK_DTYPE)[:n], k, evals, trades)
    t = torch.frombuffer(bytearray(msg), dtype=torch.uint8).to(_device_for(dist))
    out = torch.empty(world * len(msg), dtype=torch.uint8, device=t.device)
    work = dist.all_gather_into_tensor(out, t, async_op=True)
    return PendingExchange(work, out, world, k)


def make_comm(dist, device: int, k: int):
    """The C-ABI exchange (engine.Comm over RCCL) for this process group: rank 0 creates the RCCL
    unique id, the launcher's process group broadcasts it, every rank joins. Every rank raises the
    same BtError when rank 0 has no id (RCCL not loadable there), rather than ranks 1.. waiting in
    the broadcast for a rank that gave up; and the ranks agree afterwards, so a rank whose join
    failed makes every rank fall back together (bench.py: torch.distributed carrier)."""
    import torch
    from .engine import BtError, Comm
    uid, why = None, ""
    if dist.get_rank() == 0:
        try:
            uid = Comm.unique_id()
        except Exception as e:  # noqa: BLE001 — reported on every rank below
            why = str(e)
    obj = [(uid, why)]
    dist.broadcast_object_list(obj, src=0)
    uid, why = obj[0]
    if uid is None:
        raise BtError(f"no RCCL unique id on rank 0: {why}")
    comm, why = None, ""
    try:
        comm = Comm(uid, dist.get_rank(), dist.get_world_size(), device, k)
    except Exception as e:  # noqa: BLE001
        why = str(e)
    ok = torch.tensor([1 if comm is not None else 0], dtype=torch.int32, device=_device_for(dist))
    dist.all_reduce(ok, op=dist.ReduceOp.MIN)
    if int(ok.item()) == 0:
        if comm is not None:
            comm.close()
        raise BtError(f"RCCL communicator not created on every rank{': ' + why if why else ''}")
    return comm


def allreduce_counters(values, dist) -> list:
    """Sum int64 run counters (bar-evals, trades, errors) over all ranks."""
    import torch
    t = torch.tensor([int(v) for v in values], dtype=torch.int64, device=_device_for(dist))
    dist.all_reduce(t)
    return [int(x) for x in t.cpu().tolist()]
