"""One process per GPU (torch.distributed; backend "nccl" = RCCL on ROCm, "gloo" on CPU for the tests).

Three ways the path uses more than one GPU:
  * replicas of a massive-body system (ensembles, forward/backward): no data-path collective, only the timing is
    reduced (max over ranks);
  * the massless sweep: spacecraft are independent given the ephemeris -> `shard_range` over craft;
  * ONE massive-body system partitioned by target body (`shard_nbody`): one all-gather of the packed positions per
    force evaluation, RCCL over xGMI inside the library (`eph_nbody_shard`), or a caller-supplied exchange
    (`host_staged_exchange`: through host memory and any torch.distributed backend -- what the tests use to run
    two ranks on one GPU).

The massless sweep's time is the maximum over ranks, and craft differ in work by a factor 70 (a low orbit: 215 steps a day;
a heliocentric cruise: 3), so WHICH craft a rank gets matters as soon as the population arrives sorted by orbit type:
  * the estimate (`craft_cost_estimate`): span / tau per craft, tau the time scale of its orbit about its dominant body --
    the body with the smallest local dynamical time sqrt(d^3 / mu); sqrt(a^3 / mu) with the semi-major axis a from the vis-viva
    energy of the relative state when that orbit is bound, 16 x the local value when it is not. A numpy restatement of the
    library's own lane-deal estimate (k_craft_tau, csrc/craft.hip), which no C entry point exposes; it only orders and weights.
  * the rule (`balanced_partition`): the snake deal. Craft sorted by falling cost (stable: ties by index; NaN, infinite and
    non-positive costs first, in index order), position k of that order to rank r = k mod 2 world, mirrored (2 world - 1 - r)
    when r >= world. Deterministic -- every rank computes the same blocks, nothing is exchanged --, block sizes differ by at most
    one (equal memory, equal-width all-gather), and every rank gets every orbit family in proportion.
  * `sharded_sweep` is the one call: estimate (each rank a contiguous slice, all-gathered), partition, this rank's
    SpacecraftBatch, propagate, summary, `gather_craft_records` (one all-gather, scattered back into craft order).
  `bench.py --workload craft` still uses the contiguous split (`shard_range`): its population is homogeneous or interleaved.
"""
import ctypes as C
import os


def env_rank():
    """(rank, local_rank, world_size) from the torch.distributed.run environment; (0, 0, 1) when run directly."""
    return (int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")),
            int(os.environ.get("WORLD_SIZE", "1")))


def shard_range(n_items, rank, world):
    """Contiguous block partition of n_items independent work items; blocks differ by at most one item."""
    base, extra = divmod(n_items, world)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def replica_seed(base_seed, rank):
    return base_seed + rank


def reduce_timing(elapsed_s, units_local, dist=None, device="cpu"):
    """Whole-job throughput = (sum of units over ranks) / (max elapsed over ranks). `dist` is torch.distributed
    (initialised) or None for a single process. Returns (total_units, max_elapsed)."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return float(units_local), float(elapsed_s)
    import torch
    t = torch.tensor([float(elapsed_s)], dtype=torch.float64, device=device)
    u = torch.tensor([float(units_local)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dist.all_reduce(u, op=dist.ReduceOp.SUM)
    return float(u.item()), float(t.item())


def _single(dist):
    return dist is None or not dist.is_initialized() or dist.get_world_size() == 1


def _gather_blocks(mine, blocks, dist, device):
    """The all-gather behind a partition by index blocks: `mine` = this rank's rows ([len(blocks[rank]), ...], any fixed-size
    dtype) in its block's order -> all rows in craft order, on every rank. Equal-width, zero-padded byte slices, one collective,
    then out[blocks[r]] = recv[r, :len(blocks[r])]."""
    import numpy as np
    import torch
    mine = np.ascontiguousarray(mine)
    n_total = sum(len(b) for b in blocks)
    out = np.empty((n_total,) + mine.shape[1:], dtype=mine.dtype)
    if _single(dist):
        assert len(blocks) == 1 and len(mine) == n_total
        out[blocks[0]] = mine
        return out
    rank, world = dist.get_rank(), dist.get_world_size()
    assert len(blocks) == world and len(mine) == len(blocks[rank])
    row = mine.dtype.itemsize * int(np.prod(mine.shape[1:], dtype=np.int64))
    width = max(len(b) for b in blocks) * row
    if width == 0:                                                # (no craft at all: every rank knows, nothing to exchange)
        return out
    send = torch.zeros(width, dtype=torch.uint8)
    send[: mine.nbytes] = torch.from_numpy(mine.reshape(-1).view(np.uint8))
    send = send.to(device)
    recv = torch.empty(world * width, dtype=torch.uint8, device=device)
    dist.all_gather_into_tensor(recv, send)
    recv = recv.cpu().numpy().reshape(world, width)
    for r, block in enumerate(blocks):
        out[block] = recv[r, : len(block) * row].view(mine.dtype).reshape((len(block),) + mine.shape[1:])
    return out


def gather_craft_states(state, n_total, dist=None, device="cpu", blocks=None):
    """The result exchange of the massless sweep (`ncclAllGather` of the final states): every rank holds the
    final (t, position, velocity) of its contiguous block of spacecraft (`shard_range`); returns the [n_total, 7] array of
    all of them on every rank. One all-gather of equal, zero-padded slices -- RCCL over xGMI with backend "nccl" and
    device="cuda" (56 B per craft: 56 MB for 1e6), gloo on CPU in the tests. `state` = SpacecraftBatch.state().
    `blocks` (one ascending index array per rank, the same on every rank: `balanced_partition`): this rank holds the craft
    blocks[rank], in that order, instead of a contiguous block; the table comes back in craft order all the same."""
    import numpy as np
    import torch
    if isinstance(state, np.ndarray) and state.dtype.names and state.dtype.itemsize == 80:
        # SpacecraftBatch.summary(): t, pos, vel are the first seven doubles of every 80-byte record -- a view, no copy
        mine = state.view(np.float64).reshape(-1, 10)[:, :7]
    else:                                                          # the dict of arrays from SpacecraftBatch.state()
        mine = np.concatenate([np.asarray(state["t"])[:, None], np.asarray(state["pos"]), np.asarray(state["vel"])], axis=1)
    if blocks is not None:
        assert sum(len(b) for b in blocks) == n_total
        return _gather_blocks(mine, blocks, dist, device)
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        assert len(mine) == n_total
        return mine
    rank, world = dist.get_rank(), dist.get_world_size()
    width = -(-n_total // world)                                  # largest block of shard_range
    lo, hi = shard_range(n_total, rank, world)
    assert hi - lo == len(mine)
    send = torch.zeros((width, 7), dtype=torch.float64, device=device)
    send[: hi - lo] = torch.from_numpy(np.ascontiguousarray(mine)).to(device)
    recv = torch.empty((world * width, 7), dtype=torch.float64, device=device)
    dist.all_gather_into_tensor(recv, send)
    recv = recv.cpu().numpy().reshape(world, width, 7)
    return np.concatenate([recv[r, : shard_range(n_total, r, world)[1] - shard_range(n_total, r, world)[0]]
                           for r in range(world)], axis=0)


def gather_craft_records(records, blocks, dist=None, device="cpu"):
    """The result exchange of a sweep partitioned by `blocks` (`balanced_partition`; the same list on every rank): every rank
    passes the SpacecraftBatch.RECORD array (summary()) of ITS block, in its block's order, and gets the [n_total] record array in
    craft order. One all-gather of equal-width, zero-padded byte slices (80 B per craft), then out[blocks[r]] = recv[r, :len(blocks[r])].
    A single process (dist None or world 1): the input scattered through blocks[0]."""
    return _gather_blocks(records, blocks, dist, device)


def craft_cost_estimate(mu, body_pos, body_vel, pos, vel, span, chunk=32768):
    """Work estimate per craft for a sweep over `span` seconds (a scalar or [n]): span / tau, tau the time scale of the craft's
    orbit about its DOMINANT body -- the body with the smallest local dynamical time local = sqrt(d^3 / mu) (bodies with mu <= 0
    are skipped): sqrt(a^3 / mu), a = -mu / (2 energy), when the relative orbit is bound (energy < 0), 16 local when it is not.
    The library's estimate for its deal of craft to lanes (k_craft_tau, csrc/craft.hip) restated in numpy, in binary64: it only has
    to order and weight craft (log estimate against log attempts: correlation 0.98-0.99 on the mixed population).
    body_pos, body_vel: [n_bodies, 3] when all craft share one epoch, or anything that broadcasts to [n, n_bodies, 3] (the bodies at
    each craft's own epoch). Returns float64[n]; a craft with no body to orbit gets 0 (`balanced_partition` deals such craft first).
    `chunk`: craft per pass -- the [chunk, n_bodies, 3] temporaries of a pass stay near 50 MB for 32 bodies whatever n is (measured peak
    at n = 1e6: 54 MB, 1.4 s); every craft's value is the same whatever the chunk."""
    import numpy as np
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    pos, vel = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(vel, dtype=np.float64).reshape(-1, 3)
    n, nb = len(pos), len(mu)
    bp, bv = np.asarray(body_pos, dtype=np.float64), np.asarray(body_vel, dtype=np.float64)
    span = np.asarray(span, dtype=np.float64)
    heavy = mu > 0.0
    safe_mu = np.where(heavy, mu, 1.0)
    cost = np.empty(n)
    chunk = max(int(chunk), 1)

    def rows(a, lo, hi):                                           # body states of craft lo..hi-1 as [hi - lo | 1, n_bodies, 3]
        a = a.reshape((1,) * (3 - a.ndim) + a.shape)
        return a[lo:hi] if a.shape[0] != 1 else a

    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        d = pos[lo:hi, None, :] - rows(bp, lo, hi)
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        del d
        with np.errstate(all="ignore"):
            local = np.sqrt(d2 * np.sqrt(d2) / safe_mu)
            local[~(heavy[None, :] & (local == local))] = np.inf
            j = np.argmin(local, axis=1)                           # (the first of equal minima, like the kernel's local < best)
            i = np.arange(hi - lo)
            best, dist2, m = local[i, j], d2[i, j], mu[j]
            del local, d2
            ub = np.broadcast_to(rows(bv, lo, hi), (hi - lo, nb, 3))[i, j]
            u = vel[lo:hi] - ub
            energy = 0.5 * (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]) - m / np.sqrt(dist2)
            sma = -m / (2.0 * energy)
            tau = np.where(energy < 0.0, np.sqrt(sma * sma * sma / m), 16.0 * best)
            tau[~np.isfinite(best)] = np.inf                      # no massive body at all: nothing to orbit
            cost[lo:hi] = (span[lo:hi] if span.ndim else span) / tau
    return cost


def balanced_partition(cost, world):
    """Cost-balanced partition of n craft over `world` ranks: a list of `world` ascending int64 index arrays, disjoint, covering
    0..n-1, sizes differing by at most one. The snake deal: order = stable argsort of falling cost (ties by index; craft whose cost
    is NaN, infinite or <= 0 first, in index order, as if they were the most expensive); position k of `order` goes to rank
    r = k mod 2 world, or 2 world - 1 - r when r >= world. Deterministic: every rank computes the same blocks from the same costs,
    no communication. Every rank receives every cost class in proportion, so the library's own deal of a batch to the lanes sees
    the same mix on each rank. world 1: arange(n)."""
    import numpy as np
    cost = np.asarray(cost, dtype=np.float64).reshape(-1)
    world = int(world)
    if world < 1:
        raise ValueError("balanced_partition: world >= 1")
    n = len(cost)
    if world == 1:
        return [np.arange(n, dtype=np.int64)]
    with np.errstate(invalid="ignore"):
        key = np.where(np.isfinite(cost) & (cost > 0.0), cost, np.inf)
    order = np.argsort(-key, kind="stable")
    r = np.arange(n, dtype=np.int64) % (2 * world)
    r = np.where(r >= world, 2 * world - 1 - r, r)
    return [np.sort(order[r == q]).astype(np.int64) for q in range(world)]


def body_states_at(solution, t, dist=None, device="cpu", group=None):
    """(pos[n_bodies, 3], vel[n_bodies, 3]) of the massive bodies at epoch t, through Solution.eval: what `craft_cost_estimate` and
    `sharded_sweep(body_states=...)` take. With an initialised process group rank 0 evaluates and broadcasts (6 doubles per
    body: 192 for 32 bodies): the ranks that imported the table image (`broadcast_ephemeris`) hold no Solution and pass None.
    ValueError (on every rank) when t lies outside a body's spline."""
    import numpy as np
    world = 1 if _single(dist) else dist.get_world_size(group)
    rank = 0 if world == 1 else dist.get_rank(group)
    states, ok = None, True
    if rank == 0:
        nb = int(solution.n)
        states = np.zeros((2, nb, 3))
        for b in range(nb):
            p, v, inside = solution.eval(b, float(t))
            states[0, b], states[1, b] = p[0], v[0]
            ok = ok and bool(inside[0])
    if world > 1:
        import torch
        head = torch.tensor([states.shape[1] if rank == 0 else 0, int(ok)], dtype=torch.int64, device=device)
        dist.broadcast(head, src=0, group=group)
        nb, ok = int(head[0].item()), bool(head[1].item())
        buf = torch.from_numpy(states).to(device) if rank == 0 else torch.empty((2, nb, 3), dtype=torch.float64, device=device)
        dist.broadcast(buf, src=0, group=group)
        states = buf.cpu().numpy()
    if not ok:
        raise ValueError(f"body_states_at: epoch {t} is outside a body's spline")
    return states[0].copy(), states[1].copy()


def sharded_sweep(eph, t0, pos, vel, t_end, *, mu=None, body_states=None, cost=None, partition="balanced", method="Verner87",
                  params=None, burns=None, max_knots=4096, dist=None, device="cpu"):
    """One sweep of n craft over the ranks of the process group, in one call: every rank passes the SAME t0 (a scalar or [n]),
    pos, vel, burns (all craft) and gets every craft's record back.
      cost       per-craft weights ([n], e.g. the previous sweep's records["attempts"]); else estimated from `mu` and
                 body_states = (body_pos, body_vel) (`body_states_at`): rank r estimates the contiguous slice shard_range(n, r, world)
                 and the slices are all-gathered, so the estimate scales with the ranks. Not needed for "contiguous".
      partition  "balanced" (`balanced_partition` of the cost) | "contiguous" (`shard_range`).
    Then a SpacecraftBatch of this rank's craft (burns sliced per craft), propagate(t_end), summary(), `gather_craft_records`.
    The knot slabs are not drained: EPH_KNOTS_FULL shows in records["status"]. A rank whose block is empty runs an empty batch.
    Returns {"records": craft order, every rank; "blocks"; "batch": this rank's, resident (knots, events, further calls);
    "rank_attempts": int64[world]; "balance": max / mean of it; "estimate_s", "partition_s", "sweep_s", "gather_s"}."""
    import time

    import numpy as np

    from . import SpacecraftBatch
    pos, vel = np.asarray(pos, dtype=np.float64).reshape(-1, 3), np.asarray(vel, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    t0 = np.asarray(t0, dtype=np.float64)
    if partition not in ("balanced", "contiguous"):
        raise ValueError(f"sharded_sweep: partition {partition!r}")
    single = _single(dist)
    rank, world = (0, 1) if single else (dist.get_rank(), dist.get_world_size())
    tick = time.perf_counter()
    if partition == "balanced" and cost is None:
        if mu is None or body_states is None:
            raise ValueError("sharded_sweep: the balanced partition needs `cost`, or `mu` and `body_states`")
        lo, hi = shard_range(n, rank, world)
        bp, bv = (np.asarray(a, dtype=np.float64) for a in body_states)
        bp, bv = (a[lo:hi] if a.ndim == 3 and a.shape[0] == n else a for a in (bp, bv))
        span = float(t_end) - (t0[lo:hi] if t0.ndim else t0)
        mine = craft_cost_estimate(mu, bp, bv, pos[lo:hi], vel[lo:hi], span)
        edges = [shard_range(n, r, world) for r in range(world)]
        cost = _gather_blocks(mine, [np.arange(a, b, dtype=np.int64) for a, b in edges], dist, device)
    estimate_s = time.perf_counter() - tick
    tick = time.perf_counter()
    if partition == "balanced":
        if len(np.asarray(cost).reshape(-1)) != n:
            raise ValueError("sharded_sweep: one cost per craft")
        blocks = balanced_partition(cost, world)
    else:
        blocks = [np.arange(*shard_range(n, r, world), dtype=np.int64) for r in range(world)]
    partition_s = time.perf_counter() - tick
    own = blocks[rank]
    tick = time.perf_counter()
    batch = SpacecraftBatch(eph, t0[own] if t0.ndim else t0, pos[own], vel[own], method, params,
                            None if burns is None else [burns[i] for i in own], max_knots=max_knots)
    batch.propagate(float(t_end))
    rec = batch.summary()
    sweep_s = time.perf_counter() - tick
    tick = time.perf_counter()
    records = gather_craft_records(rec, blocks, dist, device)
    gather_s = time.perf_counter() - tick
    rank_attempts = np.array([int(records["attempts"][b].sum(dtype=np.int64)) for b in blocks], dtype=np.int64)
    mean = rank_attempts.mean() if world else 0.0
    return {"records": records, "blocks": blocks, "batch": batch, "rank_attempts": rank_attempts,
            "balance": float(rank_attempts.max() / mean) if mean > 0 else 1.0,
            "estimate_s": estimate_s, "partition_s": partition_s, "sweep_s": sweep_s, "gather_s": gather_s}


def _hip():
    from . import hip_runtime
    return hip_runtime()          # the runtime the library itself uses (a torch process carries a second one)


def host_staged_exchange(dist, group=None):
    """An eph_exchange_fn body: in-place all-gather of equal slices through host memory and torch.distributed
    (any backend, CPU tensors). Slow by construction (two PCIe copies and a host sync per force evaluation): it is
    the portable fallback and the test transport; production runs pass an RCCL unique id instead."""
    import numpy as np
    import torch
    hip = _hip()
    D2H, H2D = 2, 1

    def exchange(dev_ptr, slice_bytes, rank, world, stream):
        if hip.hipStreamSynchronize(stream):
            return 2
        mine = np.empty(slice_bytes, dtype=np.uint8)
        if hip.hipMemcpy(mine.ctypes.data, dev_ptr + rank * slice_bytes, slice_bytes, D2H):
            return 3
        parts = [torch.empty(slice_bytes, dtype=torch.uint8) for _ in range(world)]
        dist.all_gather(parts, torch.from_numpy(mine), group=group)
        for r, part in enumerate(parts):
            if r == rank:
                continue
            a = part.numpy()
            if hip.hipMemcpy(dev_ptr + r * slice_bytes, a.ctypes.data, slice_bytes, H2D):
                return 4
        return 0

    return exchange


def broadcast_unique_id(dist, make_id, device="cpu", group=None):
    """Rank 0 makes the 128-byte RCCL id (make_id()), every rank returns it."""
    import torch
    buf = torch.zeros(128, dtype=torch.uint8, device=device)
    if dist.get_rank() == 0:
        buf = torch.tensor(list(make_id()), dtype=torch.uint8, device=device)
    dist.broadcast(buf, src=0, group=group)
    return bytes(buf.cpu().tolist())


def broadcast_ephemeris(build, dist=None, device="cpu", group=None, from_image=None):
    """rank 0 builds the massive bodies' table ONCE (build() -> Ephemeris), exports it as one contiguous image
    (eph_ephemeris_export) and broadcasts it; every other rank imports it (eph_ephemeris_import) instead of integrating the bodies
    again. `device`: where the broadcast buffers live ("cuda" with the nccl = RCCL backend: over xGMI; "cpu" with gloo).
    Returns (ephemeris, {"build_s", "export_s", "broadcast_s", "import_s", "bytes"}); the table is bit-identical on every rank
    (tests/test_gpu_bench.py compares the images). `from_image`: Ephemeris.from_image unless given (the CPU test of this plumbing
    passes a stand-in). The importing ranks hold the table but no Solution: the bodies' states at an epoch (what the cost
    estimate of `sharded_sweep` needs) reach them through `body_states_at` -- rank 0 evaluates, 6 doubles per body are broadcast."""
    import time

    import numpy as np
    if from_image is None:
        from . import Ephemeris
        from_image = Ephemeris.from_image
    t = {"build_s": 0.0, "export_s": 0.0, "broadcast_s": 0.0, "import_s": 0.0, "bytes": 0}
    world = 1 if dist is None or not dist.is_initialized() else dist.get_world_size(group)
    rank = 0 if world == 1 else dist.get_rank(group)
    eph, image = None, None
    if rank == 0:
        t0 = time.perf_counter()
        eph = build()
        t["build_s"] = time.perf_counter() - t0
        if world > 1:
            t0 = time.perf_counter()
            image = eph.export_image()
            t["export_s"] = time.perf_counter() - t0
            t["bytes"] = int(image.size)
    if world > 1:
        import torch
        t0 = time.perf_counter()
        size = torch.tensor([image.size if rank == 0 else 0], dtype=torch.int64, device=device)
        dist.broadcast(size, src=0, group=group)
        n = int(size.item())
        buf = torch.from_numpy(image).to(device) if rank == 0 else torch.empty(n, dtype=torch.uint8, device=device)
        dist.broadcast(buf, src=0, group=group)
        if device != "cpu":
            torch.cuda.synchronize()
        t["broadcast_s"] = time.perf_counter() - t0
        t["bytes"] = n
        if rank != 0:
            t0 = time.perf_counter()
            eph = from_image(np.ascontiguousarray(buf.cpu().numpy()))
            t["import_s"] = time.perf_counter() - t0
    return eph, t


def peer_transport(dist, slot_bytes=1 << 22, group=None):
    """A connected PeerTransport over the ranks of the process group: the 64-byte hipIpc handles travel through
    torch.distributed (all_gather_object: any backend), the data never does."""
    from . import PeerTransport
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    errors = []
    for memory in ("auto", "coarse"):                # a second round in plain device memory if ANY rank could not map a mailbox
        err, t = None, None
        try:
            t = PeerTransport(rank, world, slot_bytes, memory=memory)
        except Exception as e:                       # (the collective below must still be entered by every rank)
            err = f"rank {rank} create[{memory}]: {e}"
        handles = [None] * world
        dist.all_gather_object(handles, t.handle if t is not None else None, group=group)
        if err is None and all(h is not None for h in handles):
            try:
                t.connect(handles)
            except Exception as e:
                err = f"rank {rank} connect[{memory}]: {e}"
        outcome = [None] * world
        dist.all_gather_object(outcome, (err, t.memory if t is not None else None), group=group)
        if all(o[0] is None for o in outcome):       # every rank has mapped every mailbox before the first push
            t.forms = [o[1] for o in outcome]
            t.attempts = errors
            return t
        errors += [o[0] for o in outcome if o[0] is not None]
        del t
    raise RuntimeError("peer transport could not be set up: " + " | ".join(errors))


def shard_nbody(integration, dist=None, transport="rccl", device="cpu"):
    """Partition `integration` (an NBodyIntegration every rank created identically) over the ranks of the
    initialised process group. transport "rccl": RCCL inside the library; "peer": direct writes into hipIpc-mapped
    mailboxes (csrc/peer.hip); "host": host_staged_exchange."""
    if dist is None or not dist.is_initialized() or dist.get_world_size() == 1:
        return integration
    from . import rccl_unique_id
    rank, world = dist.get_rank(), dist.get_world_size()
    if transport == "rccl":
        uid = broadcast_unique_id(dist, rccl_unique_id, device=device)
        integration.shard(rank, world, unique_id=uid)
    elif transport == "peer":
        integration.shard_peer(peer_transport(dist))
    elif transport == "host":
        integration.shard(rank, world, exchange=host_staged_exchange(dist))
    else:
        raise ValueError(transport)
    return integration
