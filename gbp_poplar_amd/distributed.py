"""The split-phase C-ABI (gbp_iterate_begin / _local / _end) driven by a CALLER-OWNED collective — test harness and
example, not the product's multi-GPU path.

The product path is the library-owned exchange: `bin/ba --ipus N` / `bin/slam --ipus N` and bench.py fork / launch one
process per GPU, csrc/gbp_comm.cpp issues the RCCL all-gather inside gbp_iterate (ONE exchange
path).  This module stays because (a) the CPU suite exercises the sharding logic on 2 gloo ranks through it with an
oracle-backed engine (tests/test_distributed_gloo.py), (b) the GPU suite emulates N shards on one GPU with it
(dist=None: the "exchange" is a copy), (c) it documents what a caller with its own collective (torch.distributed, MPI)
has to do — examples/ba_torchrun.py.

Landmark-sharded multi-GPU GBP: one process per GPU, torch.distributed (RCCL over xGMI) for the
single exchange step of an iteration.

Replaces the reference's `--ipus N` (ba.cpp:414-417,617-623: one Poplar graph spread over N x 1216
tiles, exchange compiled by Poplar).  Here a rank owns a contiguous landmark range and every factor
incident to it; factor potentials, per-factor state, both message directions and landmark beliefs are
rank-local.  Cameras are replicated: per iteration each rank reduces its factor->camera messages to a
[C x 44] partial, ONE all-gather moves the partials, and every rank adds prior + partials in rank order
(deterministic, bit-identical camera beliefs on all ranks; no float atomics, no ring all-reduce whose
association order would differ between ranks).  So a rank's read() / read_priors() hold the cameras and the
landmark and per-factor entries of its own range; read(gather=True) / read_priors(gather=True) fetch every other
entry from its owner and return complete arrays on every rank.

`engine` is a rank-local object with the split-phase verbs of the C-ABI (gbp_iterate_begin/_end,
gbp_refresh_begin/_end, gbp_linearise_factors, ...): the product passes GbpEngine (HIP); the CPU gloo
tests pass an oracle-backed stand-in to exercise this host logic without a GPU.
"""
import numpy as np

CAM_REC = 44  # GBP_CAM_REC: eta 6, pad 2, Lambda 36


def landmark_partition(lmk_id, n_lmks, world):
    """Contiguous landmark ranges balanced by incident-factor count -> bounds[world+1]."""
    deg = np.bincount(np.asarray(lmk_id, dtype=np.int64), minlength=n_lmks).astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(deg)])
    total = int(csum[-1])
    bounds = [0]
    for r in range(1, world):
        target = total * r // world
        b = int(np.searchsorted(csum, target, side="left"))
        bounds.append(min(max(b, bounds[-1]), n_lmks))
    bounds.append(n_lmks)
    return np.asarray(bounds, dtype=np.uint32)


class ShardedGbp:
    """The Poplar program list over `world` ranks.  Same verbs as GbpEngine / the oracle."""

    def __init__(self, engine, n_cams, rank, world, dist=None, device="cpu", always_collective=False, use_graph=False,
                 lmk_id=None, lmk_range=None):
        """lmk_id [E], lmk_range (begin, end): the landmark of every factor and this rank's own landmark range — what
        read(gather=True) / read_priors(gather=True) need to know who owns which entry.  Left out, they are taken from the
        engine where it keeps them (GbpEngine and the oracle engines do: `problem`, `shard`)."""
        import torch
        self.torch = torch
        self.e = engine
        self.C, self.rank, self.world = int(n_cams), int(rank), int(world)
        self.dist = dist
        self._lmk_id = None if lmk_id is None else np.ascontiguousarray(lmk_id, dtype=np.int64)
        self._lmk_range = None if lmk_range is None else (int(lmk_range[0]), int(lmk_range[1]))
        self._owners = None                          # (ranges [world, 2], factors of every rank): made by the first gathered read
        self.always_collective = always_collective   # run the all-gather even for world == 1 (exercises RCCL in tests)
        self.use_graph = use_graph                   # capture kernels + collective of `graph_unroll` iterations
        self.graph_unroll = 10
        self.graph = None
        self.graph_error = None
        self.send = torch.zeros(self.C * CAM_REC, dtype=torch.float32, device=device)
        self.recv = torch.zeros(self.world * self.C * CAM_REC, dtype=torch.float32, device=device)
        self.stream = None
        if device != "cpu":
            # One dedicated (non-default) stream carries BOTH the engine's kernels and the collective, so
            # ordering is plain stream order: kernels -> all_gather (RCCL waits on / signals this stream) -> kernels.
            self.stream = torch.cuda.Stream()
            engine.set_stream(self.stream.cuda_stream)
            torch.cuda.synchronize()       # the zero-fills above ran on the default stream
        engine.set_exchange_buffers(self.send.data_ptr(), self.recv.data_ptr())

    def _on_stream(self):
        import contextlib
        return self.torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def _exchange(self):
        with self._on_stream():
            if self.dist is None or (self.world == 1 and not self.always_collective):
                self.recv.copy_(self.send)
            else:
                self.dist.all_gather_into_tensor(self.recv, self.send)

    def upload(self, state):
        self.e.upload(state)

    def linearise(self):
        """LINEARISE_PROG (ba.cpp:890-893): prog_ub needs the exchange, then relinearise local factors."""
        self.e.refresh_begin()
        self._exchange()
        self.e.refresh_end()
        self.e.linearise_factors()

    def _one_iteration(self, overlap):
        if overlap:
            # The collective runs on RCCL's stream, ordered after the sweep that filled `send`; the rank-local landmark half of
            # the belief update fills the GPU meanwhile; the camera combine waits for it.
            self.e.iterate_begin()
            with self._on_stream():
                work = self.dist.all_gather_into_tensor(self.recv, self.send, async_op=True)
            self.e.iterate_local()
            with self._on_stream():
                work.wait()
        else:
            self.e.iterate_begin()                      # sweep + local camera partials -> send
            self._exchange()
        self.e.iterate_end()

    def _capture(self, overlap):
        """Capture `graph_unroll` iterations (kernels of this engine AND the RCCL all-gather) into one hipGraph on
        the shared stream.  Returns False (and stays on direct launches) if the runtime refuses the capture."""
        torch = self.torch
        try:
            for _ in range(3):                       # RCCL must have run on this stream before a capture
                self._one_iteration(overlap)
            self.stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self.stream):
                for _ in range(self.graph_unroll):
                    self._one_iteration(overlap)
            self.graph = g
            return 3
        except Exception as exc:                     # noqa: BLE001 - any capture failure means "no graph"
            self.graph = None
            self.graph_error = repr(exc)
            self.use_graph = False
            try:
                self.stream.synchronize()
            except Exception:
                pass
            return None

    def iterate(self, n=1):
        n = int(n)
        overlap = (self.dist is not None and (self.world > 1 or self.always_collective) and self.stream is not None
                   and hasattr(self.e, "iterate_local"))
        if self.use_graph and self.stream is not None and self.dist is not None and n >= self.graph_unroll + 3:
            if self.graph is None:
                done = self._capture(overlap)
                if done is not None:
                    n -= done
            while self.graph is not None and n >= self.graph_unroll:
                with self._on_stream():
                    self.graph.replay()
                n -= self.graph_unroll
        for _ in range(n):
            self._one_iteration(overlap)

    def weaken_priors(self):
        self.e.weaken_priors()          # priors are replicated / local: no exchange (partials unchanged)

    def new_keyframe(self, upd):
        self.e.new_keyframe(upd)

    def read(self, gather=False):
        """The local rank's view: landmark and per-factor entries outside its range are left untouched.  gather=True
        (collective: every rank calls it): COMPLETE arrays on every rank — the cameras from its own copy, every landmark
        entry from the rank that owns it, every per-factor entry from the rank that owns the factor's landmark."""
        out = self.e.read()
        if gather and self._several_ranks():
            self._gather_owned(out, (("lmk_beliefs_eta", 3), ("lmk_beliefs_lambda", 9)),
                               ("damping", "damping_count", "robust_flag"))
        return out

    def solution(self, measurements=None, active_flag=None, gather=True):
        """GbpEngine.solution() of the sharded run: means, marginal covariances and status words of every variable — and, with
        `measurements` (the whole graph's, [2E]), the residual and reprojection covariance of every edge — from read(gather).
        gather=True (collective: every rank calls it): the complete solution on every rank; gather=False: this rank's view, entries of
        other ranks' landmarks and of their factors are meaningless.  numpy arrays; blocks."""
        from . import post
        out = post.moments(self.read(gather=gather))
        if measurements is not None:
            p = self.e.problem
            n_e = int(p.n_edges)
            ids = [np.ctypeslib.as_array(a, shape=(n_e,)) if n_e else np.zeros(0, np.uint32) for a in (p.cam_id, p.lmk_id)]
            out.update(post.residuals(ids[0], ids[1], [p.K[i] for i in range(9)], out, measurements, active_flag, covs=out))
        return out

    def read_priors(self, gather=False):
        """as read(): the local view, or with gather=True the landmark priors of every range from its owner"""
        out = self.e.read_priors()
        if gather and self._several_ranks():
            self._gather_owned(out, (("lmk_priors_eta", 3), ("lmk_priors_lambda", 9)), ())
        return out

    def _several_ranks(self):
        return self.dist is not None and self.world > 1

    def _ownership(self):
        """(ranges [world][2], factors [world] -> edge indices in ascending order); the ranges are all-gathered once."""
        if self._owners is not None:
            return self._owners
        rng, lmk = self._lmk_range, self._lmk_id
        shard = getattr(self.e, "shard", None)
        if rng is None and shard is not None:
            rng = (int(shard.lmk_begin), int(shard.lmk_end)) if hasattr(shard, "lmk_begin") else (int(shard[2]), int(shard[3]))
        problem = getattr(self.e, "problem", None)
        if lmk is None and problem is not None and int(problem.n_edges) > 0:
            lmk = np.ctypeslib.as_array(problem.lmk_id, shape=(int(problem.n_edges),)).astype(np.int64)
        if rng is None or lmk is None:
            raise ValueError("read(gather=True) needs to know who owns which entry: pass lmk_id= (the landmark of every factor) "
                             "and lmk_range= (this rank's landmark range) to ShardedGbp, or an engine that keeps `problem` and `shard`")
        torch = self.torch
        with self._on_stream():
            mine = torch.tensor(rng, dtype=torch.int64, device=self.send.device)
            allr = torch.zeros(2 * self.world, dtype=torch.int64, device=self.send.device)
            self.dist.all_gather_into_tensor(allr, mine)
        if self.stream is not None:
            self.stream.synchronize()
        ranges = [(int(a), int(b)) for a, b in allr.view(self.world, 2).cpu().numpy()]
        factors = [np.nonzero((lmk >= lo) & (lmk < hi))[0] for lo, hi in ranges]
        self._owners = (ranges, factors)
        return self._owners

    def _gather_owned(self, out, lmk_members, factor_members):
        """Fills the other ranks' entries of out[...] in place.  Every rank packs what it owns — the bit patterns, as int32 — into
        one buffer padded to the longest, ONE all-gather moves them, and the entries are COPIED to their places: a belief may be
        -0.0 or a NaN and arrives with its bits (a sum over zero-filled arrays would lose them)."""
        torch = self.torch
        ranges, factors = self._ownership()
        words = [sum(w for _, w in lmk_members) * (hi - lo) + len(factor_members) * len(f) for (lo, hi), f in zip(ranges, factors)]
        longest = max(words)
        if longest == 0:
            return
        bits = {k: out[k].view(np.int32) for k in [m for m, _ in lmk_members] + list(factor_members)}

        def pieces(r):      # (member, where its entries of rank r lie in the member's array), in the order they are packed
            lo, hi = ranges[r]
            return [(k, slice(w * lo, w * hi)) for k, w in lmk_members] + [(k, factors[r]) for k in factor_members]

        mine = np.zeros(longest, np.int32)
        at = 0
        for k, where in pieces(self.rank):
            part = bits[k][where]
            mine[at:at + part.size] = part
            at += part.size
        with self._on_stream():
            send = torch.from_numpy(mine).to(self.send.device)
            recv = torch.zeros(self.world * longest, dtype=torch.int32, device=self.send.device)
            self.dist.all_gather_into_tensor(recv, send)
        if self.stream is not None:
            self.stream.synchronize()
        recv = recv.view(self.world, longest).cpu().numpy()
        for r in range(self.world):
            if r == self.rank:
                continue
            at = 0
            for k, where in pieces(r):
                n = where.stop - where.start if isinstance(where, slice) else len(where)
                bits[k][where] = recv[r, at:at + n]
                at += n

    def eval(self):
        """Local shard sums, added over ranks (integers and fp64 partials; rank order fixed by all_gather)."""
        ev = self.e.eval()
        if self.dist is None or (self.world == 1 and not self.always_collective):
            return ev
        torch = self.torch
        keys = ["sum_norm", "sum_half_sq", "n_active", "n_relin", "n_robust", "n_nonfinite", "n_nonpd"]
        with self._on_stream():
            mine = torch.tensor([float(ev[k]) for k in keys], dtype=torch.float64, device=self.send.device)
            allv = torch.zeros(self.world * len(keys), dtype=torch.float64, device=self.send.device)
            self.dist.all_gather_into_tensor(allv, mine)
        if self.stream is not None:
            self.stream.synchronize()
        allv = allv.view(self.world, len(keys)).cpu().numpy()
        out = {}
        for j, k in enumerate(keys):
            acc = 0.0
            for r in range(self.world):
                acc = acc + float(allv[r, j])
            out[k] = acc if j < 2 else int(round(acc))
        return out

    def sync(self):
        if hasattr(self.e, "sync"):
            self.e.sync()
        if self.stream is not None:
            self.stream.synchronize()
