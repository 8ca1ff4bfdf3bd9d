"""Device-resident sample pool, the caller-side data format of the path.

Mirror of the reference's ``SamplePool`` (``src/training/pool.py:5-42``) with the same
constructor, ``sample`` and ``replace`` (same argument meaning and the same Python ``random``
consumption), but the pool is ONE contiguous ``[P, C, H, W]`` device tensor instead of a list of
P separate tensors: ``sample`` is one ``index_select`` (the reference stacks B clones) and
``replace`` one ``index_copy_`` (the reference assigns B clones one by one).  On a 288 GB MI355X the
whole C4 pool (1024 x 16 x 72 x 72 fp32 = 340 MB) stays resident.

Multi-GPU (``shard=(rank, world)``): each rank keeps only its contiguous slice of the pool
(``sharding.shard_range``) and samples its share of the batch from it.  Every rank still calls
``seed_fn`` for all P samples, so the global RNG streams stay identical across ranks.  A sharded
pool draws its slot indices from its own ``random.Random``, not from the global stream: slices may
differ in length by one, and ``random.sample`` over different lengths consumes the stream
differently, which would desynchronise the per-step offset draws that every rank must share
(``sharding.py``).  That private stream is seeded from the global stream's STATE at construction
(read, not consumed: identical on every rank, and it follows the user's ``random.seed``) mixed
with the rank; ``rng_state()`` / ``set_rng_state()`` carry it through a checkpoint: every rank
calls ``checkpoint.pool_rng_states(pool)`` (collective over the pool's world), rank 0 saves the
result with ``save_checkpoint(..., pool_states=)``, and ``load_checkpoint(..., pool=)`` on each rank
restores that rank's own stream (``save_checkpoint(..., pool=)`` stores only the calling rank's).
"""
from __future__ import annotations

import ctypes
import hashlib
import random

import torch

from .sharding import shard_range


class SamplePool:
    def __init__(self, pool_size, seed_fn, device="cpu", *, shard: tuple[int, int] | None = None):
        """``seed_fn(batch_size=1)`` returns one seed state ([1,C,H,W] or [C,H,W]), called once per
        pool slot exactly as the reference does (pool.py:18)."""
        self.pool_size = int(pool_size)
        rank, world = shard if shard is not None else (0, 1)
        self.rank, self.world = int(rank), int(world)
        self.lo, self.hi = shard_range(self.pool_size, rank, world)
        seeds = []
        for i in range(self.pool_size):
            s = seed_fn(batch_size=1)
            if i >= self.lo and i < self.hi:
                seeds.append(s.reshape(s.shape[-3:]).to(device))
        self.states = torch.stack(seeds).contiguous() if seeds else torch.empty(0, device=device)
        # unsharded: the global stream, exactly as the reference; sharded: a private stream
        if world == 1:
            self._rng = random
        else:
            digest = hashlib.sha256(repr(random.getstate()).encode()).digest()
            self._rng = random.Random(int.from_bytes(digest[:8], "little") * 1_000_003 + rank * 1009 + world)
        self._last = None   # (idx list of the last sample(), its contents, its device tensor): commit reuses it

    def __len__(self):
        return self.states.shape[0]

    @property
    def pool(self):
        """The slots as a list of [C,H,W] views (the reference's attribute, for reading)."""
        return list(self.states.unbind(0))

    def sample(self, batch_size):
        """(idx, batch): ``random.sample`` over this pool's slots (pool.py:23-32) and a fresh
        [B,C,H,W] tensor (a copy: the pool is not modified through it)."""
        idx = self._rng.sample(range(len(self)), batch_size)
        sel = torch.as_tensor(idx, dtype=torch.long, device=self.states.device)
        self._last = (idx, list(idx), sel)
        return idx, self.states.index_select(0, sel)

    def rng_state(self):
        """The private slot-index stream's state (a sharded pool), else None (the global stream is
        the caller's to save).  JSON/torch.save-friendly (nested lists)."""
        if self._rng is random:
            return None
        v, st, g = self._rng.getstate()
        return [v, list(st), g]

    def set_rng_state(self, state):
        if state is not None and self._rng is not random:
            v, st, g = state
            self._rng.setstate((int(v), tuple(int(t) for t in st), g))

    def replace(self, idx, new_samples):
        """Write ``new_samples`` (detached) into slots ``idx`` (pool.py:34-42)."""
        sel = torch.as_tensor(list(idx), dtype=torch.long, device=self.states.device)
        self.states.index_copy_(0, sel, new_samples.detach().to(self.states.dtype))

    def _slots(self, idx):
        """``idx`` as an int64 tensor on the pool's device, without a blocking copy: the tensor
        ``sample`` made for this very list, else a pinned staging copy."""
        last = self._last
        if last is not None and last[0] is idx and last[1] == idx:   # (the same list, unmodified)
            return last[2]
        dev = self.states.device
        sel = torch.tensor(idx, dtype=torch.long)
        if dev.type != "cuda":
            return sel.to(dev)
        return sel.pin_memory().to(dev, non_blocking=True)

    def commit(self, idx, state, per_sample=None, *, n_reset=0, seed_fn=None, reseed=False):
        """The trainers' whole write-back (train_graph_augmented_nca.py:377-391,
        train_intermediate_loss.py:269-296): ``state`` (detached) goes back into slots ``idx``, except
        that the ``n_reset`` samples with the largest ``per_sample`` get fresh seeds and, with
        ``reseed``, one random sample gets one.  On a ROCm pool that is ONE launch
        (``gnca_pool_commit``): no ``topk``, no clone of the batch and no host wait.

        The draws are the reference's, in its order, so the torch RNG stream is consumed identically:

        1. ``reseed``: ``rand_idx = torch.randint(0, B, (1,), device=...)``, which stays on the device;
        2. ``n_reset > 0``: ``seeds = seed_fn(n_reset)``;
        3. ``reseed``: ``seed1 = seed_fn(1)``;
        4. slot ``idx[b]`` receives ``seed1`` where ``b == rand_idx`` (applied last: it wins over a
           worst-reset), else ``seeds[r]`` where the sample's descending loss rank ``r < n_reset``
           (rank 0 is the worst, ``torch.topk``'s order), else ``state[b]``.

        The caller draws ``random.random() < random_reseed_prob`` itself and passes ``reseed``: the two
        trainers draw it at different points of the iteration.

        Ordering: a NaN loss ranks above every number, as in ``torch.topk``.  Equal losses rank by lower
        batch index first; torch leaves ties unspecified, so that is this package's definition, not a
        parity claim.  ``idx`` must hold distinct slots (``random.sample`` guarantees it).  A pool that
        is not on a ROCm device does the same with torch ops."""
        idx_list = idx if isinstance(idx, list) else list(idx)
        B = len(idx_list)
        n_reset = int(n_reset)
        if not isinstance(state, torch.Tensor) or tuple(state.shape) != (B,) + tuple(self.states.shape[1:]):
            raise ValueError(f"state must be [{B}, {', '.join(map(str, self.states.shape[1:]))}] for {B} slots, "
                             f"got {tuple(state.shape) if isinstance(state, torch.Tensor) else type(state)}")
        if B == 0:
            raise ValueError("idx is empty")
        if n_reset < 0 or n_reset > B:
            raise ValueError(f"n_reset must be in 0 .. {B}, got {n_reset}")
        if (n_reset > 0 or reseed) and seed_fn is None:
            raise ValueError("n_reset > 0 and reseed need seed_fn")
        if n_reset > 0 and (not isinstance(per_sample, torch.Tensor) or tuple(per_sample.shape) != (B,)):
            raise ValueError(f"n_reset > 0 needs per_sample of shape ({B},)")
        if any(i < 0 or i >= len(self) for i in idx_list) or len(set(idx_list)) != B:
            raise ValueError("idx must hold distinct slots of this pool")
        dev, dtype = self.states.device, self.states.dtype
        shape = tuple(self.states.shape[1:])

        def seeds_of(n):
            s = seed_fn(n).detach()
            if s.numel() != n * self.states[0].numel():
                raise ValueError(f"seed_fn({n}) returned {tuple(s.shape)}, expected [{n}, ...] of {shape}")
            return s.reshape((n,) + shape).to(dev, dtype, non_blocking=True).contiguous()

        rand_idx = torch.randint(0, B, (1,), device=dev) if reseed else None
        seeds = seeds_of(n_reset) if n_reset > 0 else None
        seed1 = seeds_of(1) if reseed else None
        state = state.detach().to(dev, dtype).contiguous()
        per = per_sample.detach().to(dev, torch.float32).contiguous() if n_reset > 0 else None
        sel = self._slots(idx_list)
        if dev.type != "cuda" or dtype != torch.float32:
            return self._commit_torch(sel, state, per, seeds, seed1, rand_idx, n_reset)
        from . import _lib as L
        from .step import stream_ptr
        fn = getattr(L.load(), "gnca_pool_commit", None)
        if fn is None:
            raise L.GncaError(f"libgnca.so at {L.LIB_PATH} has no gnca_pool_commit; rebuild it")
        d = L.PoolCommitDesc()
        d.pool_slots, d.sample_elems, d.B, d.n_reset = len(self), self.states[0].numel(), B, n_reset
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        L.check(fn(ctypes.byref(d), self.states.data_ptr(), sel.data_ptr(), state.data_ptr(), ptr(per), ptr(seeds),
                   ptr(seed1), ptr(rand_idx), stream_ptr(dev)), "gnca_pool_commit")

    def _commit_torch(self, sel, state, per, seeds, seed1, rand_idx, n_reset):
        """``commit`` with torch ops (a pool that is not on a ROCm device): the same ranks and sources."""
        B = state.shape[0]
        src = state
        if n_reset > 0 or rand_idx is not None:
            src = state.clone()
        if n_reset > 0:
            # (torch.sort orders a NaN above every number; stable: ties by lower index)
            order = torch.sort(per, descending=True, stable=True).indices
            src[order[:n_reset]] = seeds
        if rand_idx is not None:
            src.index_copy_(0, rand_idx.reshape(1), seed1)
        self.states.index_copy_(0, sel, src)
