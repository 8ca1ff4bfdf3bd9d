"""A guarded, poisoned allocator for the buffers the Python layer hands to libgnca.so (test
infrastructure only; works on CPU tensors, so tests/test_poison_cpu.py tests it without a GPU).

Every workspace, output, tape and gradient buffer of the package comes from ``torch.empty`` /
``torch.empty_like``.  In a test process that memory is either fresh (zero) or a block the
caching allocator just took back from an identical call, which holds last time's correct data:
a kernel that reads a region before writing it, leaves part of an output unwritten or writes
past a buffer cannot fail a test that way.  ``Poison(fill)`` replaces the two attributes of the
``torch`` module while the call under test runs (the package's modules look them up at call
time) and hands out views into larger uint8 blocks instead::

    | guard: GUARD canary bytes (+ 0..255 to align) | body: the run's fill | pad to ALIGN | guard |

The body starts on an ALIGN (256 B) boundary, as the workspaces need; the padding up to the next
256 B is part of the trailing guard, so it is checked too.  The guards hold CANARY, which is no
fill.  ``check()`` asserts that every canary byte of every block is intact and names the block by
allocation order, shape and dtype.  ``guard(t)`` copies a test-made input into such a block whose
trailing slack holds the run's fill instead (a read past the input's end meets poison, not a
neighbour); ``check()`` also asserts that the slack and, unless ``inplace=True``, the input itself
are unchanged.

The fills: ``zero`` (the baseline), ``ones`` (0xFF: NaN as f32 / f64, -1 as int, all-ones masks and
alive bytes) and ``random`` (a seeded ``torch.Generator`` byte stream: arbitrary floats, counters
and masks).  ``run_fills`` runs one call under zero, zero, ones and random and asserts that the
named outputs are byte-identical (``same_bytes`` compares through an integer view, so a NaN or an
inf compares equal to itself): first the two zero runs, so that a difference between fills cannot
be confused with nondeterminism.

GUARD = 4096 B is a stated condition, not a measurement: wider than any quad, row or 256-B carve
slack the kernels use.
"""
from __future__ import annotations

import zlib

import torch

GUARD = 4096
ALIGN = 256
CANARY = 0xA5
FILLS = ("zero", "ones", "random")
RUNS = ("zero", "zero", "ones", "random")     # the runs of one case, in order

_EMPTY, _EMPTY_LIKE = torch.empty, torch.empty_like


def seed_of(case_id) -> int:
    """The random fill's seed of a case: a stable hash of its id."""
    return zlib.crc32(str(case_id).encode())


class _Block:
    __slots__ = ("order", "kind", "shape", "dtype", "block", "lead", "nbytes", "slack", "orig", "tensor")

    def name(self):
        return f"block #{self.order} ({self.kind}) shape={tuple(self.shape)} dtype={self.dtype}"


class Poison:
    """Context manager: ``with Poison("ones") as P: out = call(P.guard(x)); P.check()``."""

    def __init__(self, fill: str, seed: int = 0):
        if fill not in FILLS:
            raise ValueError(f"fill must be one of {FILLS}, got {fill!r}")
        self.fill, self.seed = fill, int(seed)
        self.blocks: list = []
        self._gens: dict = {}
        self._saved = None

    # ------------------------------------------------------------------------------ the patch
    def __enter__(self):
        if self._saved is not None:
            raise RuntimeError("Poison is not reentrant")
        self._saved = (torch.empty, torch.empty_like)
        torch.empty, torch.empty_like = self._empty, self._empty_like
        return self

    def __exit__(self, *exc):
        # (runs on an exception too: the with statement is the try / finally)
        torch.empty, torch.empty_like = self._saved
        self._saved = None
        return False

    def _empty(self, *size, dtype=None, device=None, requires_grad=False, layout=torch.strided,
               pin_memory=False, memory_format=torch.contiguous_format, out=None):
        if out is not None or layout is not torch.strided or pin_memory or \
                memory_format is not torch.contiguous_format:
            raise NotImplementedError("Poison: torch.empty with out= / layout / pin_memory / memory_format")
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        t = self.alloc(size, dtype or torch.get_default_dtype(), device)
        return t.requires_grad_() if requires_grad else t

    def _empty_like(self, t, *, dtype=None, device=None, requires_grad=False, layout=None,
                    pin_memory=False, memory_format=torch.preserve_format):
        if layout not in (None, torch.strided) or pin_memory:
            raise NotImplementedError("Poison: torch.empty_like with layout / pin_memory")
        if memory_format is torch.preserve_format and not t.is_contiguous():
            raise NotImplementedError("Poison: torch.empty_like of a non-contiguous tensor")
        r = self.alloc(t.shape, dtype or t.dtype, t.device if device is None else device)
        return r.requires_grad_() if requires_grad else r

    # -------------------------------------------------------------------------------- blocks
    def _bytes(self, n: int, device) -> torch.Tensor:
        """``n`` bytes of the run's fill on ``device``."""
        if self.fill == "zero":
            return torch.zeros(n, dtype=torch.uint8, device=device)
        if self.fill == "ones":
            return torch.full((n,), 0xFF, dtype=torch.uint8, device=device)
        g = self._gens.get(device)
        if g is None:
            g = self._gens[device] = torch.Generator(device=device).manual_seed(self.seed)
        return torch.randint(0, 256, (n,), dtype=torch.uint8, device=device, generator=g)

    def _block(self, kind, shape, dtype, device, slack_fill: bool) -> _Block:
        device = torch.device("cpu" if device is None else device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        shape = torch.Size(int(s) for s in shape)
        nbytes = shape.numel() * _EMPTY(0, dtype=dtype).element_size()
        body = -(-nbytes // ALIGN) * ALIGN
        block = torch.full((GUARD + ALIGN + body + GUARD,), CANARY, dtype=torch.uint8, device=device)
        lead = GUARD + (-(block.data_ptr() + GUARD)) % ALIGN
        assert lead % 8 == 0, "the allocator's block is not 8-byte aligned"
        b = _Block()
        b.order, b.kind, b.shape, b.dtype = len(self.blocks), kind, shape, dtype
        b.block, b.lead, b.nbytes = block, lead, nbytes
        b.slack = b.orig = None
        if nbytes:
            block[lead:lead + nbytes] = self._bytes(nbytes, device)
        if slack_fill:
            tail = block[lead + nbytes:]
            tail.copy_(self._bytes(tail.numel(), device))
            b.slack = tail.clone()
        b.tensor = block[lead:lead + nbytes].view(dtype).view(shape)
        assert b.tensor.data_ptr() % ALIGN == 0 or nbytes == 0
        self.blocks.append(b)
        return b

    def alloc(self, shape, dtype, device=None) -> torch.Tensor:
        """What the patched ``torch.empty`` returns: a poisoned body between two canary guards."""
        return self._block("empty", shape, dtype, device, slack_fill=False).tensor

    def guard(self, t, inplace: bool = False):
        """A copy of the input ``t`` (None passes through) in a block of its own: a canary guard in
        front, the run's fill behind.  ``inplace``: the call under test may write the tensor."""
        if t is None:
            return None
        t = t.detach()
        b = self._block("input", t.shape, t.dtype, t.device, slack_fill=True)
        b.tensor.copy_(t)
        if not inplace:
            b.orig = t.clone()
        return b.tensor

    def check(self) -> None:
        """Every canary byte of every block is intact (and every guarded input and its slack)."""
        for b in self.blocks:
            front, tail = b.block[:b.lead], b.block[b.lead + b.nbytes:]
            bad = int((front != CANARY).sum())
            assert bad == 0, f"{b.name()}: {bad} canary byte(s) overwritten BEFORE the buffer ({self.fill} fill)"
            if b.slack is None:
                bad = (tail != CANARY).nonzero()
                assert bad.numel() == 0, (f"{b.name()}: {bad.numel()} canary byte(s) overwritten AFTER the buffer, "
                                          f"the first {int(bad[0])} B past its end ({self.fill} fill)")
            else:
                assert torch.equal(tail, b.slack), f"{b.name()}: the slack behind the input was written"
                if b.orig is not None:
                    assert same_bytes(b.tensor, b.orig), f"{b.name()}: the input was written"


def same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Shape, dtype and every byte equal (an integer view: NaN == NaN, +inf == +inf, -0 != +0)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    va = a.detach().contiguous().reshape(-1).view(torch.uint8)
    vb = b.detach().contiguous().reshape(-1).view(torch.uint8)
    return bool(torch.equal(va, vb.to(va.device)))


def diff(a: torch.Tensor, b: torch.Tensor) -> str:
    """A short description of where two tensors of one shape differ bytewise."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"{tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    n = a.element_size()
    va = a.detach().contiguous().reshape(-1).view(torch.uint8).reshape(-1, n)
    vb = b.detach().contiguous().reshape(-1).view(torch.uint8).reshape(-1, n).to(va.device)
    bad = (va != vb).any(dim=1).nonzero().reshape(-1)
    if bad.numel() == 0:
        return "equal"
    i = int(bad[0])
    return (f"{bad.numel()} of {va.shape[0]} elements differ, first at flat index {i}: "
            f"{a.detach().contiguous().reshape(-1)[i].item()!r} vs {b.detach().contiguous().reshape(-1)[i].item()!r}")


def _sync(outs: dict) -> None:
    if any(t.is_cuda for t in outs.values()):
        torch.cuda.synchronize()


def run_fills(call, case_id, runs=RUNS) -> dict:
    """Run ``call(P)`` once per entry of ``runs`` under ``Poison(fill, seed_of(case_id))``.  ``call``
    passes its inputs through ``P.guard`` and returns ``{name: tensor}`` of its DEFINED outputs.
    Asserts after every run that no canary was touched, then that the outputs of all runs are
    byte-identical to the first's (the second zero run first).  Returns the outputs of the last
    ``ones`` run (or of the last run), cloned."""
    got = []
    for fill in runs:
        with Poison(fill, seed_of(case_id)) as P:
            outs = call(P)
            _sync(outs)
        P.check()
        got.append((fill, {k: v.detach().clone() for k, v in outs.items()}))
        del P, outs
    f0, base = got[0]
    bad = []
    for i, (fill, outs) in enumerate(got[1:], 1):
        assert list(outs) == list(base), (case_id, list(outs), list(base))
        for k in base:
            if same_bytes(base[k], outs[k]):
                continue
            if fill == f0:      # stop here: a difference between fills would mean nothing
                raise AssertionError(f"{case_id}: output '{k}' is nondeterministic: two runs of the {f0} fill "
                                     f"differ (run {i}): {diff(base[k], outs[k])}")
            bad.append(f"output '{k}' depends on the buffers' prior contents: {f0} fill vs {fill} fill "
                       f"(run {i}): {diff(base[k], outs[k])}")
    assert not bad, f"{case_id}: " + "; ".join(bad)
    pick = [o for f, o in got if f == "ones"]
    return pick[-1] if pick else got[-1][1]
