"""Where and when a call runs: side streams, delayed inputs, graph capture (test infrastructure only).

include/gnca.h promises that every entry point's work is stream-ordered on the caller's stream, that
no entry point synchronises the device, allocates or copies host<->device, and that a call can be
captured into a hipGraph.  On the null stream none of that can fail a test.  A ``Case`` is one library
call (or a short chain of calls) from NAMED DEVICE INPUTS to named outputs::

    Case(case_id, (inputs_1, inputs_2), call)         # inputs_n: {name: device tensor}
    call(bufs) -> {name: tensor}                      # bufs: {name: tensor} shaped like the inputs

Every host-side value (descriptor, offsets, schedule) is fixed in ``call``; the two input sets have the
same shapes and dtypes and different device data.  ``call`` reads its inputs from ``bufs`` ONLY (it may
write a buffer in place and return it as an output: loading a set restores it) and uploads nothing.

``run(case)`` runs three legs:

* **eager**: the call on the default stream for set #1 and set #2; the cloned outputs are the expected
  values, and the call's duration is measured with events (the warm second run).
* **side stream, delayed inputs**: the buffers hold 0xFF bytes (NaN as a float, -1 as an int).  On a
  fresh ``torch.cuda.Stream()``, with no host synchronisation in between: a delay of at least
  ``max(10 x eager duration, 5 ms)`` (asserted from events around it), the copy of the real inputs into
  the buffers, the call, the clone of its outputs, the buffers poisoned again.  Then THAT stream alone
  is synchronised.  A launch that is not ordered after the copy reads poison, one that is not ordered
  before the clone is missing from it: the outputs must be bitwise the eager ones.  Run for both sets.
* **capture and replay**: after the side-stream leg, which created the lazy helper streams, events and
  function attributes.  ``torch.cuda.graph(g, stream=s)`` (``capture_error_mode="global"``) around the
  call while the buffers hold poison; then set #2 is loaded and the graph replayed, then set #1: each
  replay's outputs must be bitwise the eager ones.  Work that ran eagerly while capturing, or a value
  baked into the graph, leaves at least one of the two replays wrong.

A library status other than GNCA_OK or a capture error propagates as the exception it is: a failure.
"""
from __future__ import annotations

import torch

from tests.poison import diff, same_bytes

MIN_DELAY_MS = 5.0
DELAY_FACTOR = 10.0
LEGS = ("eager", "side", "capture")

_CYCLES_PER_MS = None


class Case:
    """One call with its two input sets; ``eager`` caches the expected outputs and the duration."""

    def __init__(self, case_id, sets, call):
        s1, s2 = sets
        assert list(s1) == list(s2), (case_id, list(s1), list(s2))
        for k in s1:
            a, b = s1[k], s2[k]
            assert a.is_cuda and a.is_contiguous() and b.is_contiguous(), (case_id, k)
            assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device, (case_id, k)
        self.id, self.sets, self.call = case_id, (s1, s2), call
        self.bufs = {k: torch.empty_like(v) for k, v in s1.items()}
        self.device = next(iter(s1.values())).device if s1 else torch.device("cuda", torch.cuda.current_device())
        self.eager = None       # ([outputs of set #1, outputs of set #2], milliseconds)

    def load(self, n: int) -> None:
        """Copy input set ``n`` (0 or 1) into the buffers, on the current stream."""
        for k, v in self.sets[n].items():
            self.bufs[k].copy_(v, non_blocking=True)

    def poison(self) -> None:
        for v in self.bufs.values():
            _fill_ff(v)


def _fill_ff(t: torch.Tensor) -> None:
    if t.numel():
        t.view(-1).view(torch.uint8).fill_(0xFF)


def _clone(outs: dict) -> dict:
    assert isinstance(outs, dict) and outs, "the call returns {name: tensor} of its defined outputs"
    return {k: v.detach().clone() for k, v in outs.items()}


def _compare(case, leg, n, got, want) -> None:
    assert list(got) == list(want), (case.id, leg, list(got), list(want))
    bad = [f"output '{k}': {diff(want[k], got[k])}" for k in want if not same_bytes(want[k], got[k])]
    assert not bad, f"{case.id}: the {leg} differs from the eager call on input set #{n + 1}: " + "; ".join(bad)


# -------------------------------------------------------------------------------------------------
# The delay
# -------------------------------------------------------------------------------------------------
def _cycles_per_ms() -> float:
    """``torch.cuda._sleep`` cycles per millisecond, measured once per process."""
    global _CYCLES_PER_MS
    if _CYCLES_PER_MS is None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)                  # (loads the kernel)
        best = None
        for n in (1_000_000, 4_000_000):
            torch.cuda.synchronize()
            e0.record()
            torch.cuda._sleep(n)
            e1.record()
            torch.cuda.synchronize()
            best = n / max(e0.elapsed_time(e1), 1e-3)
        _CYCLES_PER_MS = best
    return _CYCLES_PER_MS


_BUSY = {}


def delay(ms: float) -> None:
    """Keep the current stream busy for about ``ms`` milliseconds (sized with a margin; the caller
    asserts the real figure from events): ``torch.cuda._sleep``, else a chain of large matmuls."""
    if hasattr(torch.cuda, "_sleep"):
        cycles = int(1.5 * ms * _cycles_per_ms()) + 1
        while cycles > 0:                        # (in pieces that fit an int32 argument)
            torch.cuda._sleep(min(cycles, 1 << 30))
            cycles -= 1 << 30
        return
    a, out, one = _busy()
    for _ in range(int(1.5 * ms / one) + 1):
        torch.mm(a, a, out=out)


def _busy():
    dev = torch.cuda.current_device()
    if dev not in _BUSY:
        a = torch.randn(4096, 4096, device="cuda")
        out = torch.empty_like(a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.mm(a, a, out=out)
        torch.cuda.synchronize()
        e0.record()
        torch.mm(a, a, out=out)
        e1.record()
        torch.cuda.synchronize()
        _BUSY[dev] = (a, out, max(e0.elapsed_time(e1), 1e-3))
    return _BUSY[dev]


def prepare_delay() -> None:
    """Calibrate the delay on the current device (it synchronises: not inside a leg)."""
    if hasattr(torch.cuda, "_sleep"):
        _cycles_per_ms()
    else:
        _busy()


def delay_ms(eager_ms: float) -> float:
    return max(DELAY_FACTOR * eager_ms, MIN_DELAY_MS)


# -------------------------------------------------------------------------------------------------
# The legs
# -------------------------------------------------------------------------------------------------
def run_eager(case: Case):
    """Both input sets on the default stream: ``case.eager`` = (expected outputs, milliseconds)."""
    if case.eager is not None:
        return case.eager
    with torch.cuda.device(case.device):
        assert torch.cuda.current_stream().cuda_stream == 0, "the eager leg runs on the default stream"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        want, ms = [], 0.0
        for n in (0, 1):
            case.load(n)
            torch.cuda.synchronize()
            e0.record()
            outs = case.call(case.bufs)
            e1.record()
            torch.cuda.synchronize()
            want.append(_clone(outs))
            ms = e0.elapsed_time(e1)         # the second, warm run's is kept
            del outs
        case.poison()
        torch.cuda.synchronize()
    case.eager = (want, ms)
    return case.eager


def run_side(case: Case) -> None:
    """The side-stream leg, for both sets (module docstring)."""
    want, ms = run_eager(case)
    need = delay_ms(ms)
    with torch.cuda.device(case.device):
        prepare_delay()
        for n in (0, 1):
            case.poison()
            torch.cuda.synchronize()
            s = torch.cuda.Stream()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record()
                delay(need)
                e1.record()
                case.load(n)
                outs = case.call(case.bufs)
                got = _clone(outs)
                case.poison()
            s.synchronize()                  # this stream only
            slept = e0.elapsed_time(e1)
            assert slept >= need, (f"{case.id}: the delay took {slept:.2f} ms, the leg needs {need:.2f} ms "
                                   f"(eager call: {ms:.3f} ms)")
            _compare(case, "side-stream leg", n, got, want[n])
            del outs, got
            torch.cuda.synchronize()


def run_capture(case: Case) -> None:
    """Capture on a side stream with poisoned inputs, then replay set #2 and set #1."""
    want, _ = run_eager(case)
    with torch.cuda.device(case.device):
        case.poison()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            outs = case.call(case.bufs)
        assert isinstance(outs, dict) and outs
        torch.cuda.synchronize()
        for n in (1, 0):
            for k, v in outs.items():        # (an output that is an input buffer is loaded next)
                _fill_ff(v.detach())
            case.load(n)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            _compare(case, "replay of the captured call", n, outs, want[n])
        del g, outs
        case.poison()
        torch.cuda.synchronize()


def run(case: Case, legs=LEGS) -> None:
    assert set(legs) <= set(LEGS) and "eager" in legs, legs
    run_eager(case)
    if "side" in legs:
        run_side(case)
    if "capture" in legs:
        run_capture(case)
