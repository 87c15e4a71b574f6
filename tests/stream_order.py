"""Inputs still in production on the caller's stream: the harness of
test_gpu_stream_order.py.

Test helper (a plain module, imported like block_paths.py).  The suite's other
tests hand the library inputs that were finished and synchronised long before
the call, on the default stream, and read the outputs after a device-wide
synchronise: a step that runs on the wrong stream, or skips an event wait
between the caller's stream and an internal one, passes all of them.  Here
every input sits *behind a delay on the caller's own, non-default stream*:

    S = fresh_stream(gpu)                   a fresh torch.cuda.Stream, not ordered against
                                            stream 0 and on a hardware queue apart from its
    x = decoy                               allocated and filled under S
    hold(S, H)                              a device-side delay of H ms on S
    x = real                                queued behind it (a copy kernel)
    out.fill_(0xEE)                         a caller-supplied output, behind it too
    result = call(x, out, stream=S)         the entry point under test
    snap = result.clone()                   on S
    x = decoy                               on S: the write-after-read probe
    S.synchronize(); snap == reference(real)

A launch that does not wait for S reads the decoy -- a valid input of the same
length with another answer, so an early read is a wrong result, never an error
path -- or has its early result overwritten by the 0xEE fill; a read that is
not finished in S's order sees the decoy come back.  H is not chosen in
advance: the test module times every scenario's call on the idle device and
holds for ten times the longest (at least 5 ms), so that a call on the wrong
stream finishes entirely inside the hold.
"""
import time

import numpy as np
import torch

PREFILL = 0xEE
MIN_HOLD_MS = 5.0
HOLD_FACTOR = 10.0
_PROBE_CYCLES = 2_000_000
_MARGIN = 1.25  # the probe's own launch is part of its time; the hold must not come out short
_PIECES = 16

_holds = {}
shortest_hold = [float("inf")]  # measured / asked, over the holds that settle() checked

_cycles_per_ms = {}


def cycles_per_ms(device) -> float:
    """How many cycles of torch.cuda._sleep's counter make one millisecond on
    `device`: one _sleep timed with two events, once per process (after one
    short _sleep that loads the kernel).  No clock rate is assumed."""
    key = torch.device(device).index or 0
    if key not in _cycles_per_ms:
        with torch.cuda.device(key):
            torch.cuda._sleep(1000)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(_PROBE_CYCLES)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
        assert ms > 0
        _cycles_per_ms[key] = _PROBE_CYCLES / ms
    return _cycles_per_ms[key]


def hold(stream, ms: float) -> None:
    """A device-side delay of at least `ms` milliseconds queued on `stream`
    (nothing is allocated), between two events that `held_ms` reads.

    The delay is a row of short _sleep kernels, half as many again as `ms`
    needs.  One long one can end early: a spinning wave that is switched out
    and in again -- a first allocation from a memory pool during the hold does
    that -- came back with its _sleep over after 6 of 87 ms.  A short one
    loses its own few ms at the most."""
    piece = ms / _PIECES
    cycles = int(piece * cycles_per_ms(stream.device) * _MARGIN) + 1
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        start.record()
        for _ in range(_PIECES + _PIECES // 2):
            torch.cuda._sleep(cycles)
        end.record()
    _holds[stream.cuda_stream] = (start, end, ms)


def held_ms(stream):
    """(measured, asked) milliseconds of the last hold on `stream`, which has
    run past it."""
    start, end, ms = _holds[stream.cuda_stream]
    return start.elapsed_time(end), ms


def runs_beside(held, other) -> bool:
    """Whether work queued on `other` runs while `held` is busy.  The runtime
    spreads its streams over a few hardware queues, and two streams that share
    one run in the order of submission: a launch on `other` would then wait
    for a hold on `held`, and a misplaced launch would look ordered."""
    hold(held, 2.0)
    with torch.cuda.stream(other):
        torch.cuda._sleep(1)
        done = torch.cuda.Event()
        done.record()
    done.synchronize()
    beside = not held.query()
    held.synchronize()
    return beside


def fresh_stream(device, apart_from=None, beside=None):
    """A fresh torch.cuda.Stream(device) that shares its hardware queue with
    none of `apart_from` (default: the device's default stream), so that
    holding it holds nothing else back.  `beside`, if given, is a call that
    must also get through while the stream is held: one that keeps the
    library's internal streams busy, which a test cannot name."""
    others = list(apart_from) if apart_from is not None else [torch.cuda.default_stream(device)]
    for _ in range(64):
        s = torch.cuda.Stream(device)
        with torch.cuda.stream(s):  # the stream's share of the caching allocator's pools exists before any hold
            for n in (1, 2 << 20):
                torch.empty(n, dtype=torch.uint8, device=device)
        if not all(runs_beside(s, o) for o in others):
            continue
        if beside is not None:
            hold(s, 20.0)
            beside()
            got_through = not s.query()
            s.synchronize()
            if not got_through:
                continue
        return s
    raise RuntimeError("no stream runs beside the others: the hold would prove nothing")


def hold_ms(longest_call_ms: float) -> float:
    return max(MIN_HOLD_MS, HOLD_FACTOR * longest_call_ms)


def shifted(n: int, dtype, shift: int, device) -> torch.Tensor:
    """n elements of `dtype`, uninitialised, the first `shift` bytes past a
    16-byte boundary.  Allocated on the current stream."""
    size = torch.empty(0, dtype=dtype).element_size()
    assert shift % size == 0
    raw = torch.empty(n * size + 32, dtype=torch.uint8, device=device)
    lead = (shift - raw.data_ptr()) % 16
    return raw[lead:lead + n * size].view(dtype)


def kernel_copy(dst: torch.Tensor, src: torch.Tensor) -> None:
    """dst = src by an elementwise kernel on the current stream, not
    dst.copy_(src): that is a DMA copy, and one that waits behind a hold keeps
    the copy engine's queue waiting with it -- the library's own DMA copies on
    its internal streams then line up behind it and look ordered after the
    caller's stream when nothing orders them (write_to_fd given the wrong
    stream wrote the real bytes, or half of them, in one run out of three)."""
    torch.bitwise_or(src, src, out=dst)


def pending(stream, real: dict, decoy: dict, H: float, shift=None, out=None):
    """The scenario's inputs, still in production on `stream`.

    `real` and `decoy` map names to device tensors of the same shapes,
    prepared and synchronised by the caller.  Every input is allocated under
    `stream` (`shift[name]` bytes past a 16-byte boundary, default 0) and
    holds the decoy; then the hold, then the copies of the real contents and
    the PREFILL of the caller-supplied outputs `out` = {name: (shape, dtype)}
    -- also allocated under `stream` -- are queued behind it.  Returns
    (inputs, outputs)."""
    shift, out = shift or {}, out or {}
    with torch.cuda.stream(stream):
        x = {}
        for name, d in decoy.items():
            assert real[name].shape == d.shape and real[name].dtype == d.dtype, name
            x[name] = shifted(d.numel(), d.dtype, shift.get(name, 0), d.device).view(d.shape)
            kernel_copy(x[name], d)
        o = {name: torch.empty(shape, dtype=dtype, device=stream.device) for name, (shape, dtype) in out.items()}
        stream.synchronize()  # the decoy is there before anything can read it
        hold(stream, H)
        for name, r in real.items():
            kernel_copy(x[name], r)
        for t in o.values():
            t.view(torch.uint8).fill_(PREFILL)
    return x, o


def _plain(t: torch.Tensor) -> torch.Tensor:
    """uint32 results (sizes) as int32: results are compared by their bytes."""
    return t.view(torch.int32) if t.dtype == torch.uint32 else t


def settle(stream, x: dict, decoy: dict, result):
    """After the call, on `stream`: every tensor of `result` (a tuple of
    tensors and plain values) cloned, then every input overwritten with its
    decoy again (a read of the call's that is not finished in the stream's
    order sees it), then the stream synchronised and the hold's length
    checked.  Returns the result with numpy arrays in place of the tensors."""
    with torch.cuda.stream(stream):
        snap = [_plain(r).clone() if isinstance(r, torch.Tensor) else r for r in result]
        for name, d in decoy.items():
            kernel_copy(x[name], d)
    stream.synchronize()
    measured, asked = held_ms(stream)
    shortest_hold[0] = min(shortest_hold[0], measured / asked)
    assert measured >= asked, f"the hold lasted {measured:.1f} of {asked:.1f} ms: this run proves nothing"
    return tuple(s.cpu().numpy() if isinstance(s, torch.Tensor) else s for s in snap)


def same(got, want) -> bool:
    """Two results of settle's form, exactly equal (tensors by bytes)."""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if isinstance(g, np.ndarray) or isinstance(w, np.ndarray):
            g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
            if g.shape != w.shape or g.dtype.itemsize != w.dtype.itemsize or g.tobytes() != w.tobytes():
                return False
        elif g != w:
            return False
    return True


def first_difference(got, want):
    """Which element of two results differs, for an assertion's message."""
    for i, (g, w) in enumerate(zip(got, want)):
        if not same((g,), (w,)):
            if isinstance(g, np.ndarray) and isinstance(w, np.ndarray) and g.shape == w.shape:
                bad = np.flatnonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8))
                return i, bad[:8].tolist(), g.reshape(-1).view(np.uint8)[bad[:8]].tolist()
            return i, g if not isinstance(g, np.ndarray) else g.shape, w if not isinstance(w, np.ndarray) else w.shape
    return None if len(got) == len(want) else ("length", len(got), len(want))


def timed_ms(call, device) -> float:
    """Host wall clock around one call and a synchronise, on the idle device."""
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) * 1e3
