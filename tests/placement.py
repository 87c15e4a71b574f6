"""Outputs among guard bytes: the harness of test_gpu_written_extent.py.

Test helper (a plain module, imported like stream_order.py).  The suite's other
tests give the library fresh torch allocations as outputs -- 256-byte aligned
and rounded up to 512 bytes, so a row written past `cap`, or a store that
spills over the end of a table, lands in slack nobody reads.  Here every
output of a call is carved from ONE uint8 allocation filled with a pattern:

    a = Arena(gpu, 0xA5)
    dig = a.carve("digests", 20 * cap, torch.uint8, phase=4)    # 4 bytes past a 256-byte boundary
    weak = a.carve("weak", 4 * cap, torch.int32, phase=12)
    a.watch(data=data)                                          # inputs: copied to the host now
    rc = lib().sf_index_device_fixed_weak(..., dig.data_ptr(), weak.data_ptr(), ...)
    a.check({"digests": want_digests, "weak": want_weak})

`check` brings the WHOLE allocation back once and compares it with a host
image: the pattern everywhere, and in each output the bytes the host reference
gives for the rows the call may write (`None`, or an output not named: it may
write none).  So a row past the written ones, a byte of the guards (at least
64 before, between and after the outputs) and every byte the test does not
name must still hold the pattern; the watched inputs must be what they were.
Each scenario runs under two patterns, 0xA5 and 0x5A: a stray store that
happens to write one of them is caught under the other.
"""
import numpy as np
import torch

GUARD = 64
PATTERNS = (0xA5, 0x5A)
ALIGN = 256  # phases count from such a boundary (a device allocation's own alignment)


def as_bytes(a) -> np.ndarray:
    """The bytes of an expected value: a numpy array of any dtype, or bytes."""
    if isinstance(a, (bytes, bytearray)):
        return np.frombuffer(bytes(a), np.uint8)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Arena:
    def __init__(self, device, pattern: int, capacity: int = 1 << 16):
        assert capacity % ALIGN == 0
        self.pattern = pattern
        self.buf = torch.full((capacity,), pattern, dtype=torch.uint8, device=device)
        assert self.buf.data_ptr() % ALIGN == 0
        self.carved = []  # (name, offset, nbytes), in address order
        self.inputs = {}  # name -> (device tensor, host copy)
        self._end = 0     # end of the last output

    def carve(self, name: str, nbytes: int, dtype, phase: int) -> torch.Tensor:
        """`nbytes` of the arena as a contiguous 1-D view of `dtype`, starting
        `phase` bytes past a 256-byte boundary and at least GUARD bytes after
        the output before it (or the arena's start)."""
        size = torch.empty(0, dtype=dtype).element_size()
        assert 0 <= phase < ALIGN and phase % size == 0 and nbytes % size == 0, (name, phase, nbytes, size)
        assert all(name != c[0] for c in self.carved), name
        at = -(-(self._end + GUARD) // ALIGN) * ALIGN + phase
        assert at + nbytes + GUARD <= self.buf.numel(), f"arena too small for {name}"
        self.carved.append((name, at, nbytes))
        self._end = at + nbytes
        view = self.buf[at:at + nbytes].view(dtype)
        assert view.data_ptr() % ALIGN == phase and view.is_contiguous()
        return view

    def watch(self, **tensors) -> None:
        """Inputs of the call: copied to the host now, compared by `check`."""
        for name, t in tensors.items():
            self.inputs[name] = (t, t.detach().cpu().numpy().copy())

    def _owner(self, off: int) -> str:
        before = "the arena's start"
        for name, at, n in self.carved:
            if off < at:
                return f"guard between {before} and {name} ({at - off} bytes before {name})"
            if off < at + n:
                return f"{name} + {off - at}"
            before = name
        return f"guard after {before} ({off - self._end} bytes past its end)"

    def check(self, expected: dict) -> None:
        """`expected`: output name -> the bytes the call must have written from
        the output's first byte on (an array, bytes, or None for nothing).
        Synchronises the device and compares the whole arena, then the
        watched inputs."""
        torch.cuda.synchronize(self.buf.device)
        got = self.buf.cpu().numpy()
        want = np.full(got.size, self.pattern, np.uint8)
        where = {name: (at, n) for name, at, n in self.carved}
        assert set(expected) <= set(where), set(expected) - set(where)
        written = {}
        for name, value in expected.items():
            if value is None:
                continue
            b = as_bytes(value)
            at, n = where[name]
            assert b.size <= n, f"{name}: {b.size} expected bytes in an output of {n}"
            want[at:at + b.size] = b
            written[name] = b.size
        bad = np.flatnonzero(got != want)
        if bad.size:
            lines = [f"  byte {int(o)}: {self._owner(int(o))}: got {int(got[o]):#04x}, want {int(want[o]):#04x}"
                     for o in bad[:8]]
            outs = ", ".join(f"{name} at {at} ({written.get(name, 0)} of {n} bytes to be written)"
                             for name, at, n in self.carved)
            raise AssertionError(f"{bad.size} bytes of the arena (pattern {self.pattern:#04x}) differ; outputs: {outs}\n"
                                 + "\n".join(lines))
        for name, (t, before) in self.inputs.items():
            after = t.detach().cpu().numpy()
            if before.tobytes() != after.tobytes():
                first = np.flatnonzero(as_bytes(before) != as_bytes(after))[:8].tolist()
                raise AssertionError(f"input {name} was modified: first bytes {first}")


def phases(align: int):
    """The three phases an output of alignment `align` is tried at."""
    return (0, align, 16 - align)


def phase(placement: int, j: int, align: int) -> int:
    """The phase of a call's j-th output at `placement` (0, 1, 2): all outputs
    shift at once, neighbours to different phases."""
    return phases(align)[(placement + j) % 3]
