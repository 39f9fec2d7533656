"""Guarded buffers for the C-ABI contract tests (tests/test_contract_gpu.py, tests/test_guarded_cpu.py).

A Guarded region is ONE allocation laid out as [guard | body | guard] floats.  The guards hold a canary bit pattern; the body is what the
library sees as the tensor.  A store past either end of the tensor lands in the test's own guard (1 MiB on each side by default, far more
than any plausible overrun), where guards_intact() finds it, instead of in the caching allocator's slack where nothing would.

Both bit patterns are quiet NaNs, so a kernel that LOADS past a tensor and lets the value reach its arithmetic (multiplying it by a zero
weight, say) turns a valid output into NaN -- what an Inf or NaN neighbour in an application would do.  Patterns are compared as int32,
never as floats (NaN != NaN).
"""
from __future__ import annotations

import numpy as np
import torch

CANARY = 0x7FC0A5A5  # guards
POISON = 0x7FC05A5A  # bodies the library must write (outputs, scratch, packed weights before Init)
GUARD = 1 << 18      # floats on each side: 1 MiB


class Guarded:
    """Guarded(n, fill, offset=0, guard=GUARD, device="cuda").

    n floats of body, `offset` in {0, 1} floats past a 16-byte boundary (so the 4-byte-aligned forms of every kernel run too).
    fill: "poison" (a body the library must write), "nan" (a NaN body: the bias the library must NOT read), or an array of n values
    (an input)."""

    def __init__(self, n: int, fill="poison", offset: int = 0, guard: int = GUARD, device="cuda"):
        if offset not in (0, 1):
            raise ValueError("offset must be 0 or 1")
        self.n, self.offset, self.guard = int(n), offset, guard
        self.raw = torch.full((2 * guard + offset + self.n,), CANARY, dtype=torch.int32, device=device)
        self.lo = guard + offset  # first body word
        self.body = self.raw.view(torch.float32)[self.lo:self.lo + self.n]
        self.fill(fill)
        assert self.raw.data_ptr() % 16 == 0 and (self.ptr - self.raw.data_ptr()) % 16 == 4 * offset

    @property
    def ptr(self) -> int:
        """Device address of the body; for an empty body, a valid address between two guards (never NULL)."""
        return self.raw.data_ptr() + 4 * self.lo

    def fill(self, fill="poison"):
        bits = self.raw[self.lo:self.lo + self.n]
        if isinstance(fill, str):
            bits.fill_({"poison": POISON, "nan": 0x7FC00000}[fill])
        else:
            a = np.ascontiguousarray(np.asarray(fill, dtype=np.float32).reshape(-1))
            if a.size != self.n:
                raise ValueError(f"fill has {a.size} values for a body of {self.n}")
            if self.n:
                self.body.copy_(torch.from_numpy(a))
        return self

    def _guard_words(self):
        return self.raw[:self.lo], self.raw[self.lo + self.n:]

    def guards_intact(self):
        """None when both guards still hold the canary, else (index relative to the body start, int32 value) of the first bad word:
        negative indices are before the body, indices >= n after it."""
        before, after = self._guard_words()
        bad = torch.nonzero(before != CANARY)
        if bad.numel():
            i = int(bad[-1])  # the word closest to the body
            return i - self.lo, int(before[i])
        bad = torch.nonzero(after != CANARY)
        if bad.numel():
            i = int(bad[0])
            return self.n + i, int(after[i])
        return None

    def unwritten(self, live=None) -> int:
        """Body words still equal to the poison; `live` (a bool mask or index over the body) restricts the count."""
        bits = self.raw[self.lo:self.lo + self.n]
        if live is not None:
            bits = bits[live]
        return int((bits == POISON).sum())

    def snapshot(self) -> torch.Tensor:
        return self.raw.clone()

    def unchanged(self, snap: torch.Tensor) -> bool:
        """Bitwise: body AND guards."""
        return bool(torch.equal(self.raw, snap))

    def first_change(self, snap: torch.Tensor):
        """(index relative to the body start, old word, new word) of the first changed word, or None."""
        d = torch.nonzero(self.raw != snap)
        if not d.numel():
            return None
        i = int(d[0])
        return i - self.lo, int(snap[i]), int(self.raw[i])

    def values(self) -> np.ndarray:
        return self.body.detach().cpu().numpy().copy()

    def bits(self) -> torch.Tensor:
        return self.raw[self.lo:self.lo + self.n]


def describe(bad) -> str:
    if bad is None:
        return "intact"
    i, v = bad
    return f"word {i} (body is [0, n)) holds 0x{v & 0xFFFFFFFF:08X}"
