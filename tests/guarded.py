"""Guarded allocations for the memory-contract tests: where a kernel writes, not only what.

Every tensor a contract case hands to a kernel -- and every tensor hot_ops allocates for it -- is an interior view of
one larger uint8 arena whose two guards carry a known byte pattern:

    [ guard | interior | guard ]        guards: a multiple of 512 bytes each, at least one full row tile of the tensor

`place` puts an existing tensor into such an arena; `guarded_allocations` makes torch.empty / torch.empty_like /
torch.zeros (the allocation forms hot_ops uses) return such interiors for the duration of a block and records them.
An `empty` interior is pattern-filled too, so an element a kernel leaves unwritten -- or a result that depends on what
a workspace held before the launch -- differs between two runs made under the two PATTERNS, which differ in every byte;
the first is a NaN as float32 and as float64.  `record_lib_calls` notes which soc_* entry points a block called.

Plain module (no fixtures, no pytest hooks); works on any device, so the helper itself is tested on the CPU.
"""
from __future__ import annotations

import contextlib
from typing import Callable, List, Optional, Sequence

import torch

PATTERNS = (0xFF, 0x5A)          # 0xFFFFFFFF / 0xFFFF...FF: NaN as f32 and f64; 0x5A: every byte (and bit 0, 2, 5, 7) differs
GUARD_UNIT = 512                 # torch's device allocations are 512-byte aligned: an interior keeps that alignment
TILE_ROWS = 256                  # the tallest row tile of any kernel here (K20's 256 x 128 / 256 x 96 tiles)
_FLAT_GUARD_CAP = 1 << 20        # guards of 1-D byte buffers (workspaces, packed images): their own size, up to 1 MiB


def _itemsize(dtype: torch.dtype) -> int:
    return torch._utils._element_size(dtype)          # no allocation: this runs inside the patched torch.empty


def _round_up(n: int, unit: int = GUARD_UNIT) -> int:
    return max(unit, -(-int(n) // unit) * unit)


def default_guard_for(shape: Sequence[int], dtype: torch.dtype) -> int:
    """Guard bytes for a tensor: TILE_ROWS rows of its last dimension (a whole-tile rounding error of a row-wise kernel
    lands inside the guard), for a 1-D buffer its own size (capped); always a multiple of GUARD_UNIT."""
    item = _itemsize(dtype)
    shape = tuple(int(s) for s in shape)
    if len(shape) >= 2:
        return _round_up(TILE_ROWS * max(shape[-1], 1) * item)
    n = (shape[0] if shape else 1) * item
    return _round_up(min(max(n, GUARD_UNIT), _FLAT_GUARD_CAP))


class Guarded:
    """One arena: `view` is the interior (the tensor handed out), the rest of `arena` is guard."""

    def __init__(self, arena: torch.Tensor, guard: int, nbytes: int, view: torch.Tensor, pattern: int, kind: str):
        self.arena, self.guard, self.nbytes, self.view, self.pattern, self.kind = arena, guard, nbytes, view, pattern, kind

    @property
    def front(self) -> torch.Tensor:
        return self.arena[:self.guard]

    @property
    def back(self) -> torch.Tensor:
        return self.arena[self.guard + self.nbytes:]

    @property
    def interior(self) -> torch.Tensor:
        """The interior as bytes (a view: it follows what kernels write)."""
        return self.arena[self.guard:self.guard + self.nbytes]

    def snapshot(self) -> torch.Tensor:
        return self.interior.clone()

    def guards_bad(self) -> torch.Tensor:
        """0-d bool tensor on the arena's device: some guard byte no longer equals the pattern (no host sync)."""
        return (self.front != self.pattern).any() | (self.back != self.pattern).any()

    def guards_intact(self) -> bool:
        return not bool(self.guards_bad())

    def violations(self, limit: int = 4) -> List[str]:
        """Where the guards were overwritten, as byte offsets relative to the interior (negative: in front of it)."""
        out = []
        for name, g, base in (("front", self.front, -self.guard), ("back", self.back, self.nbytes)):
            idx = (g != self.pattern).nonzero().flatten()
            if idx.numel():
                first = [int(i) + base for i in idx[:limit]]
                out.append(f"{name} guard: {idx.numel()} bytes changed, first at interior offset(s) {first}")
        return out

    def describe(self) -> str:
        return f"{self.kind} {tuple(self.view.shape)} {self.view.dtype} ({self.nbytes} B, guards {self.guard} B)"


def _arena(real_empty: Callable, shape, dtype, device, guard: Optional[int], pattern: int, kind: str, zero: bool) -> Guarded:
    shape = tuple(int(s) for s in shape)
    numel = 1
    for s in shape:
        numel *= s
    nbytes = numel * _itemsize(dtype)
    guard = default_guard_for(shape, dtype) if guard is None else int(guard)
    if guard <= 0 or guard % GUARD_UNIT:
        raise ValueError(f"guard must be a positive multiple of {GUARD_UNIT} bytes, got {guard}")
    arena = real_empty(2 * guard + nbytes, dtype=torch.uint8, device=device)
    arena.fill_(pattern)
    interior = arena[guard:guard + nbytes]
    if zero:
        interior.zero_()
    view = interior.view(dtype).view(shape)
    return Guarded(arena, guard, nbytes, view, pattern, kind)


def place(tensor: torch.Tensor, guard_bytes: Optional[int] = None, pattern: int = PATTERNS[0], device=None):
    """Copy `tensor` into the middle of a pattern-filled arena (on `device`, default the tensor's): returns
    (interior view with the tensor's shape, dtype and values; the Guarded handle that re-checks the guards)."""
    device = tensor.device if device is None else torch.device(device)
    src = tensor.detach().contiguous()
    g = _arena(torch.empty, src.shape, src.dtype, device, guard_bytes, pattern, "placed", zero=False)
    g.view.copy_(src)
    return g.view, g


def _same_device(a, b: torch.device) -> bool:
    a = torch.device(a)
    if a.type != b.type:
        return False
    if a.type == "cpu":
        return True
    cur = torch.cuda.current_device() if a.type == "cuda" else 0
    return (cur if a.index is None else a.index) == (cur if b.index is None else b.index)


def _shape_of(args):
    """The shape of torch.empty(*args): ints, or one sequence of ints; None for anything else."""
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    if all(isinstance(a, int) and not isinstance(a, bool) for a in args):
        return tuple(int(a) for a in args)
    return None


@contextlib.contextmanager
def guarded_allocations(device, pattern: int = PATTERNS[0], guard_for: Optional[Callable] = None, monkeypatch=None):
    """Inside the block torch.empty(shape, dtype=, device=), torch.zeros(...) and torch.empty_like(t) ON `device` return
    interiors of pattern-filled arenas (zeros: a zero interior; empty: an all-pattern interior) and every allocation served
    is appended to the list the block receives.  Any other call -- another device, a keyword beyond dtype / device, a
    non-contiguous empty_like -- goes to the real function unchanged: the patch is process-wide while the block runs, and
    torch's own Python code may allocate too.  `guard_for(shape, dtype) -> bytes` overrides default_guard_for.  Restored on
    exit through `monkeypatch` when one is given, in a `finally` otherwise."""
    device = torch.device(device)
    real_empty, real_zeros, real_like = torch.empty, torch.zeros, torch.empty_like
    served: List[Guarded] = []
    sizer = guard_for or default_guard_for

    def serve(shape, dtype, kind, zero):
        g = _arena(real_empty, shape, dtype, device, sizer(shape, dtype), pattern, kind, zero)
        served.append(g)
        return g.view

    def make(real, kind, zero):
        def patched(*args, **kw):
            shape = _shape_of(args)
            if shape is None or set(kw) - {"dtype", "device"} or not _same_device(kw.get("device", "cpu"), device):
                return real(*args, **kw)
            dtype = kw.get("dtype") or torch.get_default_dtype()
            return serve(shape, dtype, kind, zero)
        return patched

    def patched_like(t, *args, **kw):
        if args or kw or not isinstance(t, torch.Tensor) or not _same_device(t.device, device) or not t.is_contiguous():
            return real_like(t, *args, **kw)
        return serve(t.shape, t.dtype, "empty_like", False)

    patches = (("empty", make(real_empty, "empty", False)), ("zeros", make(real_zeros, "zeros", True)),
               ("empty_like", patched_like))
    if monkeypatch is not None:
        with monkeypatch.context() as mp:
            for name, fn in patches:
                mp.setattr(torch, name, fn)
            yield served
        return
    try:
        for name, fn in patches:
            setattr(torch, name, fn)
        yield served
    finally:
        torch.empty, torch.zeros, torch.empty_like = real_empty, real_zeros, real_like


class RecordingLib:
    """Proxy around the ctypes library object: every soc_* function fetched through it notes its name when called."""

    def __init__(self, lib, calls: List[str]):
        self.__dict__["_lib"], self.__dict__["_calls"] = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("soc_"):
            return fn
        calls = self._calls

        def call(*args):
            calls.append(name)
            return fn(*args)
        return call


@contextlib.contextmanager
def record_lib_calls():
    """Inside the block `_lib.load()` returns a RecordingLib; yields the list of soc_* names called, in order."""
    from neurips2023_soc_amd import _lib
    real = _lib.load()
    calls: List[str] = []
    _lib._lib = RecordingLib(real, calls)
    try:
        yield calls
    finally:
        _lib._lib = real


# ---------------------------------------------------------------------------------------------------------------------
# the five checks of a contract case, device-agnostic (the GPU table and the helper's own CPU tests both run this)

class ContractViolation(AssertionError):
    pass


def _as_tuple(out):
    return tuple(out) if isinstance(out, (tuple, list)) else (out,)


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().reshape(-1).view(torch.uint8)


def run_guarded(inputs: dict, call: Callable, device, pattern: int, inplace: Sequence[str] = (), guard_for=None,
                record: bool = True):
    """One run of `call(tensors)` under `pattern`: tensor inputs placed, allocations guarded.  Returns (outputs tuple,
    list of failure strings for checks 1 and 3, soc_* calls seen).  One host synchronisation for all device-side checks."""
    handles, args = {}, {}
    for name, v in inputs.items():
        if isinstance(v, torch.Tensor):
            gb = guard_for(v.shape, v.dtype) if guard_for else None
            args[name], handles[name] = place(v, gb, pattern, device)
        else:
            args[name] = v
    before = {n: h.snapshot() for n, h in handles.items() if n not in inplace}
    rec = record_lib_calls() if record else contextlib.nullcontext([])
    with rec as calls, guarded_allocations(device, pattern, guard_for) as served:
        outs = _as_tuple(call(args))
    named = [(f"input {n}", h) for n, h in handles.items()] + [(f"allocation #{i}", h) for i, h in enumerate(served)]
    owned = {h.arena.untyped_storage().data_ptr() for _, h in named}
    flags = [h.guards_bad() for _, h in named] + [(handles[n].interior != b).any() for n, b in before.items()]
    flags = torch.stack(flags).cpu().tolist() if flags else []          # the one synchronisation
    failures = []
    for (name, h), bad in zip(named, flags):
        if bad:
            failures.append(f"guards of {name} [{h.describe()}] overwritten: " + "; ".join(h.violations()))
    for n, bad in zip(before, flags[len(named):]):
        if bad:
            failures.append(f"input {n} was modified by the call")
    for i, o in enumerate(outs):        # an output that did not come out of an arena was never poisoned: check 2 would be vacuous
        if isinstance(o, torch.Tensor) and o.untyped_storage().data_ptr() not in owned:
            failures.append(f"output {i} does not live in a guarded arena (allocated in a form guarded_allocations does not serve)")
    return outs, failures, list(calls), served


def check_contract(inputs: dict, call: Callable, device, *, entry=None, inplace: Sequence[str] = (),
                   reference: Optional[Callable] = None, compare: Optional[Callable] = None, guard_for=None):
    """The five checks: two runs on identical inputs, one per pattern.
      1 guards intact   2 outputs bit-identical between the runs (fully written, independent of prior contents)
      3 inputs untouched (except `inplace`)   4 run 1 agrees with `reference(inputs)` as judged by `compare(i, got, want)`
        per output i (it asserts)   5 `entry` (a name or several) is among the soc_* functions the call reached.
    Raises ContractViolation listing everything that failed; returns run 1's outputs."""
    runs, failures = [], []
    entries = () if entry is None else ((entry,) if isinstance(entry, str) else tuple(entry))
    for pattern in PATTERNS:
        outs, bad, calls, _served = run_guarded(inputs, call, device, pattern, inplace, guard_for, record=bool(entries))
        failures += [f"pattern 0x{pattern:02X}: {b}" for b in bad]
        failures += [f"pattern 0x{pattern:02X}: entry point {e} was not called (saw {sorted(set(calls))})"
                     for e in entries if e not in calls]
        runs.append(outs)
    if len(runs[0]) != len(runs[1]):
        failures.append("the two runs returned a different number of outputs")
    for i, (a, b) in enumerate(zip(*runs)):
        if a is None or b is None:
            continue
        ab, bb = _bytes(a), _bytes(b)
        if ab.shape != bb.shape or not torch.equal(ab, bb):
            n = int((ab != bb).sum()) if ab.shape == bb.shape else -1
            first = int((ab != bb).nonzero()[0]) if n > 0 else -1
            failures.append(f"output {i} differs between the two patterns in {n} bytes (first at byte {first} of {ab.numel()}): "
                            "an element was left unwritten, or the result depends on prior memory contents")
    if reference is not None:
        want = _as_tuple(reference(inputs))
        for i, (g, w) in enumerate(zip(runs[0], want)):
            if w is None:
                continue
            try:
                compare(i, g.detach().cpu(), w)
            except AssertionError as exc:
                failures.append(f"output {i} disagrees with the reference: {exc}")
    if failures:
        raise ContractViolation("\n".join(failures))
    return runs[0]
