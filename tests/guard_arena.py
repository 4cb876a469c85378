"""Guarded allocations for the GPU tests: every device tensor the library allocates while a GuardArena is active is carved out of a
private arena [guard | body | guard] that is pre-filled with a 32-bit quiet-NaN sentinel.

What this shows (nothing here ever touches memory that is not allocated -- the guards are ordinary device memory):
  * a store outside the output lands in a guard and is reported at teardown with (shape, dtype, side, first bad byte offset);
  * an fp32 element no kernel stored reads as NaN and fails the test's own comparison; `zeros` bodies are zeroed as usual, so a
    split-padded buffer keeps its contract (zero border, never written);
  * the body starts 16-byte aligned and not more (offset = 16 mod 256 from the arena's base): include/mvsgi.h documents 16 bytes,
    torch's caching allocator hands out 512.

Guard size is a condition, not a measurement: on each side at least 1 MiB and at least one frame (nbytes // shape[0]), capped at
64 MiB, so that a store that is off by a row, a plane or a frame still lands inside.

Guards are compared with the sentinel on the device when the returned tensor dies (weakref.finalize) and, for everything still alive
(module-owned buffers such as _mvsgi_rs_bufs live on), at the end of the test; the comparisons are OR-ed into one device flag
that is read once at teardown.  An arena is released as soon as it has been checked.

Passed straight through to torch's own factory functions: CPU / pinned tensors, everything while the current stream is capturing
(no fills or checks may be recorded into a graph), and every call this module does not fully understand (keyword arguments beyond
dtype / device / requires_grad, a memory_format, an empty_like of a non-contiguous tensor, sizes that are not plain ints).  A
pass-through only loses coverage.

The GPU test modules switch this on with an autouse fixture whose body is `fixture_body`.  Exempt tests (by function name) and why:
  test_cold_compile_and_load_on_this_box            compiles and loads the library in a subprocess
  test_bench_default_submission_line                runs bench.py in a subprocess
  test_bench_plain_line_and_dumped_outputs          runs bench.py in a subprocess
  test_bench_two_ranks_frame_sharded_on_one_gpu     runs bench.py under torch.distributed.run in subprocesses
  test_bench_self_launches_its_ranks                runs bench.py in subprocesses
  test_overlapping_copy_stream_overlaps_uploads_with_compute      times the overlap of two streams
No test that calls a kernel through hip_ops directly is exempt; captured paths pass through by design and their eager twins run
guarded.
"""
from __future__ import annotations

import contextlib
import threading
import weakref

import torch

SENTINEL = 0x7FC0BEEF                    # a quiet NaN as fp32; its upper half (0x7FC0) is a NaN as fp16 and bf16 too
SENTINEL_BYTES = tuple(SENTINEL.to_bytes(4, "little"))
MIN_GUARD = 1 << 20
MAX_GUARD = 64 << 20
SKEW = 16                                # body offset modulo 256 from the arena's base

EXEMPT = {
    "test_cold_compile_and_load_on_this_box",
    "test_bench_default_submission_line",
    "test_bench_plain_line_and_dumped_outputs",
    "test_bench_two_ranks_frame_sharded_on_one_gpu",
    "test_bench_self_launches_its_ranks",
    "test_overlapping_copy_stream_overlaps_uploads_with_compute",
}

_PATCHED = ("empty", "zeros", "empty_like", "zeros_like")
_REAL = {name: getattr(torch, name) for name in _PATCHED}      # torch's own functions, bound before anything is replaced
_UNDERSTOOD = {"dtype", "device", "requires_grad"}


def guard_bytes(shape, nbytes: int) -> int:
    """Guard size for a request: >= 1 MiB and >= one frame, <= 64 MiB, a multiple of 256."""
    frame = nbytes // shape[0] if len(shape) and shape[0] > 0 else nbytes
    g = min(max(MIN_GUARD, frame), MAX_GUARD)
    return -(-g // 256) * 256


class _Entry:
    __slots__ = ("arena", "body_off", "nbytes", "shape", "dtype", "fin", "__weakref__")

    def __init__(self, arena, body_off, nbytes, shape, dtype):
        self.arena, self.body_off, self.nbytes, self.shape, self.dtype = arena, body_off, nbytes, tuple(shape), dtype
        self.fin = None


class GuardArena:
    """Context manager.  patch=True replaces torch.empty / zeros / empty_like / zeros_like for device tensors while active;
    alloc() / guarded() carve explicitly (any device, CPU included)."""

    def __init__(self, patch: bool = True):
        self.patch = patch
        self._lock = threading.RLock()
        self._live = {}              # id(entry) -> entry
        self._flags = {}             # device -> 0-dim bool tensor: OR of every guard comparison so far
        self._records = []           # (shape, dtype, side, byte offset of the compared range relative to the body start or end, hit, first)
        self._pat = {}
        self._active = False
        self._paused = False
        self.n_guarded = 0
        self.n_passed = 0

    # ---- carving ----
    def alloc(self, shape, dtype=torch.float32, device="cpu", zero: bool = False) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        nbytes = n * dtype.itemsize
        g = guard_bytes(shape, nbytes)
        body_off = g + SKEW
        total = -(-(body_off + nbytes + g) // 4) * 4
        arena = _REAL["empty"](total // 4, dtype=torch.int32, device=device)
        arena.fill_(SENTINEL)
        body = arena.view(torch.uint8)[body_off:body_off + nbytes]
        if zero:
            body.zero_()
        view = body.view(dtype).view(shape)
        e = _Entry(arena, body_off, nbytes, shape, dtype)
        with self._lock:
            self._live[id(e)] = e
            self.n_guarded += 1
        e.fin = weakref.finalize(view, self._on_death, id(e))
        e.fin.atexit = False
        view._guard_entry = weakref.ref(e)
        return view

    def guarded(self, t: torch.Tensor) -> torch.Tensor:
        """A copy of t (contiguous) inside an arena of its own."""
        g = self.alloc(t.shape, t.dtype, t.device)
        g.copy_(t)
        return g

    @staticmethod
    def entry_of(view: torch.Tensor) -> _Entry:
        e = view._guard_entry()
        if e is None:
            raise RuntimeError("the arena of this tensor has been released")
        return e

    def snapshot(self, view: torch.Tensor) -> torch.Tensor:
        """A copy of the whole arena (guards and body) of a tensor made by alloc() / guarded()."""
        return self.entry_of(view).arena.clone()

    def unchanged(self, view: torch.Tensor, snap: torch.Tensor) -> bool:
        return bool(torch.equal(self.entry_of(view).arena, snap))

    @contextlib.contextmanager
    def paused(self):
        """The replaced factory functions pass through (torch's own allocator) inside this block: the plain twin of a guarded call."""
        old, self._paused = self._paused, True
        try:
            yield
        finally:
            self._paused = old

    # ---- checking ----
    def _flag(self, device):
        f = self._flags.get(device)
        if f is None:
            f = self._flags[device] = _REAL["zeros"]((), dtype=torch.bool, device=device)
        return f

    def _pattern(self, device):
        p = self._pat.get(device)
        if p is None:
            p = self._pat[device] = torch.tensor(SENTINEL_BYTES, dtype=torch.uint8, device=device)
        return p

    def _compare(self, e, side, rel, got, want):
        """OR (got != want) into the device flag and keep (hit, first bad index) on the device: no host synchronisation."""
        bad = got != want
        hit = bad.any()
        first = bad.view(torch.uint8).argmax()          # the first of several maxima: the first bad element
        self._flag(e.arena.device).logical_or_(hit)
        self._records.append((e.shape, e.dtype, side, rel, got.element_size(), hit, first))

    def _check(self, e) -> None:
        a = e.arena
        end = e.body_off + e.nbytes
        end4 = -(-end // 4) * 4
        self._compare(e, "before", -e.body_off, a[:e.body_off // 4], SENTINEL)
        if end4 != end:              # a body that does not end on a word: the rest of that word, byte by byte
            self._compare(e, "after", 0, a.view(torch.uint8)[end:end4], self._pattern(a.device)[end % 4:])
        self._compare(e, "after", end4 - end, a[end4 // 4:], SENTINEL)

    def _on_death(self, key) -> None:
        with self._lock:
            e = self._live.pop(key, None)
        if e is None or not self._active:
            return
        dev = e.arena.device
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return                   # nothing may be recorded into a graph; the arena is released unchecked
        try:
            if dev.type == "cuda" and dev.index is not None and dev.index != torch.cuda.current_device():
                with torch.cuda.device(dev):
                    self._check(e)
            else:
                self._check(e)
        except Exception as ex:      # a finaliser must not raise; the failure is reported at teardown instead
            self._records.append((e.shape, e.dtype, f"check failed: {ex!r}", 0, 1, True, 0))

    def check_live(self) -> None:
        """Check and release everything still alive (the tensors themselves stay valid: their storage is theirs)."""
        with self._lock:
            live, self._live = list(self._live.values()), {}
        for e in live:
            if e.fin is not None:
                e.fin.detach()
            self._check(e)

    def report(self) -> list:
        """Read the device flag(s) once; -> one line per guard that no longer holds the sentinel (empty: all clean)."""
        hit_any = any(bool(f) for f in self._flags.values())
        out = []
        for shape, dtype, side, rel, esz, hit, first in self._records:
            if isinstance(hit, bool):
                out.append(f"{side} for {shape} {dtype}")
            elif hit_any and bool(hit):
                off = rel + int(first) * esz
                out.append(f"guard {side} the body of {shape} {dtype} overwritten: first bad 32-bit word (or byte of a ragged end) at byte offset {off:+d} from the body's "
                           f"{'start' if side == 'before' else 'end'}")
        self._records = []
        for f in self._flags.values():
            f.zero_()
        return out

    # ---- the replaced factory functions ----
    @staticmethod
    def _size_of(args):
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            args = tuple(args[0])
        if not args or not all(type(s) is int and s >= 0 for s in args):
            return None
        return tuple(args)

    def _wants(self, device) -> bool:
        if device is None or not self._active or self._paused:
            return False
        try:
            d = torch.device(device) if not isinstance(device, torch.device) else device
        except Exception:
            return False
        return d.type == "cuda" and not torch.cuda.is_current_stream_capturing()

    def _factory(self, name, zero):
        real = _REAL[name]

        def f(*args, **kw):
            size = self._size_of(args)
            if size is None or not set(kw) <= _UNDERSTOOD or not self._wants(kw.get("device")) or 0 in size:
                self.n_passed += 1
                return real(*args, **kw)
            dtype = kw.get("dtype") or torch.get_default_dtype()
            t = self.alloc(size, dtype, kw["device"], zero)
            return t.requires_grad_() if kw.get("requires_grad") else t
        f.__name__ = name
        return f

    def _factory_like(self, name, zero):
        real = _REAL[name]

        def f(*args, **kw):
            t = args[0] if len(args) == 1 else None
            if not isinstance(t, torch.Tensor) or type(t) is not torch.Tensor or not set(kw) <= _UNDERSTOOD or not t.is_contiguous() \
                    or t.numel() == 0 or t.layout != torch.strided or not self._wants(kw.get("device") or t.device):
                self.n_passed += 1
                return real(*args, **kw)
            r = self.alloc(t.shape, kw.get("dtype") or t.dtype, kw.get("device") or t.device, zero)
            return r.requires_grad_() if kw.get("requires_grad") else r
        f.__name__ = name
        return f

    def __enter__(self):
        self._active = True
        if self.patch:
            for name in _PATCHED:
                if getattr(torch, name) is not _REAL[name]:
                    raise RuntimeError(f"torch.{name} is already replaced")
            torch.empty = self._factory("empty", False)
            torch.zeros = self._factory("zeros", True)
            torch.empty_like = self._factory_like("empty_like", False)
            torch.zeros_like = self._factory_like("zeros_like", True)
        return self

    def __exit__(self, *exc):
        if self.patch:
            for name in _PATCHED:
                setattr(torch, name, _REAL[name])
        try:
            if exc[0] is None:
                self.check_live()
        finally:
            self._active = False
            with self._lock:
                for e in self._live.values():
                    if e.fin is not None:
                        e.fin.detach()
                self._live = {}
        return False


def fixture_body(request):
    """Body of the autouse fixture of a GPU test module: `yield from guard_arena.fixture_body(request)`."""
    if request.node.originalname in EXEMPT or request.node.get_closest_marker("gpu") is None or not torch.cuda.is_available():
        yield None
        return
    with GuardArena() as ga:
        yield ga
    hits = ga.report()
    assert not hits, "stores outside a library-allocated tensor:\n  " + "\n  ".join(hits)
