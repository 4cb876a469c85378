"""Host test of tests/guard_arena.py: carving, alignment skew, prefill, restore on exit, pass-through, and detection of a store one
element before and one element after the body.  The stores are made on a CPU arena through as_strided: allocated memory only."""
import math
import struct

import pytest
import torch

import guard_arena as G


def _arena_of(t):
    return G.GuardArena.entry_of(t)


def test_sentinel_is_a_quiet_nan_in_every_float_format():
    assert math.isnan(struct.unpack("<f", struct.pack("<I", G.SENTINEL))[0])
    assert G.SENTINEL < 2 ** 31                                               # fits the int32 fill
    half = torch.tensor([G.SENTINEL >> 16], dtype=torch.int32).to(torch.int16)
    assert bool(half.view(torch.float16).isnan()) and bool(half.view(torch.bfloat16).isnan())


@pytest.mark.parametrize("shape,dtype", [((3, 5, 7), torch.float32), ((13,), torch.uint8), ((2, 3, 4, 5, 16), torch.int32),
                                         ((1, 1), torch.float64), ((7, 3), torch.float16), ((2, 300000), torch.float32)])
def test_carving_alignment_and_prefill(shape, dtype):
    with G.GuardArena(patch=False) as ga:
        t = ga.alloc(shape, dtype, "cpu")
        z = ga.alloc(shape, dtype, "cpu", zero=True)
        e = _arena_of(t)
        nbytes = t.numel() * t.element_size()
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
        # 16-byte aligned and not more, measured from the arena's own base
        off = t.data_ptr() - e.arena.data_ptr()
        assert off == e.body_off and off % 256 == G.SKEW and t.data_ptr() % 16 == 0
        # guards: a condition, not a measurement
        g_front, g_back = off, e.arena.numel() * 4 - off - nbytes
        frame = nbytes // shape[0]
        for g in (g_front, g_back):
            assert g >= G.MIN_GUARD and g >= min(frame, G.MAX_GUARD) and g <= G.MAX_GUARD + 256
        # prefill: sentinel everywhere for empty, zero body for zeros
        assert bool((e.arena == G.SENTINEL).all())
        if dtype == torch.float32:
            assert bool(t.isnan().all())
        assert bool((z.view(torch.uint8) == 0).all())
        ez = _arena_of(z)
        u8 = ez.arena.view(torch.uint8)
        pat = torch.tensor(G.SENTINEL_BYTES, dtype=torch.uint8).repeat(ez.arena.numel())
        outside = torch.ones(u8.numel(), dtype=torch.bool)
        outside[ez.body_off:ez.body_off + nbytes] = False
        assert bool((u8[outside] == pat[outside]).all())                       # nothing but the body was zeroed
    assert ga.report() == []


def test_guard_covers_a_frame_and_is_capped():
    assert G.guard_bytes((4, 10), 40) == G.MIN_GUARD
    assert G.guard_bytes((2, 1 << 20), 8 << 20) == 4 << 20                # one frame of 4 MiB
    assert G.guard_bytes((2, 1 << 28), 2 << 30) == G.MAX_GUARD
    assert G.guard_bytes((), 4) == G.MIN_GUARD


def test_patching_restores_and_passes_cpu_and_unknown_calls_through():
    real = {n: getattr(torch, n) for n in ("empty", "zeros", "empty_like", "zeros_like")}
    with G.GuardArena() as ga:
        assert all(getattr(torch, n) is not real[n] for n in real)
        a = torch.empty(3, 4)                                                 # no device: torch's own
        b = torch.zeros((2, 2), dtype=torch.float64, device="cpu")            # CPU: passed through
        c = torch.empty_like(b)
        d = torch.zeros_like(b, memory_format=torch.preserve_format)
        e = torch.empty((2, 3), dtype=torch.float32, device="cpu", pin_memory=False)
        f = torch.empty(0, device="cpu")
        for t in (a, b, c, d, e, f):
            assert not hasattr(t, "_guard_entry")
        assert tuple(a.shape) == (3, 4) and float(b.sum()) == 0.0 and c.dtype == torch.float64 and tuple(d.shape) == (2, 2)
        assert ga.n_guarded == 0 and ga.n_passed == 6
    assert all(getattr(torch, n) is real[n] for n in real)
    with pytest.raises(ZeroDivisionError):                                    # restored when the body raises, too
        with G.GuardArena():
            1 / 0
    assert all(getattr(torch, n) is real[n] for n in real)
    assert ga.report() == []


def _elem_at(t, k):
    """One-element view k elements from the start of t's body, inside t's own arena (k may be -1 or numel)."""
    return torch.as_strided(t, (1,), (1,), t.storage_offset() + k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.float16])
@pytest.mark.parametrize("side", ["before", "after"])
def test_a_store_one_element_outside_the_body_is_reported(dtype, side):
    with G.GuardArena(patch=False) as ga:
        t = ga.alloc((5, 3), dtype, "cpu")
        clean = ga.alloc((5, 3), dtype, "cpu")
        flat = t.view(-1)
        flat.fill_(1)                                                          # writing the body itself is no hit
        clean.fill_(1)
        _elem_at(flat, -1 if side == "before" else flat.numel()).fill_(3)
    rep = ga.report()
    assert len(rep) == 1, rep
    want = -4 if side == "before" else 0                                      # guards are compared word by word
    assert f"guard {side} the body of (5, 3) {dtype}" in rep[0] and f"offset {want:+d} " in rep[0], rep
    assert ga.report() == []                                                   # read once, then clean again


def test_guards_are_checked_when_the_tensor_dies_and_the_arena_is_released():
    with G.GuardArena(patch=False) as ga:
        t = ga.alloc((4, 4), torch.float32, "cpu")
        ref = _arena_of(t)
        import weakref
        wr = weakref.ref(ref)
        _elem_at(t.view(-1), 16).fill_(0.0)
        del t, ref
        assert wr() is None                                                    # checked and released at death, not at exit
        assert len(ga._live) == 0
    rep = ga.report()
    assert len(rep) == 1 and "after" in rep[0] and "offset +0 " in rep[0], rep


def test_snapshot_sees_a_changed_input():
    with G.GuardArena(patch=False) as ga:
        x = ga.guarded(torch.arange(12, dtype=torch.float32).view(3, 4))
        snap = ga.snapshot(x)
        assert ga.unchanged(x, snap)
        x[1, 1] = -1.0
        assert not ga.unchanged(x, snap)
    assert ga.report() == []
