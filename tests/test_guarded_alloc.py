"""The guard-band helper (tests/_guarded.py) itself, on the CPU: a stand-in module takes the place of imagine360_amd.kernels and
plain tensor writes the place of kernels.  Every corruption is planted inside the helper's own buffer."""
import re
import types

import pytest
import torch

import _guarded
from _guarded import ALIGN, MIN_GUARD, PATTERN, Guarded

DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.uint8]


def stand_in():
    """A module that allocates its results the way kernels.py does: through ITS global name `torch`."""
    m = types.ModuleType("stand_in_kernels")
    m.torch = torch
    m.double = lambda x: _write(m.torch.empty(x.shape, dtype=x.dtype, device=x.device), x * 2, x.shape[0])
    m.double_skip_last = lambda x: _write(m.torch.empty(x.shape, dtype=x.dtype, device=x.device), x * 2, x.shape[0] - 1)
    m.double_like = lambda x: _write(m.torch.empty_like(x), x * 2, x.shape[0])
    m.counters = lambda n: m.torch.zeros((n,), dtype=torch.int32, device="cpu")
    return m


def _write(dst, val, rows):
    dst[:rows].copy_(val[:rows])
    return dst


def raw_of(g, t):
    a = g.find(t)
    return a, a.raw


@pytest.mark.parametrize("dt", DTYPES)
def test_clean_run_passes_and_the_pattern_is_what_it_claims(dt):
    m = stand_in()
    g = Guarded(m)
    x = g.guard(torch.arange(15).reshape(3, 5).to(dt))
    real = m.torch
    with g:
        assert m.torch is not real and m.torch.float16 is torch.float16 and torch.empty is real.empty      # only the module's name
        y = g.out(m.double(x))
    assert m.torch is real
    assert torch.equal(y, (torch.arange(15).reshape(3, 5) * 2).to(dt)) and len(g.allocs) == 2
    a, raw = raw_of(g, y)
    assert a.off >= MIN_GUARD and raw.numel() - a.off - a.span >= MIN_GUARD
    words = raw[:a.off].view(torch.int16)
    assert bool((words == PATTERN).all())
    assert bool(words.view(torch.bfloat16).isnan().all()) and bool(words.view(torch.float16).isnan().all())
    assert bool(raw[:a.off // 4 * 4].view(torch.float32).isnan().all())


def test_guards_cover_256_rows_of_a_wide_tensor():
    g = Guarded(stand_in())
    x = g.guard(torch.zeros(2, 5120, dtype=torch.float32))
    a = g.find(x)
    assert a.off >= 256 * 5120 * 4 and a.raw.numel() - a.off - a.span >= 256 * 5120 * 4


@pytest.mark.parametrize("where,delta", [("front", -1), ("front", -MIN_GUARD), ("back", 0), ("back", MIN_GUARD - 1)])
def test_one_scribbled_guard_byte_is_reported_with_its_offset(where, delta):
    m = stand_in()
    g = Guarded(m)
    x = g.guard(torch.ones(7, 6, dtype=torch.bfloat16))
    with pytest.raises(AssertionError) as e:
        with g:
            y = g.out(m.double(x))
            a, raw = raw_of(g, y)
            pos = a.off + delta if where == "front" else a.off + a.span + delta
            raw[pos] = raw[pos] ^ 0x10
    rel = pos - a.off
    msg = str(e.value)
    assert f"{where} guard overwritten, bytes {rel}..{rel} relative to the tensor" in msg, msg
    assert "empty #1: shape (7, 6) torch.bfloat16" in msg, msg                      # which allocation: shape, dtype, index
    assert msg.count("overwritten") == 1 and "sentinel" not in msg


def test_a_scribbled_row_gap_is_reported_and_a_clean_one_passes():
    m = stand_in()
    g = Guarded(m)
    dst = g.empty((2, 3, 8), torch.float16, "cpu", strides=(100, 16, 1))          # row stride 16 > 8, batch stride 100 > 3 rows
    assert dst.stride() == (100, 16, 1) and bool(dst.isnan().all())
    with g:
        dst.copy_(torch.ones(2, 3, 8))
        g.out(dst)
    g2 = Guarded(m)
    dst = g2.guard(torch.ones(2, 3, 8, dtype=torch.float16), row_stride=16)
    assert dst.stride() == (48, 16, 1)
    with pytest.raises(AssertionError, match=re.escape("row gap overwritten, bytes 16..19 relative to the tensor")):
        with g2:
            a = g2.find(dst)
            a.raw[a.off + 16:a.off + 20] = 0                                        # the first two elements behind row 0
            g2.out(dst)


def test_an_unwritten_interior_is_reported():
    m = stand_in()
    g = Guarded(m)
    x = g.guard(torch.ones(5, 4, dtype=torch.float32))
    with pytest.raises(AssertionError) as e:
        with g:
            g.out(m.double_skip_last(x))
    msg = str(e.value)
    assert "empty #1: shape (5, 4) torch.float32: 4 element(s) still hold the sentinel" in msg and "bytes 64..79 relative" in msg, msg
    # one-byte results: a run of pattern bytes (a lone 0xC1 or 0x7F is an ordinary value)
    g = Guarded(m)
    with pytest.raises(AssertionError, match=re.escape("bytes 8..15 relative")):
        with g:
            y = m.torch.empty((4, 5), dtype=torch.uint8, device="cpu")
            y.reshape(-1)[:8] = 0xC1
            y.reshape(-1)[16:] = 0x7F
            g.out(y)


def test_zeros_interiors_are_zero_between_poisoned_guards():
    m = stand_in()
    g = Guarded(m)
    with g:
        c = m.counters(9)
        assert c.dtype == torch.int32 and bool((c == 0).all())
        a = g.find(c)
        assert a is not None and bool((a.raw[:a.off].view(torch.int16) == PATTERN).all())
        assert bool((a.raw[a.off + a.span:a.off + a.span + 64].view(torch.int16) == PATTERN).all())
        g.out(c)
    with g:
        s = g.out(m.torch.zeros((), dtype=torch.float32, device="cpu"))             # a scalar workspace
        assert s.shape == () and float(s) == 0.0


def test_a_result_that_is_not_guarded_is_reported():
    m = stand_in()
    g = Guarded(m)
    x = g.guard(torch.ones(3, 3))
    with pytest.raises(AssertionError, match="not guarded: a result of shape \\(3, 3\\)"):
        with g:
            g.out(m.double_like(x))                                                  # empty_like goes round the proxy
    assert m.torch is torch                                                          # restored on the way out of a failure too


@pytest.mark.parametrize("misalign", [0, 2, 8])
def test_interior_alignment(misalign):
    m = stand_in()
    g = Guarded(m)
    x = g.guard(torch.ones(33, 7, dtype=torch.bfloat16), misalign=misalign)
    assert x.data_ptr() % ALIGN == misalign and x.is_contiguous()
    with g:
        y = g.out(m.double(x))
        assert y.data_ptr() % ALIGN == 0                                             # what the module allocates is always aligned
    assert torch.equal(y, x * 2)


def test_unwritten_reports_offsets_of_a_strided_view():
    t = torch.zeros(4, 6, dtype=torch.int16)
    v = t[:, :4]
    v[2, 1] = PATTERN
    v[3, 3] = PATTERN
    assert _guarded.unwritten(v) == (2, (2 * 6 + 1) * 2, (3 * 6 + 3) * 2 + 1)
    assert _guarded.unwritten(t[:2]) is None
