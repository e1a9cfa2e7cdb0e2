"""Host logic of the fused feed-forward route (layers.FeedForward -> kernels.ff_fused / ff_fused_ln), without a GPU: which
(K, inner, N, M, residual, device, knob) take it, and that the stand-in path of the CPU tier (tests/_emu_kernels.py under ROUTE_ON_CPU)
still issues today's pair of launches and never asks the library for the knob."""
import pytest
import torch

import _emu_kernels as E
from imagine360_amd import kernels, layers


def test_route_truth_table(monkeypatch):
    monkeypatch.setattr(layers, "ROUTE_MIN_TOKENS", 65536)
    take = layers.ff_fused_route
    assert kernels.FF_FUSED_SHAPE == (320, 1280)
    assert take(True, 320, 1280, 320, 655360, True, True)
    assert take(True, 320, 1280, 320, 65536, True, True)             # the threshold itself
    assert not take(True, 320, 1280, 320, 65535, True, True)         # below it the GEMMs are hipBLASLt's
    assert not take(False, 320, 1280, 320, 655360, True, True)       # CPU tensors (the stand-ins of the CPU tier)
    assert not take(True, 320, 1280, 320, 655360, False, True)       # no residual
    assert not take(True, 320, 1280, 320, 655360, True, False)       # knob ff_fused = 0
    assert not take(True, 640, 2560, 640, 163840, True, True)        # level 1: OUT 128 x 640 does not fit the registers
    assert not take(True, 1280, 5120, 1280, 655360, True, True)
    assert not take(True, 320, 2560, 320, 655360, True, True)        # another multiplier
    assert not take(True, 320, 1280, 640, 655360, True, True)        # dim_out != dim
    monkeypatch.setattr(layers, "ROUTE_MIN_TOKENS", 0)
    assert take(True, 320, 1280, 320, 1, True, True)


def test_knob_is_registered():
    assert kernels.KNOBS["ff_fused"] == 27 and len(set(kernels.KNOBS.values())) == len(kernels.KNOBS)
    src = open(kernels.__file__.replace("kernels.py", "csrc/abi.cpp")).read()
    assert '{im360::KNOB_FF_FUSED, "IM360_FF_FUSED", 1}' in src      # default on; tools/ab_step.py reads the default from here
    assert "KNOB_FF_FUSED = 27" in open(kernels.__file__.replace("kernels.py", "csrc/prof.h")).read()


@pytest.mark.parametrize("with_stats", [False, True])
def test_stand_in_path_is_unchanged(monkeypatch, with_stats):
    """Under ROUTE_ON_CPU a 320-channel FeedForward with a residual issues the GEGLU launch and the Linear-with-residual launch of
    before (never the fused one, never a knob query), and computes LayerNorm -> GEGLU -> Linear + residual."""
    def boom(*a, **k):
        raise AssertionError("the fused launch / the knob must not be reached on the CPU tier")
    for name in ("ff_fused", "ff_fused_ln", "tuning_get"):
        monkeypatch.setattr(kernels, name, boom)
    torch.manual_seed(5)
    M, C = 96, 320
    ff = layers.FeedForward(C).float()
    norm = torch.nn.LayerNorm(C).float()
    x = torch.randn(M, C) + 0.3
    xs = x.reshape(M, C // kernels.ROW_SLICE, kernels.ROW_SLICE)
    stats = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], dim=-1).contiguous() if with_stats else None
    calls = []
    with torch.no_grad(), E.patched_kernels(), E.routed_gemms(0):
        for name in ("linear_geglu", "linear_geglu_ln", "conv2d", "layer_norm"):
            real = getattr(kernels, name)
            monkeypatch.setattr(kernels, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
        assert not ff.takes_fused(x, x)
        y = ff(x, residual=x, ln=norm, stats=stats)
        monkeypatch.undo()
    assert calls == (["linear_geglu_ln", "conv2d"] if with_stats else ["layer_norm", "linear_geglu", "conv2d"]), calls
    h = ff.net[0].proj(norm(x))
    ref = ff.net[2](h[:, :4 * C] * torch.nn.functional.gelu(h[:, 4 * C:])) + x
    assert torch.allclose(y, ref, atol=2e-4, rtol=2e-4), float((y - ref).abs().max())
