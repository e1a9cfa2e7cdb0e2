"""What the pipeline tests of ``guidance_interval`` share (test_guidance_interval.py on emulated kernels, test_guidance_interval_gpu.py on
the MI355X): a recorder of every model forward of a run -- batch size, the two predictions -- of the start latents and of the variance
noises, and the recomputation of every step of an eager run from those records with the GUIDED step of the scheduler: (u, c) on a
guided step, (c, c) on an unguided one.  The traced latents must come out bit for bit."""
import contextlib

import torch

from imagine360_amd import pipeline as P

INTERVAL = (0.2, 0.6)                    # 4 steps (timesteps 751, 501, 251, 1): unguided, guided, guided, unguided
KINDS = [False, True, True, False]
G = 7.5


class Record:
    def __init__(self):
        self.forwards, self.noises, self.start = [], [], None

    def batches(self):
        return [f[0] for f in self.forwards]


@contextlib.contextmanager
def recording(mv, monkeypatch):
    """Hooks ``mv`` (MultiViewBaseModel), ``pipeline.variance_noise`` and ``AnimationPipeline.init_noise`` for the runs inside."""
    rec = Record()

    def hook(module, args, kwargs, output):
        pers, pano = output
        rec.forwards.append((kwargs["pano_latent"].shape[0], pano.clone(), pers.clone(), module._ip_noise_half))
    handle = mv.register_forward_hook(hook, with_kwargs=True)
    real_noise, real_init = P.variance_noise, P.AnimationPipeline.init_noise

    def noise(*a, **k):
        z = real_noise(*a, **k)
        rec.noises.append(z.clone())
        return z

    def init_noise(self, *a, **k):
        out = real_init(self, *a, **k)
        rec.start = tuple(t.clone() for t in out)
        return out
    monkeypatch.setattr(P, "variance_noise", noise)
    monkeypatch.setattr(P.AnimationPipeline, "init_noise", init_noise)
    try:
        yield rec
    finally:
        handle.remove()
        monkeypatch.setattr(P, "variance_noise", real_noise)
        monkeypatch.setattr(P.AnimationPipeline, "init_noise", real_init)


def recompute_trace(sch, rec, steps, kinds, eta=0.0, plan=None):
    """The panorama latent after every step of one eager run from pure noise, recomputed from ``rec`` with ``sch.fused_cfg_step``
    (``plan``: ``fused_cfg_step_windows``) at guidance 7.5: the unguided steps' single prediction in both places."""
    nW = 1 if plan is None else len(plan)
    assert len(rec.forwards) == len(steps) * nW and rec.start is not None
    x = rec.start[0].clone()
    hist = dict(history=sch.new_history(x)) if hasattr(sch, "new_history") else {}
    out = []
    for i, (t, guided) in enumerate(zip(steps, kinds)):
        fw = rec.forwards[i * nW:(i + 1) * nW]
        assert all(f[0] == (2 if guided else 1) for f in fw), (i, [f[0] for f in fw])
        assert all(f[3] == (None if guided else (1, 2)) for f in fw)
        pairs = [f[1].to(x.dtype) if guided else torch.cat([f[1], f[1]]).to(x.dtype) for f in fw]
        kw = dict(eta=eta, noise=rec.noises[2 * i]) if eta > 0 else {}
        if plan is None:
            x = sch.fused_cfg_step(pairs[0][0:1], pairs[0][1:2], G, t, x, **kw, **hist)
        else:
            x = sch.fused_cfg_step_windows(torch.stack(pairs), plan.starts_dev, plan.weights, G, t, x, ring=plan.loop, **kw, **hist)
        out.append(x)
    return out
