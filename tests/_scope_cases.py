"""Scope-heterogeneous cases of the reducing kernels (tests/test_scope_cases.py on the CPU, tests/test_scope_kernels_gpu.py on the GPU).

A reduction SCOPE is the set of samples one statistic is taken over: an (image, group) for GroupNorm, a row for LayerNorm, the
LayerNorm-folded linears and ``softmax_rows``, a (batch, head) / a query row for attention, a (batch, pixel, head) for temporal attention.
The parity tests elsewhere draw inputs that are statistically the same in every scope, so statistics taken from the wrong or an
incomplete set of samples move the result by 1 / sqrt(n) only.  Here every scope has its own mean and scale, and the samples inside a
GroupNorm scope carry profiles along H (the last slab differs), along W (the wrapped columns differ) and across the group's channels.

Every family is a ``Fam``: cases, ``build(case, dt, P)`` (seeded host fp32 operands already rounded with ``q16``), ``run(case, d, P, mk,
**variant)`` through the kernel module ``P`` (imagine360_amd.kernels or the stand-ins of tests/_emu_kernels.py), ``ref(case, ops, results)``
(fp64, of the STORED inputs: a producer's output is read back from ``results``), ``scopes`` (tensor -> [scopes, samples]) and
``perturb(case, ops, dt)`` -> [(label, ops', inside)] for the isolation check: ops' differs from ops inside ONE scope (8 x larger, shifted),
``inside(name, tensor)`` marks the result elements of that scope.

Criteria: ``close`` of test_kernel_bounds_gpu.py unchanged, plus ``scoperel`` < 2 TOL (the relative L2 error per scope, denominator
floored as in ``blockrel``); isolation is bit for bit.
"""
import torch
import torch.nn.functional as F

import _emu_kernels as EMU
import _pair_cases as PC
from _pair_cases import Host, emu, emu_gn_partials, gn64, gn_shape  # noqa: F401
from test_kernel_bounds_gpu import close, sdpa64  # noqa: F401
from test_kernels_gpu import TOL, blockrel, q16, rel, rnd  # noqa: F401

GROUPS = 32
BF16, FP16 = torch.bfloat16, torch.float16
DTYPES = [BF16, FP16]
ROOM = 3.0          # the fp64 reference rounded once keeps this much room under every threshold; a mutant trips one by this factor


def gen(seed):
    return torch.Generator().manual_seed(seed)


def grid(n, lo, hi, g):
    """n values covering [lo, hi] evenly, in a seeded order: the span is reached at every n, not only in expectation."""
    return torch.linspace(lo, hi, n)[torch.randperm(n, generator=g)]


def pick_slabs(N, HW):
    """groupnorm.hip's slab count per image (the host restatement the 'last slab' properties and mutant use)."""
    return max(1, min(-(-2048 // N), max(HW // 64, 1), 1024))


# ================================================================================================ criteria
def gn_scopes(t):
    N, H, W, C = t.shape
    return t.reshape(N, H * W, GROUPS, C // GROUPS).permute(0, 2, 1, 3).reshape(N * GROUPS, -1)


def row_scopes(t):
    return t.reshape(-1, t.shape[-1])


def scoperel(out, ref, scopes):
    """max over the reduction scopes of the scope's relative L2 error (denominator floored as in ``blockrel``): a column-shaped scope --
    one group's channels over all pixels -- cannot hide in blockrel's row blocks."""
    a, b = scopes(out.detach().double().cpu()), scopes(ref.detach().double().cpu())
    num, den = (a - b).norm(dim=1), b.norm(dim=1)
    return float((num / den.clamp_min(1e-30 + 1e-3 * float(den.max()))).max())


def measures(out, ref, scopes, rows=32):
    return dict(rel=rel(out, ref), blockrel=blockrel(out, ref, rows), scoperel=scoperel(out, ref, scopes))


def factor(m, dt):
    """The largest measure / threshold ratio (>= 1: a miss; NaN counts as infinite)."""
    thr = dict(rel=TOL[dt], blockrel=2 * TOL[dt], scoperel=2 * TOL[dt])
    return max((m[k] / thr[k]) if m[k] == m[k] else float("inf") for k in thr)


def passes(out, ref, dt, scopes, rows=32):
    return bool(close(out, ref, dt, rows=rows) and scoperel(out, ref, scopes) < 2 * TOL[dt])


def other(t, dt, shift):
    """Other finite data for a scope: 8 x larger, shifted, and in reversed order along the first dimension -- a normalisation is
    invariant under an affine map of its whole scope, so scaling and shifting alone would leave the scope's own result unchanged."""
    return q16(8 * t.flip(0) + shift, dt)


def bits(t):
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Fam:
    def __init__(self, name, cases, build, run, ref, scopes, perturb, outputs=("out",), place=None, variants=({},), wants_pack=False):
        self.name, self.cases, self.build_, self.run, self.ref, self.scopes, self.perturb = name, cases, build, run, ref, scopes, perturb
        self.outputs = tuple(outputs)          # the results the isolation check compares (the judged ones are the reference's keys)
        self.place = place or (lambda ops, mk: {k: (mk.to(v) if torch.is_tensor(v) else v) for k, v in ops.items()})
        self.variants, self.wants_pack = list(variants), wants_pack

    def build(self, case, dt, P):
        return self.build_(case, dt, P) if self.wants_pack else self.build_(case, dt)


def run_case(fam, case, P, dt, mk=None, ops=None, **variant):
    """(ops, results, refs) of one case through ``P``."""
    mk = mk or Host()
    ops = fam.build(case, dt, P) if ops is None else ops
    results = fam.run(case, fam.place(ops, mk), P, mk, **variant)
    return ops, results, fam.ref(case, ops, results)


def judge(fam, results, refs, dt, round_to=None):
    """{result name: measures} and the worst factor; ``round_to``: round the (fp32 stand-in) results once to that dtype first."""
    ms = {}
    for name, ref in refs.items():
        out = results[name]
        assert tuple(out.shape) == tuple(ref.shape), (name, tuple(out.shape), tuple(ref.shape))
        ms[name] = measures(q16(out, round_to) if round_to is not None else out, ref, fam.scopes)
    return ms, max(factor(m, dt) for m in ms.values())


def isolation(fam, case, ops, results, P, dt, mk_of=Host, **variant):
    """[(label, result name, what)] of the isolation failures: outside the perturbed scope the results must be bit-identical, inside
    they must differ."""
    bad = []
    for label, ops2, inside in fam.perturb(case, ops, dt):
        mk = mk_of()
        res2 = fam.run(case, fam.place(ops2, mk), P, mk, **variant)
        for name in fam.outputs:
            a, b = results[name].detach().cpu(), res2[name].detach().cpu()
            m = inside(name, a)
            assert m.shape == a.shape and bool(m.any()) and not bool(m.all())
            if not torch.isfinite(b.float()).all():
                bad.append((label, name, "non-finite result of the perturbed run"))
            if not torch.equal(bits(a)[~m], bits(b)[~m]):
                n = int((bits(a) != bits(b))[~m].sum())
                bad.append((label, name, f"{n} element(s) outside the scope changed"))
            if torch.equal(bits(a)[m], bits(b)[m]):
                bad.append((label, name, "nothing inside the scope changed (vacuous)"))
    return bad


# ================================================================================================ GroupNorm: the heterogeneous field
RAMP_H = 3.5          # the H profile runs from -RAMP_H (first row) to +RAMP_H (last row): the last slab's mean is off the scope's
PAD_STEP = 5.0        # the outer PAD_COLS columns on each side sit this far above the interior: the wrapped columns' mean is off the scope's
PAD_COLS = 2
MEAN_SPAN = 6.0       # per-scope means over +- MEAN_SPAN within-scope standard deviations (|mean| / std <= 8 keeps var = E[x^2] - mean^2 safe)
SCALE_LOG2 = 1.6      # per-scope scales over 2^+-1.6: 9.2 x


def profiles(H, W):
    t = torch.arange(H, dtype=torch.float32) / max(H - 1, 1)
    rh = RAMP_H * (2 * t - 1)
    rw = torch.zeros(W)
    if W > 2 * PAD_COLS:
        rw[:PAD_COLS] = PAD_STEP
        rw[W - PAD_COLS:] = PAD_STEP
    return rh, rw


def gn_field(N, H, W, C, g):
    """s[n, g] (m[n, g] + noise + c[channel] + r_H(y) + r_W(x)), fp32 [N, H, W, C], unrounded."""
    cpg = C // GROUPS
    rh, rw = profiles(H, W)
    base = torch.randn(N, H, W, C, generator=g) + 0.5 * torch.randn(C, generator=g) + rh[None, :, None, None] + rw[None, None, :, None]
    sigma0 = float(base.std())
    m = grid(N * GROUPS, -MEAN_SPAN * sigma0, MEAN_SPAN * sigma0, g).reshape(N, GROUPS).repeat_interleave(cpg, 1)
    s = (2.0 ** grid(N * GROUPS, -SCALE_LOG2, SCALE_LOG2, g)).reshape(N, GROUPS).repeat_interleave(cpg, 1)
    return (base + m[:, None, None, :]) * s[:, None, None, :]


SRC_K = PC.GN_SRC_K


def gn_producer(N, H, W, C, g, cpg):
    """Operands of a SRC_K -> C producer whose stored output is heterogeneous: src = sc[n] (noise + (m[n] + r_H + r_W) u) with the unit
    vector u = 1 / 8, weight rows gs[group] (noise / 8 + a[c] u) with a[c] in [0.9, 1.1] (``cpg`` channels per group), so that
    y[c] = gs sc[n] (noise' + a[c] (m[n] + r_H + r_W + noise'')) + b[c]: per-image offset and scale from src, per-group row scales and a
    per-channel slope from the weight."""
    rh, rw = profiles(H, W)
    u = torch.full((SRC_K,), SRC_K ** -0.5)
    m = torch.tensor([-14.0, 14.0, 8.0, -8.0])[torch.arange(N) % 4]
    sc = torch.tensor([0.5, 1.0, 2.0, 1.5])[torch.arange(N) % 4]
    prof = m[:, None, None] + rh[None, :, None] + rw[None, None, :]
    src = (torch.randn(N, H, W, SRC_K, generator=g) + prof[..., None] * u) * sc[:, None, None, None]
    groups = -(-C // cpg)
    gs = (2.0 ** grid(groups, -1.5, 1.5, g)).repeat_interleave(cpg)[:C]
    a = 0.9 + 0.2 * torch.rand(C, generator=g)
    w = gs[:, None] * (torch.randn(C, SRC_K, generator=g) * SRC_K ** -0.5 + a[:, None] * u[None, :])
    b = 0.5 * gs * torch.randn(C, generator=g)

    def more(n):
        """n further channels with the statistics of the producer's last group (a plain member that completes a straddling group)."""
        noise = torch.randn(N, H, W, n, generator=g) + (prof + torch.randn(N, H, W, generator=g))[..., None]
        return noise * (gs[-1] * sc)[:, None, None, None]
    return src, w.reshape(C, SRC_K, 1, 1), b, more


def _gn_case(id, n, hw, ch, pad=0, eps=1e-5, silu=True, tag="none", kind="hetero"):
    return dict(id=id, n=n, hw=hw, chans=tuple(ch), pad=pad, eps=eps, silu=silu, tag=tag, kind=kind, form="pair" if len(ch) == 2 else "single")


GN_CASES = [
    # 8 slabs of 64 pixels (9 in the padded apply pass); 40 chunks -> 6 pixel lanes, 16 idle threads
    _gn_case("320-16x32-pad0", 3, "16x32", (320,)), _gn_case("320-16x32-pad2", 3, "16x32", (320,), pad=2),
    # 2 slabs of 65 pixels: slab edges inside a row, pix % W across them
    _gn_case("64-10x13-pad0", 2, "10x13", (64,), silu=False), _gn_case("64-10x13-pad2", 2, "10x13", (64,), pad=2),
    _gn_case("2560-8x16", 2, "8x16", (2560,)),                                   # 2 slabs, two chunk passes (256 + 64 chunks)
    _gn_case("vae-128-9x7", 1, "9x7", (128,), eps=1e-6),                         # the VAE site, one slab
    _gn_case("pair-640+320-16x32", 3, "16x32", (640, 320)),                      # 30 channels per group, group 21 straddles the tensors
    _gn_case("pair-1280+640-8x8", 2, "8x8", (1280, 640), silu=False),            # 60 channels per group, group 21 straddles
    _gn_case("pair-320+320-6x10-pad2", 2, "6x10", (320, 320), pad=2),            # aligned groups
    _gn_case("tagged-320-16x16", 3, "16x16", (320,), tag="linear"),              # the producer's partial sums, one 256-row tile per image
    _gn_case("tagged-first-320+640-16x16", 3, "16x16", (320, 640), tag="first"),  # ... on the first member; group 10 straddles
    _gn_case("scope-of-8", 3, "2x2", (64,), silu=False, kind="small"),           # pins the biased variance
    _gn_case("flat-eps1e-5", 2, "8x16", (64,), kind="flat"), _gn_case("flat-eps1e-6", 2, "8x16", (64,), eps=1e-6, kind="flat"),
    # partial sums from conv2d's epilogue: written from 512 tiles of 256 x 320 on, so gn_shape makes it 512 images (a 1 x 1 convolution)
    dict(_gn_case("tagged-conv2d-320-16x16", 1, "16x16", (320,), tag="conv2d"), ch="320"),
]
GN_MODES = ["partials", "three"]
FLAT_CONST = (1, 5, 0.375)          # (image, group, value) of the exactly constant group of the 'flat' cases


def _seed(case, salt=0):
    return PC._seed_of({k: v for k, v in case.items() if k != "mode"}, 100 + salt)


def gn_build(case, dt):
    g = gen(_seed(case))
    N, H, W = gn_shape(case)
    c1, c2 = (case["chans"] + (0,))[:2]
    C = c1 + c2
    ops = dict(gamma=q16(1 + 0.1 * torch.randn(C, generator=g), dt), beta=q16(0.1 * torch.randn(C, generator=g), dt))
    if case["kind"] == "small":
        cpg = C // GROUPS
        m = grid(N * GROUPS, -2.0, 2.0, g).reshape(N, GROUPS).repeat_interleave(cpg, 1)
        s = (2.0 ** grid(N * GROUPS, -SCALE_LOG2, SCALE_LOG2, g)).reshape(N, GROUPS).repeat_interleave(cpg, 1)
        x = (torch.randn(N, H, W, C, generator=g) + m[:, None, None, :]) * s[:, None, None, :]
    elif case["kind"] == "flat":          # scopes of std 2^-8 and 2^-6 around 0, alternating; one exactly constant group
        cpg = C // GROUPS
        sd = torch.where((torch.arange(N * GROUPS) % 2) == 0, 2.0 ** -8, 2.0 ** -6).reshape(N, GROUPS).repeat_interleave(cpg, 1)
        x = torch.randn(N, H, W, C, generator=g) * sd[:, None, None, :]
        n, gr, v = FLAT_CONST
        x[n, :, :, gr * cpg:(gr + 1) * cpg] = v
    else:
        x = gn_field(N, H, W, C, g)
    if case["tag"] != "none":
        cpg = C // GROUPS
        src, w, b, more = gn_producer(N, H, W, c1, g, cpg)
        ops.update(src_a=q16(src, dt), w_a=q16(w, dt), b_a=q16(b, dt))
        if c2 and c1 % cpg:          # the straddling group stays ONE population: its plain channels continue the producer's statistics
            hi = (c1 // cpg + 1) * cpg
            x[..., c1:hi] = more(hi - c1)
        if c2:
            ops["x_b"] = q16(x[..., c1:], dt).contiguous()
    else:
        ops["x_a"] = q16(x[..., :c1], dt).contiguous()
        if c2:
            ops["x_b"] = q16(x[..., c1:], dt).contiguous()
    return ops


def gn_run(case, d, P, mk, mode="partials"):
    return PC.gn_call(dict(case, mode=mode), d, P, mk)


def gn_ref(case, ops, results):
    return dict(out=PC.gn_ref(case, ops, results)["out"])


def gn_stored(results):
    return torch.cat([results["x_" + n].detach().float().cpu() for n in "ab" if "x_" + n in results], -1)


def gn_group_channels(case, gr):
    cpg = sum(case["chans"]) // GROUPS
    return gr * cpg, (gr + 1) * cpg


def gn_probe_group(case):
    """The group the (image, group) isolation perturbs: the one that straddles the two tensors where there is one; inside the plain
    member where the first is a producer's output (its channels cannot be changed for one image alone)."""
    c1 = case["chans"][0]
    cpg = sum(case["chans"]) // GROUPS
    if case["tag"] == "first":
        return GROUPS - 1
    return c1 // cpg if (len(case["chans"]) == 2 and c1 % cpg) else GROUPS // 2 - 1


def gn_perturb(case, ops, dt):
    N = gn_shape(case)[0]
    n_star = N - 1
    big = lambda t: other(t, dt, 3)          # [H, W, channels] of one image: the rows upside down
    c1 = case["chans"][0]
    out = []
    # one image
    o2 = dict(ops)
    for k in ("x_a", "x_b", "src_a"):
        if k in ops:
            t = ops[k].clone()
            t[n_star] = other(t[n_star], dt, 3 if k != "src_a" else 0.25)
            o2[k] = t
    if N > 1:          # (one image alone: the image is the whole tensor)
        out.append(("image", o2, lambda name, t: _mask(t, lambda m: m[n_star].fill_(True))))
    # one (image, group): a producer's output cannot be changed for one image and group alone
    if case["tag"] in ("none", "first"):
        gr = gn_probe_group(case)
        lo, hi = gn_group_channels(case, gr)
        o3 = dict(ops)
        for k, off, width in (("x_a", 0, c1), ("x_b", c1, sum(case["chans"]) - c1)):
            a, b = max(lo - off, 0), min(hi - off, width)
            if k in ops and a < b:
                t = ops[k].clone()
                t[n_star, :, :, a:b] = big(t[n_star, :, :, a:b])
                o3[k] = t
        out.append(("image-group", o3, lambda name, t: _mask(t, lambda m: m[n_star, :, :, lo:hi].fill_(True))))
    return out


def _mask(t, fill):
    m = torch.zeros(t.shape, dtype=torch.bool)
    fill(m)
    return m


GN = Fam("group_norm", GN_CASES, gn_build, gn_run, gn_ref, gn_scopes, gn_perturb, variants=[dict(mode=m) for m in GN_MODES])


def hetero_report(x, pad=PAD_COLS):
    """Heterogeneity of a STORED tensor [N, H, W, C]: (spread of the scope means / median within-scope std, max |mean| / std,
    min over the scopes of |mean of the outer columns - mean| / std, the same for the last slab or None with one slab)."""
    x = x.double()
    N, H, W, C = x.shape
    cpg = C // GROUPS
    t = x.reshape(N, H * W, GROUPS, cpg)
    mean, std = t.mean(dim=(1, 3)), t.std(dim=(1, 3), unbiased=False)
    cols = torch.zeros(W, dtype=torch.bool)
    cols[:pad] = True
    cols[W - pad:] = True
    pix = cols[None, :].expand(H, W).reshape(-1)
    pad_dev = float(((t[:, pix].mean(dim=(1, 3)) - mean).abs() / std).min()) if W > 2 * pad else None
    S = pick_slabs(N, H * W)
    pps = -(-H * W // S)
    slab_dev = float(((t[:, (S - 1) * pps:].mean(dim=(1, 3)) - mean).abs() / std).min()) if S > 1 else None
    return dict(spread=float(mean.std() / std.median()), ratio=float((mean.abs() / std).max()), pad_dev=pad_dev, slab_dev=slab_dev,
                scale_span=float(std.max() / std.min()))


# ================================================================================================ GroupNorm: defective stand-ins
def gn_stats64(x, gamma, beta, eps, pad=0, mut=None):
    """fp64 (scale, shift) of GroupNorm with ONE defect ``mut`` in how the statistics are gathered; the sums and the sample count stay
    consistent (the mild form of each defect: a mean scaled by a wrong count would show on any off-zero input)."""
    c1 = x[0].shape[-1] if isinstance(x, (tuple, list)) else None
    x = EMU._cat(x)
    N, H, W, C = x.shape
    cpg = C // GROUPS
    wgt = torch.ones(H, W, dtype=torch.float64)
    if pad and mut != "pad_once":
        wgt[:, :pad] = 2
        wgt[:, W - pad:] = 2
    wgt = wgt.reshape(-1)
    if mut == "last_slab":
        S = pick_slabs(N, H * W)
        if S > 1:
            wgt[(S - 1) * -(-H * W // S):] = 0
    xd = x.double().reshape(N, H * W, C)
    s1, s2 = torch.einsum("npc,p->nc", xd, wgt), torch.einsum("npc,p->nc", xd * xd, wgt)
    cnt = torch.full((C,), float(wgt.sum()), dtype=torch.float64)
    if mut == "skip_second" and c1 is not None and c1 % cpg:
        sl = slice(c1, (c1 // cpg + 1) * cpg)
        s1[:, sl], s2[:, sl], cnt[sl] = 0, 0, 0
    group_of = torch.arange(C) // cpg
    # 'late': the sums of group g are gathered over the channels [g cpg + 1, (g + 1) cpg + 1) (the last group wraps to channel 0)
    hot = F.one_hot(((torch.arange(C) - 1) % C) // cpg if mut == "late" else group_of, GROUPS).double()
    g1, g2, gc = s1 @ hot, s2 @ hot, cnt @ hot
    mean = g1 / gc
    var = g2 / gc - mean * mean
    if mut == "unbiased":
        var = var * gc / (gc - 1)
    if mut == "image0":
        mean, var = mean[:1].expand_as(mean), var[:1].expand_as(var)
    if mut == "prev_image":
        mean, var = mean.roll(1, 0), var.roll(1, 0)
    e = {"eps_other": 1e-6 if eps > 5e-6 else 1e-5, "no_eps": 0.0}.get(mut, eps)
    rstd = (var.clamp_min(0) + e).rsqrt()
    scale = rstd[:, group_of] * gamma.double()[None]
    return scale, beta.double()[None] - mean[:, group_of] * scale


def gn_mutant(mut):
    def group_norm(x, gamma, beta, groups, eps, silu=False, pad=0):
        scale, shift = gn_stats64(x, gamma, beta, eps, pad, mut)
        return EMU.group_norm_apply(x, scale.float(), shift.float(), silu, pad)
    return emu(group_norm=group_norm)


def gn64_mutant(x, gamma, beta, eps, pad, silu, mut):
    """The defective GroupNorm + act wholly in fp64 (what the motivation test rounds once)."""
    scale, shift = gn_stats64(x, gamma, beta, eps, pad, mut)
    y = PC.OG.pad_pano(x.double().permute(0, 3, 1, 2), pad).permute(0, 2, 3, 1) * scale[:, None, None, :] + shift[:, None, None, :]
    return F.silu(y) if silu else y


# ================================================================================================ rows
ROW_LOG2 = 2.2          # per-row scales over 2^+-2.2: 21 x
LOW_STD = 2.0 ** -8
ROW_CONST = 0.375


def special_rows(M):
    """(rows of std 2^-8 around 0, the exactly constant row)."""
    return (sorted({1, M // 2, M - 1} - {3}) if M >= 16 else [1]), 3


def rows_field(M, C, g, slices=False):
    x = torch.randn(M, C, generator=g) + grid(M, -3.0, 3.0, g)[:, None]
    if slices and C % 160 == 0:          # a per-160-column-slice offset inside the row
        x = x + (1.5 * torch.randn(M, C // 160, generator=g)).repeat_interleave(160, 1)
    x = x * (2.0 ** grid(M, -ROW_LOG2, ROW_LOG2, g))[:, None]
    low, const = special_rows(M)
    x[low] = LOW_STD * torch.randn(len(low), C, generator=g)
    x[const] = ROW_CONST
    return x


def row_probe(M):
    """The row the isolation perturbs: an ordinary one (the last of the first 256-row tile where there is one)."""
    return 255 if M > 256 else 2


def _row_mask(r):
    return lambda name, t: _mask(t, lambda m: m.reshape(-1, t.shape[-1])[r].fill_(True))


# ------------------------------------------------------------------------------------------------ layer_norm
LN_CASES = [dict(id=f"C{C}-rows{rows}", C=C, rows=rows) for C in (320, 640, 64, 1280, 2048) for rows in (5, 1003)]
LN_EPS = 1e-5
LN_PRE, LN_POST, LN_POST_DIV = 7, 5, 3


def ln_build(case, dt):
    g = gen(_seed(case, 1))
    C, M = case["C"], case["rows"]
    r = lambda *s, scale=1.0: q16(torch.randn(*s, generator=g) * scale, dt)
    return dict(x=q16(rows_field(M, C, g), dt), gamma=q16(1 + 0.1 * torch.randn(C, generator=g), dt), beta=r(C, scale=0.1),
                pre=r(LN_PRE, C), post=r(LN_POST, C))


def ln_run(case, d, P, mk):
    f = lambda **kw: P.layer_norm(d["x"], d["gamma"], d["beta"], LN_EPS, **kw)
    return dict(plain=f(), pre=f(pre=d["pre"]), post=f(post=d["post"], post_div=LN_POST_DIV))


def ln_ref(case, ops, results=None):
    x, C = ops["x"].double(), case["C"]
    r = torch.arange(x.shape[0])
    ln = lambda t: F.layer_norm(t, (C,), ops["gamma"].double(), ops["beta"].double(), LN_EPS)
    return dict(plain=ln(x), pre=ln(x + ops["pre"].double()[r % LN_PRE]), post=ln(x) + ops["post"].double()[(r // LN_POST_DIV) % LN_POST])


def ln_perturb(case, ops, dt):
    r = row_probe(case["rows"])
    x = ops["x"].clone()
    x[r] = other(x[r], dt, 3)
    return [("row", dict(ops, x=x), _row_mask(r))]


LN = Fam("layer_norm", LN_CASES, ln_build, ln_run, ln_ref, row_scopes, ln_perturb, outputs=("plain", "pre", "post"))


def ln_mutant(mut):
    def layer_norm(x, gamma, beta, eps=1e-5, pre=None, post=None, post_div=1):
        C = x.shape[-1]
        t = x.reshape(-1, C).double()
        r = torch.arange(t.shape[0])
        if pre is not None:
            t = t + pre.double()[r % pre.shape[0]]
        mean, var = t.mean(1), t.var(1, unbiased=False)
        if mut == "swap01":          # rows 0 and 1 of every group of 8 rows (one wave of the packed kernel) swap statistics
            p = r.clone()
            first = (r % 8 == 0) & (r + 1 < t.shape[0])
            p[first] += 1
            p[(r % 8 == 1)] -= 1
            mean, var = mean[p], var[p]
        e = {"eps_other": 1e-6, "no_eps": 0.0}.get(mut, eps)
        y = (t - mean[:, None]) * (var + e).rsqrt()[:, None] * gamma.double() + beta.double()
        if post is not None:
            y = y + post.double()[(r // post_div) % post.shape[0]]
        return y.float().reshape(x.shape)
    return emu(layer_norm=layer_norm)


# ------------------------------------------------------------------------------------------------ the LayerNorm-folded linears
FOLD_M = "441"          # 3 x 128 + 57 rows: 256-row tiles 0 and 1, the second ragged


def _fold_case(entry, k, n, tab="none", res="none"):
    return dict(id=f"{entry}-K{k}-N{n}" + ("" if tab == "none" else "-tab"), entry=entry, k=k, n=n, tab=tab, res=res, bias=True, row_stats=False,
                gn_hw="none", m=FOLD_M)


FOLD_CASES = (
    [_fold_case("linear_ln", k, 320) for k in (320, 640, 1280)] + [_fold_case("linear_ln", 320, 960, tab="c2/1"), _fold_case("linear_ln", 640, 320, tab="plain/1")]
    + [_fold_case("linear_geglu_ln", k, 640) for k in (320, 640, 1280)]
    # ff_fused_ln takes K = N = 320 only (kernels.py FF_FUSED_SHAPE, asserted in _ff_fused; ff_fused.hip's launcher refuses the rest)
    + [_fold_case("ff_fused_ln", 320, 320, res="alias")])


def fold_build(case, dt, P):
    """PC.lin_build's weights, folding and tables; the rows are the STORED output of a 64 -> K ``linear(row_stats=True)`` whose residual
    is the heterogeneous field (the special rows get a zero src row: the stored row IS the residual row)."""
    ops = PC.lin_build(case, dt, P)
    g = gen(_seed(case, 2))
    M, k = ops.pop("x").shape
    ops.pop("stats")
    src = 0.25 * torch.randn(M, SRC_K, generator=g)
    low, const = special_rows(M)
    src[low + [const]] = 0
    ops.update(hres=q16(rows_field(M, k, g, slices=True), dt), src=q16(src, dt), wsrc=q16(torch.randn(k, SRC_K, 1, 1, generator=g) * SRC_K ** -0.5, dt))
    return ops


def fold_run(case, d, P, mk):
    h, st = P.linear(d["src"], P.pack_conv_weight(d["wsrc"]), case["k"], res=d["hres"], row_stats=True)
    return dict(out=PC.lin_call(case, dict(d, x=h, stats=st), P, mk)["out"], h=h, stats=st)


def fold_ref(case, ops, results):
    return dict(out=PC.lin_ref(case, dict(ops, x=results["h"].detach().float().cpu()))["out"])


def fold_perturb(case, ops, dt):
    r = row_probe(int(case["m"]))
    hres = ops["hres"].clone()
    hres[r] = other(hres[r], dt, 0.5)
    return [("row", dict(ops, hres=hres), _row_mask(r))]


FOLD = Fam("folded_ln", FOLD_CASES, fold_build, fold_run, fold_ref, row_scopes, fold_perturb, outputs=("out", "h"), place=PC.lin_place, wants_pack=True)


def fold_mutant(mut):
    assert mut == "slice_twice"          # the first 160-column slice's sums stand in for the second's

    def twice(stats):
        s = stats.clone()
        s[:, 1] = s[:, 0]
        return s
    return emu(linear_ln=lambda x, wp, c1, c2, stats, *a, **k: EMU.linear_ln(x, wp, c1, c2, twice(stats), *a, **k),
               linear_geglu_ln=lambda x, wp, c1, c2, stats, *a, **k: EMU.linear_geglu_ln(x, wp, c1, c2, twice(stats), *a, **k))


# ------------------------------------------------------------------------------------------------ softmax_rows
SM_CASES = [dict(id="37x1000", rows=37, cols=1000, scale=3.0)]          # rows offset by up to +- 30 under scale 3: exp overflows without the maximum
SM_EQUAL = 3


def sm_build(case, dt):
    g = gen(_seed(case, 3))
    M, C = case["rows"], case["cols"]
    x = grid(M, -30.0, 30.0, g)[:, None] + torch.randn(M, C, generator=g) * (2.0 ** grid(M, -2.0, 2.0, g))[:, None]
    x[SM_EQUAL] = ROW_CONST
    return dict(x=q16(x, dt))


def sm_run(case, d, P, mk):
    return dict(out=P.softmax_rows(d["x"], case["scale"]))


def sm_ref(case, ops, results=None):
    return dict(out=torch.softmax(ops["x"].double() * case["scale"], -1))


def sm_perturb(case, ops, dt):
    r = 17
    x = ops["x"].clone()
    x[r] = other(x[r], dt, 3)
    return [("row", dict(ops, x=x), _row_mask(r))]


SM = Fam("softmax_rows", SM_CASES, sm_build, sm_run, sm_ref, row_scopes, sm_perturb)


def sm_mutant(mut):
    assert mut == "leak"          # the last 8 columns of the row above enter the row's sum

    def softmax_rows(x, scale=1.0, out=None):
        t = x.double() * scale
        mx = t.max(1, keepdim=True).values
        e = (t - mx).exp()
        leak = (t.roll(1, 0)[:, -8:] - mx).exp().sum(1)
        leak[0] = 0
        return (e / (e.sum(1) + leak)[:, None]).float()
    return emu(softmax_rows=softmax_rows)


FAMILIES = {f.name: f for f in (GN, LN, FOLD, SM)}

# {mutant: (family, stand-ins with the defect)}
MUTANTS = {
    "image0": (GN, lambda: gn_mutant("image0")), "prev_image": (GN, lambda: gn_mutant("prev_image")), "last_slab": (GN, lambda: gn_mutant("last_slab")),
    "pad_once": (GN, lambda: gn_mutant("pad_once")), "late": (GN, lambda: gn_mutant("late")), "skip_second": (GN, lambda: gn_mutant("skip_second")),
    "unbiased": (GN, lambda: gn_mutant("unbiased")), "eps_other": (GN, lambda: gn_mutant("eps_other")), "no_eps": (GN, lambda: gn_mutant("no_eps")),
    "ln_eps_other": (LN, lambda: ln_mutant("eps_other")), "ln_no_eps": (LN, lambda: ln_mutant("no_eps")), "ln_swap01": (LN, lambda: ln_mutant("swap01")),
    "slice_twice": (FOLD, lambda: fold_mutant("slice_twice")), "softmax_leak": (SM, lambda: sm_mutant("leak")),
}


# ================================================================================================ attention: isolation only
ATTN_HEADS = 2
ATTN_SHAPE = dict(B=2, nq=100, nk=77)          # ragged query blocks (3 x 32 + 4) and keys
ATTN_PROBE = dict(b=1, head=1, row=97)


def attn_build(d, dt, two=False):
    g = gen(1000 + d + int(two))
    C = ATTN_HEADS * d
    B, nq, nk = ATTN_SHAPE["B"], ATTN_SHAPE["nq"], ATTN_SHAPE["nk"]
    r = lambda *s, scale=1.0: q16(torch.randn(*s, generator=g) * scale, dt)
    ops = dict(q=r(B, nq, C, scale=0.5), k=r(B, nk, C), v=r(B, nk, C))
    if two:
        ops.update(k2=r(B, 4, C), v2=r(B, 4, C))
    return ops


def attn_run(ops, P, mk, d):
    dd = {k: mk.to(v) for k, v in ops.items()}
    if "k2" in ops:
        return P.attention2(dd["q"], dd["k"], dd["v"], dd["k2"], dd["v2"], ATTN_HEADS)
    return P.attention(dd["q"], dd["k"], dd["v"], ATTN_HEADS)


def attn_perturb(ops, d, dt):
    """[(label, ops', mask of the result elements of the scope)]: one (batch, head)'s keys and values; one query row."""
    b, h, row = ATTN_PROBE["b"], ATTN_PROBE["head"], ATTN_PROBE["row"]
    cols = slice(h * d, (h + 1) * d)
    kv = dict(ops)
    for n in ("k", "v", "k2", "v2"):
        if n in ops:
            t = ops[n].clone()
            t[b, :, cols] = other(t[b, :, cols], dt, 0.5)
            kv[n] = t
    q = ops["q"].clone()
    q[b, row] = other(q[b, row], dt, 0.5)
    shape = ops["q"].shape
    m_kv, m_q = torch.zeros(shape, dtype=torch.bool), torch.zeros(shape, dtype=torch.bool)
    m_kv[b, :, cols] = True
    m_q[b, row] = True
    return [("batch-head keys and values", kv, m_kv), ("query row", dict(ops, q=q), m_q)]


TATTN_SHAPE = dict(B=2, Fr=16, P=9, heads=8, d=40)          # the motion modules' head shape; all eight heads of a pixel share one workgroup
TATTN_PROBE = dict(b=1, p=7, head=5)


def tattn_build(dt):
    s = TATTN_SHAPE
    return dict(qkv=q16(torch.randn(s["B"] * s["Fr"] * s["P"], 3 * s["heads"] * s["d"], generator=gen(1100)), dt))


def tattn_run(ops, P, mk, frame_major):
    s = TATTN_SHAPE
    return P.temporal_attention(mk.to(ops["qkv"]), s["B"], s["Fr"], s["P"], s["heads"], frame_major=frame_major)


def tattn_perturb(ops, dt, frame_major):
    s = TATTN_SHAPE
    B, Fr, P, C, d = s["B"], s["Fr"], s["P"], s["heads"] * s["d"], s["d"]
    b, p, h = TATTN_PROBE["b"], TATTN_PROBE["p"], TATTN_PROBE["head"]
    f = torch.arange(Fr)
    rows = (f * B + b) * P + p if frame_major else (b * Fr + f) * P + p
    qkv = ops["qkv"].clone()
    for third in range(3):
        c = slice(third * C + h * d, third * C + (h + 1) * d)
        qkv[rows, c] = other(qkv[rows, c], dt, 0.5)
    m = torch.zeros(B * Fr * P, C, dtype=torch.bool)
    m[rows, h * d:(h + 1) * d] = True
    return [("batch-pixel-head", dict(qkv=qkv), m)]


def outside_same_inside_differs(a, b, m):
    a, b = a.detach().cpu(), b.detach().cpu()
    bad = []
    if not torch.isfinite(b.float()).all():
        bad.append("non-finite result of the perturbed run")
    if not torch.equal(bits(a)[~m], bits(b)[~m]):
        bad.append(f"{int((bits(a) != bits(b))[~m].sum())} element(s) outside the scope changed")
    if torch.equal(bits(a)[m], bits(b)[m]):
        bad.append("nothing inside the scope changed (vacuous)")
    return bad
