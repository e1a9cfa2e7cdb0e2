"""One fp64 restatement of every sampler-step entry point (csrc/sampler_step.hip) and the per-element rounding bound its kernels and
their torch stand-ins are held to.  Used by test_step_rounding.py (CPU tier: the stand-ins, the mutants) and test_step_rounding_gpu.py
(the kernels).

Every function takes the 16-bit inputs (and the fp32 history) and returns, in float64,
    ref   the formula, and
    T     its running-error majorant: the same formula with every input and coefficient replaced by its absolute value and every
          subtraction turned into an addition.  The clamp of x0 leaves T unclamped (|clamp(a)| <= |a|); through the windows T goes
          through the weighted blend divided by the weight sum; the guidance rescale multiplies it by |r|.
The multistep functions return (ref, T, x0, X0): x0 is what the fp32 history has to hold afterwards, X0 its majorant.

The bound.  Each fp32 operation a (op) b returns (a (op) b)(1 + d), |d| <= u = 2^-24 (the fast-math reciprocal: 2 u), so by the usual
running-error induction the fp32 value v of a chain of n such operations differs from the exact one by at most n u T (1 + O(u)),
whatever the order in which a fast-math compiler evaluates or contracts them -- T is invariant under reassociation.  Then v is rounded
once to the 16-bit type, to nearest:
    |out - ref| <= ulp_dt(ref) / 2 + (K u + extra) T,      K = 32.
The operations on the longest path (ring / line windows + rescale + epsilon prediction + clamp + clipped model output + noise), each
counted once although an fma would save some; rounding a fp64 coefficient to fp32 counts as one:
    guided prediction  c - u, g -> fp32, g *, u +                                                   4
    blend              w *, two additions (three covering windows), reciprocal of the sum (2), *    6
    rescale            r *  (the error of r itself is `extra`)                                      1
    x0                 sb -> fp32, sb * m, x -, sa -> fp32, reciprocal (2), *                       7
    e from x0          sa * x0, x -, sb reciprocal (2), *                                           5
    update             sap -> fp32, sap * x0, dir -> fp32, dir * e, +, sigma -> fp32, sigma * z, +   8
                                                                                                    31  <= K = 32
The multistep path ends after x0 (18) with cx, c0, c1 -> fp32, three products and two additions: 26.  The history is the fp32 x0 itself,
never rounded to 16 bits: |hist - x0| <= 16 u X0, with or without the rescale (test_guidance_rescale_gpu.py observes r within 1e-8 .. 5e-8 of fp64, below u);
the worst-case count of x0 above is 18 for the windows with rescale and epsilon prediction and 11 for the plain kernel, and the observed
errors (independent roundings) stay several times below either.
`extra` is the relative error allowed to the rescale factor r (FACTOR_TOL of test_guidance_rescale_gpu.py): r multiplies m, and
|r| M is part of every term of T that m reaches.

Sharpness.  The check is only as sharp as the half-ulp term: `within_rounding` also asserts that the slop term (K u + extra) T exceeds
ulp / 2 on at most SHARP_SHARE of the elements, so that a test case cannot hide an error behind a large T.  The share is a property of
the inputs and of the formula alone, not of what is tested: it is the probability that |ref| < T / kappa with kappa = (ulp / 2 |ref|) /
(K u + extra), i.e. the density of ref / T at zero divided by kappa.  1 % is the limit in bf16.  fp16 has three more significant bits,
its kappa is 8 times smaller and the same inputs give 8 times the share, so its limit is 8 %: on predictions scaled by 0.25 (a guided
x0 on both sides of +-1, which the clamp needs) the epsilon-prediction modes subtract sap sb / sa m from dir m, T is several times the
standard deviation of ref and the fp16 share reaches 6 %; no choice of such inputs brings it below 1 %.  Where the slop term is the
larger one the bound is still at most 2 (K u + extra) T."""
import torch

K_OPS = 32
K_HIST = 16
U32 = 2.0 ** -24
MANT_BITS = {torch.bfloat16: 8, torch.float16: 11}          # significant bits
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14}        # exponent of the smallest normal number
SHARP_SHARE = {torch.bfloat16: 0.01, torch.float16: 0.08}      # see "Sharpness" above


# ------------------------------------------------------------------------------------------------ pieces
def guided(u, c, g):
    """(m, M) of m = u + g (c - u)."""
    u, c = u.double(), c.double()
    return u + g * (c - u), u.abs() + abs(g) * (c.abs() + u.abs())


def blends(preds, sample, starts, weights, g, ring=False):
    """(m, M, cb): the per-frame blends over the windows (slot k ascending) of the guided prediction, of its majorant and of the text
    half, each sum of w[j] * value divided by the sum of w[j]; window k covers the frames starts[k] + j, j < L, modulo F on a ring."""
    fd = sample.dim() - 3
    F, L = sample.shape[fd], preds.shape[fd + 1]
    assert preds.shape[1] == 2 and len(starts) == preds.shape[0] and len(weights) == L <= F
    shape = [1] * sample.dim()
    shape[fd] = L
    wv = weights.double().reshape(shape)
    m, M, cb, ws = (torch.zeros(sample.shape, dtype=torch.float64) for _ in range(4))
    for k, s in enumerate(int(v) for v in starts):
        assert 0 <= s < F and (ring or s + L <= F)
        idx = (s + torch.arange(L)) % F
        mk, Mk = guided(preds[k, 0:1], preds[k, 1:2], g)
        m.index_add_(fd, idx, wv * mk)
        M.index_add_(fd, idx, wv.abs() * Mk)
        cb.index_add_(fd, idx, wv * preds[k, 1:2].double())
        ws.index_add_(fd, idx, wv.expand_as(mk).contiguous())
    assert (ws > 0).all(), "a frame is covered by no window"
    return m / ws, M / ws, cb / ws


def factor(m, c, phi):
    """r = phi std(c) / std(m) + 1 - phi (correction 1, over everything) as a host float; 1 for phi == 0."""
    return 1.0 if phi == 0.0 else float(phi * c.double().std() / m.double().std() + (1.0 - phi))


def _x0(m, M, x, X, mode, sa, sb):
    pred = mode & 3
    assert pred != 3
    if pred == 0:
        x0, X0 = (x - sb * m) / sa, (X + abs(sb) * M) / abs(sa)
    elif pred == 1:
        x0, X0 = sa * x - sb * m, abs(sa) * X + abs(sb) * M
    else:
        x0, X0 = m, M
    if mode & 4:
        x0 = x0.clamp(-1, 1)
    return x0, X0


def ddim_on(m, M, x, z, mode, coefs):
    """(ref, T) of DDIMScheduler.step on the guided prediction m with majorant M; z None: no noise term."""
    _, sa, sb, sap, direction, sigma = (float(v) for v in coefs)
    x = x.double()
    X = x.abs()
    x0, X0 = _x0(m, M, x, X, mode, sa, sb)
    pred = mode & 3
    e, E = (sa * m + sb * x, abs(sa) * M + abs(sb) * X) if pred == 1 else (m, M)
    if mode & 8:
        e, E = (x - sa * x0) / sb, (X + abs(sa) * X0) / abs(sb)
    ref, T = sap * x0 + direction * e, abs(sap) * X0 + abs(direction) * E
    if z is not None:
        ref, T = ref + sigma * z.double(), T + abs(sigma) * z.double().abs()
    return ref, T


def multistep_on(m, M, x, h, mode, coefs):
    """(ref, T, x0, X0) of the DPM-Solver++ 2M update cx x + c0 x0 + c1 h on the guided prediction m; h is read only when c1 != 0."""
    _, sa, sb, cx, c0, c1 = (float(v) for v in coefs)
    assert not mode & 8
    x = x.double()
    X = x.abs()
    x0, X0 = _x0(m, M, x, X, mode, sa, sb)
    ref, T = cx * x + c0 * x0, abs(cx) * X + abs(c0) * X0
    if c1 != 0.0:
        h = h.double().reshape(x.shape)
        ref, T = ref + c1 * h, T + abs(c1) * h.abs()
    return ref, T, x0, X0


def _rescaled(m, M, c, phi):
    r = factor(m, c, phi)
    return m * r, M * abs(r)


# ------------------------------------------------------------------------------------------------ the entry points
def cfg_ddim_update(uncond, cond, sample, guidance, cx, cv):
    m, M = guided(uncond, cond, guidance)
    x = sample.double()
    return cx * x + cv * m, abs(cx) * x.abs() + abs(cv) * M


def cfg_ddim_step(uncond, cond, sample, noise, mode, coefs, rescale=0.0):
    m, M = guided(uncond, cond, coefs[0])
    m, M = _rescaled(m, M, cond, rescale)
    return ddim_on(m, M, sample, noise, mode, coefs)


def cfg_ddim_step_windows(preds, sample, noise, starts, weights, mode, coefs, rescale=0.0, ring=False):
    m, M, cb = blends(preds, sample, starts, weights, coefs[0], ring)
    m, M = _rescaled(m, M, cb, rescale)
    return ddim_on(m, M, sample, noise, mode, coefs)


def cfg_multistep_step(uncond, cond, sample, hist, mode, coefs, rescale=0.0):
    m, M = guided(uncond, cond, coefs[0])
    m, M = _rescaled(m, M, cond, rescale)
    return multistep_on(m, M, sample, hist, mode, coefs)


def cfg_multistep_step_windows(preds, sample, hist, starts, weights, mode, coefs, rescale=0.0, ring=False):
    m, M, cb = blends(preds, sample, starts, weights, coefs[0], ring)
    m, M = _rescaled(m, M, cb, rescale)
    return multistep_on(m, M, sample, hist, mode, coefs)


# ------------------------------------------------------------------------------------------------ the bound
def ulp(ref, dt):
    """Spacing of the 16-bit type ``dt`` at |ref| (float64): 2^(e - p + 1) for 2^e <= |ref| < 2^(e + 1), e no smaller than the
    type's least normal exponent (the subnormal floor)."""
    _, e = torch.frexp(ref.abs())                                   # |ref| = f 2^e, f in [0.5, 1)
    e = torch.where(ref == 0, torch.full_like(e, MIN_EXP[dt]), e - 1).clamp_min(MIN_EXP[dt])
    return torch.ldexp(torch.ones_like(ref), e - (MANT_BITS[dt] - 1))


class Outside(AssertionError):
    """An element outside the bound; ``worst``: the largest |err| / bound (inf for a NaN)."""
    def __init__(self, message, worst):
        super().__init__(message)
        self.worst = worst


def _worst(ratio, bad, what):
    flat = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio).reshape(-1)
    i = int(flat.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
    return float(flat[i]), f"{what}: worst |err| / bound {float(flat[i]):.4g} at {idx}, {float(bad.double().mean()) * 100:.3g} % of {ratio.numel()} elements outside the bound"


def within_rounding(out, ref, T, dt, extra=0.0, what="", sharp=True):
    """Assert |out - ref| <= ulp_dt(ref) / 2 + (K u + extra) T for every element (a NaN anywhere fails).  Returns the worst ratio
    |err| / bound.  ``sharp``: also assert that the slop term exceeds the half-ulp term on at most SHARP_SHARE[dt] of the elements."""
    assert out.dtype == dt and out.shape == ref.shape, (out.dtype, out.shape, ref.shape)
    half, slop = 0.5 * ulp(ref, dt), (K_OPS * U32 + extra) * T
    if sharp:
        share = float((slop > half).double().mean())
        assert share <= SHARP_SHARE[dt], f"{what}: the slop term exceeds half an ulp on {share * 100:.3g} % of the elements: the case is not sharp"
    ratio = (out.detach().cpu().double() - ref).abs() / (half + slop)
    bad = ~(ratio <= 1.0)
    if bad.any():
        raise Outside(*_worst(ratio, bad, what)[::-1])
    return float(ratio.max())


def history_within(hist, x0, X0, what=""):
    """Assert |hist - x0| <= 16 u X0 for every element of the fp32 history (a NaN anywhere fails); returns the worst ratio."""
    assert hist.dtype == torch.float32 and hist.numel() == x0.numel()
    bound = K_HIST * U32 * X0
    ratio = (hist.detach().cpu().double().reshape(x0.shape) - x0).abs() / bound.clamp_min(1e-300)
    bad = ~(ratio <= 1.0)
    if bad.any():
        raise Outside(*_worst(ratio, bad, what + " history")[::-1])
    return float(ratio.max())
