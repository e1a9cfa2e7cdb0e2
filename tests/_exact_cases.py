"""Inputs whose correct kernel result is known EXACTLY, and the exact results (pure torch on the host; the CPU self-checks are in
tests/test_exact_cases.py, the launches in tests/test_exact_kernels_gpu.py).

Two methods.
  * Integer GEMM / convolution: inputs, weights, bias, time embedding and residual are small integers.  Every partial sum is an integer
    below 2^24, so ANY fp32 accumulation order gives the same bits and the expected output is RNE(exact integer).  The "exact" cases keep
    every output representable in the 16-bit type by construction (a fixed number of non-zero +-1 weights per output channel); the
    "round" cases make the outputs large enough that many of them are exact ties or non-representable, which pins the rounding mode.
  * Attention as selection: queries and keys are signed two-hot codes amp (s_a e_a + s_b e_b).  A query scores 2 amp^2 against the keys
    that carry its code and at most amp^2 against any other, and amp is large enough that every other weight underflows to 0 in fp32:
    the expected output is a gather of V (a mean over 2 or 4 rows where codes are duplicated), built by indexing, never by a softmax.

Rounding points of the conv / GEMM epilogue that the references model (imagine360_amd/csrc/conv3x3.hip, tile_epilogue): with Cout % 8 == 0 the tile is
transposed through LDS as 16-bit rows -- ``pack2<T>(acc + bias + temb)`` -- and the residual is added to the UNPACKED 16-bit value and packed
again (conv3x3.hip:464-473: ``unpack_lo<T>(o.x) + unpack_lo<T>(w.x)`` ... ``pack2<T>``), i.e. RNE(RNE(conv + bias + temb) + res).  With
Cout % 8 != 0 the fragments are stored directly and rounded once (conv3x3.hip:585-589)."""
import math

import torch
import torch.nn.functional as F

LOG2E = 1.4426950408889634
BF16, FP16 = torch.bfloat16, torch.float16
DTYPES = [BF16, FP16]
EXACT_MAX = {BF16: 256, FP16: 2048}          # every integer of at most this magnitude is representable
FP32_EXACT = 2 ** 24
UNDERFLOW_GAP = 160.0                       # log2 units: exp2(-160) is below the smallest fp32 subnormal (2^-149)
ROW_SLICE = 160


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, lo, hi, g):
    """iid integers in [lo, hi] as float32."""
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def rne(t, dt):
    """Round once, to nearest even, to the 16-bit type (torch's conversion); ``t`` holds integers below 2^24, exact in float32."""
    return t.float().to(dt)


SIGNIFICAND = {BF16: 8, FP16: 11}          # bits, the implicit one included


def spacing(t, dt):
    """Distance between neighbouring values of the 16-bit type at the magnitude of ``t`` (normal range), float64."""
    _, e = torch.frexp(t.double().abs().clamp_min(1e-30))          # |t| = m 2^e, m in [0.5, 1)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - SIGNIFICAND[dt]).double())


def truncate(t, dt):
    """Round toward zero to the 16-bit type (a wrong epilogue)."""
    t = t.double()
    sp = spacing(t, dt)
    return (torch.sign(t) * torch.floor(t.abs() / sp) * sp).float().to(dt)


def shares(pre, dt):
    """(share of exact ties, share of non-representable non-ties) of the exact values ``pre`` under the 16-bit type."""
    p = pre.double().abs()
    r = p / spacing(p, dt)
    frac = r - torch.floor(r)
    tie = frac == 0.5
    return float(tie.double().mean()), float(((frac != 0) & ~tie).double().mean())


def pad_w(x, p):
    """Circular pad along the last axis."""
    return torch.cat([x[..., -p:], x, x[..., :p]], dim=-1) if p else x


# ================================================================================================ integer convolution / GEMM
def sparse_weight(cout, k, nnz, g):
    """[cout, k] with exactly ``nnz`` entries of +-1 per row at random places."""
    w = torch.zeros(cout, k)
    idx = torch.rand(cout, k, generator=g).argsort(dim=1)[:, :nnz]
    w.scatter_(1, idx, torch.randint(0, 2, (cout, nnz), generator=g).float() * 2 - 1)
    return w


def round_amplitude(k, dt):
    """Integer amplitude a of x and w in [-a, a] for the rounding cases: the smallest with std(y) = sqrt(k) a (a + 1) / 3 at least twice
    the last exactly-representable magnitude, so that the ties' binade and the binades above it both hold a large share of the outputs."""
    a = 1
    while math.sqrt(k) * a * (a + 1) / 3 < 2.0 * EXACT_MAX[dt]:
        a += 1
    return a


class ConvCase:
    """One integer convolution with its exact result.  kind "exact": x in [-2, 2], ``nnz`` weights of +-1 per output channel, so that
    |conv| <= 2 nnz and |y| <= limit by construction; kind "round": x and w iid in [-a, a] (round_amplitude).  bias / temb in [-4, 4],
    res in [-8, 8]."""

    def __init__(self, dt, kind, N, H, W, Cin, Cout, taps=9, stride=1, up=False, wrap=False, x_off=0, temb_fr=0, res=False, bias=True,
                 seed=0, limit=None):
        self.dt, self.kind = dt, kind
        self.N, self.H, self.W, self.Cin, self.Cout, self.taps = N, H, W, Cin, Cout, taps
        self.stride, self.up, self.wrap, self.x_off = stride, up, wrap, x_off
        g = gen(seed)
        kk = 3 if taps == 9 else 1
        K = taps * Cin
        extra = (4 if bias else 0) + (4 if temb_fr else 0) + (8 if res else 0)
        if kind == "exact":
            limit = limit or min(EXACT_MAX.values())
            self.limit = limit
            nnz = min((limit - extra) // 2, K // 2)
            self.xmax, self.wmax, self.nnz = 2, 1, nnz
            w = sparse_weight(Cout, K, nnz, g).reshape(Cout, Cin, kk, kk)
            x = ints((N, H, W + 2 * x_off, Cin), -2, 2, g)
            self.acc_bound = 2 * nnz
        else:
            a = round_amplitude(K, dt)
            self.xmax, self.wmax, self.nnz = a, a, K
            w = ints((Cout, Cin, kk, kk), -a, a, g)
            x = ints((N, H, W + 2 * x_off, Cin), -a, a, g)
            self.acc_bound = K * a * a
        self.x, self.w = x, w
        self.bias = ints((Cout,), -4, 4, g) if bias else None
        self.temb_fr = temb_fr
        self.temb = ints((N // temb_fr, Cout), -4, 4, g) if temb_fr else None
        ho, wo = self.out_hw()
        self.res = ints((N, ho, wo, Cout), -8, 8, g) if res else None
        self.bound = self.acc_bound + extra          # of every partial sum of conv + bias + temb + res

    def out_hw(self):
        hc, wc = (2 * self.H, 2 * self.W) if self.up else (self.H, self.W)
        return hc // self.stride, wc // self.stride

    def _conv(self, x, w):
        """The convolution in the dtype of x / w ([N, H, W(+2 x_off), Cin] channels-last in, [N, Ho, Wo, Cout] out)."""
        xr = x.permute(0, 3, 1, 2)
        if self.taps == 1:
            return F.conv2d(xr, w).permute(0, 2, 3, 1)
        if self.x_off:                       # the input is already W + 2 x_off wide: output column j reads input column j + x_off
            y = F.conv2d(xr, w, padding=1)[..., self.x_off:self.x_off + self.W]
        elif self.up:
            xr = F.interpolate(pad_w(xr, 1) if self.wrap else xr, scale_factor=2.0, mode="nearest")
            y = F.conv2d(xr, w, padding=1)
            y = y[..., 2:-2] if self.wrap else y
        elif self.stride == 2:
            y = F.conv2d(pad_w(xr, 2), w, stride=2, padding=1)[..., 1:-1] if self.wrap else F.conv2d(xr, w, stride=2, padding=1)
        else:
            y = F.conv2d(F.pad(pad_w(xr, 1), (0, 0, 1, 1)), w) if self.wrap else F.conv2d(xr, w, padding=1)
        return y.permute(0, 2, 3, 1)

    def pre(self, wide=torch.float64, x=None, w=None):
        """conv + bias + temb, exact (float64) or through the fp32 operator."""
        y = self._conv((self.x if x is None else x).to(wide), (self.w if w is None else w).to(wide))
        if self.bias is not None:
            y = y + self.bias.to(wide)
        if self.temb is not None:
            y = y + self.temb.to(wide).repeat_interleave(self.temb_fr, 0)[:, None, None, :]
        return y

    def rounds_before_residual(self):
        """The LDS-transposed epilogue (Cout % 8 == 0) rounds to 16 bits before it adds the residual; the direct-store one rounds once."""
        return self.Cout % 8 == 0

    def finish(self, pre, rnd=rne):
        """The epilogue's roundings (module docstring)."""
        if self.res is None:
            return rnd(pre, self.dt)
        if self.rounds_before_residual():
            return rnd(rnd(pre, self.dt).double() + self.res.double(), self.dt)
        return rnd(pre.double() + self.res.double(), self.dt)

    def expected(self, wide=torch.float32):
        return self.finish(self.pre(wide))


def conv_gpu_args(case, K):
    """(x, packed weight, keyword arguments) of ``K.conv2d`` for a ConvCase, on the GPU."""
    dt = case.dt
    d = lambda t: None if t is None else t.to(dt).cuda()
    kw = dict(bias=d(case.bias), stride=case.stride, up=case.up, wrap=case.wrap)
    if case.x_off:
        kw.update(x_off=case.x_off, wout=case.W)
    if case.temb is not None:
        kw.update(temb=d(case.temb), imgs_per_temb=case.temb_fr)
    if case.res is not None:
        kw.update(res=d(case.res))
    return d(case.x), K.pack_conv_weight(d(case.w)), kw


class LinearCase:
    """Integer token-major Linear x [M, K] W^T [K, n] + bias (+ res), same two kinds as ConvCase; the "exact" kind keeps |y| <= 256 so
    that a 160-column slice's sum of squares stays below 2^24 (160 * 256^2 < 2^24): the row statistics are exact in fp32 too."""

    def __init__(self, dt, kind, M, Kd, n, res=True, seed=0, limit=256):
        self.dt, self.kind, self.M, self.Kd, self.n = dt, kind, M, Kd, n
        g = gen(seed)
        extra = 4 + (8 if res else 0)
        if kind == "exact":
            nnz = min((limit - extra) // 2, Kd // 2)
            self.w = sparse_weight(n, Kd, nnz, g)
            self.x = ints((M, Kd), -2, 2, g)
            self.acc_bound, self.limit = 2 * nnz, limit
        else:
            a = round_amplitude(Kd, dt)
            self.w, self.x = ints((n, Kd), -a, a, g), ints((M, Kd), -a, a, g)
            self.acc_bound = Kd * a * a
        self.bias = ints((n,), -4, 4, g)
        self.res = ints((M, n), -8, 8, g) if res else None
        self.bound = self.acc_bound + extra

    def pre(self, wide=torch.float64, skip_chunk=None):
        x, w = self.x.to(wide), self.w.to(wide)
        if skip_chunk is not None:
            x = x.clone()
            x[:, 64 * skip_chunk:64 * skip_chunk + 64] = 0
        return x @ w.t() + self.bias.to(wide)

    def rounds_before_residual(self):
        return True          # n % 320 == 0: the LDS-transposed epilogue

    def finish(self, pre, rnd=rne):
        if self.res is None:
            return rnd(pre, self.dt)
        return rnd(rnd(pre, self.dt).double() + self.res.double(), self.dt)

    def expected(self, wide=torch.float32):
        return self.finish(self.pre(wide))


def row_stats(y):
    """(sum, sum of squares) per row and 160-column slice of the STORED 16-bit values, float64 [M, n / 160, 2]."""
    M, n = y.shape
    t = y.double().reshape(M, n // ROW_SLICE, ROW_SLICE)
    return torch.stack([t.sum(-1), (t * t).sum(-1)], dim=-1)


# ================================================================================================ attention as exact selection
def amplitude(d, scale=None):
    """The smallest power of two amp with amp^2 scale log2(e) >= UNDERFLOW_GAP."""
    scale = d ** -0.5 if scale is None else scale
    amp = 1
    while amp * amp * scale * LOG2E < UNDERFLOW_GAP:
        amp *= 2
    return amp


def n_codes(d):
    return 2 * d * (d - 1)          # 4 C(d, 2)


def code_rows(ids, d, amp):
    """Signed two-hot codes [..., d] of the code numbers ``ids`` (any shape, values below n_codes(d)): code (pair, signs) =
    amp (s_a e_a + s_b e_b) with a < b."""
    pairs = torch.combinations(torch.arange(d), 2)                                 # [C(d, 2), 2]
    ids = torch.as_tensor(ids)
    pr, sg = ids // 4, ids % 4
    a, b = pairs[pr, 0], pairs[pr, 1]
    sa, sb = 1.0 - 2.0 * (sg // 2).float(), 1.0 - 2.0 * (sg % 2).float()
    out = torch.zeros(ids.shape + (d,))
    out.scatter_(-1, a.unsqueeze(-1), (amp * sa).unsqueeze(-1))
    out.scatter_(-1, b.unsqueeze(-1), (amp * sb).unsqueeze(-1))
    return out


def edge_keys(Nk):
    """The keys a selection must reach: the first, the last, and both sides of every 32-key boundary (64-key ones included)."""
    ks = {0, Nk - 1}
    for b in range(32, Nk, 32):
        ks.update((b - 1, b))
    return sorted(ks)


def make_sel(Nq, Nk, g, offset=0):
    """Key selected by each query, meeting the edge conditions of the test plan.  The edge keys are dealt out in turn (continuing at
    ``offset`` from one (batch, head) slice to the next) over the even queries -- over all of them where there are more edge keys than
    even queries -- the other queries take random keys; then query 0 takes the first key and the last query the last key (with more than
    64 keys these two share a code, AttnCase), query 1 the first key of the last tile and the second-to-last query the last key of the
    first tile.  Returns (sel [Nq], slots used)."""
    edges = edge_keys(Nk)
    sel = torch.randint(0, Nk, (Nq,), generator=g)
    fixed = {0, Nq - 1} | ({1, Nq - 2} if Nq >= 4 else set())
    step = 2 if len(edges) <= Nq // 2 - 2 else 1
    slots = [i for i in range(0, Nq, step) if i not in fixed]
    for n, i in enumerate(slots):
        sel[i] = edges[(offset + n) % len(edges)]
    sel[0] = 0
    sel[Nq - 1] = Nk - 1
    if Nq >= 4:
        sel[1] = (Nk - 1) - (Nk - 1) % 64          # first key of the last tile
        sel[Nq - 2] = min(63, Nk - 1)              # last key of the first tile
    return sel, len(slots)


def make_sels(n, Nq, Nk, g):
    out, off = [], 0
    for _ in range(n):
        s, used = make_sel(Nq, Nk, g, off)
        out.append(s)
        off += used
    return torch.stack(out)


def sel_properties(sel, Nq, Nk, full=True):
    """The five edge properties of a selection [..., Nq] -> dict of booleans (per property, over the union of all leading slices)."""
    s = sel.reshape(-1, Nq)
    seen = set(s.flatten().tolist())
    last_tile0 = (Nk - 1) - (Nk - 1) % 64
    props = {"last_key": Nk - 1 in seen, "first_key": 0 in seen,
             "max_in_last_tile": bool((s >= last_tile0).any()), "max_in_first_tile": bool((s < 64).any()),
             "last_query": all(int(k) in edge_keys(Nk) for k in s[:, Nq - 1])}          # the last query (of a ragged block) takes an edge key
    if full:
        props["boundaries"] = all(k in seen for k in edge_keys(Nk))
    return props


class AttnCase:
    """q [B, Nq, H d], k / v [B / kv_group, Nk, H d] for ``K.attention`` with a known gather as the result.  Per (key batch, head) the keys
    carry distinct random codes, except ``dups`` groups of 2 or 4 keys that share one; query (b, h, i) carries the code of key
    sel[b, h, i], so its output is the mean of the V rows of that key's group.  V holds integers in [-vmax, vmax]; rows of
    duplicated keys in [-vmax / 4, vmax / 4] so that their sums stay below 256 (a mean of 2 or 4 of them is then representable in bf16)."""

    def __init__(self, B, H, Nq, Nk, d, kv_group=1, scale=None, dups=True, vmax=128, seed=0, suppress=False):
        assert Nk <= n_codes(d)
        self.B, self.H, self.Nq, self.Nk, self.d, self.kv_group = B, H, Nq, Nk, d, kv_group
        self.scale = d ** -0.5 if scale is None else scale
        self.amp = amplitude(d, self.scale)
        g = gen(seed)
        Bk = B // kv_group
        # group id of every key: identity, then a few duplicate groups (key j joins the group of key `to`)
        grp = torch.arange(Nk).repeat(Bk, H, 1)
        if suppress:            # "bias as selection": EVERY selected key has a twin carrying the same code, which the bias suppresses
            dups = False
        self.sel = make_sels(B * H, Nq, Nk, g).reshape(B, H, Nq)
        if dups and Nk >= 16:             # groups of 2 and 4 keys rooted at keys some query selects, and the pair (first key, last key) across all the tiles
            for bk in range(Bk):
                for h in range(H):
                    chosen = [k for k in self.sel[bk * kv_group, h].unique().tolist() if 0 < k < Nk - 1]
                    roots = [chosen[i] for i in torch.randperm(len(chosen), generator=g).tolist()][:min(4, Nk // 8) + min(2, Nk // 16)]
                    spare = [k for k in (1 + torch.randperm(Nk - 2, generator=g)).tolist() if k not in roots]
                    for n, r in enumerate(roots):
                        for _ in range(3 if n < min(2, Nk // 16) else 1):          # the first roots head quadruples, the others pairs
                            grp[bk, h, spare.pop()] = r
                    if Nk > 64:
                        grp[bk, h, Nk - 1] = 0
        self.grp = grp
        codes = torch.stack([torch.stack([torch.randperm(n_codes(d), generator=g)[:Nk] for _ in range(H)]) for _ in range(Bk)])   # [Bk, H, Nk]
        key_code = torch.gather(codes, 2, grp)
        kb = torch.arange(B) // kv_group
        q_code = torch.gather(key_code[kb], 2, self.sel)
        self.q = code_rows(q_code, d, self.amp).permute(0, 2, 1, 3).reshape(B, Nq, H * d)
        self.k = code_rows(key_code, d, self.amp).permute(0, 2, 1, 3).reshape(Bk, Nk, H * d)
        v = ints((Bk, H, Nk, d), -vmax, vmax, g)
        size = torch.zeros(Bk, H, Nk).scatter_add_(2, grp, torch.ones(Bk, H, Nk))
        multi = torch.gather(size, 2, grp) > 1
        small = ints((Bk, H, Nk, d), -(vmax // 4), vmax // 4, g)
        v = torch.where(multi[..., None], small, v)
        self.v4 = v
        self.v = v.permute(0, 2, 1, 3).reshape(Bk, Nk, H * d)
        self.bias = None
        if suppress:
            self._suppress(g)

    def _suppress(self, g):
        """Bias as selection: ONE code per key pair (j, twin(j)) shared by all (batch, head) -- the bias [Nq, Nk] is shared by them too;
        query i carries the code of key sel[i], and bias[i, twin(sel[i])] = -B removes the twin: the output is row sel[i] alone."""
        B, H, Nq, Nk, d = self.B, self.H, self.Nq, self.Nk, self.d
        Bk = B // self.kv_group
        assert Nk % 2 == 0
        half = Nk // 2
        twin = (torch.arange(Nk) + half) % Nk
        codes = torch.randperm(n_codes(d), generator=g)[:half]
        key_code = torch.cat([codes, codes]).repeat(Bk, H, 1)
        sel = make_sel(Nq, Nk, g)[0]
        self.sel = sel.repeat(B, H, 1)
        self.grp = torch.arange(Nk).repeat(Bk, H, 1)
        kb = torch.arange(B) // self.kv_group
        q_code = torch.gather(key_code[kb], 2, self.sel)
        self.q = code_rows(q_code, d, self.amp).permute(0, 2, 1, 3).reshape(B, Nq, H * d)
        self.k = code_rows(key_code, d, self.amp).permute(0, 2, 1, 3).reshape(Bk, Nk, H * d)
        self.v4 = ints((Bk, H, Nk, d), -128, 128, g)
        self.v = self.v4.permute(0, 2, 1, 3).reshape(Bk, Nk, H * d)
        self.bias_mag = 256.0                                 # 256 log2(e) = 369 log2 units, representable in bf16 and fp16
        self.bias = torch.zeros(Nq, Nk)
        self.bias[torch.arange(Nq), twin[sel]] = -self.bias_mag
        self.bias_alt = torch.zeros(Nq, Nk)                   # the alternate mask suppresses the selected key instead: the twin's row comes out
        self.bias_alt[torch.arange(Nq), sel] = -self.bias_mag
        self.twin = twin

    def weights(self):
        """[B, H, Nq, Nk] selection weights by index arithmetic: 1 / (group size) on the keys of the selected key's group."""
        kb = torch.arange(self.B) // self.kv_group
        grp = self.grp[kb]                                                                  # [B, H, Nk]
        hit = grp[:, :, None, :] == torch.gather(grp, 2, self.sel)[..., None]             # [B, H, Nq, Nk]
        if self.bias is not None:
            hit = torch.zeros_like(hit).scatter_(3, self.sel[..., None], True)
        return hit.double() / hit.double().sum(-1, keepdim=True)

    def expected(self, dt, alt=False):
        """out [B, Nq, H d] in the 16-bit type: the gather (mean over a duplicate group), by indexing."""
        kb = torch.arange(self.B) // self.kv_group
        if self.bias is not None:
            idx = self.twin[self.sel] if alt else self.sel
            out = torch.gather(self.v4[kb], 2, idx[..., None].expand(-1, -1, -1, self.d)).double()
        else:
            out = self.weights() @ self.v4[kb].double()
        out = out.permute(0, 2, 1, 3).reshape(self.B, self.Nq, self.H * self.d)
        assert torch.equal(out.float().to(dt).double(), out), "the expected rows must be representable"
        return out.float().to(dt)

    def gap_log2(self):
        """Smallest gap, in log2 units, between a query's best logit and its best logit among the keys that must get weight 0
        (bias included), from the built tensors in float64."""
        B, H, Nq, Nk, d = self.B, self.H, self.Nq, self.Nk, self.d
        kb = torch.arange(B) // self.kv_group
        q = self.q.double().reshape(B, Nq, H, d).permute(0, 2, 1, 3)
        k = self.k.double().reshape(-1, Nk, H, d).permute(0, 2, 1, 3)[kb]
        s = q @ k.transpose(-1, -2) * self.scale * LOG2E
        if self.bias is not None:
            s = s + self.bias.double() * LOG2E
        w = self.weights() > 0
        best = torch.where(w, s, torch.full_like(s, -math.inf)).amax(-1)
        worst_sel = torch.where(w, s, torch.full_like(s, math.inf)).amin(-1)
        assert torch.equal(best, worst_sel)                    # the selected keys tie exactly
        rest = torch.where(w, torch.full_like(s, -math.inf), s).amax(-1)
        return float((best - rest).min())


class Attn2Case:
    """``K.attention2``: ONE query attends to two key sets.  Set 1's keys carry distinct codes; key m of set 2 carries the code of set-1 key
    map[m] (map injective, its image holds set 1's edge keys); query i carries the code of set-2 key sel2[i], i.e. of set-1 key
    sel1[i] = map[sel2[i]].  V1, V2 integers in [-64, 64]: V1[sel1] + s2 V2[sel2] is exact for s2 = 1/2."""

    def __init__(self, B, H, Nq, n1, n2, d, kv_group, seed=0):
        assert n2 <= n1 <= n_codes(d)
        self.B, self.H, self.Nq, self.n1, self.n2, self.d, self.kv_group = B, H, Nq, n1, n2, d, kv_group
        self.amp = amplitude(d)
        g = gen(seed)
        Bk = B // kv_group
        codes1 = torch.rand(Bk, H, n_codes(d), generator=g).argsort(dim=-1)[..., :n1]
        e1, e2 = edge_keys(n1), edge_keys(n2)
        maps = []
        for _ in range(Bk * H):
            rest1 = [k for k in torch.randperm(n1, generator=g).tolist() if k not in e1]
            rest2 = [m for m in torch.randperm(n2, generator=g).tolist() if m not in e2]
            m = torch.zeros(n2, dtype=torch.long)
            for pos, key in zip(e2 + rest2, e1 + rest1):          # set 1's edge keys sit behind set 2's edge keys first
                m[pos] = key
            maps.append(m)
        self.map = torch.stack(maps).reshape(Bk, H, n2)
        kb = torch.arange(B) // kv_group
        self.sel2 = make_sels(B * H, Nq, n2, g).reshape(B, H, Nq)
        self.sel1 = torch.gather(self.map[kb], 2, self.sel2)
        lay = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], H * d)
        self.q = lay(code_rows(torch.gather(codes1[kb], 2, self.sel1), d, self.amp))
        self.k1 = lay(code_rows(codes1, d, self.amp))
        self.k2 = lay(code_rows(torch.gather(codes1, 2, self.map), d, self.amp))
        self.v1_4, self.v2_4 = ints((Bk, H, n1, d), -64, 64, g), ints((Bk, H, n2, d), -64, 64, g)
        self.v1, self.v2 = lay(self.v1_4), lay(self.v2_4)

    def expected(self, dt, s2):
        kb = torch.arange(self.B) // self.kv_group
        pick = lambda v, sel: torch.gather(v[kb], 2, sel[..., None].expand(-1, -1, -1, self.d)).double()
        out = (pick(self.v1_4, self.sel1) + s2 * pick(self.v2_4, self.sel2)).permute(0, 2, 1, 3).reshape(self.B, self.Nq, self.H * self.d)
        assert torch.equal(out.float().to(dt).double(), out)
        return out.float().to(dt)


def softmax_attention(q, k, v, H, scale, kv_group=1, wide=torch.float32, drop_last_key=False, swap_keys=None):
    """Plain softmax attention in ``wide`` on the host (the CPU self-check: fp32 lands on the gather; the wrong emulations do not)."""
    B, Nq, C = q.shape
    d = C // H
    kb = torch.arange(B) // kv_group
    sp = lambda t: t.to(wide).reshape(t.shape[0], t.shape[1], H, d).permute(0, 2, 1, 3)
    qq, kk, vv = sp(q), sp(k)[kb], sp(v)[kb]
    if drop_last_key:
        kk, vv = kk[:, :, :-1], vv[:, :, :-1]
    if swap_keys is not None:
        i, j = swap_keys
        vv = vv.clone()
        vv[:, :, [i, j]] = vv[:, :, [j, i]]
    p = torch.softmax(qq @ kk.transpose(-1, -2) * scale, dim=-1)
    return (p @ vv).permute(0, 2, 1, 3).reshape(B, Nq, C)


# ------------------------------------------------------------------------------------------------ temporal attention
def derangements(n_groups, Fr, g):
    """[n_groups, Fr] random cyclic permutations (Sattolo): no frame selects itself."""
    perm = torch.arange(Fr).repeat(n_groups, 1)
    rows = torch.arange(n_groups)
    for i in range(Fr - 1, 0, -1):
        j = (torch.rand(n_groups, generator=g) * i).long().clamp_(max=i - 1)
        a, b = perm[rows, i].clone(), perm[rows, j].clone()
        perm[rows, i], perm[rows, j] = b, a
    return perm


class TemporalCase:
    """qkv [B F P, 3 C] (rows (batch, frame, pixel); ``frame_major``: (frame, batch, pixel)) for ``K.temporal_attention``: per
    (batch, pixel, head) the frames' keys carry distinct codes and frame f's query the code of frame sel[f] != f; V integers in
    [-128, 128]; the result is V[sel]."""

    def __init__(self, B, Fr, P, heads, d, frame_major=False, seed=0, identity=False):
        assert Fr <= n_codes(d)
        self.B, self.Fr, self.P, self.heads, self.d, self.frame_major = B, Fr, P, heads, d, frame_major
        self.amp = amplitude(d)
        g = gen(seed)
        G = B * P * heads
        self.sel = torch.arange(Fr).repeat(G, 1) if identity else derangements(G, Fr, g)          # [G, Fr]
        codes = torch.rand(G, n_codes(d), generator=g).argsort(dim=1)[:, :Fr]
        k = code_rows(codes, d, self.amp)                                                           # [G, Fr, d]
        q = code_rows(torch.gather(codes, 1, self.sel), d, self.amp)
        v = ints((G, Fr, d), -128, 128, g)
        self.q, self.k, self.v = q, k, v
        lay = lambda t: t.reshape(B, P, heads, Fr, d).permute(0, 3, 1, 2, 4).reshape(B, Fr, P, heads * d)     # [B, F, P, C]
        qkv = torch.cat([lay(q), lay(k), lay(v)], dim=-1)
        out = lay(torch.gather(v, 1, self.sel[..., None].expand(-1, -1, d)))
        if frame_major:
            qkv, out = qkv.permute(1, 0, 2, 3), out.permute(1, 0, 2, 3)
        self.qkv = qkv.reshape(B * Fr * P, 3 * heads * d).contiguous()
        self.out = out.reshape(B * Fr * P, heads * d).contiguous()

    def gap_log2(self):
        s = self.q.double() @ self.k.double().transpose(-1, -2) * self.d ** -0.5 * LOG2E           # [G, Fr, Fr]
        best = torch.gather(s, 2, self.sel[..., None]).squeeze(-1)
        rest = s.scatter(2, self.sel[..., None], -math.inf).amax(-1)
        assert torch.equal(best, s.amax(-1))
        return float((best - rest).min())


class WindowsPECase:
    """``K.temporal_attention_windows`` with the selector in the PE rows only: base q and k are zero, pe_qkv's q part at position p is
    the code of position pi(p), its k part the code of position p (codes per head; pi a cyclic permutation of the L positions), its v
    part zero; base v holds integers in [-60, 60].  Window k then returns, at position p, row V[(starts[k] + pi(p)) % F]; with uniform
    weights 1 and every frame in 1, 2 or 4 windows the fusion is a dyadic mean."""

    def __init__(self, B, Fr, P, heads, d, L, starts, ring, seed=0):
        self.B, self.Fr, self.P, self.heads, self.d, self.L, self.starts, self.ring = B, Fr, P, heads, d, L, list(starts), ring
        self.amp = amplitude(d)
        g = gen(seed)
        C = heads * d
        self.pi = derangements(1, L, g)[0]
        codes = torch.rand(heads, n_codes(d), generator=g).argsort(dim=1)[:, :L]                   # [heads, L]
        kpe = code_rows(codes, d, self.amp).permute(1, 0, 2).reshape(L, C)
        qpe = code_rows(codes[:, self.pi], d, self.amp).permute(1, 0, 2).reshape(L, C)
        self.pe = torch.cat([qpe, kpe, torch.zeros(L, C)], dim=-1)
        self.v = ints((B, Fr, P, C), -60, 60, g)
        self.qkv = torch.cat([torch.zeros(B, Fr, P, 2 * C), self.v], dim=-1).reshape(B * Fr * P, 3 * C)
        self.weights = [1.0] * L
        self.cover = [0] * Fr
        for s in self.starts:
            for p in range(L):
                assert ring or s + p < Fr
                self.cover[(s + p) % Fr] += 1

    def expected(self, pi=None, wrap=True):
        """By host index arithmetic, float64 [B F P, C].  ``pi`` / ``wrap`` = False: the wrong emulations (positions that do not restart
        per window; a ring that clamps instead of wrapping)."""
        pi = self.pi if pi is None else pi
        acc = torch.zeros(self.B, self.Fr, self.P, self.v.shape[-1], dtype=torch.float64)
        for s in self.starts:
            for p in range(self.L):
                f = (s + p) % self.Fr
                src = s + int(pi[p])
                src = src % self.Fr if wrap else min(src, self.Fr - 1)
                acc[:, f] += self.v[:, src].double()
        acc = acc / torch.tensor(self.cover, dtype=torch.float64)[None, :, None, None]
        return acc.reshape(self.B * self.Fr * self.P, -1)


# ================================================================================================ GroupNorm statistics
def gn_sums(x, pad):
    """Integer (sum, sum of squares) per image and channel of the circularly W-padded x [N, H, W, C] -> float64 [N, 2, C]; the wrapped
    columns (the first and last ``pad``) count twice (pad = 0: every column once)."""
    xp = x.double()
    if pad > 0:
        xp = torch.cat([xp[:, :, -pad:], xp, xp[:, :, :pad]], dim=2)
    return torch.stack([xp.sum((1, 2)), (xp * xp).sum((1, 2))], dim=1)


def gn_structured_input(N, H, W, C, dt, seed, offset=8.0):
    """Unit-variance noise with the two leftmost and two rightmost columns ``offset`` standard deviations away (+ left, + right): the
    padded statistics, which count exactly those columns twice, differ visibly from the unpadded ones."""
    g = gen(seed)
    x = torch.randn(N, H, W, C, generator=g)
    x[:, :, :2] += offset
    x[:, :, -2:] += offset
    return x.to(dt).float()


def gn_reference(x, gamma, beta, groups, eps, pad, single_weight=False):
    """F.group_norm in float64 of the padded tensor [N, H, W + 2 pad, C] (channels-last in and out).  ``single_weight``: normalise the
    padded tensor with the statistics of the UNPADDED one (wrapped columns weighted once) -- the defect the structured test must catch."""
    xr = x.double().permute(0, 3, 1, 2)
    xp = pad_w(xr, pad)
    if not single_weight:
        return F.group_norm(xp, groups, gamma.double(), beta.double(), eps).permute(0, 2, 3, 1)
    N, C = xr.shape[:2]
    t = xr.reshape(N, groups, -1)
    mu, var = t.mean(-1), t.var(-1, unbiased=False)
    tp = xp.reshape(N, groups, -1)
    y = ((tp - mu[..., None]) / (var[..., None] + eps).sqrt()).reshape(xp.shape)
    return (y * gamma.double()[None, :, None, None] + beta.double()[None, :, None, None]).permute(0, 2, 3, 1)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ================================================================================================ the case tables (shared by the CPU and GPU tests)
KINDS = ["exact", "round"]
RAGGED = dict(N=2, H=9, W=7, Cin=96, Cout=200)                    # 126 pixels, Cin % 64 != 0, Cout % 128 != 0: the 128 x 128 tile, every edge ragged
RAGGED_EVEN = dict(N=2, H=10, W=14, Cin=96, Cout=200)             # stride 2 halves even sizes: 5 x 7 outputs
CONV_FORMS = {
    "plain": dict(RAGGED),
    "wrap": dict(RAGGED, wrap=True),
    "stride2": dict(RAGGED_EVEN, stride=2),
    "stride2_wrap": dict(RAGGED_EVEN, stride=2, wrap=True),
    "up": dict(RAGGED, up=True),
    "up_wrap": dict(RAGGED, up=True, wrap=True),
    "x_off2": dict(RAGGED, x_off=2),
    "1x1": dict(RAGGED, taps=1),
    "temb_res": dict(RAGGED, N=6, temb_fr=3, res=True),
    "temb_res_wrap": dict(RAGGED, N=6, temb_fr=2, res=True, wrap=True),
    "temb_res_1x1": dict(RAGGED, N=6, taps=1, temb_fr=3, res=True),
    "res_cout_not_8": dict(RAGGED, Cout=196, temb_fr=1, res=True),   # Cout % 8 != 0: the direct-store epilogue, ONE rounding
}
SMALL_TILE = {                                                     # knob conv_small 0 / 1: 256 x 64 tiles, Cout % 128 in (0, 64]
    "ragged": dict(N=2, H=9, W=7, Cin=96, Cout=192, temb_fr=1, res=True),
    "wrap_7_tiles": dict(N=3, H=16, W=36, Cin=128, Cout=192, wrap=True, res=True),
    "cout_320": dict(N=3, H=15, W=17, Cin=64, Cout=320),
}
KSPLIT = {                                                         # knob conv_ksplit 2 / 3 / 4 (9 with wrap): 256 x 320 tiles, >= 64 of them
    "64_tiles": dict(N=16, H=32, W=32, Cin=256, Cout=320, temb_fr=4, res=True),
    "ragged_tile": dict(N=17, H=31, W=31, Cin=256, Cout=320, temb_fr=1, res=True),
    "wrap": dict(N=16, H=32, W=32, Cin=256, Cout=320, wrap=True, res=True),
}
BIG_TILE = {                                                       # 256 x 320 tiles unsplit: >= 512 tiles
    "512_tiles": dict(N=128, H=32, W=32, Cin=64, Cout=320, temb_fr=1, res=True),
    "wrap_528_tiles": dict(N=33, H=32, W=64, Cin=128, Cout=640, wrap=True, temb_fr=3, res=True),
}
HALO = {                                                           # knob conv_halo 1 (`make ablate` builds): launches that fill 256 x 320 tiles
    "8_rows_per_tile": dict(N=128, H=32, W=32, Cin=64, Cout=320, temb_fr=4, res=True),
    "x_off2_window": dict(N=16, H=64, W=128, Cin=64, Cout=320, x_off=2, temb_fr=4, res=True),
}
K_ORDER = {                                                        # knobs conv_cm 0 / 1 (chunk-major K order), conv_bk 32
    "below_a_tile": dict(N=3, H=5, W=7, Cin=64, Cout=64, res=True),
    "ragged_3_chunks": dict(N=5, H=30, W=31, Cin=192, Cout=96, res=True),
}
UP2 = {                                                            # K.conv_up2: four sub-pixel 2 x 2 convolutions
    "ragged": dict(N=7, H=5, W=9, Cin=128, Cout=96, up=True),
    "wrap": dict(N=3, H=4, W=6, Cin=64, Cout=64, up=True, wrap=True),
    "512_tiles": dict(N=512, H=16, W=16, Cin=64, Cout=320, up=True),          # 256 x 320 tiles of low-resolution pixels per parity
}
CAT = {"c1_128_c2_64": (3, 9, 7, 128, 64, 200, True), "c1_64_c2_192": (2, 16, 17, 64, 192, 320, False)}          # N, H, W, C1, C2, Cout, res
LINEAR = [(65536 + 77, 64, 320), (65536 + 77, 320, 320), (65536 + 77, 1280, 320), (300, 64, 640), (300, 320, 640), (300, 1280, 640)]

ALL_CONV = {f"{t}/{n}": kw for t, tab in (("forms", CONV_FORMS), ("small", SMALL_TILE), ("ksplit", KSPLIT), ("big", BIG_TILE), ("korder", K_ORDER), ("halo", HALO), ("up2", UP2))
            for n, kw in tab.items()}


def conv_case(name, dt, kind):
    return ConvCase(dt, kind, seed=sum(map(ord, name)) + (7 if kind == "round" else 0), **ALL_CONV[name])


def cat_case(name, dt, kind):
    """conv1x1_cat: a 1 x 1 ConvCase over C1 + C2 channels whose input the kernel takes as the pair (x[..., :C1], x[..., C1:])."""
    N, H, W, C1, C2, Cout, res = CAT[name]
    return ConvCase(dt, kind, N, H, W, C1 + C2, Cout, taps=1, res=res, seed=sum(map(ord, name))), C1


def linear_case(M, Kd, n, dt, kind):
    return LinearCase(dt, kind, M, Kd, n, seed=M + Kd + n)


# attention: (B, H, Nq, Nk, d, kv_group)
ATTN_SHAPES = [(4, 2, nq, nk, d, 2) for d in (64, 32) for nq in (16, 48, 200) for nk in (63, 64, 65, 77, 1288)]
ATTN_PIPE_SHAPES = [(2, 3, 320, 448, 64, 1), (1, 2, 200, 1344, 64, 1)]          # whole 64-key tiles, Nq >= 128: what attn_pipe.hip takes
ATTN_BIAS_SHAPES = [(2, 3, 200, 328, 32, 1), (2, 2, 40, 80, 32, 1), (4, 2, 200, 1288, 32, 2), (2, 2, 100, 136, 64, 1)]
ATTN2_SHAPES = [(4, 64, 77, 64, 2), (4, 320, 77, 64, 2), (6, 40, 77, 64, 3), (6, 320, 65, 33, 2), (6, 20, 65, 33, 2),
                (64, 1024, 77, 64, 16)]          # 8192 query blocks: the twelve-wave ring variant of attn_x 3 (from 3072 up)          # B, Nq, n1, n2, kv_group  (H = 4, d = 64)
TEMPORAL_SHAPES = [(2, 16, 96, 8, 40), (3, 8, 33, 8, 8), (1, 48, 20, 8, 16), (2, 16, 7, 8, 160), (2, 24, 50, 8, 40), (1, 33, 17, 8, 80), (1, 64, 9, 8, 160),
                   (1, 17, 5, 4, 24), (1, 13, 20, 8, 16)]          # B, F, P, heads, d
# windows: (B, F, P, heads, d, L, starts, ring); uniform weights, every frame in 1, 2 or 4 windows
WINDOW_SHAPES = [(2, 32, 33, 8, 40, 16, (0, 8, 16), False),               # coverage 1 / 2
                 (1, 32, 9, 8, 40, 16, (0, 8, 16, 24), True),             # ring, coverage 2, the last window wraps
                 (1, 32, 5, 4, 24, 16, (0, 4, 8, 12, 16, 20, 24, 28), True),      # ring, coverage 4
                 (3, 20, 7, 8, 8, 8, (0, 4, 8, 12), False),               # coverage 1 / 2, d = 8
                 (1, 64, 9, 8, 160, 16, (0, 16, 32, 48), False),          # the LDS limit, coverage 1
                 (1, 12, 5, 8, 16, 5, (0, 5, 7), False)]                  # L no multiple of 4; frames 7 .. 9 twice
GN_PARTIAL_SHAPES = [(3, 8, 16, 64, 0), (3, 8, 16, 64, 2), (2, 6, 10, 320, 2), (2, 6, 10, 320, 0), (1, 64, 128, 320, 2)]          # N, H, W, C, pad
GN_STRUCTURED = [(2, 6, 10, 320, 0), (2, 16, 32, 320, 0), (2, 6, 10, 320, 320), (3, 8, 16, 64, 64)]          # N, H, W, C1, C2 (pad = 2)


def attn_case(shape, suppress=False, vmax=128):
    B, H, Nq, Nk, d, group = shape
    return AttnCase(B, H, Nq, Nk, d, kv_group=group, seed=Nq * 7 + Nk * 3 + d, suppress=suppress, vmax=vmax)
