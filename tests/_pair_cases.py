"""Family tables of the pairwise parity sweep (tests/test_pair_cases.py on the CPU, tests/test_kernel_pairs_gpu.py on the GPU).

Every family is a ``Family``: ordered factors, NAMED constraints (name, predicate, reason citing the wrapper / entry-point line that
forbids the combination), seeds (the production call sites, first in the list), and four functions

    build(case, dt)            -> ops: host fp32 tensors already rounded to the 16-bit dtype ``dt`` (seeded generators)
    call(case, d, P, mk)       -> results: runs the case through the kernel module ``P`` (imagine360_amd.kernels or the plain-torch
                                  stand-ins of tests/_emu_kernels.py) on the placed operands ``d``; ``mk`` places tensors (``Host`` here,
                                  guard bands on the GPU)
    ref(case, ops, results)    -> {result name: fp64 CPU reference}, written plainly (F.conv2d on pad_pano / unpad_pano, sdpa64,
                                  F.group_norm, F.linear)
    optional(case)             -> names of the optional operands the case carries (``without`` drops one from ``ops``)

Shapes are the smallest at which the addressed edge exists.
"""
import hashlib
import json
import types

import torch
import torch.nn.functional as F

import _emu_kernels as EMU
from _pairwise import cover, legal_from, legal_pairs, uncovered  # noqa: F401
from im360_oracle import geometry as OG
from test_kernel_bounds_gpu import close, sdpa64  # noqa: F401
from test_kernels_gpu import TOL, blockrel, q16, rel, rnd  # noqa: F401

GN_SUM_BOUND = 256 * 2.0 ** -24          # any-order fp32 summation of the 256 terms of a slab: |fl(sum) - sum| <= (n - 1) u sum|t|
ROW_SUM_BOUND = 160 * 2.0 ** -24         # ... of the 160 columns of a row-statistics slice


class Host:
    """Places operands for a CPU run: fp32 copies (strided where asked), NaN-filled destinations."""

    def to(self, t, strides=None):
        if strides is None:
            return t.clone()
        o = torch.empty_strided(t.shape, strides, dtype=t.dtype)
        o.copy_(t)
        return o

    to32 = to

    def empty(self, shape, strides=None):
        o = torch.empty(shape) if strides is None else torch.empty_strided(shape, strides)
        return o.fill_(float("nan"))


class Family:
    def __init__(self, name, factors, constraints, seeds, build, call, ref, optional=lambda case: (), f=1.0, rows=32, rng_seed=0, cost=None):
        self.name, self.factors, self.constraints, self.seeds = name, factors, constraints, seeds
        self.build, self.call, self.ref, self.optional, self.f, self.rows = build, call, ref, optional, f, rows
        self.legal = legal_from(constraints)
        self._cases = None
        self.rng_seed, self.cost = rng_seed, cost
        self.wants_pack = False          # build(case, dt, P): the builder takes the packing functions of the module under test

    @property
    def cases(self):
        if self._cases is None:
            self._cases = cover(self.factors, self.legal, self.seeds, self.rng_seed, self.cost)
        return self._cases

    def core(self, case):
        return {n: case[n] for n in self.factors}

    def case_id(self, case):
        return "-".join(f"{n}={_short(case[n])}" for n in self.factors)

    def digest(self):
        return hashlib.sha256(json.dumps([self.core(c) for c in self.cases], sort_keys=True).encode()).hexdigest()[:16]

    def place(self, ops, mk):
        return {k: (mk.to(v) if torch.is_tensor(v) else v) for k, v in ops.items()}


def _short(v):
    return {True: "y", False: "n"}.get(v, v) if isinstance(v, bool) else v


def without(ops, name):
    """``ops`` with one optional operand dropped (a scale: set to 1)."""
    o = dict(ops)
    o[name] = 1.0 if name in ("out_scale", "scale2") else None
    return o


def seeded(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *shape, scale=1.0, shift=0.0: torch.randn(*shape, generator=g) * scale + shift


def _seed_of(case, salt=0):
    return int(hashlib.sha256((repr(sorted(case.items(), key=repr)) + str(salt)).encode()).hexdigest()[:7], 16)


# ================================================================================================ conv2d
CONV_FACTORS = {
    "taps": [1, 9],
    "geom": ["s1", "s2", "up", "pre", "vae"],       # stride 1; stride 2; up; pre-padded x_off = 2, wout = W; x_off = y_off = 1 stride 2
    "wrap": [False, True],
    "bias": [False, True],
    "temb": ["none", "t1", "t3"],                   # imgs_per_temb 1 / 3
    "res": [False, True],
    "gn": [False, True],
    "cin": [32, 64, 96, 128, 320],
    "cout": [4, 64, 200, 320, 640],
    # 128 x 128 tiles under 64 tiles: one image under 256 pixels / a ragged last tile (297 = 2 x 128 + 41) / several 16-pixel images
    # per tile; the K-split rule (64 tiles of 256 x 320 in 4 parts); the 256 x 320 tile from 512 tiles
    "launch": ["one", "ragged", "many", "ksplit", "big"],
}
KSPLIT_PARTS = 4          # ksplit_plan's rule at 64 tiles and Cin / 64 = 5 chunks: 4 parts cost 0.28 rounds against 0.4875 unsplit

CONV_CONSTRAINTS = [
    ("taps1_is_plain", lambda c: c["taps"] == 9 or (c["geom"] == "s1" and not c["wrap"]),
     "kernels.py:598 conv2d is '3x3 pad 1 or 1x1'; the 1 x 1 call sites (unet3d.py:96, layers.py:165) pass no wrap / x_off / stride / up"),
    ("offsets_exclude_wrap", lambda c: not (c["wrap"] and c["geom"] in ("pre", "vae")),
     "unet3d.py:97 / vae.py:75: x_off addresses columns that are IN the tensor, no call site wraps them too"),
    ("gn_needs_the_big_tile", lambda c: not c["gn"] or (c["launch"] == "big" and c["geom"] != "up"),
     "kernels.py:613-615 and conv3x3.hip:1361-1362,1375: im360_conv_gn_slabs > 0 (>= 512 tiles of 256 x 320, whole 256-pixel slabs) and not up"),
    ("big_tile_shape", lambda c: c["launch"] != "big" or (c["cin"] == 64 and c["cout"] % 320 == 0),
     "conv3x3.hip:1313 takes the 256 x 320 tile for Cout % 320 == 0, Cin % 64 == 0; Cin = 64 keeps the CPU reference at seconds"),
    ("ksplit_shape", lambda c: c["launch"] != "ksplit" or (c["taps"] == 9 and c["cin"] == 320 and c["cout"] == 320 and not c["wrap"] and c["geom"] != "up"),
     "conv3x3.hip:1275-1276,1296-1302 ksplit_plan: 3 x 3, no up, no wrap under the rule, Cout % 320 == 0; at 64 tiles two chunks (Cin = 128) "
     "give 1 part (0.52 > 0.93 x 0.4875), five chunks (Cin = 320) give 4"),
    ("temb3_needs_three_images", lambda c: c["temb"] != "t3" or c["launch"] != "one",
     "kernels.py:611 temb.shape[0] * imgs_per_temb == N: the 'one' class is a single image"),
]

CONV_SEEDS = [
    dict(site="unet3d.py:97", taps=9, geom="pre", wrap=False, bias=True, temb="none", res=True, gn=True, cin=64, cout=320, launch="big"),
    dict(site="unet3d.py:91", taps=9, geom="s1", wrap=False, bias=True, temb="t3", res=False, gn=True, cin=64, cout=320, launch="big"),
    dict(site="unet3d.py:115", taps=9, geom="s2", wrap=True, bias=True, temb="none", res=False, gn=False, cin=64, cout=320, launch="big"),
    dict(site="unet3d.py:115", taps=9, geom="s2", wrap=False, bias=True, temb="none", res=False, gn=True, cin=64, cout=640, launch="big"),
    dict(site="unet3d.py:132", taps=9, geom="up", wrap=True, bias=True, temb="none", res=False, gn=False, cin=320, cout=320, launch="ragged"),
    dict(site="vae.py:75", taps=9, geom="vae", wrap=False, bias=True, temb="none", res=False, gn=False, cin=128, cout=64, launch="ragged"),
    dict(site="vae.py:75", taps=9, geom="vae", wrap=False, bias=True, temb="none", res=False, gn=False, cin=320, cout=320, launch="ksplit"),
]


def conv_geometry(case):
    """(N, Hout, Wout, Hin, Win) of the unpadded input the case starts from."""
    launch, t3 = case["launch"], case["temb"] == "t3"
    N, H, W = {"one": (1, 9, 11), "ragged": (3, 9, 11), "many": (6, 4, 4), "ksplit": ((3, 72, 75) if t3 else (16, 32, 32)),
               "big": ((513 if t3 else 512), 16, 16)}[launch]
    if case["geom"] == "up":
        hin, win = (H + 1) // 2, (W + 1) // 2
        return N, 2 * hin, 2 * win, hin, win
    if case["geom"] in ("s2", "vae"):
        return N, H, W, 2 * H, 2 * W
    return N, H, W, H, W


def conv_build(case, dt):
    r = seeded(_seed_of(case))
    N, H, W, hin, win = conv_geometry(case)
    k = 3 if case["taps"] == 9 else 1
    cin, cout = case["cin"], case["cout"]
    ops = dict(x=q16(r(N, hin, win, cin), dt), w=q16(r(cout, cin, k, k, scale=(k * k * cin) ** -0.5), dt), bias=None, temb=None, res=None)
    if case["geom"] == "pre":          # what GroupNorm(pad = 2) hands to conv2 (unet3d.py:87,97): the circularly padded tensor itself
        ops["x"] = OG.pad_pano(ops["x"].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
    if case["bias"]:
        ops["bias"] = q16(r(cout, scale=0.5), dt)
    if case["temb"] != "none":
        ops["temb"] = q16(r(N // (3 if case["temb"] == "t3" else 1), cout, scale=0.5), dt)
    if case["res"]:
        ops["res"] = q16(r(N, H, W, cout), dt)
    if case["gn"]:
        ops["gamma"], ops["beta"] = q16(1 + 0.1 * r(cout), dt), q16(0.1 * r(cout), dt)
    return ops


def conv_kwargs(case, d):
    N, H, W, _, _ = conv_geometry(case)
    kw = dict(bias=d["bias"], wrap=case["wrap"], res=d["res"])
    if d["temb"] is not None:
        kw.update(temb=d["temb"], imgs_per_temb=3 if case["temb"] == "t3" else 1)
    kw.update({"s1": {}, "s2": dict(stride=2), "up": dict(up=True), "pre": dict(x_off=2, wout=W), "vae": dict(stride=2, x_off=1, y_off=1)}[case["geom"]])
    return kw


def emu_gn_partials(y, slabs):
    """The layout of the producers' partial sums, [N][S][2][C] fp32, from a stored output y [N, H, W, C]."""
    N, C = y.shape[0], y.shape[-1]
    t = y.float().reshape(N, slabs, -1, C)
    return torch.stack([t.sum(2), (t * t).sum(2)], dim=2).reshape(-1)


def gn_of(P, y, slabs, **ctx):
    """(partials, slabs) the producer left on ``y``: the real tag, or the stand-in's sums."""
    if hasattr(P, "_gn_of"):
        return P._gn_of(y)
    return getattr(P, "gn_partials_of", lambda y, slabs, **_: emu_gn_partials(y, slabs))(y, slabs, **ctx), slabs


def conv_call(case, d, P, mk):
    wp = P.pack_conv_weight(d["w"])
    kw = conv_kwargs(case, d)
    out = P.conv2d(d["x"], wp, case["cout"], gn_stats=case["gn"], **kw)
    res = dict(out=out)
    if case["gn"]:
        N, H, W, _, _ = conv_geometry(case)
        tag = gn_of(P, out, H * W // 256, mod=P, x=d["x"], wp=wp, case=case, kw=kw)
        assert tag is not None, "conv2d(gn_stats=True) left no producer tag"
        res["part"], res["slabs"], res["want_slabs"] = tag[0], tag[1], H * W // 256
        res["gn_out"] = P.group_norm(out, d["gamma"], d["beta"], 32, 1e-5)
        res["out_plain"] = P.conv2d(d["x"], wp, case["cout"], gn_stats=False, **kw)
    return res


def conv_core64(case, ops, dtype=torch.float64):
    x, w = ops["x"].to(dtype).permute(0, 3, 1, 2), ops["w"].to(dtype)
    geom, wrap, pad = case["geom"], case["wrap"], ops["w"].shape[-1] // 2
    if geom == "pre":
        y = OG.unpad_pano(F.conv2d(x, w, padding=pad), 2)
    elif geom == "vae":
        y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2)
    elif geom == "s2":          # pad 2 -> conv -> unpad 1 == circular W (Downsample3D)
        y = OG.unpad_pano(F.conv2d(OG.pad_pano(x, 2), w, stride=2, padding=pad), 1) if wrap else F.conv2d(x, w, stride=2, padding=pad)
    elif geom == "up":          # pad 1 -> up -> conv -> unpad 2 (Upsample3D)
        xu = F.interpolate(OG.pad_pano(x, 1) if wrap else x, scale_factor=2.0, mode="nearest")
        y = OG.unpad_pano(F.conv2d(xu, w, padding=pad), 2 if wrap else 0)
    else:
        y = OG.unpad_pano(F.conv2d(OG.pad_pano(x, 1), w, padding=pad), 1) if wrap and pad else F.conv2d(x, w, padding=pad)
    return y.permute(0, 2, 3, 1)


def conv_ref(case, ops, results=None):
    # (the >= 512-tile class alone: an fp32 CPU reference, as test_conv3x3_256x320_tiles -- 2^-24 against the 2^-9 / 2^-12 that is measured)
    y = conv_core64(case, ops, torch.float32 if case["launch"] == "big" else torch.float64).double()
    if ops["bias"] is not None:
        y = y + ops["bias"].double()
    if ops["temb"] is not None:
        y = y + ops["temb"].double().repeat_interleave(y.shape[0] // ops["temb"].shape[0], 0)[:, None, None, :]
    if ops["res"] is not None:
        y = y + ops["res"].double()
    return dict(out=y)


def gn64(x, gamma, beta, eps, pad=0, silu=False, groups=32):
    y = F.group_norm(OG.pad_pano(x.detach().double().cpu().permute(0, 3, 1, 2), pad), groups, gamma.double(), beta.double(), eps)
    return (F.silu(y) if silu else y).permute(0, 2, 3, 1)


CONV = Family("conv", CONV_FACTORS, CONV_CONSTRAINTS, CONV_SEEDS, conv_build, conv_call, conv_ref,
              optional=lambda c: [n for n in ("bias", "temb", "res") if (c[n] if n != "temb" else c[n] != "none")],
              cost=lambda c: {"big": 2, "ksplit": 1}.get(c["launch"], 0))


# ------------------------------------------------------------------------------------------------ conv_up2
UP2_FACTORS = {"wrap": [False, True], "bias": [False, True], "cin": [64, 128], "cout": [8, 320], "shape": ["one", "ragged"]}


def up2_build(case, dt):
    r = seeded(_seed_of(case, 1))
    N, H, W = (1, 4, 4) if case["shape"] == "one" else (3, 5, 7)          # 105 low-resolution pixels: one ragged 128-row tile
    cin, cout = case["cin"], case["cout"]
    return dict(x=q16(r(N, H, W, cin), dt), w=q16(r(cout, cin, 3, 3, scale=(9 * cin) ** -0.5), dt), bias=q16(r(cout, scale=0.5), dt) if case["bias"] else None)


def up2_call(case, d, P, mk):
    return dict(out=P.conv_up2(d["x"], P.pack_conv_up2_weight(d["w"]), case["cout"], bias=d["bias"], wrap=case["wrap"]))


def up2_ref(case, ops, results=None):
    y = conv_core64(dict(geom="up", wrap=case["wrap"]), ops)
    return dict(out=y if ops["bias"] is None else y + ops["bias"].double())


UP2 = Family("conv_up2", UP2_FACTORS, [], [dict(site="unet3d.py:132", wrap=True, bias=True, cin=64, cout=320, shape="ragged")], up2_build, up2_call, up2_ref,
             optional=lambda c: ["bias"] if c["bias"] else [])

# ------------------------------------------------------------------------------------------------ conv1x1_cat
CAT_FACTORS = {"c1": [64, 128], "c2": [64, 192], "bias": [False, True], "res": [False, True], "cout": [96, 320], "m": [99, 128, 297]}


def cat_build(case, dt):
    r = seeded(_seed_of(case, 2))
    N, H, W = {99: (1, 9, 11), 128: (2, 8, 8), 297: (3, 9, 11)}[case["m"]]
    c1, c2, co = case["c1"], case["c2"], case["cout"]
    return dict(xa=q16(r(N, H, W, c1), dt), xb=q16(r(N, H, W, c2), dt), w=q16(r(co, c1 + c2, 1, 1, scale=(c1 + c2) ** -0.5), dt),
                bias=q16(r(co, scale=0.5), dt) if case["bias"] else None, res=q16(r(N, H, W, co), dt) if case["res"] else None)


def cat_call(case, d, P, mk):
    return dict(out=P.conv1x1_cat(d["xa"], d["xb"], P.pack_conv_weight(d["w"]), case["cout"], bias=d["bias"], res=d["res"]))


def cat_ref(case, ops, results=None):
    y = F.linear(torch.cat([ops["xa"], ops["xb"]], -1).double(), ops["w"].double().reshape(case["cout"], -1), None if ops["bias"] is None else ops["bias"].double())
    return dict(out=y if ops["res"] is None else y + ops["res"].double())


CAT = Family("conv1x1_cat", CAT_FACTORS, [], [dict(site="unet3d.py:94", c1=128, c2=192, bias=True, res=False, cout=320, m=297)], cat_build, cat_call, cat_ref,
             optional=lambda c: [n for n in ("bias", "res") if c[n]])


# ================================================================================================ attention
ATTN_FACTORS = {
    "d": [32, 64],
    "nq": [5, 32, 33, 100, 256],
    "nk": [1, 8, 76, 77, 128, 130],
    "group": [1, 2, 3],
    "bias": ["none", "plain", "packed", "packed_map", "alt0", "alt1"],       # alt: bias_alt + bias_sel = 0 / 1, packed with block maps where it can be
    "out": ["new", "strided", "acc"],                                        # acc: accumulate into a strided out with out_scale = 0.5
    "scale": ["default", "one"],
    "views": [False, True],                                                  # q / k / v as views of fused projections, row stride 3 C + 8
}
ATTN_CONSTRAINTS = [
    ("bias_needs_nk_mod_4", lambda c: c["bias"] == "none" or (c["nk"] % 4 == 0 and c["nk"] >= 4),
     "attn_fwd.hip:1084: a bias needs Nk % 4 == 0, Nk >= 4 and 8-byte aligned rows"),
    ("packed_needs_can_pack", lambda c: c["bias"] not in ("packed", "packed_map") or (c["d"] == 32 and c["nk"] % 8 == 0),
     "kernels.py:212 can_pack_attn_bias(d, nk) / attn_fwd.hip:1086: packed bias is head dim 32, Nk % 8 == 0"),
]
ATTN_SEEDS = [
    dict(site="unet3d.py:186", d=32, nq=100, nk=77, group=3, bias="none", out="acc", scale="one", views=False),
    dict(site="unet3d.py:185", d=32, nq=33, nk=77, group=2, bias="none", out="new", scale="default", views=False),
    dict(site="mv_model.py:143", d=32, nq=100, nk=128, group=1, bias="alt1", out="new", scale="default", views=True),
    dict(site="mv_model.py:149", d=64, nq=256, nk=76, group=1, bias="alt0", out="new", scale="default", views=True),
    dict(site="mv_model.py:143", d=32, nq=33, nk=8, group=1, bias="packed_map", out="new", scale="default", views=True),
]
ATTN_HEADS = 2


def attn_packs(case):
    return case["bias"] in ("packed", "packed_map") or (case["bias"] in ("alt0", "alt1") and case["d"] == 32 and case["nk"] % 8 == 0)


def attn_build(case, dt):
    r = seeded(_seed_of(case, 3))
    g = torch.Generator().manual_seed(_seed_of(case, 4))
    C = ATTN_HEADS * case["d"]
    bk, nq, nk = 2, case["nq"], case["nk"]
    B = bk * case["group"]
    wide = 3 * C + 8 if case["views"] else C
    fq, fk = r(B, nq, wide), r(bk, nk, wide)
    fq[..., :C] *= 0.5                                        # the query third: logits of std 1 / 2 under d^-1/2, sqrt(d) / 2 under scale 1
    ops = dict(fq=q16(fq, dt), fk=q16(fk, dt), fv=None if case["views"] else q16(r(bk, nk, C), dt), bias=None, alt=None, prev=None)
    if case["bias"] != "none":
        ops["bias"] = q16(torch.rand(nq, nk, generator=g) * 4 - 2, dt)
        if case["bias"] in ("alt0", "alt1"):
            ops["alt"] = q16(torch.rand(nq, nk, generator=g) * 4 - 2, dt)
        if attn_packs(case):                                  # whole 32 x 32 blocks of zeros for the block maps to skip
            ops["bias"][32:, :32] = 0
            if ops["alt"] is not None:
                ops["alt"][:32, 32:64] = 0
    if case["out"] == "acc":
        ops["prev"] = q16(r(B, nq, C, scale=0.1), dt)          # of the size of an average over ~ 100 values: neither summand hides the other
    return ops


def attn_qkv(case, d):
    C = ATTN_HEADS * case["d"]
    if case["views"]:
        return d["fq"][..., :C], d["fk"][..., C:2 * C], d["fk"][..., 2 * C:3 * C]
    return d["fq"], d["fk"], d["fv"]


def attn_out_strides(case):
    C = ATTN_HEADS * case["d"]
    return ((case["nq"] + 3) * (C + 8), C + 8, 1)              # row stride C + 8, three rows between the batches


def attn_place(ops, mk, case):
    d = {k: (mk.to(v) if torch.is_tensor(v) and k != "prev" else v) for k, v in ops.items()}
    if ops["prev"] is not None:
        d["prev"] = mk.to(ops["prev"], strides=attn_out_strides(case))
    d["sel"] = mk.to(torch.tensor([1 if case["bias"] == "alt1" else 0], dtype=torch.int32)) if case["bias"] in ("alt0", "alt1") else None
    return d


def attn_call(case, d, P, mk):
    q, k, v = attn_qkv(case, d)
    B, nq, C = q.shape
    kw = dict(kv_group=case["group"])
    if case["scale"] == "one":
        kw["scale"] = 1.0
    if d["bias"] is not None:
        packed = attn_packs(case)
        b, a = d["bias"], d["alt"]
        if packed:
            b, a = P.pack_attn_bias(b), (None if a is None else P.pack_attn_bias(a))
        kw.update(bias=b, bias_packed=packed)
        if a is not None:
            kw.update(bias_alt=a, bias_sel=d["sel"])
        if packed and case["bias"] != "packed":
            kw["bias_blocks"] = P.attn_bias_blocks(b)
            if a is not None:
                kw["bias_blocks_alt"] = P.attn_bias_blocks(a)
    if case["out"] == "strided":
        kw["out"] = mk.empty((B, nq, C), strides=attn_out_strides(case))
    elif case["out"] == "acc":
        kw.update(out=d["prev"], accumulate=True, out_scale=0.5)
    return dict(out=P.attention(q, k, v, ATTN_HEADS, **kw))


def attn_ref(case, ops, results=None):
    q, k, v = attn_qkv(case, ops)
    rep = lambda t: t.repeat_interleave(case["group"], 0)
    bias = ops["alt"] if (case["bias"] == "alt1" and ops["alt"] is not None) else ops["bias"]
    y = sdpa64(q, rep(k), rep(v), ATTN_HEADS, scale=1.0 if case["scale"] == "one" else None, bias=bias)
    if case["out"] == "acc":
        y = (0.0 if ops["prev"] is None else ops["prev"].double()) + ops.get("out_scale", 0.5) * y
    return dict(out=y)


def attn_optional(case):
    # ("alt" is the bias matrix of the alt1 cases: dropping it falls back to ``bias``)
    names = [] if case["bias"] == "none" else (["alt"] if case["bias"] == "alt1" else ["bias"])
    return names + (["out_scale"] if case["out"] == "acc" else [])


ATTN = Family("attention", ATTN_FACTORS, ATTN_CONSTRAINTS, ATTN_SEEDS, attn_build, attn_call, attn_ref, optional=attn_optional)
ATTN.place = lambda ops, mk, case=None: attn_place(ops, mk, case)

# ------------------------------------------------------------------------------------------------ attention2
ATTN2_FACTORS = {"n12": ["65+33", "96+64", "77+4"], "group": [1, 2, 3], "scale2": [1.0, 0.7], "nq": [64, 40, 33], "scale": ["default", "one"]}


def attn2_build(case, dt):
    r = seeded(_seed_of(case, 5))
    C, bk = ATTN_HEADS * 64, 2
    n1, n2 = (int(s) for s in case["n12"].split("+"))
    ops = dict(q=q16(r(bk * case["group"], case["nq"], C, scale=0.3), dt))
    ops.update({n: q16(r(bk, m, C), dt) for n, m in (("k1", n1), ("v1", n1), ("k2", n2), ("v2", n2))})
    return ops


def attn2_call(case, d, P, mk):
    kw = dict(scale=1.0) if case["scale"] == "one" else {}
    return dict(out=P.attention2(d["q"], d["k1"], d["v1"], d["k2"], d["v2"], ATTN_HEADS, out_scale2=case["scale2"], kv_group=case["group"], **kw))


def attn2_ref(case, ops, results=None):
    rep = lambda t: t.repeat_interleave(case["group"], 0)
    sc = 1.0 if case["scale"] == "one" else None
    s2 = ops.get("scale2", case["scale2"])
    return dict(out=sdpa64(ops["q"], rep(ops["k1"]), rep(ops["v1"]), ATTN_HEADS, scale=sc) + s2 * sdpa64(ops["q"], rep(ops["k2"]), rep(ops["v2"]), ATTN_HEADS, scale=sc))


# (f = 1.5: two attention results summed, as test_attention_two_key_sets_edges)
ATTN2 = Family("attention2", ATTN2_FACTORS, [], [dict(site="unet3d.py:183", n12="77+4", group=3, scale2=1.0, nq=64, scale="default"),
                                                  dict(site="unet3d.py:183", n12="77+4", group=3, scale2=0.7, nq=40, scale="one")],
               attn2_build, attn2_call, attn2_ref, f=1.5)


# ================================================================================================ group_norm
GN_FACTORS = {
    "form": ["single", "pair"],
    "pad": [0, 2],
    "silu": [False, True],
    "ch": ["64", "128", "320", "1280", "640+320"],
    "hw": ["4x4", "8x16", "16x32", "9x7", "32x32"],
    "n": [1, 3],
    "mode": ["partials", "three"],
    "tag": ["none", "conv2d", "linear", "first"],          # whose epilogue left partial sums on the input(s)
    "eps": [1e-5, 1e-6],
}
GN_SPLIT = {"64": (32, 32), "128": (64, 64), "320": (256, 64), "1280": (640, 640), "640+320": (640, 320)}


def gn_channels(case):
    c1, c2 = GN_SPLIT[case["ch"]]
    return (c1, c2) if case["form"] == "pair" else (c1 + c2, 0)


def gn_shape(case):
    """(images, H, W): a conv2d producer writes partial sums from 512 tiles of 256 x 320 on (conv3x3.hip:1362), so those cases run the
    smallest multiple of ``n`` images that reaches them."""
    H, W = (int(s) for s in case["hw"].split("x"))
    N = case["n"]
    if case["tag"] == "conv2d":
        c1, c2 = gn_channels(case)
        need = -(-512 * 256 // (H * W * (min(c1, c2 or c1) // 320)))
        N = -(-need // N) * N
    return N, H, W


def _gn_tagged(case):
    c1, c2 = gn_channels(case)
    return [c for c in ((c1,) if case["tag"] == "first" else (c1, c2)) if c]


GN_CONSTRAINTS = [
    ("tag_needs_whole_slabs", lambda c: c["tag"] == "none" or c["hw"] in ("16x32", "32x32"),
     "kernels.py:686 (gn_hw % 256 == 0) / conv3x3.hip:1361 (hw % 256 == 0): partial sums are per whole 256-pixel slab"),
    ("tag_needs_320_columns", lambda c: c["tag"] == "none" or all(ch % 320 == 0 for ch in _gn_tagged(c)),
     "kernels.py:679 linear needs n % 320 == 0 / conv3x3.hip:1361 Cout % 320 == 0: the tagged member is a 256 x 320-tile output"),
    ("first_is_a_pair", lambda c: c["tag"] != "first" or c["form"] == "pair", "kernels.py:408-423: 'first member only' exists for a pair"),
    ("conv2d_tag_is_single", lambda c: c["tag"] != "conv2d" or c["form"] == "single",
     "conv3x3.hip:1362: each conv2d-tagged member needs 512 tiles of its own (a 640 + 320 pair: 126 M elements); the consumer reads a conv2d and a "
     "linear tag through the same (buffer, slabs) pair (kernels.py:409-426), so the pair forms run with the linear producer"),
]
GN_SEEDS = [
    dict(site="unet3d.py:87", form="pair", pad=0, silu=True, ch="640+320", hw="16x32", n=3, mode="partials", tag="first", eps=1e-5),
    dict(site="unet3d.py:87", form="single", pad=2, silu=True, ch="320", hw="16x32", n=3, mode="partials", tag="conv2d", eps=1e-5),
    dict(site="unet3d.py:92", form="single", pad=0, silu=True, ch="320", hw="32x32", n=1, mode="partials", tag="conv2d", eps=1e-5),
    dict(site="vae.py:33", form="single", pad=0, silu=True, ch="128", hw="9x7", n=1, mode="partials", tag="none", eps=1e-6),
]
GN_SRC_K = 64          # K of the producer that writes a tagged member


def gn_build(case, dt):
    r = seeded(_seed_of(case, 6))
    N, H, W = gn_shape(case)
    c1, c2 = gn_channels(case)
    ops = dict(gamma=q16(1 + 0.1 * r(c1 + c2), dt), beta=q16(0.1 * r(c1 + c2), dt))
    tagged = {"none": (), "first": ("a",), "conv2d": ("a", "b"), "linear": ("a", "b")}[case["tag"]]
    for name, c, shift, scale in (("a", c1, 0.5, 1.0), ("b", c2, 0.0, 1.5)):
        if not c:
            continue
        if name in tagged:          # the member is the stored output of a 64 -> c producer with a bias that takes the mean off zero
            ops["src_" + name] = q16(r(N, H, W, GN_SRC_K), dt)
            ops["w_" + name] = q16(r(c, GN_SRC_K, 1, 1, scale=scale * GN_SRC_K ** -0.5), dt)
            ops["b_" + name] = q16(r(c, scale=0.2, shift=shift), dt)
        else:
            ops["x_" + name] = q16(r(N, H, W, c, scale=scale, shift=shift), dt)
    return ops


def gn_call(case, d, P, mk):
    N, H, W = gn_shape(case)
    xs = []
    for name in ("a", "b"):
        if "x_" + name in d:
            xs.append(d["x_" + name])
        elif "src_" + name in d:
            c = d["w_" + name].shape[0]
            wp = P.pack_conv_weight(d["w_" + name])
            if case["tag"] == "conv2d":
                x = P.conv2d(d["src_" + name], wp, c, bias=d["b_" + name], gn_stats=True)
            else:
                y = P.linear(d["src_" + name].reshape(N * H * W, GN_SRC_K), wp, c, bias=d["b_" + name], gn_hw=H * W)
                x = P.carry_gn(y.reshape(N, H, W, c), y)
            if hasattr(P, "_gn_of"):
                tag = P._gn_of(x)
                assert tag is not None and tag[1] == H * W // 256, ("the producer left no tag", case, tag and tag[1])
            xs.append(x)
    saved = getattr(P, "GN_MODE", None), getattr(P, "GN_FUSED", None)
    try:
        P.GN_MODE, P.GN_FUSED = case["mode"], False
        out = P.group_norm(xs[0] if len(xs) == 1 else tuple(xs), d["gamma"], d["beta"], 32, case["eps"], silu=case["silu"], pad=case["pad"])
    finally:
        P.GN_MODE, P.GN_FUSED = saved
    return dict(out=out, **{"x_" + n: x for n, x in zip("ab", xs)})


def gn_ref(case, ops, results):
    """Of the STORED members: a tagged one is whatever its producer wrote (``results``)."""
    xs = [results["x_" + n].detach().double().cpu() for n in "ab" if "x_" + n in results]
    return dict(out=gn64(torch.cat(xs, -1), ops["gamma"], ops["beta"], case["eps"], case["pad"], case["silu"]))


GN = Family("group_norm", GN_FACTORS, GN_CONSTRAINTS, GN_SEEDS, gn_build, gn_call, gn_ref, cost=lambda c: int(c["tag"] == "conv2d"))

# ================================================================================================ the token-major linears
LIN_FACTORS = {
    "entry": ["linear", "linear_ln", "linear_geglu", "linear_geglu_ln", "ff_fused", "ff_fused_ln"],
    "bias": [False, True],
    "res": ["none", "tensor", "alias"],                        # alias: the residual IS x
    "row_stats": [False, True],
    "gn_hw": ["none", 256, 1024],
    "tab": ["none", "plain/1", "plain/7", "c2/1", "c2/7"],     # plain / tab_has_c2, tab_div in 256-row tiles (conv3x3.hip:1577: one table row per tile)
    # < 128; 128; 2 x 128 + 57; 2048 = two images of 1024 rows (the least M at which both gn_hw values see more than one image);
    # ring = the least M with 512 tiles (a workgroup of the persistent walk takes a second tile; im360_linear_geglu's ring route)
    "m": ["57", "128", "313", "2048", "ring"],
    "k": [64, 320, 640, 1280],
    "n": [320, 640, 960],
}
_GEGLU, _FF, _LN = ("linear_geglu", "linear_geglu_ln"), ("ff_fused", "ff_fused_ln"), ("linear_ln", "linear_geglu_ln", "ff_fused_ln")
LIN_CONSTRAINTS = [
    ("res_is_linears_or_ffs", lambda c: c["res"] == "none" or c["entry"] in ("linear",) + _FF,
     "kernels.py:697,721,806: linear_ln / linear_geglu / linear_geglu_ln take no residual"),
    ("ff_needs_a_residual", lambda c: c["entry"] not in _FF or c["res"] != "none", "kernels.py:828 / ff_fused.hip:289: res is not optional"),
    ("alias_needs_k_eq_n", lambda c: c["res"] != "alias" or c["k"] == c["n"], "kernels.py:681 res.numel() == y.numel(): x can be the residual only where K == N"),
    ("row_stats_is_linears", lambda c: not c["row_stats"] or c["entry"] == "linear", "kernels.py:671: only linear() has row_stats"),
    ("gn_hw_is_linears", lambda c: c["gn_hw"] == "none" or (c["entry"] == "linear" and c["m"] in ("2048", "ring")),
     "kernels.py:671,686: only linear() has gn_hw, and it writes partial sums only for m % gn_hw == 0 (the other row counts here are no multiple of 256)"),
    ("tab_is_linear_lns", lambda c: c["tab"] == "none" or c["entry"] == "linear_ln", "kernels.py:697: only linear_ln has tab"),
    ("geglu_inner_mod_128", lambda c: c["entry"] not in _GEGLU or c["n"] == 640, "conv3x3.hip:1494,1597 / kernels.py:801: inner % 128 == 0 (320 and 960 are not)"),
    ("ff_shape", lambda c: c["entry"] not in _FF or (c["k"] == 320 and c["n"] == 320), "kernels.py:819 FF_FUSED_SHAPE / ff_fused.hip:291: K = N = 320 only"),
]
LIN_SEEDS = [
    dict(site="layers.py:160", entry="linear", bias=True, res="tensor", row_stats=True, gn_hw="none", tab="none", m="313", k=320, n=320),
    dict(site="layers.py:163", entry="linear", bias=True, res="tensor", row_stats=False, gn_hw=1024, tab="none", m="ring", k=320, n=320),
    dict(site="layers.py:188", entry="linear_ln", bias=False, res="none", row_stats=False, gn_hw="none", tab="c2/7", m="ring", k=320, n=960),
    dict(site="layers.py:223", entry="linear_geglu_ln", bias=True, res="none", row_stats=False, gn_hw="none", tab="none", m="313", k=640, n=640),
    dict(site="layers.py:228", entry="linear_geglu", bias=True, res="none", row_stats=False, gn_hw="none", tab="none", m="ring", k=64, n=640),
    dict(site="layers.py:275", entry="ff_fused_ln", bias=True, res="alias", row_stats=False, gn_hw="none", tab="none", m="313", k=320, n=320),
    dict(site="layers.py:279", entry="ff_fused", bias=True, res="tensor", row_stats=False, gn_hw="none", tab="none", m="128", k=320, n=320),
]
LIN_EPS = 1e-5
FF_INNER = 1280


def lin_rows(case):
    if case["m"] != "ring":
        return int(case["m"])
    if case["entry"] in _FF:
        return 256 * 128 + 1                                   # 257 tiles of 128 rows on 256 CUs
    if case["entry"] in _GEGLU:
        return (-(-512 // (2 * case["n"] // 256)) - 1) * 256 + 1          # im360_linear_geglu's ring route: 512 tiles of 256 x 256 (conv3x3.hip:1508)
    rt = -(-512 // (case["n"] // 320))                         # 512 tiles of 256 x 320
    if case["gn_hw"] != "none":
        return -(-rt * 256 // case["gn_hw"]) * case["gn_hw"]   # whole images
    return (rt - 1) * 256 + 1


def row_stats64(x, sl=160):
    """(sum, sum of squares) per row and 160-column slice, the producer's layout (one slice where K is no multiple of 160)."""
    M, kd = x.shape
    xs = x.double().reshape(M, kd // sl, sl) if kd % sl == 0 else x.double().reshape(M, 1, kd)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], dim=-1).float().contiguous()


def lin_build(case, dt, P):
    """``P``: whose ``interleave_geglu`` orders the GEGLU rows (the kernels' 32-row interleave, the stand-ins' plain order); the LayerNorm
    folding is kernels.fold_layer_norm's host algebra on the 16-bit operands."""
    from imagine360_amd import kernels as K
    r = seeded(_seed_of(case, 7))
    e, M, k, n = case["entry"], lin_rows(case), case["k"], case["n"]
    f16 = lambda t: None if t is None else t.to(dt)
    ops = dict(x=q16(r(M, k, shift=0.3), dt), res=None, tab=None)
    rows = n if e in ("linear", "linear_ln") else 2 * (FF_INNER if e in _FF else n)
    w = r(rows, k, scale=k ** -0.5)
    if rows != n:
        w[rows // 2:] *= 2.0                                   # gates of std ~ 2: some beyond the +- 4.2 clamp of the kernels' GELU
    ops["w"] = q16(w, dt)
    ops["b"] = q16(r(rows, scale=0.5), dt) if case["bias"] else None
    if e in _LN:
        ops["gamma"], ops["beta"] = q16(1 + 0.1 * r(k), dt), q16(0.1 * r(k), dt)
        wf, c1, c2 = K.fold_layer_norm(f16(ops["w"]), f16(ops["b"]), f16(ops["gamma"]), f16(ops["beta"]))
        ops["stats"] = row_stats64(ops["x"])
        if rows != n:
            wi, c1 = P.interleave_geglu(wf, c1)
            c2 = P.interleave_geglu(wf, c2)[1]
            wf = wi
        ops.update(wk=wf.float().reshape(rows, k, 1, 1).contiguous(), c1=c1.float().contiguous(), c2=c2.float().contiguous())
    elif rows != n:
        wi, bi = P.interleave_geglu(f16(ops["w"]), f16(ops["b"]))
        ops.update(wk=wi.float().reshape(rows, k, 1, 1).contiguous(), bk=None if bi is None else bi.float().contiguous())
    else:
        ops["wk"] = ops["w"].reshape(rows, k, 1, 1).contiguous()
    if e in _FF:
        ops["w2"] = q16(r(n, FF_INNER, 1, 1, scale=FF_INNER ** -0.5), dt)
        ops["b2"] = q16(r(n, scale=0.5), dt) if case["bias"] else None
    if case["res"] == "tensor":
        ops["res"] = q16(r(M, n, scale=0.5), dt)
    if case["tab"] != "none":
        ops["tab"] = r(3, n)
        if case["tab"].startswith("c2"):
            ops["tab_c2"] = (ops["tab"] + ops["c2"][None, :]).contiguous()
    return ops


def lin_place(ops, mk):
    keep32 = ("stats", "c1", "c2", "tab", "tab_c2")            # fp32 operands stay fp32
    return {k: (v if not torch.is_tensor(v) else (mk.to32(v) if k in keep32 else mk.to(v))) for k, v in ops.items()}


def lin_call(case, d, P, mk):
    e, n = case["entry"], case["n"]
    x = d["x"]
    res = x if case["res"] == "alias" else d["res"]
    wp = P.pack_conv_weight(d["wk"])
    if e == "linear":
        gn_hw = None if case["gn_hw"] == "none" else case["gn_hw"]
        y = P.linear(x, wp, n, bias=d["b"], res=res, row_stats=case["row_stats"], gn_hw=gn_hw)
        out = dict(out=y[0], stats=y[1]) if case["row_stats"] else dict(out=y)
        if gn_hw:
            tag = gn_of(P, out["out"].reshape(-1, gn_hw, 1, n), gn_hw // 256) if not hasattr(P, "_gn_of") else P._gn_of(out["out"])
            assert tag is not None, "linear(gn_hw=...) left no producer tag"
            out["part"], out["slabs"] = tag
            out["want_slabs"], out["images"] = gn_hw // 256, x.shape[0] // gn_hw
        return out
    if e == "linear_ln":
        kw = {}
        if case["tab"] != "none":
            kind, div = case["tab"].split("/")
            kw = dict(tab=d["tab_c2"] if kind == "c2" else d["tab"], tab_div=256 * int(div), tab_has_c2=kind == "c2")
        return dict(out=P.linear_ln(x, wp, d["c1"], d["c2"], d["stats"], LIN_EPS, n, **kw))
    if e == "linear_geglu":
        return dict(out=P.linear_geglu(x, wp, d["bk"], n))
    if e == "linear_geglu_ln":
        return dict(out=P.linear_geglu_ln(x, wp, d["c1"], d["c2"], d["stats"], LIN_EPS, n))
    w2p = P.pack_conv_weight(d["w2"])
    if not hasattr(P, "ff_fused"):          # the stand-ins have no fused form: the pair of launches it replaces
        h = P.linear_geglu(x, wp, d["bk"], FF_INNER) if e == "ff_fused" else P.linear_geglu_ln(x, wp, d["c1"], d["c2"], d["stats"], LIN_EPS, FF_INNER)
        M = x.shape[0]
        return dict(out=P.conv2d(h.reshape(M, 1, 1, FF_INNER), w2p, n, bias=d["b2"], res=res.reshape(M, 1, 1, n)).reshape(M, n))
    if e == "ff_fused":
        return dict(out=P.ff_fused(x, wp, d["bk"], w2p, d["b2"], res))
    return dict(out=P.ff_fused_ln(x, wp, d["c1"], d["c2"], d["stats"], LIN_EPS, w2p, d["b2"], res))


def lin_ref(case, ops, results=None):
    e, n = case["entry"], case["n"]
    x = ops["x"].double()
    xin = F.layer_norm(x, (x.shape[1],), ops["gamma"].double(), ops["beta"].double(), LIN_EPS) if e in _LN else x
    y = F.linear(xin, ops["w"].double(), None if ops["b"] is None else ops["b"].double())
    if e not in ("linear", "linear_ln"):
        i = y.shape[1] // 2
        y = y[:, :i] * F.gelu(y[:, i:])
    if e in _FF:
        y = F.linear(y, ops["w2"].double().reshape(n, FF_INNER), None if ops["b2"] is None else ops["b2"].double())
    if case["res"] == "alias":
        y = y + x
    elif ops["res"] is not None:
        y = y + ops["res"].double()
    if ops["tab"] is not None:
        div = 256 * int(case["tab"].split("/")[1])
        y = y + ops["tab"].double()[(torch.arange(y.shape[0]) // div) % ops["tab"].shape[0]]
    return dict(out=y)


def lin_optional(case):
    # (bias of the LayerNorm-folded entries lives inside c2; an aliased residual is x itself: neither is an operand that can be dropped)
    names = ["b"] if case["bias"] and case["entry"] in ("linear", "linear_geglu") else []
    return names + (["res"] if case["res"] == "tensor" else []) + (["tab"] if case["tab"] != "none" else [])


LIN = Family("linear", LIN_FACTORS, LIN_CONSTRAINTS, LIN_SEEDS, lin_build, lin_call, lin_ref, optional=lin_optional, cost=lambda c: int(c["m"] == "ring"))
LIN.place = lin_place
LIN.wants_pack = True

FAMILIES = {f.name: f for f in (CONV, UP2, CAT, ATTN, ATTN2, GN, LIN)}


# ================================================================================================ the criterion and the extra checks
def place(fam, case, ops, mk):
    return fam.place(ops, mk, case) if fam is ATTN else fam.place(ops, mk)


def slab_sums_ok(part, slabs, y, bound=GN_SUM_BOUND):
    """Per (image, channel): fp64 sum over the slabs of the fp32 partial sums against the fp64 sums of the STORED output, within
    bound x sum|y| and bound x sum y^2.  Returns (worst ratio to the bound for the sums, for the squares)."""
    y = y.detach().double().cpu()
    N, C = y.shape[0], y.shape[-1]
    t = y.reshape(N, -1, C)
    p = part.detach().double().cpu().reshape(N, slabs, 2, C).sum(1)
    e1 = ((p[:, 0] - t.sum(1)).abs() / (bound * t.abs().sum(1)).clamp_min(1e-300)).max()
    e2 = ((p[:, 1] - (t * t).sum(1)).abs() / (bound * (t * t).sum(1)).clamp_min(1e-300)).max()
    return float(e1), float(e2)


def failures(fam, case, results, refs, dt):
    """Names of the checks the results miss under the project's criterion (``close`` of test_kernel_bounds_gpu.py) and the extra
    checks the case asks for; empty = pass.  Also returns the observed (rel, blockrel) of the main result."""
    bad = []
    out, ref = results["out"], refs["out"]
    if tuple(out.shape) != tuple(ref.shape):
        return [f"shape {tuple(out.shape)} != {tuple(ref.shape)}"], (float("nan"), float("nan"))
    obs = rel(out, ref), blockrel(out, ref, fam.rows)
    if not close(out, ref, dt, rows=fam.rows, f=fam.f):
        bad.append(f"out: rel {obs[0]:.3e} blockrel {obs[1]:.3e}")
    if "part" in results:
        if results["slabs"] != results["want_slabs"]:
            bad.append(f"slabs {results['slabs']} != {results['want_slabs']}")
        e1, e2 = slab_sums_ok(results["part"], results["slabs"], out.reshape(results.get("images", out.shape[0]), -1, out.shape[-1]))
        if not (e1 <= 1.0 and e2 <= 1.0):
            bad.append(f"partial sums: {e1:.3g} / {e2:.3g} of the summation bound")
    if "stats" in results:          # row statistics: of the STORED output, per 160-column slice, within the summation bound at n = 160
        t = out.detach().double().cpu().reshape(out.shape[0], -1, 160)
        st = results["stats"].detach().double().cpu()
        e1 = ((st[..., 0] - t.sum(-1)).abs() / (ROW_SUM_BOUND * t.abs().sum(-1)).clamp_min(1e-300)).max()
        e2 = ((st[..., 1] - (t * t).sum(-1)).abs() / (ROW_SUM_BOUND * (t * t).sum(-1)).clamp_min(1e-300)).max()
        if tuple(st.shape) != (out.shape[0], out.shape[1] // 160, 2) or not (float(e1) <= 1.0 and float(e2) <= 1.0):
            bad.append(f"row statistics: {float(e1):.3g} / {float(e2):.3g} of the summation bound")
    if "gn_out" in results:
        if not torch.equal(results["out"], results["out_plain"]):
            bad.append("gn_stats changes the output bits")
        gref = gn64(results["out"], refs["gamma"], refs["beta"], 1e-5)
        if not close(results["gn_out"], gref, dt, rows=fam.rows):
            bad.append(f"group_norm of the tagged output: rel {rel(results['gn_out'], gref):.3e}")
    return bad, obs


def build(fam, case, dt, P):
    return fam.build(case, dt, P) if fam.wants_pack else fam.build(case, dt)


def run_case(fam, case, P, dt=torch.bfloat16, mk=None, ops=None, tol_dt=None):
    """Build, place, call, reference, judge: (failures, observed, results, refs) -- the CPU tier's path (the GPU tier wraps the call
    in guard bands)."""
    mk = mk or Host()
    ops = build(fam, case, dt, P) if ops is None else ops
    results = fam.call(case, place(fam, case, ops, mk), P, mk)
    refs = fam.ref(case, ops, results)
    refs.update({k: ops[k] for k in ("gamma", "beta") if k in ops})
    bad, obs = failures(fam, case, results, refs, tol_dt or dt)
    return bad, obs, results, refs


def emu(**overrides):
    """The stand-ins as a namespace a mutant can override one function of."""
    ns = types.SimpleNamespace(**{n: getattr(EMU, n) for n in dir(EMU) if not n.startswith("__")})
    ns.gn_partials_of = lambda y, slabs, **_: emu_gn_partials(y, slabs)
    for k, v in overrides.items():
        setattr(ns, k, v)
    return ns
