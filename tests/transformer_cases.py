"""Cases, fp64 restatements, error bounds and host-dispatch census of tests/test_transformer_cpu.py and tests/test_transformer_gpu.py: the
kernels of csrc/attention.hip (mf_attention_f32) and the linear / LayerNorm / GEGLU kernels of csrc/small_ops.hip against fp64 at the edges of
their paths.  Importable without a GPU.

Inputs are functions of the case (and regime) alone.  Every (batch, head) of the attention values v has its own magnitude, 8^(b H + h) times
N(0, 1); the rows of the linear and LayerNorm inputs carry scales 2^6 apart (cycle of 5, so rows 8 apart -- two passes of linear_kernel --
differ too): a value taken from the wrong head, sample or row is off by orders of magnitude, not by rounding.

ATTENTION.  Restatement `attn_terms` (fp64): softmax_j((q s) . (k s)) v per (batch, head), s = d^-0.25 as a float; q s and k s are the fp32
products (the kernels and the reference both scale before the dot product).  Four input regimes (`attn_inputs`):

  uniform   q = 0, k random, v = integers in [-8, 8] times 4 times the head's power of 8.  Every score is exactly 0, every p exactly 1,
            l = Nk and every partial sum of v is exact in fp32 in any order: out = Sum v / Nk with two roundings (1 / l, the product),
            held to 2 fp32 ulp of the fp64 quotient.  A dropped, doubled or unmasked key moves the result by >= 1 / Nk of a unit.
  onehot    q_i = c (pi(i), 1, 0...), k_j = c (2 j, -j^2, 0...), pi(i) = (7 i + 3) mod Nk (11 i where 7 divides Nk): score = (c s)^2 (2 pi(i) j - j^2), largest at
            j = pi(i).  c is sqrt(200) / s rounded UP to 8 significand bits, so c pi, 2 c j and c j^2 are exact in fp32 (only the product with
            s rounds) and (c s)^2 lies in [200, 203.2]: the gap to every other key is >= 200 (tests/test_transformer_cpu.py asserts it on the
            rounded products).  The winner's p is exp(0) = 1, every other p and every stale alpha is exp(<= -200) = 0 in fp32, l = 1:
            out[i] = v[pi(i)] bit for bit.  d = 1: k_j = c j and q_i = c, every query selects the last key.
  diffuse   q, k ~ N(0, 1)
  steep     q, k ~ 3 N(0, 1) plus a component along the head's first axis that lifts the score by about 80 from the first key to the last;
  steep-rev the same keys and values in reversed order (the running maximum rises at every tile, or never after the first)

(a) per (batch, head): RMS error of the kernel against fp64, relative to the RMS of the fp64 result, <= 4 x the same figure of `attn_chain`
    (softmax((q s) @ (k s)^T) @ v, plain fp32 torch on the CPU, from the same inputs).  The margin 4 covers the per-tile rescales and a 1-ulp
    exponential where the CPU's is 0.5 ulp; independent roundings add in quadrature.
(b) the elementwise ceiling `attn_bound_E`, u = 2^-24, every quantity the fp64 one, T the tile length of the case's path:
      A_ij  = Sum_c |q s|_c |k s|_c                       x_ij = score_ij - max_j score_ij
      e_ij  = (d + 3) u A_ij + u (3 + 2 |x_ij|)           the score's accumulation (d roundings; 3 for the products with s and slack);
                                                          s - m (1 rounding), __expf at 1 ulp (2 u) and the |x| 6e-8 of its argument
                                                          (csrc/common.h on v_exp_f32; 6e-8 = u)
      E_ic  = Sum_j w_ij e_ij |v_jc| + (Sum_j w_ij e_ij) |out_ic|           numerator and denominator of the softmax
            + u (min(Nk, T) + 2 ceil(Nk / T)) Sum_j w_ij |v_jc| + 3 u |out_ic|    the P.V chain inside a tile, one rescale and one addition
                                                                              per tile; 1 / l, the final product, the rounding of l
    E is a worst case, linear in d.

LINEAR.  y = f(x) W^T + b, f = swish or identity on either side, optionally accumulated onto `out`.  `lin_bound_E`:
      E = slope [ (ceil(In / 64) + 8) u S + (5 u Sum |f(x) w| + TINY Sum |w| if act_in) ] + (5 u |f(y)| + TINY if act_out) + (u |out| if accumulate)
    S = Sum_i |f(x_i) w_i| + |b|  (the bias is the last term of the sum: its addition rounds at u |y| <= u S).  A lane chains ceil(In / 64)
    fused multiply-adds (one rounding each), the wave reduction adds 6 and the bias 1; 1 spare.  (The float4 loop chains 4 ceil(In / 256),
    up to 3 more than ceil(In / 64), for the FIRST terms of its longest lane only; the bound is a sum over terms weighted by their depth and
    the constant holds for it unless those few terms carry the whole sum.)  swish_acc (csrc/common.h) is x * (1 / (1 + expf(-x))): expf at
    its documented 1 ulp (2 u, damped by e / (1 + e) <= 1), the addition, the IEEE division and the product one rounding each: 5 u |f|;
    TINY = 2^-126 where f underflows.  slope = 1.1 bounds |d/dy y sigmoid(y)| when act_out, else 1.

LAYERNORM (two passes, one wave per row).  `ln_bound_E`, n = ceil(C / 64), mean / var / rstd / z / t the fp64 ones:
      dm  = (n + 7) u mean_c |x_c|                        the mean: n additions per lane, 6 in the wave reduction, the division
      rho = dm^2 / (2 (var + eps)) + (n / 2 + 8) u        rstd: the variance about the ROUNDED mean is var + dm^2 exactly (second order);
                                                          d^2 (2 u), n + 6 accumulations, / C, + eps: (n + 10) u halved by the square root;
                                                          sqrtf at 1 ulp (2 u), the IEEE division (u)
      E   = |gamma| (dm rstd + (2 u + rho) |z|) + u (|z gamma| + |t|)      x - mean and the product with rstd; gamma; beta
    The first term is the conditioning |mean| / sigma that the second input regime (mean = 1000 sigma) raises; a one-pass variance would
    lose |mean|^2 / sigma^2 u = 6 % of the variance there and leaves E by orders of magnitude.

GEGLU.  out = a gelu_erf(g).  `geglu_bound_E0` is the bound WITHOUT the error of erff itself (ROCm's figure for erff is not in this tree):
      E0 = |a| [ |g| / 2 ( 2 u |t| erf'(t) + u |1 + erf(t)| ) + 2 u |gelu| ] + u |a g|,   t = g / sqrt 2
    the rounding of t and of the constant; 1 + erf; the two products; and the absolute term of the cancellation in 1 + erf below g = -5
    (erf(t) near -1 is stored with an absolute error of u / 2).  The kernel is held to 4 x the per-case max of |a * F.gelu(g) (fp32, CPU) - fp64| / E0.

No constant here comes from a run of the kernels.  The census functions restate the host dispatch (mf_attention_f32: MFMA iff d in
{8, 16, 32, 64, 128}, Nk >= 8 and all four pointers 16-byte aligned; the LDS bytes of the VALU launch; linear's float4 loop and 8-row passes;
the loops of layernorm_kernel; geglu's 2048-workgroup cap) so that the CPU suite can assert which path every case lands on."""
import functools
import math

import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
TINY = 2.0 ** -126
LN_EPS = float(torch.tensor(1e-5, dtype=torch.float32))   # the kernel takes eps as a float

# (B, H, Nq, Nk, d, aligned)
ATTN_CASES = [
    (1, 1, 1, 8, 8, True),          # smallest MFMA problem: three idle waves, one query
    (2, 3, 33, 7, 8, True),         # Nk < 8 sends an MFMA head dim to VALU
    (2, 2, 31, 31, 16, True),       # wave edge and 32-key tile edge of MFMA: below,
    (1, 2, 32, 32, 16, True),       # at,
    (2, 2, 33, 33, 16, True),       # above (one key in the second tile)
    (1, 2, 127, 63, 32, True),      # block edge; 64-key edge
    (1, 1, 128, 64, 32, True),
    (2, 1, 129, 65, 32, True),      # second workgroup with one query; one key in the last tile
    (1, 2, 40, 47, 64, True),       # DT = 2
    (1, 1, 70, 130, 128, True),     # DT = 4, five key tiles
    (2, 2, 33, 47, 16, False),      # misaligned base (q, k, v 4 bytes off): the MFMA head dims on VALU
    (1, 1, 70, 130, 128, False),    # d = 128: both column halves full, 99 840 B of LDS
    (1, 2, 40, 97, 64, False),      # d = 64: exactly one half
    (2, 2, 40, 97, 65, True),       # VALU by head dim: one lane in the upper half
    (1, 1, 20, 70, 84, True),       # the first d over 64 KiB of LDS
    (1, 2, 17, 65, 127, True),
    (2, 3, 9, 33, 12, True),        # d < 64
    (1, 2, 5, 64, 1, True),         # d = 1
    (2, 4, 64, 1, 4, True),         # the 1-key cross-attention
]
REGIMES = ("uniform", "onehot", "diffuse", "steep", "steep-rev")
EXACT_REGIMES = ("uniform", "onehot")
CANARY_CASES = [(2, 2, 33, 33, 16, True), (2, 2, 40, 97, 65, True)]
NAN_CASES = [(2, 2, 33, 33, 16, True), (2, 2, 40, 97, 65, True)]      # one MFMA, one VALU

# (B, In, Out)
LIN_CASES = [(1, 1, 1), (8, 3, 5), (9, 4, 4), (17, 260, 7), (3, 1027, 5), (9, 2048, 4)]
# (act_in, act_out, bias, x is a slice, out is a slice, accumulate)
LIN_VARIANTS = [
    (False, False, True, False, False, False),
    (True, False, True, True, False, False),
    (False, True, True, False, True, False),
    (True, True, False, True, True, True),
    (False, False, False, False, True, True),
]
# (rows, C)
LN_CASES = [(1, 1), (5, 63), (4, 64), (7, 65), (3, 320), (9, 1280)]
LN_REGIMES = ("centred", "offset")
GEGLU_CASES = [(1, 1), (3, 33), (1025, 513)]
GEGLU_PLANTED = (5.0, -5.0, 0.0, 9.0, -6.0, -9.0)


def case_id(case) -> str:
    return "-".join(str(int(v)) if isinstance(v, bool) else str(v) for v in case)


def _gen(tag, case):
    return torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(tag + case_id(case))))


def row_scales(n):
    return torch.tensor([2.0 ** (6 * (i % 5) - 6) for i in range(n)])


def ulp32(x):
    """the fp32 unit in the last place at |x| (fp64 tensor); 0 at 0"""
    m, e = torch.frexp(x.abs().double())
    return torch.where(x == 0, torch.zeros_like(m), torch.exp2(e.double() - 24.0))


# ---------------------------------------------------------------- attention: inputs

def attn_scale(d) -> float:
    """s = d^-0.25 as the float the library receives"""
    return float(torch.tensor(d ** -0.25, dtype=torch.float32))


def _ceil_bits(x, bits):
    m, e = math.frexp(x)
    return math.ldexp(math.ceil(m * 2 ** bits) / 2 ** bits, e)


def onehot_c(d) -> float:
    return _ceil_bits(math.sqrt(200.0) / attn_scale(d), 8)


def onehot_pi(nq, nk, d):
    """pi(i) = (7 i + 3) mod Nk -- with 11 in place of 7 where 7 divides Nk (7, 63, 70), so that every key slot wins for some query wherever Nq >= Nk"""
    m = 7 if nk % 7 else 11
    assert math.gcd(m, nk) == 1
    return [nk - 1] * nq if d == 1 else [(m * i + 3) % nk for i in range(nq)]


def head_scales(B, H):
    return torch.tensor([[8.0 ** (b * H + h) for h in range(H)] for b in range(B)]).view(B, 1, H, 1)


@functools.lru_cache(maxsize=8)
def attn_inputs(case, regime):
    """(q [B, Nq, C], k, v [B, Nk, C]) on the CPU, fp32, contiguous; head h in columns h d .. (h + 1) d"""
    B, H, Nq, Nk, d, _ = case
    C = H * d
    base = "steep" if regime == "steep-rev" else regime
    g = _gen("attn" + base, case)
    hs = head_scales(B, H)
    q = torch.randn((B, Nq, H, d), generator=g)
    k = torch.randn((B, Nk, H, d), generator=g)
    v = torch.randn((B, Nk, H, d), generator=g) * hs
    if regime == "uniform":
        q = torch.zeros_like(q)
        v = torch.randint(-8, 9, (B, Nk, H, d), generator=g).float() * 4.0 * hs
    elif regime == "onehot":
        c = onehot_c(d)
        q, k = torch.zeros_like(q), torch.zeros_like(k)
        j = torch.arange(Nk, dtype=torch.float32).view(1, Nk, 1)
        if d == 1:
            q[..., 0] = c
            k[..., 0] = c * j
        else:
            q[..., 0] = c * torch.tensor(onehot_pi(Nq, Nk, d), dtype=torch.float32).view(1, Nq, 1)
            q[..., 1] = c
            k[..., 0] = c * 2.0 * j
            k[..., 1] = -c * j * j
    elif base == "steep":
        a = math.sqrt(80.0) / attn_scale(d)
        q, k = 3.0 * q, 3.0 * k
        q[..., 0] += a
        if Nk > 1:
            k[..., 0] += a * (torch.arange(Nk, dtype=torch.float32) / (Nk - 1)).view(1, Nk, 1)
        if regime == "steep-rev":
            k, v = k.flip(1), v.flip(1)
    else:
        assert regime == "diffuse", regime
    return q.reshape(B, Nq, C).contiguous(), k.reshape(B, Nk, C).contiguous(), v.reshape(B, Nk, C).contiguous()


def heads(t, H):
    """[B, N, H d] -> [B, H, N, d]"""
    B, N, C = t.shape
    return t.reshape(B, N, H, C // H).permute(0, 2, 1, 3)


# ---------------------------------------------------------------- attention: restatement, bound, chain

def attn_terms(q, k, v, H, scale=None, drop_last_key=False):
    """the fp64 restatement, everything in head layout [B, H, ., .].  scale / drop_last_key: the mutations of tests/test_transformer_cpu.py"""
    d = q.shape[-1] // H
    s = torch.tensor(attn_scale(d) if scale is None else scale, dtype=torch.float32)
    qs, ks, vd = heads(q * s, H).double(), heads(k * s, H).double(), heads(v, H).double()
    if drop_last_key:
        ks, vd = ks[:, :, :-1], vd[:, :, :-1]
    sc = qs @ ks.transpose(-1, -2)
    w = torch.softmax(sc, dim=-1)
    return {"out": w @ vd, "w": w, "x": sc - sc.amax(dim=-1, keepdim=True), "A": qs.abs() @ ks.abs().transpose(-1, -2), "absv": vd.abs(), "d": d, "score": sc}


def attn_bound_E(tm, T):
    """the elementwise ceiling (b) of the module docstring, [B, H, Nq, d]; T: the tile length of the path"""
    u, d = U24, tm["d"]
    nk = tm["w"].shape[-1]
    we = tm["w"] * ((d + 3) * u * tm["A"] + u * (3.0 + 2.0 * tm["x"].abs()))
    out = tm["out"].abs()
    return we @ tm["absv"] + we.sum(dim=-1, keepdim=True) * out + u * (min(nk, T) + 2 * -(-nk // T)) * (tm["w"] @ tm["absv"]) + 3.0 * u * out


def attn_chain(q, k, v, H):
    """the reference formula as a plain fp32 torch chain on the CPU, head layout"""
    s = torch.tensor(attn_scale(q.shape[-1] // H), dtype=torch.float32)
    out = torch.softmax(heads(q * s, H) @ heads(k * s, H).transpose(-1, -2), dim=-1) @ heads(v, H)
    assert out.dtype == torch.float32
    return out


def rms_rel(got, want):
    """per (batch, head): RMS of got - want over the RMS of want, [B, H] fp64 (got, want in head layout)"""
    e = ((got.double() - want) ** 2).mean(dim=(-1, -2)).sqrt()
    return e / (want ** 2).mean(dim=(-1, -2)).sqrt()


def ratio_heads(got, want, E):
    """per (batch, head): max |got - want| / E (0 / 0 counts as 0: an exact result under a bound of zero)"""
    err = (got.double() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / E)
    return r.amax(dim=(-1, -2))


def uniform_expected(v, H):
    """fp64 Sum v / Nk, [B, H, 1, d]"""
    vd = heads(v, H).double()
    return vd.sum(dim=2, keepdim=True) / vd.shape[2]


def onehot_expected(case, v):
    """v[pi(i)] as fp32, [B, Nq, C]"""
    _, _, Nq, Nk, d, _ = case
    return v[:, torch.tensor(onehot_pi(Nq, Nk, d))]


def onehot_gap(case):
    """the smallest distance of the winning score to any other key's, over every query of the case, on the rounded fp32 products (inf: one key)"""
    B, H, Nq, Nk, d, _ = case
    q, k, v = attn_inputs(case, "onehot")
    sc = attn_terms(q, k, v, H)["score"]
    pi = torch.tensor(onehot_pi(Nq, Nk, d)).view(1, 1, Nq, 1).expand(B, H, Nq, 1)
    win = sc.gather(-1, pi)
    assert bool((win == sc.amax(dim=-1, keepdim=True)).all()), case
    rest = sc.scatter(-1, pi, float("-inf"))
    return float((win - rest.amax(dim=-1, keepdim=True)).min())


def misaligned(t, dev):
    """a contiguous copy of t on `dev` whose base is 4 bytes past a 16-byte boundary: buf[1:]"""
    buf = torch.empty((t.numel() + 1,), dtype=t.dtype, device=dev)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


# ---------------------------------------------------------------- attention: the host dispatch, restated

MFMA_DIMS = (8, 16, 32, 64, 128)


def attn_census(case) -> dict:
    """mf_attention_f32: the path, its key tiles, its workgroups and waves, the dynamic LDS of the VALU launch"""
    B, H, Nq, Nk, d, aligned = case
    mfma = d in MFMA_DIMS and Nk >= 8 and aligned
    T, qblock, qwave = (32, 128, 32) if mfma else (64, 64, 16)
    tiles = -(-Nk // T)
    lds = 2 * 32 * (d + 4) * 4 if mfma else (2 * 64 * (d + 1) + 4 * 16 * d + 4 * 64) * 4
    blocks = -(-Nq // qblock)
    return {"path": "mfma" if mfma else "valu", "T": T, "tiles": tiles, "last_tile_keys": Nk - (tiles - 1) * T, "ragged": Nk % T != 0,
            "lds_bytes": lds, "over_64k": (not mfma) and lds > 64 * 1024, "upper_half": (not mfma) and d > 64, "upper_lanes": max(0, d - 64) if not mfma else 0,
            "blocks": blocks, "idle_waves": 4 * blocks - -(-Nq // qwave) if mfma else 0, "ragged_wave": Nq % qwave != 0,
            "DT": (d + 31) // 32 if mfma else 0, "mfma_dim_on_valu": (not mfma) and d in MFMA_DIMS}


# ---------------------------------------------------------------- linear

def swish64(x):
    return x * torch.sigmoid(x)


@functools.lru_cache(maxsize=None)
def lin_inputs(case):
    """(x_wide [B, In + 8], w [Out, In], bias [Out], out_wide [B, Out + 8]) on the CPU; x is x_of(x_wide), out0 is out_of(out_wide)"""
    B, In, Out = case
    g = _gen("linear", case)
    sc = row_scales(B).view(B, 1)
    x_wide = torch.randn((B, In + 8), generator=g) * sc
    w = torch.randn((Out, In), generator=g) / math.sqrt(In)
    bias = 0.1 * torch.randn((Out,), generator=g)
    out_wide = torch.randn((B, Out + 8), generator=g) * sc.flip(0)
    return x_wide, w, bias, out_wide


def x_of(x_wide):
    x = x_wide[:, 8:]
    assert x.stride(0) == x.shape[1] + 8 and x.stride(1) == 1
    return x


def out_of(out_wide):
    out = out_wide[:, 4:-4]
    assert out.stride(0) == out.shape[1] + 8 and out.stride(1) == 1 and out.shape[1] >= 1
    return out


def lin_terms(x, w, bias, act_in, act_out, out0=None):
    """fp64 terms of y = f(x) W^T + b, out = [out0 +] f(y)"""
    fx = swish64(x.double()) if act_in else x.double()
    wd = w.double()
    b = bias.double() if bias is not None else torch.zeros((), dtype=torch.float64, device=x.device)
    y = fx @ wd.t() + b
    fy = swish64(y) if act_out else y
    return {"S": fx.abs() @ wd.abs().t() + b.abs(), "Sfw": fx.abs() @ wd.abs().t(), "absw": wd.abs().sum(dim=1), "fy": fy, "act_in": act_in, "act_out": act_out,
            "acc": out0 is not None, "out": fy + out0.double() if out0 is not None else fy, "In": x.shape[1]}


def lin_bound_E(tm):
    u = U24
    E = (-(-tm["In"] // 64) + 8) * u * tm["S"]
    if tm["act_in"]:
        E = E + 5.0 * u * tm["Sfw"] + TINY * tm["absw"]
    if tm["act_out"]:
        E = 1.1 * E + 5.0 * u * tm["fy"].abs() + TINY
    if tm["acc"]:
        E = E + u * tm["out"].abs()
    return E


def lin_chain(x, w, bias, act_in, act_out, out0=None):
    """plain fp32 torch on the CPU"""
    fx = x * torch.sigmoid(x) if act_in else x
    y = F.linear(fx, w, bias)
    y = y * torch.sigmoid(y) if act_out else y
    return y + out0 if out0 is not None else y


def ratio_rows(got, want, E):
    """per row: max |got - want| / E (0 / 0 counts as 0)"""
    err = (got.double() - want).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / E)
    return [float(v) for v in r.reshape(r.shape[0], -1).amax(dim=1)]


def lin_census(case) -> dict:
    """mf_linear_f32 / linear_kernel: the float4 loop, the 8-row passes, the dynamic LDS"""
    B, In, Out = case
    float4 = In % 4 == 0
    lds = 8 * In * 4
    return {"float4": float4, "float4_turns": -(-In // 256) if float4 else 0, "float4_ragged_last_turn": float4 and In > 256 and In % 256 != 0,
            "passes": -(-B // 8), "last_pass_rows": B - (-(-B // 8) - 1) * 8, "lds_bytes": lds, "lds_at_limit": lds == 64 * 1024, "refused": lds > 64 * 1024,
            "blocks": -(-Out // 4), "idle_waves": 4 * -(-Out // 4) - Out}


# ---------------------------------------------------------------- LayerNorm

@functools.lru_cache(maxsize=None)
def ln_inputs(case, regime):
    """(x [rows, C], gamma [C], beta [C]) on the CPU"""
    rows, C = case
    g = _gen("layernorm", case)
    sc = row_scales(rows).view(rows, 1)
    x = torch.randn((rows, C), generator=g) * sc
    if regime == "offset":
        x = x + 1000.0 * sc
    else:
        assert regime == "centred", regime
    return x, 1.0 + 0.3 * torch.randn((C,), generator=g), 0.2 * torch.randn((C,), generator=g)


def ln_terms(x, gamma, beta, eps=LN_EPS):
    xd = x.double()
    mean = xd.mean(dim=-1, keepdim=True)
    var = ((xd - mean) ** 2).mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = (xd - mean) * rstd
    t = z * gamma.double() + beta.double()
    return {"mean": mean, "var": var, "rstd": rstd, "z": z, "t": t, "out": t, "absmean": xd.abs().mean(dim=-1, keepdim=True), "ga": gamma.double(), "eps": eps, "C": x.shape[-1]}


def ln_bound_E(tm):
    u, n = U24, -(-tm["C"] // 64)
    dm = (n + 7) * u * tm["absmean"]
    rho = dm * dm / (2.0 * (tm["var"] + tm["eps"])) + (n / 2.0 + 8.0) * u
    z = tm["z"].abs()
    return tm["ga"].abs() * (dm * tm["rstd"] + (2.0 * u + rho) * z) + u * ((tm["z"] * tm["ga"]).abs() + tm["t"].abs())


def ln_chain(x, gamma, beta, eps=LN_EPS):
    """two passes in plain fp32 torch on the CPU"""
    mean = x.mean(dim=-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(dim=-1, keepdim=True) + eps)
    return d * rstd * gamma + beta


def ln_one_pass(x, gamma, beta, eps=LN_EPS):
    """what the kernel must NOT be: var = E[x^2] - E[x]^2 in fp32"""
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x * x).mean(dim=-1, keepdim=True) - mean * mean).clamp_min(0.0)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def ln_census(case) -> dict:
    rows, C = case
    n = -(-C // 64)
    return {"lane_turns": n, "last_turn_lanes": C - (n - 1) * 64, "idle_lanes": max(0, 64 - C), "blocks": -(-rows // 4), "idle_waves": 4 * -(-rows // 4) - rows}


# ---------------------------------------------------------------- GEGLU

@functools.lru_cache(maxsize=None)
def geglu_inputs(case):
    """h [rows, 2 C] on the CPU: a | gate; the planted gates go down column 0 (and on into the next columns where the rows run out)"""
    rows, C = case
    g = _gen("geglu", case)
    a = torch.randn((rows, C), generator=g) * row_scales(rows).view(rows, 1)
    gate = 2.0 * torch.randn((rows, C), generator=g)
    if rows >= 6:
        gate[:, 0] = torch.tensor(GEGLU_PLANTED)[torch.arange(rows) % 6]
    else:
        for n in range(6):
            r, c = n % rows, n // rows
            if c < C:
                gate[r, c] = GEGLU_PLANTED[n]
    return torch.cat([a, gate], dim=-1).contiguous()


def geglu_terms(h):
    a, g = h.double().chunk(2, dim=-1)
    t = g / math.sqrt(2.0)
    erf = torch.erf(t)
    gelu = 0.5 * g * torch.erfc(-t)      # 1 + erf(t) without the cancellation
    return {"a": a, "g": g, "t": t, "erf": erf, "one_plus_erf": torch.erfc(-t), "gelu": gelu, "out": a * gelu}


def geglu_bound_E0(tm):
    u = U24
    a, g, t = tm["a"].abs(), tm["g"].abs(), tm["t"].abs()
    derf = 2.0 / math.sqrt(math.pi) * torch.exp(-t * t)
    return a * (0.5 * g * (2.0 * u * t * derf + u * tm["one_plus_erf"]) + 2.0 * u * tm["gelu"].abs()) + u * a * g


def geglu_chain(h):
    a, g = h.chunk(2, dim=-1)
    return a * F.gelu(g)


def geglu_ratio(got, tm):
    """max over the case of |got - fp64| / E0 (0 / 0 counts as 0)"""
    err = (got.double() - tm["out"]).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / geglu_bound_E0(tm)).max())


def geglu_census(case) -> dict:
    rows, C = case
    total = rows * C
    blocks = min(2048, -(-total // 256))
    return {"total": total, "blocks": blocks, "second_round": total > blocks * 256}
