"""Float64 references, per-element rounding bounds, inputs, mutants and the dispatch restatement for the attention kernels
(csrc/attention_bf16.hip + attn_bf16_dev.h: the 16-bit MFMA path; csrc/attention_f32.hip: the fp32 path).  Nothing here touches
the GPU; tests/test_attention_cpu.py pins the references and the conditions on the inputs, tests/test_attention_gpu.py compares
the kernels.

Layout.  Mathematics lives on [B, H, n, d] float64 tensors, n = n_main + n_extra with the extra ([cls]) token LAST.  The kernels
read token-major [rows, >= H*d] buffers in the cls-last layout of include/vfmseg_hip.h: row b*n_main + i for patch token i of
image b, row B*n_main + b for its [cls] token (`to_tokens` / `from_tokens`).  `Operands` puts those rows into device buffers
whose every element outside the view is NaN: separate buffers, or q | k | v (dq | dk | dv) as column slices of one packed
[rows, 3*H*d + pad] buffer.

Bounds.  u16 = one rounding of the loaded library's 16-bit type (2^-8 bf16, 2^-11 fp16), U = 2^-24.  The 16-bit kernels round in
two places: P (forward, dV) or dS (dQ, dK) is converted to 16 bits as the second MFMA's operand, and the result is rounded on the
store.  The softmax denominator l is summed from the unrounded fp32 values.  With exact fp32 arithmetic that gives, per element,
    o   u16 (P|v| + |o|)            dV  u16 (P^T|dO| + |dV|)
    dQ  u16 (scale |dS||k| + |dQ|)  dK  u16 (scale |dS|^T|q| + |dK|)
and there is no other factor.  The rank-1 [cls] forms, the light [cls] block and the fp32 scratch rows keep P / dS of the extra
token in fp32: they round less, the same bound covers them.  Below its smallest normal number (2^-14 for fp16) a 16-bit type
rounds absolutely, by at most TINY = smallest_normal * u16: every rounded element may be off by that much, so a sum of n of them
times |x| carries TINY sum|x|, and a store carries TINY (bf16: 2^-134, nothing; fp16: 2^-25, about 1 % of the bound).

The fp32 allowance on top, as relative error `rho` of one P (natural-log domain, per query row i):
    (d + 2) U scale max_j |q_i|.|k_j|   the fp32 chain of the score (d products) and its scaling
    2 U X_i                             the rounded exponent argument, |x| <= X_i = 8 ln 2 + the row's score range under the lazy
                                        rescale (forward), = max|s| + |lse| (backward)
    U max_j |s_ij|                      the rounded product m * c that every argument of a tile shares (forward) / lse * log2 e
    2 U exp2_ulps                       the hardware exp2, measured away from the kernels (tests/test_elementwise_gpu._allowances)
and per rescale of the running sums one more exp2 with its argument: 1 + ceil(range / 8 octaves) rescales at most in the lazy
form, one per AT_TILE keys on the fp32 path.  The backward adds the error of the lse handed in (U |lse| for a float32 rounding of
the exact value, the forward's own lse bound when the passes are chained).  Accumulations add chain-length terms (nk or nq) U.
    dS = P (dP - delta): rho |dS| + 3 U |dS| + (d + 2) U P (|dO_i|.|v_j| + |dO_i|.|o_i|).
lse (absolute, per row): a score error passes one to one (it is in rho), plus the relative error of l (rho, nk U), the rounded
m * scale (U max|s|), the log allowance in units of 2^-23 max(1, |log l|) with |log l| <= ln nk + 8 ln 2, and U |lse| for the sum.
The fp32 path uses the same formulas with U in place of u16 for P / dS (they stay fp32) and u16 for the store only when the
storage is 16-bit.

Inputs: N(0, 1) rounded to the 16-bit type; e = 0.25 in every fourth column (|e| = 1); 4e added to every query row, 8e to the
sentinel key rows (their scores rise by 4: each sentinel key holds a visible share of every row; 12e beyond 1024 keys,
`key_boost`), sentinel rows of dO times 32;
re-rounded after each step.  Sentinels sit at the edges of the 64-row tiles and 128-row blocks and at the [cls] token."""
import math

import torch

U = 2.0 ** -24
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
NAN = float("nan")
AT_TILE = 32            # attention_f32.hip: keys per tile (256 queries per block)
ATTN_EXTRA_MAX = 2048   # attn_bf16_dev.h: longest key sequence of the light [cls] block
CPU_ALLOW = {"exp2": 4.0, "log": 4.0}   # stand-ins where no GPU measures them (the fp32 terms are ~1e-3 of the 16-bit terms)


def half_dtype():
    from vfmseg_amd import lib as L
    return L.half_dtype()


def u16_of(dt):
    """One rounding (round to nearest) of a 16-bit type: 2^-8 for bf16, 2^-11 for fp16."""
    return torch.finfo(dt).eps / 2.0


def tiny_of(dt):
    return torch.finfo(dt).smallest_normal * u16_of(dt)


def rnd(x, dt):
    """x rounded once to dt, as float64"""
    return x.to(dt).double()


class Shape:
    def __init__(self, B, H, d, nq_main, nq_extra, nk_main, nk_extra, scale=None):
        self.B, self.H, self.d = B, H, d
        self.nq_main, self.nq_extra, self.nk_main, self.nk_extra = nq_main, nq_extra, nk_main, nk_extra
        self.nq, self.nk = nq_main + nq_extra, nk_main + nk_extra
        # the value the kernels are handed is a float: the reference uses that float
        self.scale = float(torch.tensor(d ** -0.5 if scale is None else scale, dtype=torch.float32).item())

    def key(self):
        return (self.B, self.H, self.d, self.nq_main, self.nq_extra, self.nk_main, self.nk_extra)

    def __repr__(self):
        return f"B{self.B} H{self.H} d{self.d} nq {self.nq_main}+{self.nq_extra} nk {self.nk_main}+{self.nk_extra}"


# ------------------------------------------------------------------------------------------------------------ layout
def to_tokens(x, n_main, n_extra):
    """[B, H, n_main + n_extra, d] -> token-major [B*n_main + B*n_extra, H*d], cls-last"""
    B, H, n, d = x.shape
    assert n == n_main + n_extra
    g = x.permute(0, 2, 1, 3)
    main = g[:, :n_main].reshape(B * n_main, H * d)
    return torch.cat([main, g[:, n_main:].reshape(B * n_extra, H * d)], 0) if n_extra else main


def from_tokens(t, B, H, d, n_main, n_extra):
    """token-major [rows, >= H*d] -> [B, H, n_main + n_extra, d]"""
    t = t[:, :H * d]
    main = t[:B * n_main].reshape(B, n_main, H, d)
    if n_extra:
        main = torch.cat([main, t[B * n_main:B * n_main + B * n_extra].reshape(B, n_extra, H, d)], 1)
    return main.permute(0, 2, 1, 3)


def nan_view(rows, cols, ld, dt, device):
    """The first `cols` columns of a NaN-filled [rows, ld] buffer."""
    return torch.full((rows, ld), NAN, dtype=dt, device=device)[:, :cols]


def outside_is_nan(t):
    """Every element of t's storage outside the view t is still NaN (tests/launch_replay.outside_is_nan)."""
    n = t.untyped_storage().nbytes() // t.element_size()
    inside = torch.zeros(n, dtype=torch.bool, device=t.device)
    torch.as_strided(inside, t.shape, t.stride(), t.storage_offset()).fill_(True)
    flat = torch.as_strided(t, (n,), (1,), 0)
    return bool(torch.isnan(flat[~inside].float()).all())


def view_ok(*views):
    """Everything inside every view is finite; everything outside the union of the views that share a storage is still NaN."""
    groups = {}
    for v in views:
        if not bool(torch.isfinite(v.float()).all()):
            return False
        groups.setdefault(v.untyped_storage().data_ptr(), []).append(v)
    for vs in groups.values():
        t = vs[0]
        n = t.untyped_storage().nbytes() // t.element_size()
        inside = torch.zeros(n, dtype=torch.bool, device=t.device)
        for v in vs:
            torch.as_strided(inside, v.shape, v.stride(), v.storage_offset()).fill_(True)
        if not bool(torch.isnan(torch.as_strided(t, (n,), (1,), 0)[~inside].float()).all()):
            return False
    return True


class Operands:
    """Device buffers of one case.  packed=False: every operand contiguous in a buffer of its own.  packed=True: q | k | v are
    column slices of one [rows, 3*H*d + pad] buffer (rows = the longer side), dq | dk | dv of another, o and dO have leading
    dimension H*d + pad.  Inputs are written into their views, outputs are NaN; everything outside a view is NaN."""

    def __init__(self, shp, dt, device, packed, pad=8):
        self.shp, self.dt, self.packed = shp, dt, packed
        hd = shp.H * shp.d
        rq, rk = shp.B * shp.nq, shp.B * shp.nk
        if packed:
            rows, ld3 = max(rq, rk), 3 * hd + pad
            a = torch.full((rows, ld3), NAN, dtype=dt, device=device)
            g = torch.full((rows, ld3), NAN, dtype=dt, device=device)
            self.q, self.k, self.v = a[:rq, :hd], a[:rk, hd:2 * hd], a[:rk, 2 * hd:3 * hd]
            self.dq, self.dk, self.dv = g[:rq, :hd], g[:rk, hd:2 * hd], g[:rk, 2 * hd:3 * hd]
            self.o, self.do = (nan_view(rq, hd, hd + pad, dt, device) for _ in range(2))
        else:
            self.q, self.o, self.do, self.dq = (nan_view(rq, hd, hd, dt, device) for _ in range(4))
            self.k, self.v, self.dk, self.dv = (nan_view(rk, hd, hd, dt, device) for _ in range(4))
        self.lse = torch.full((shp.B, shp.H, shp.nq), NAN, dtype=torch.float32, device=device)

    def put(self, **named):
        """named [B, H, n, d] float64 values -> the views"""
        s = self.shp
        for name, x in named.items():
            ne, nm = (s.nq_extra, s.nq_main) if name in ("q", "o", "do") else (s.nk_extra, s.nk_main)
            getattr(self, name).copy_(to_tokens(x, nm, ne).to(self.dt))

    def get(self, name):
        """a view -> [B, H, n, d] float64 on the CPU"""
        s = self.shp
        ne, nm = (s.nq_extra, s.nq_main) if name in ("q", "o", "do", "dq") else (s.nk_extra, s.nk_main)
        return from_tokens(getattr(self, name).detach().cpu().double(), s.B, s.H, s.d, nm, ne)


# ------------------------------------------------------------------------------------------------------------ inputs
def sentinels(n_main, n_extra):
    """Sequence positions at the tile / block edges and the [cls] token (position n_main)."""
    pos = [p for p in (0, 63, 64, 127, 128, 255, 256) if p < n_main] + [n_main - 1]
    if n_extra:
        pos.append(n_main)
    return sorted(set(pos))


def unit_e(d):
    e = torch.zeros(d, dtype=torch.float64)
    e[::4] = 0.25
    return e     # d = 64: sixteen entries of 0.25, |e| = 1


def key_boost(nk):
    """8 (e^4 = 55 times the weight of an ordinary key); 12 beyond 1024 keys, where a sentinel's share of a row would otherwise fall
    under the 16-bit rounding of the other two thousand (tests/test_attention_cpu.py: the visibility condition failed at 2048 + 1)"""
    return 8.0 if nk <= 1024 else 12.0


def make_inputs(shp, dt, seed=0):
    """-> dict q, k, v, do: [B, H, n, d] float64 values exact in dt, with the sentinels of the module docstring"""
    g = torch.Generator().manual_seed(1000 + seed)
    B, H, d = shp.B, shp.H, shp.d
    q, k, v, do = (rnd(torch.randn(B, H, n, d, generator=g, dtype=torch.float64), dt) for n in (shp.nq, shp.nk, shp.nk, shp.nq))
    e = unit_e(d)
    q = rnd(q + 4.0 * e, dt)
    ks = sentinels(shp.nk_main, shp.nk_extra)
    k[:, :, ks] = rnd(k[:, :, ks] + key_boost(shp.nk) * e, dt)
    qs = sentinels(shp.nq_main, shp.nq_extra)
    do[:, :, qs] = rnd(do[:, :, qs] * 32.0, dt)
    return {"q": q, "k": k, "v": v, "do": do}


# ------------------------------------------------------------------------------------------------------------ references
def forward_ref(q, k, v, scale, drop_key=None):
    """softmax(scale q k^T) v in float64 -> (o, lse, P, s); drop_key: that key does not exist (a mutant)"""
    s = scale * (q @ k.transpose(-1, -2))
    if drop_key is not None:
        s = s.clone()
        s[..., drop_key] = -math.inf
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    return P @ v, lse, P, s


def backward_ref(q, k, v, o, lse, do, scale, drop_key=None, drop_query=None):
    """The backward by hand, float64: P from the float64 softmax (lse is the kernels' operand, not the reference's), delta from the
    o that is handed to the kernel.  -> (dq, dk, dv, P, dS).  drop_key: dS loses that column for dQ; drop_query: P and dS lose
    that row for dK / dV (mutants)."""
    s = scale * (q @ k.transpose(-1, -2))
    P = torch.softmax(s, -1)
    delta = (do * o).sum(-1, keepdim=True)
    dS = P * (do @ v.transpose(-1, -2) - delta)
    dSq, Pk, dSk = dS, P, dS
    if drop_key is not None:
        dSq = dS.clone()
        dSq[..., drop_key] = 0.0
    if drop_query is not None:
        Pk, dSk = P.clone(), dS.clone()
        Pk[..., drop_query, :] = 0.0
        dSk[..., drop_query, :] = 0.0
    dq = scale * (dSq @ k)
    dk = scale * (dSk.transpose(-1, -2) @ q)
    dv = Pk.transpose(-1, -2) @ do
    return dq, dk, dv, P, dS


# ------------------------------------------------------------------------------------------------------------ bounds
def _absdot(a, b):
    return a.abs() @ b.abs().transpose(-1, -2)


def _rho_fwd(q, k, s, scale, d, allow, f32_path):
    """relative fp32 error of one unnormalised P and of the running sums, per query row [B, H, nq] (module docstring)"""
    nk = k.shape[-2]
    smax, smin = s.max(-1).values, s.min(-1).values
    rng = smax - smin
    X = rng + 8.0 * LN2
    base = (d + 2) * U * scale * _absdot(q, k).max(-1).values + 2 * U * X + U * s.abs().max(-1).values + 2 * U * allow["exp2"]
    resc = 2 * U * allow["exp2"] + 2 * U * X + U
    n_resc = torch.full_like(rng, math.ceil(nk / AT_TILE)) if f32_path else 1.0 + torch.ceil(rng * LOG2E / 8.0)
    return base + n_resc * resc


def forward_bounds(q, k, v, scale, dt_store, allow=CPU_ALLOW, f32_path=False, ref=None):
    """-> (bound_o [B, H, nq, d], bound_lse [B, H, nq]).  dt_store: the storage type (its rounding on the store; on the 16-bit path
    also the rounding of P)."""
    o, lse, P, s = forward_ref(q, k, v, scale) if ref is None else ref
    d, nk = q.shape[-1], k.shape[-2]
    half = dt_store != torch.float32
    u_out = u16_of(dt_store) if half else U
    u_p = U if f32_path else u_out
    tiny = tiny_of(dt_store) if half else 0.0
    rho = _rho_fwd(q, k, s, scale, d, allow, f32_path)
    Pv = P @ v.abs()
    b_o = u_p * Pv + u_out * o.abs() + (1.0 + u_p) * (2.0 * rho + (nk + 4) * U)[..., None] * Pv
    if not f32_path:
        # P below the type's normal range rounds absolutely: sum_j TINY |v_j| / l, and l (relative to the reference maximum the
        # lazy rescale keeps, which is never above the row's maximum) >= sum_j exp(s_j - max s) = exp(lse - max s)
        b_o = b_o + tiny * (v.abs().sum(-2, keepdim=True) / torch.exp(lse - s.max(-1).values)[..., None])
    b_o = b_o + tiny
    logl = math.log(nk) + 8.0 * LN2
    b_lse = rho + nk * U + U * s.abs().max(-1).values + 2 * U * allow["log"] * max(1.0, logl) + U * lse.abs()
    return b_o, b_lse


def backward_bounds(q, k, v, o, lse, do, scale, dt_store, allow=CPU_ALLOW, f32_path=False, lse_err=None, ref=None):
    """-> (bound_dq, bound_dk, bound_dv).  lse_err [B, H, nq]: absolute error of the lse handed to the kernel (default: its
    float32 rounding, U |lse|)."""
    dq, dk, dv, P, dS = backward_ref(q, k, v, o, lse, do, scale) if ref is None else ref
    d, nq, nk = q.shape[-1], q.shape[-2], k.shape[-2]
    half = dt_store != torch.float32
    u_out = u16_of(dt_store) if half else U
    u_p = U if f32_path else u_out
    tiny = tiny_of(dt_store) if half else 0.0
    s = scale * (q @ k.transpose(-1, -2))
    if lse_err is None:
        lse_err = U * lse.abs()
    smx = s.abs().max(-1).values
    rho = ((d + 2) * U * scale * _absdot(q, k).max(-1).values + 2 * U * (smx + lse.abs()) + U * (smx + lse.abs())
           + 2 * U * allow["exp2"] + lse_err)[..., None]
    aP, adS, ado = P, dS.abs(), do.abs()
    E_dS = rho * adS + 3 * U * adS + (d + 2) * U * P * (_absdot(do, v) + (ado * o.abs()).sum(-1, keepdim=True))
    Pdo = aP.transpose(-1, -2) @ ado
    b_dv = (u_p * Pdo + u_out * dv.abs() + (1.0 + u_p) * ((rho * aP).transpose(-1, -2) @ ado + (nq + 2) * U * Pdo)
            + tiny * (1.0 + (0.0 if f32_path else 1.0) * ado.sum(-2, keepdim=True)))
    dSk = adS @ k.abs()
    b_dq = (u_p * scale * dSk + u_out * dq.abs() + (1.0 + u_p) * scale * (E_dS @ k.abs() + (nk + 2) * U * dSk)
            + tiny * (1.0 + (0.0 if f32_path else 1.0) * scale * k.abs().sum(-2, keepdim=True)))
    dSq = adS.transpose(-1, -2) @ q.abs()
    b_dk = (u_p * scale * dSq + u_out * dk.abs() + (1.0 + u_p) * scale * (E_dS.transpose(-1, -2) @ q.abs() + (nq + 2) * U * dSq)
            + tiny * (1.0 + (0.0 if f32_path else 1.0) * scale * q.abs().sum(-2, keepdim=True)))
    return b_dq, b_dk, b_dv


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (inf where got is not finite)"""
    r = (got - ref).abs() / bound
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))
    return r.max().item()


def within(got, ref, bound):
    """The verdict of the per-element comparison (the GPU tests assert it; the mutant self-checks expect False)."""
    return worst_ratio(got, ref, bound) <= 1.0


# ------------------------------------------------------------------------------------------------------------ rounding model
def rounding_model(inp, scale, dt):
    """What an exact-arithmetic kernel that rounds where the 16-bit kernels round would return: P / dS rounded to dt as MFMA
    operands, every output rounded on the store; o handed to the backward is the rounded float64 output."""
    q, k, v, do = inp["q"], inp["k"], inp["v"], inp["do"]
    o, lse, P, _ = forward_ref(q, k, v, scale)
    o16 = rnd(o, dt)
    _, _, _, _, dS = backward_ref(q, k, v, o16, lse, do, scale)
    P16, dS16 = rnd(P, dt), rnd(dS, dt)
    return {"o": rnd(P16 @ v, dt), "dq": rnd(scale * (dS16 @ k), dt), "dk": rnd(scale * (dS16.transpose(-1, -2) @ q), dt),
            "dv": rnd(P16.transpose(-1, -2) @ do, dt)}


# ------------------------------------------------------------------------------------------------------------ mutants
def swap_cls(x, n_main):
    """every image reads the [cls] row of the next image"""
    x = x.clone()
    x[:, :, n_main] = torch.roll(x[:, :, n_main], -1, 0)
    return x


def next_head(x):
    """every head reads the columns of head h + 1"""
    return torch.roll(x, -1, 1)


def mutants(shp, inp, o16, lse):
    """Wrong results a kernel with one index error would return, from the float64 reference alone.
    -> {name: {output name: mutated reference}}; an output a mutant leaves alone is absent."""
    q, k, v, do, sc = inp["q"], inp["k"], inp["v"], inp["do"], shp.scale
    out = {}
    for j in sentinels(shp.nk_main, shp.nk_extra):
        out[f"drop_key{j}"] = {"o": forward_ref(q, k, v, sc, drop_key=j)[0], "dq": backward_ref(q, k, v, o16, lse, do, sc, drop_key=j)[0]}
    for i in sentinels(shp.nq_main, shp.nq_extra):
        r = backward_ref(q, k, v, o16, lse, do, sc, drop_query=i)
        out[f"drop_query{i}"] = {"dk": r[1], "dv": r[2]}

    def rerun(mq, mk, mv, mo, mdo):
        r = backward_ref(mq, mk, mv, mo, lse, mdo, sc)
        return {"o": forward_ref(mq, mk, mv, sc)[0], "dq": r[0], "dk": r[1], "dv": r[2]}

    if shp.B > 1 and (shp.nq_extra or shp.nk_extra):
        fq = (lambda x: swap_cls(x, shp.nq_main)) if shp.nq_extra else (lambda x: x)
        fk = (lambda x: swap_cls(x, shp.nk_main)) if shp.nk_extra else (lambda x: x)
        out["other_image_cls"] = rerun(fq(q), fk(k), fk(v), fq(o16), fq(do))
    if shp.H > 1:
        out["next_head"] = rerun(next_head(q), next_head(k), next_head(v), next_head(o16), next_head(do))
    return out


def visible_share(mut, ref, bound, factor=4.0):
    """share of the rows the mutant changes at all in which some element moves by >= factor x its bound"""
    moved = (mut - ref).abs()
    rows = moved.amax(-1) > 0
    if not bool(rows.any()):
        return 0.0
    seen = (moved >= factor * bound).any(-1)
    return (seen & rows).sum().item() / rows.sum().item()


# ------------------------------------------------------------------------------------------------------------ dispatch
def _cdiv(a, b):
    return (a + b - 1) // b


def form_of(desc, short_grid=256, half=True, xcd=1):
    """The dispatch of vfm_attn_fwd / vfm_attn_bwd restated (attention.hip, vfm_attn_bf16_fwd_impl / _bwd_impl, k_attn_bf16_q,
    k_attn_bf16_dkv).  desc: a Shape; half: 16-bit storage; short_grid / xcd: the vfm_tune knobs."""
    s = desc
    if not (half and s.d == 64):
        return {"path": "f32", "q_blocks": _cdiv(s.nq, 256), "k_blocks": _cdiv(s.nk, 256), "k_tail": s.nk % AT_TILE != 0,
                "q_tail": s.nq % AT_TILE != 0}
    pairs = s.B * s.H

    def short(n):
        return _cdiv(n, 128) * pairs < short_grid

    f = {"path": "mfma", "xcd_map": bool(xcd) and pairs % 8 == 0}
    # forward
    nw = 2 if short(s.nq) else 4
    f["fwd_waves"] = nw
    f["light"] = nw == 4 and s.nq_extra == 1 and s.nq_main % 128 == 0 and s.nk <= ATTN_EXTRA_MAX
    f["r1"] = nw == 4 and s.nk_extra == 1
    f["fwd_k_tail"] = (s.nk_main if f["r1"] else s.nk) % 64 != 0
    f["fwd_q_ragged"] = s.nq % (32 * nw) != 0 and not f["light"]
    f["cls_query_alone"] = nw == 4 and s.nq_extra == 1 and not f["light"] and s.nq_main % 128 == 0
    # backward
    cls = s.nq_extra == 1 and s.nk_extra == 1 and s.nq_main == s.nk_main and s.nq_main % 128 == 0 and not short(s.nq)
    f["cls"] = cls
    f["dq_waves"] = 2 if short(s.nq) else 4
    f["dkv_waves"] = 2 if short(s.nk) else 4
    f["dq_r1"] = f["dq_waves"] == 4 and s.nk_extra == 1 and cls
    f["dq_k_tail"] = (s.nk_main if f["dq_r1"] else s.nk) % 64 != 0
    dkv_r1 = f["dkv_waves"] == 4 and s.nq_extra == 1 and cls
    f["dkv_q_tail"] = (s.nq_main if dkv_r1 else s.nq) % 64 != 0
    return f


def form_name(f, bwd=False):
    if f["path"] == "f32":
        return "f32"
    if bwd:
        return (f"dq{f['dq_waves']}w+dkv{f['dkv_waves']}w" + ("+cls" if f["cls"] else "") + ("+ktail" if f["dq_k_tail"] else "")
                + ("+qtail" if f["dkv_q_tail"] else "") + ("+xcd" if f["xcd_map"] else ""))
    return (f"fwd{f['fwd_waves']}w" + ("+r1" if f["r1"] else "") + ("+light" if f["light"] else "") + ("+ktail" if f["fwd_k_tail"] else "")
            + ("+qragged" if f["fwd_q_ragged"] else "") + ("+xcd" if f["xcd_map"] else ""))


# ------------------------------------------------------------------------------------------------------------ cases
TWO_WAVE, FOUR_WAVE = 1 << 30, 0      # vfm_tune("attn_short_grid"): every grid is short / none is


def _case(B, H, nq, nqe, nk, nke, short_grid, d=64, **want):
    return {"shape": Shape(B, H, d, nq, nqe, nk, nke), "short_grid": short_grid, "want": want}


# name -> shape, the attn_short_grid knob, and the entries of form_of the case is named for
FWD_CASES = {
    "F1": _case(2, 3, 130, 0, 70, 0, TWO_WAVE, fwd_waves=2, fwd_k_tail=True, fwd_q_ragged=True, r1=False, light=False),
    "F1b": _case(2, 3, 130, 0, 5, 0, TWO_WAVE, fwd_waves=2, fwd_k_tail=True, fwd_q_ragged=True),
    "F2": _case(2, 3, 200, 1, 200, 1, TWO_WAVE, fwd_waves=2, r1=False, light=False, fwd_k_tail=True),
    "F3-xcd": _case(2, 4, 200, 1, 200, 1, FOUR_WAVE, fwd_waves=4, r1=True, light=False, fwd_k_tail=True, fwd_q_ragged=True, xcd_map=True),
    "F3-plain": _case(2, 3, 200, 1, 200, 1, FOUR_WAVE, fwd_waves=4, r1=True, light=False, fwd_k_tail=True, fwd_q_ragged=True, xcd_map=False),
    "F4-xcd": _case(2, 4, 256, 1, 256, 1, FOUR_WAVE, fwd_waves=4, r1=True, light=True, fwd_k_tail=False, xcd_map=True),
    "F4-plain": _case(2, 3, 256, 1, 256, 1, FOUR_WAVE, fwd_waves=4, r1=True, light=True, fwd_k_tail=False, xcd_map=False),
    "F5": _case(2, 1, 128, 1, 2048, 1, FOUR_WAVE, fwd_waves=4, r1=True, light=False, cls_query_alone=True),
    "F6a": _case(2, 3, 200, 0, 200, 1, FOUR_WAVE, fwd_waves=4, r1=True, light=False, fwd_k_tail=True),
    "F6a-2w": _case(2, 3, 200, 0, 200, 1, TWO_WAVE, fwd_waves=2, r1=False, light=False, fwd_k_tail=True),
    "F6b": _case(2, 3, 128, 1, 192, 0, FOUR_WAVE, fwd_waves=4, r1=False, light=True, fwd_k_tail=False),
    "F6b-2w": _case(2, 3, 128, 1, 192, 0, TWO_WAVE, fwd_waves=2, r1=False, light=False, fwd_q_ragged=True),
    "F7": _case(2, 4, 256, 0, 256, 0, FOUR_WAVE, fwd_waves=4, r1=False, light=False, fwd_k_tail=False, fwd_q_ragged=False),
}
BWD_CASES = {
    "B1": _case(2, 3, 200, 1, 200, 1, TWO_WAVE, dq_waves=2, dkv_waves=2, cls=False),
    "B2": _case(2, 4, 256, 1, 256, 1, FOUR_WAVE, dq_waves=4, dkv_waves=4, cls=True, dq_r1=True, xcd_map=True),
    "B3": _case(2, 3, 200, 1, 200, 1, FOUR_WAVE, dq_waves=4, dkv_waves=4, cls=False, dq_r1=False, dq_k_tail=True, dkv_q_tail=True),
    "B4-dq2w": _case(2, 4, 100, 0, 300, 0, 12, dq_waves=2, dkv_waves=4, cls=False),
    "B4-dkv2w": _case(2, 4, 300, 0, 100, 0, 12, dq_waves=4, dkv_waves=2, cls=False),
    "B4-extras": _case(2, 4, 100, 1, 300, 1, 12, dq_waves=2, dkv_waves=4, cls=False),
}
CHAIN_CASES = {
    "B5-4w": _case(2, 4, 256, 1, 256, 1, FOUR_WAVE, fwd_waves=4, light=True, r1=True, cls=True),
    "B5-2w": _case(2, 3, 200, 1, 200, 1, TWO_WAVE, fwd_waves=2, dq_waves=2, dkv_waves=2, cls=False),
}
# attention_f32.hip: AT_TILE = 32 keys per tile, 256 queries (keys) per block; d = 80 has a forward only (SAM ViT-H's fallback)
F32_CASES = {
    "X1": _case(2, 2, 257, 1, 33, 0, 256, path="f32", q_blocks=2, k_blocks=1, k_tail=True),
    "X2": _case(2, 2, 31, 0, 65, 1, 256, path="f32", q_blocks=1, k_blocks=1, k_tail=True, q_tail=True),
    "X3-d80": _case(2, 2, 200, 0, 197, 0, 256, d=80, path="f32", k_tail=True),
}
BACKBONE_SHAPES = [(B, H, n) for n in (1024, 1369, 2048) for (B, H) in ((2, 16), (1, 16))]


def landed(case, half=True, xcd=1):
    """form_of at the case's knob; asserts the entries the case is named for -> the form"""
    f = form_of(case["shape"], short_grid=case["short_grid"], half=half, xcd=xcd)
    for key, val in case["want"].items():
        assert f[key] == val, (case["shape"], key, f[key], val)
    return f
