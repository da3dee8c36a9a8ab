"""Every entry of csrc/sam.hip, the row-softmax trio, vfm_resize_bicubic and vfm_scale_by_device_scalar against the float64
restatements of tests/sam_window_helpers.py (pinned to the oracle by tests/test_sam_window_cpu.py), at small shapes that take every
kernel form and every selector of the dispatchers.  Output buffers start as NaN, or as a sentinel where the contract says "left
untouched".  The 16-bit type is spelled torch.bfloat16 so that the fp16 pass (tests/test_fp16_twin_gpu.py) re-types it.

Which case reaches which kernel of sam.hip:
  k_sam_relpos               test_relpos_table (all six (L, S))
  k_sam_prep_rows            test_prep: every float32 case with S <= 32 and d <= 128; 16-bit (7,7,16) (odd S), (4,4,9) (odd d),
                             and 16-bit (14,20,80) / (6,15,10) in the variants "oddld" and "offset2" (the x2 form must decline)
  k_sam_prep_rows_bf16x2     test_prep: 16-bit (14,20,80) and (6,15,10), variants "plain" and "nobias_wide_padded"
  k_sam_prep                 test_prep: (33,33,8) (S > 32) and (4,8,130) (d > 128), both dtypes
  k_softmax_rows             test_softmax_rows (register form n <= 1024, loop form n = 1025 / 1100)
  k_softmax_rows_b           test_softmax_rows_batched_and_bwd (forward + backward, register and loop forms, dead rows)
  k_sam_merge                test_merge: float32, odd d, odd ld
  k_sam_merge_bf16x2         test_merge: 16-bit (14,20,2,80) and (6,15,3,10)
  k_sam_bwd_prep_tiles       test_bwd_prep "tiles" (NP = 256, dp = 128)
  k_sam_bwd_prep             test_bwd_prep "np200" (NP % 32 != 0) and "dp192" (dp > 128)
  k_sam_bwd_merge            test_bwd_merge
and all of them together in test_materialised_attention_* (SamEngine.attention / attention_bwd with the flash path off)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests import sam_window_helpers as W  # noqa: E402
from tests.helpers import _half_ulp, _rounded, _within, rel_err  # noqa: E402,F401
from vfmseg_amd import ops  # noqa: E402

U24 = 2.0 ** -24
SENT = -77.0                      # exact in float32, bf16 and fp16
FLT_MIN = 2.0 ** -126


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _dtname(dt):
    return "f32" if dt == torch.float32 else "h16"


DTYPES = [torch.float32, torch.bfloat16]


# ------------------------------------------------------------------------------------------------------------ relpos table
@pytest.mark.parametrize("L,S", [(27, 14), (13, 7), (27, 7), (9, 7), (127, 32), (5, 33)])
def test_relpos_table(L, S):
    """Exact-length gather (L = 2S-1), down- and up-interpolation.  Against ATen's float32 linear interpolation (same float32 source
    index): 4 ulp, one ulp being 2^-23 max|rel| - the blend (1-l) a + l b rounds at the magnitude of its operands, not of the (possibly
    cancelling) result.  Against float64: the float32 source index is off by at most 2^-22 L (two roundings at magnitude <= L), which
    moves the blend by that times the largest step between neighbouring rows, plus the blend's own rounding."""
    d = 10
    rel = torch.randn(L, d, generator=_gen(L, S))
    out = torch.full((S, S, d), float("nan"), device="cuda")
    ops.sam_relpos_table(rel.cuda(), S, out)
    amax = rel.abs().max().item()
    step = (rel[1:] - rel[:-1]).abs().max().item()
    maxrel = 2 * S - 1
    ref32 = W.relpos_table(rel, S).double()
    ref64 = W.relpos_table(rel.double(), S)
    _within(f"relpos L={L} S={S} vs ATen float32", out, ref32, torch.full_like(ref32, 4 * 2.0 ** -23 * amax))
    _within(f"relpos L={L} S={S} vs float64", out, ref64, torch.full_like(ref64, maxrel * (L / maxrel) * 2.0 ** -22 * step + 2.0 ** -23 * amax))
    if L == maxrel:
        assert torch.equal(out.cpu(), ref32.float())


# ------------------------------------------------------------------------------------------------------------ prep
PREP_CASES = [(14, 20, 80, 2, 1), (6, 15, 10, 3, 2), (7, 7, 16, 2, 2), (4, 4, 9, 3, 2), (33, 33, 8, 1, 1), (4, 8, 130, 2, 1)]  # S, G, d, H, nimg


def _strided_qkv(qkv, variant):
    """The same values behind another layout: column slice of a wider buffer (ld > 3C, even / odd) or a view that starts 2 bytes
    (one 16-bit element) past an aligned address."""
    M, C3 = qkv.shape
    if variant in ("nobias_wide_padded", "oddld"):
        wide = torch.full((M, C3 + (6 if variant == "nobias_wide_padded" else 5)), float("nan"), dtype=qkv.dtype, device="cuda")
        wide[:, 2:2 + C3] = qkv
        return wide[:, 2:2 + C3]
    if variant == "offset2":
        flat = torch.full((M * C3 + 1,), float("nan"), dtype=qkv.dtype, device="cuda")
        flat[1:] = qkv.reshape(-1)
        return flat[1:].view(M, C3)
    return qkv.cuda()


@pytest.mark.parametrize("variant", ["plain", "nobias_wide_padded", "oddld", "offset2"])
@pytest.mark.parametrize("dt", DTYPES, ids=_dtname)
@pytest.mark.parametrize("S,G,d,H,nimg", PREP_CASES)
def test_prep(S, G, d, H, nimg, dt, variant):
    g = _gen(S, G, d, 1)
    C, S2, M = H * d, S * S, nimg * G * G
    Dq = W.pad64(d + 2 * S)
    padded = variant == "nobias_wide_padded"
    rpb = NP = W.pad64(S2) if padded else S2
    qkv = (torch.randn(M, 3 * C, generator=g) * 1.5).to(dt)
    bias = None if padded else torch.randn(3 * C, generator=g) * 0.5 + 0.25
    rh, rw = torch.randn(S, S, d, generator=g) * 0.3, torch.randn(S, S, d, generator=g) * 0.3
    scale = d ** -0.5
    nws = (G + S - 1) // S
    nb = nimg * nws * nws * H
    qa = torch.full((nb, rpb, Dq), SENT, dtype=dt, device="cuda")
    ka = torch.full((nb, rpb, Dq), SENT, dtype=dt, device="cuda")
    vw = torch.full((nb, NP, d), SENT, dtype=dt, device="cuda")
    ops.sam_attn_prep(_strided_qkv(qkv.cuda(), variant), None if bias is None else bias.cuda(), rh.cuda(), rw.cuda(), qa, ka, vw,
                      nimg, G, S, H, d, scale)
    qa, ka, vw = qa.cpu(), ka.cpu(), vw.cpu()
    q, k, v, inside = W.window_qkv(qkv.float(), bias, nimg, G, S, H, d)                  # float32 copies: exact
    if G % S:
        assert not inside.all()                                                           # the case really has padded tokens
    _, ka32, _ = W.prep_ref(qkv.float(), bias, rh, rw, nimg, G, S, H, d, Dq, scale)
    name = f"prep S={S} G={G} d={d} {_dtname(dt)} {variant}"
    assert torch.equal(qa[:, :S2, :d], (q * torch.tensor(scale, dtype=torch.float32)).to(dt)), name + ": scale*q"
    assert torch.equal(ka[:, :S2, :d], k.to(dt)), name + ": k copy"
    assert torch.equal(vw[:, :S2], v.to(dt)), name + ": v copy"
    assert torch.equal(ka[:, :S2, d:], ka32[..., d:].to(dt)), name + ": one-hot / zero columns of k_aug"
    assert (qa[:, :S2, d + 2 * S:] == 0).all(), name + ": zero columns of q_aug"
    assert (qa[:, S2:] == SENT).all() and (ka[:, S2:] == SENT).all() and (vw[:, S2:] == SENT).all(), name + ": rows past S*S touched"
    b64 = None if bias is None else bias.double()
    ref = W.prep_ref(qkv.double(), b64, rh.double(), rw.double(), nimg, G, S, H, d, Dq, scale)[0][..., d:d + 2 * S]
    mag = W.prep_bias_magnitude(qkv.double(), b64, rh.double(), rw.double(), nimg, G, S, H, d)
    _within(name + " bias columns", qa[:, :S2, d:d + 2 * S], ref, _rounded(ref, d * U24 * mag, dt))


# ------------------------------------------------------------------------------------------------------------ merge
@pytest.mark.parametrize("S,G,H,d,NP,ldx,dt", [
    (14, 20, 2, 80, 256, 6, torch.bfloat16), (6, 15, 3, 10, 64, 2, torch.bfloat16),      # x2 form: padded windows, NP > S*S, ld > H*d
    (14, 20, 2, 80, 256, 6, torch.float32), (6, 15, 3, 10, 36, 0, torch.float32),        # generic via float32
    (4, 4, 3, 9, 16, 4, torch.bfloat16), (7, 7, 2, 16, 64, 3, torch.bfloat16),           # generic via odd d, via odd ld
], ids=lambda v: _dtname(v) if isinstance(v, torch.dtype) else str(v))
def test_merge(S, G, H, d, NP, ldx, dt):
    nimg = 2
    nws = (G + S - 1) // S
    nb, M = nimg * nws * nws * H, nimg * G * G
    ow = torch.randn(nb, NP, d, generator=_gen(S, G, d, 2)).to(dt)
    out = torch.full((M, H * d + ldx), SENT, dtype=dt, device="cuda")
    ops.sam_attn_merge(ow.cuda(), out, nimg, G, S, H, d)
    out = out.cpu()
    assert torch.equal(out[:, :H * d], W.merge_ref(ow, nimg, G, S, H, d))
    assert (out[:, H * d:] == SENT).all()


# ------------------------------------------------------------------------------------------------------------ backward prep
@pytest.mark.parametrize("dt", DTYPES, ids=_dtname)
@pytest.mark.parametrize("form,S,G,H,d,dp,NP,with_bias", [("tiles", 14, 20, 2, 80, 128, 256, True), ("np200", 14, 20, 2, 80, 128, 200, True),
                                                          ("dp192", 14, 20, 2, 80, 192, 256, False), ("tiles_small", 6, 15, 3, 10, 64, 64, True)])
def test_bwd_prep(form, S, G, H, d, dp, NP, with_bias, dt):
    g = _gen(S, G, dp, NP)
    nimg, C = 1, H * d
    M = nimg * G * G
    nws = (G + S - 1) // S
    nb = nimg * nws * nws * H
    qkv = (torch.randn(M, 3 * C, generator=g) * 1.5).to(dt)
    dao = torch.randn(M, C, generator=g).to(dt)
    bias = torch.randn(3 * C, generator=g) * 0.5 + 0.25 if with_bias else None
    scale = d ** -0.5
    dao_w = torch.full((M, C + 4), float("nan"), dtype=dt, device="cuda")              # ld_dao > C
    dao_w[:, :C] = dao
    nan = lambda *s: torch.full(s, float("nan"), dtype=dt, device="cuda")               # noqa: E731
    dow, dowT, vp, qsT = nan(nb, NP, dp), nan(nb, dp, NP), nan(nb, NP, dp), nan(nb, dp, NP)
    ops.sam_attn_bwd_prep(dao_w[:, :C], qkv.cuda(), None if bias is None else bias.cuda(), dow, dowT, vp, qsT, nimg, G, S, H, d, scale)
    ref = W.bwd_prep_ref(dao.float(), qkv.float(), bias, nimg, G, S, H, d, dp, NP, torch.tensor(scale, dtype=torch.float32))
    for nm, got, want in zip(("dow", "dowT", "vp", "qsT"), (dow, dowT, vp, qsT), ref):
        assert torch.equal(got.cpu(), want.to(dt)), (form, nm)                            # NaN left anywhere fails too


# ------------------------------------------------------------------------------------------------------------ backward merge
@pytest.mark.parametrize("dt", DTYPES, ids=_dtname)
@pytest.mark.parametrize("S,G,d,H,nimg", PREP_CASES)
def test_bwd_merge(S, G, d, H, nimg, dt):
    g = _gen(S, G, d, 3)
    C, S2, M = H * d, S * S, nimg * G * G
    Dq, NP, dp = W.pad64(d + 2 * S), W.pad64(S2), W.pad64(d)
    nws = (G + S - 1) // S
    nb = nimg * nws * nws * H
    dqa = torch.randn(nb, NP, Dq, generator=g).to(dt)
    dkT, dvT = torch.randn(nb, dp, NP, generator=g).to(dt), torch.randn(nb, dp, NP, generator=g).to(dt)
    rh, rw = torch.randn(S, S, d, generator=g) * 0.3, torch.randn(S, S, d, generator=g) * 0.3
    scale = d ** -0.5
    dqkv = torch.full((M, 3 * C), float("nan"), dtype=dt, device="cuda")
    ops.sam_attn_bwd_merge(dqa.cuda(), dkT.cuda(), dvT.cuda(), rh.cuda(), rw.cuda(), dqkv, nimg, G, S, H, d, scale)
    dqkv = dqkv.cpu()
    exact = W.bwd_merge_ref(dqa.float(), dkT.float(), dvT.float(), rh, rw, nimg, G, S, H, d, scale)
    assert torch.equal(dqkv[:, C:], exact[:, C:].to(dt)), "dk / dv are copies"
    ref = W.bwd_merge_ref(dqa.double(), dkT.double(), dvT.double(), rh.double(), rw.double(), nimg, G, S, H, d, scale)[:, :C]
    mag = W.bwd_merge_ref(dqa.double().abs(), dkT.double(), dvT.double(), rh.double().abs(), rw.double().abs(), nimg, G, S, H, d, scale)[:, :C]
    _within(f"bwd merge S={S} G={G} d={d} {_dtname(dt)} dq", dqkv[:, :C], ref, _rounded(ref, (2 * S + 1) * U24 * mag, dt))


# ------------------------------------------------------------------------------------------------------------ softmax trio
NS = [1, 63, 64, 65, 100, 196, 1000, 1024, 1025, 1100]
N_NPAD = sorted({(n, n) for n in NS} | {(n, W.pad64(n)) for n in NS} | {(1000, 1088)})


def _scores(rows, n, sigma, g):
    s = torch.randn(rows, n, generator=g) * sigma
    return s + (torch.arange(rows) % 2 * 2 - 1).float()[:, None] * 60.0                 # per-row offset of -60 / +60


def _wide(t, extra, fill, dtype=None):
    """t behind a leading dimension larger than its row length; the extra columns hold `fill`."""
    w = torch.full((t.shape[0], t.shape[1] + extra), fill, dtype=dtype or t.dtype, device="cuda")
    w[:, :t.shape[1]] = t
    return w


def _softmax_fwd_bound(s, p, n, dt, live=None):
    """|err| <= p (R log2(e) + 8) 2^-23 + half an ulp of the output type, R = max(row) - min(row): the fast exponential rounds its
    argument (s - max) log2(e), of magnitude up to R log2(e), to float32; the 8 covers the exponential itself, the sum and the
    normalisation.  The fast exponential (v_exp_f32) has no subnormal results: what would land below the float32 normal range comes
    out as 0, an absolute error of up to 2^-126 that no relative term covers, so the bound carries + 2^-126 (measured: 1.16e-38)."""
    R = (s.max(-1, keepdim=True).values - s.min(-1, keepdim=True).values).double()
    b = torch.zeros(p.shape, dtype=torch.float64)
    b1 = p[:, :n] * (R * 1.4426950408889634 + 8.0) * 2.0 ** -23 + FLT_MIN
    b[:, :n] = _rounded(p[:, :n], b1, dt)
    if live is not None:
        b[~live] = 0.0                                # dead rows: exactly 0
    return b


@pytest.mark.parametrize("dt", DTYPES, ids=_dtname)
@pytest.mark.parametrize("n,npad", N_NPAD)
def test_softmax_rows(n, npad, dt):
    """vfm_softmax_rows (Rein's token attention with rows_per_batch = valid_rows = 1 goes through the batched entry, below).  The
    (1000, 1088) case is the register-resident form with npad beyond its 1024 columns: columns 1024..1087 must be written."""
    for rows in (1, 5, 7):
        for sigma in (1.0, 20.0):
            s = _scores(rows, n, sigma, _gen(n, npad, rows, int(sigma)))
            out = torch.full((rows, npad + 3), SENT, dtype=dt, device="cuda")
            ops.softmax_rows(_wide(s, 5, float("nan"))[:, :n], out[:, :npad], n)
            out = out.cpu()
            p = torch.zeros(rows, npad, dtype=torch.float64)
            p[:, :n] = W.softmax_ref(s)
            _within(f"softmax_rows n={n} npad={npad} rows={rows} sigma={sigma:g} {_dtname(dt)}", out[:, :npad], p, _softmax_fwd_bound(s, p, n, dt))
            assert (out[:, npad:] == SENT).all()


@pytest.mark.parametrize("dt", DTYPES, ids=_dtname)
@pytest.mark.parametrize("n,npad", N_NPAD)
def test_softmax_rows_batched_and_bwd(n, npad, dt):
    """vfm_softmax_rows_batched and vfm_softmax_rows_bwd: dead rows (row % rows_per_batch >= valid_rows) hold NaN scores / dp and
    must come out exactly 0, as must the pad columns n..npad-1.  The backward is held to float64 p o (dp - sum p o dp) of the same
    rounded p: the dot product of n terms is within n 2^-24 sum|p dp|, the result scales it by p <= max p."""
    for rows, rpb, valid in ((1, 1, 1), (5, 1, 1), (7, 4, 3), (261, 256, 196)):
        for sigma in (1.0, 20.0):
            g = _gen(n, npad, rows, rpb, int(sigma))
            live = (torch.arange(rows) % rpb) < valid
            s = _scores(rows, n, sigma, g)
            s[~live] = float("nan")
            out = torch.full((rows, npad + 3), SENT, dtype=dt, device="cuda")
            ops.softmax_rows_batched(_wide(s, 5, float("nan"))[:, :n], out[:, :npad], n, rpb, valid)
            out = out.cpu()
            p = torch.zeros(rows, npad, dtype=torch.float64)
            p[:, :n] = W.softmax_ref(s, rpb, valid)
            sl = torch.where(live[:, None], s, torch.zeros(()))
            name = f"n={n} npad={npad} rows={rows} rpb={rpb} valid={valid} sigma={sigma:g} {_dtname(dt)}"
            _within("softmax_rows_batched " + name, out[:, :npad], p, _softmax_fwd_bound(sl, p, n, dt, live))
            assert (out[:, npad:] == SENT).all()
            # ---- backward from the reference probabilities rounded to the output type
            pr = p.to(dt)
            dp = torch.randn(rows, n, generator=g)
            dp[~live] = float("nan")
            ds = torch.full((rows, npad + 3), SENT, dtype=dt, device="cuda")
            ops.softmax_rows_bwd(_wide(pr, 3, 0.0)[:, :npad], _wide(dp, 5, float("nan"))[:, :n], ds[:, :npad], n, rpb, valid)
            ds = ds.cpu()
            ref = torch.zeros(rows, npad, dtype=torch.float64)
            ref[:, :n] = W.softmax_bwd_ref(pr[:, :n], dp, rpb, valid)
            pd, dl = pr[:, :n].double(), torch.where(live[:, None], dp, torch.zeros(())).double()
            b1 = n * U24 * (pd * dl).abs().sum(-1, keepdim=True) * pd.max(-1, keepdim=True).values
            bound = torch.zeros(rows, npad, dtype=torch.float64)
            bound[:, :n] = _rounded(ref[:, :n], b1.expand(rows, n), dt)
            bound[~live] = 0.0
            _within("softmax_rows_bwd " + name, ds[:, :npad], ref, bound)
            assert (ds[:, npad:] == SENT).all()


# ------------------------------------------------------------------------------------------------------------ whole materialised path
PATH_CASES = [(14, 20, 2, 80, 27), (6, 15, 3, 10, 13), (7, 7, 2, 16, 27)]   # S, G, H, d, L  (L != 2S-1 for the last two)


def _path_inputs(S, G, H, d, L, nimg):
    g = _gen(S, G, H, d, L)
    C = H * d
    qkv = torch.randn(nimg * G * G, 3 * C, generator=g) * 1.5
    bias = torch.randn(3 * C, generator=g) * 0.5 + 0.25
    rel_h, rel_w = torch.randn(L, d, generator=g) * 0.3, torch.randn(L, d, generator=g) * 0.3
    dout = torch.randn(nimg * G * G, C, generator=g)
    return qkv, bias, rel_h, rel_w, dout


def _run_engine(qkv, bias, rel_h, rel_w, dout, nimg, G, S, H, d, cd):
    """SamEngine.attention (inference and training form) and attention_bwd with a hand-made layer record; they use nothing of self."""
    from vfmseg_amd.sam import SamEngine
    dev = "cuda"
    rh, rw = torch.empty(S, S, d, device=dev), torch.empty(S, S, d, device=dev)
    ops.sam_relpos_table(rel_h.cuda(), S, rh)
    ops.sam_relpos_table(rel_w.cuda(), S, rw)
    Lp = dict(S=S, rh=rh, rw=rw, qkv_b=bias.cuda())
    x = qkv.to(cd).cuda()
    ao = SamEngine.attention(None, x, Lp, nimg, G, H, d, cd, dev)
    ao_t, pr = SamEngine.attention(None, x, Lp, nimg, G, H, d, cd, dev, keep=True)
    assert torch.is_tensor(pr), "the materialised path keeps the probabilities"
    dqkv = SamEngine.attention_bwd(None, dout.to(cd).cuda(), x, pr, Lp, nimg, G, H, d, cd, dev)
    return ao.float().cpu(), ao_t.float().cpu(), dqkv.float().cpu()


def _reference(qkv, bias, rel_h, rel_w, dout, nimg, G, S, H, d, dtype):
    x = qkv.to(dtype).requires_grad_(True)
    o = W.window_attention_ref(x, bias, rel_h, rel_w, nimg, G, S, H, d, dtype=dtype)
    o.backward(dout.to(dtype))
    return o.detach(), x.grad


@pytest.mark.parametrize("S,G,H,d,L", PATH_CASES)
def test_materialised_attention_float32(S, G, H, d, L):
    """prep -> batched GEMM -> row softmax -> GEMM -> merge and its backward on float32 qkv (the only SAM attention of the f32 and
    bf16x3 precision modes) against the float64 restatement and its autograd.  No tolerance is fixed: the same restatement run in
    float32 on the CPU gives e32, and the kernels must stay within 4 x e32 (accumulation order, fast exponential)."""
    nimg = 2
    qkv, bias, rel_h, rel_w, dout = _path_inputs(S, G, H, d, L, nimg)
    ao, ao_t, dqkv = _run_engine(qkv, bias, rel_h, rel_w, dout, nimg, G, S, H, d, torch.float32)
    ref_o, ref_g = _reference(qkv, bias, rel_h, rel_w, dout, nimg, G, S, H, d, torch.float64)
    o32, g32 = _reference(qkv, bias, rel_h, rel_w, dout, nimg, G, S, H, d, torch.float32)
    C = H * d
    checks = [("out", ao, ref_o, o32), ("out (training form)", ao_t, ref_o, o32)]
    checks += [(nm, dqkv[:, sl], ref_g[:, sl], g32[:, sl]) for nm, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C)))]
    bad = []
    for nm, got, ref, r32 in checks:
        e, e32 = rel_err(got, ref), rel_err(r32, ref)
        print(f"[sam materialised f32 S={S} G={G}] {nm} rel err {e:.2e}, float32 restatement {e32:.2e} (ratio {e / e32:.2f}, bound 4)")
        if not (torch.isfinite(got).all() and e <= 4 * e32):
            bad.append((nm, e, e32))
    assert not bad, bad


@pytest.mark.parametrize("S,G,H,d,L", PATH_CASES)
def test_materialised_attention_16bit(S, G, H, d, L, monkeypatch):
    """The same path with 16-bit operands and the flash kernels switched off, held to the bounds the flash tests use for the same
    operand precision (16-bit P and bias columns): 2e-2 forward, 3e-2 backward."""
    monkeypatch.setenv("VFMSEG_SAM_FLASH", "0")
    nimg = 2
    qkv, bias, rel_h, rel_w, dout = _path_inputs(S, G, H, d, L, nimg)
    qkv, dout = qkv.to(torch.bfloat16).float(), dout.to(torch.bfloat16).float()
    ao, ao_t, dqkv = _run_engine(qkv, bias, rel_h, rel_w, dout, nimg, G, S, H, d, torch.bfloat16)
    ref_o, ref_g = _reference(qkv, bias, rel_h, rel_w, dout, nimg, G, S, H, d, torch.float64)
    C = H * d
    checks = [("out", ao, ref_o, 2e-2), ("out (training form)", ao_t, ref_o, 2e-2)]
    checks += [(nm, dqkv[:, sl], ref_g[:, sl], 3e-2) for nm, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C)))]
    bad = []
    for nm, got, ref, tol in checks:
        e = rel_err(got, ref)
        print(f"[sam materialised 16-bit S={S} G={G}] {nm} rel err {e:.2e} (bound {tol:g})")
        if not (torch.isfinite(got).all() and e < tol):
            bad.append((nm, e))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ bicubic
@pytest.mark.parametrize("C", [1, 3, 70])
@pytest.mark.parametrize("s,hp,wp", [(5, 7, 3), (6, 2, 11), (4, 4, 9), (3, 1, 1), (37, 5, 5)])
def test_resize_bicubic(s, hp, wp, C):
    """Source scales as DinoEngine.pos_tokens passes them.  16 * 2^-24 * sum|w||x|: the cubic weights overshoot, so the rounding of the
    4 x 4 products is bounded by the tap magnitudes, not by the output."""
    x = torch.randn(s, s, C, generator=_gen(s, hp, wp, C))
    sy, sx = s / (hp + 0.1), s / (wp + 0.1)
    out = torch.full((hp * wp, C), float("nan"), device="cuda")
    ops.resize_bicubic(x.view(s * s, C).cuda(), s, s, C, out, hp, wp, sy, sx)
    ref = W.bicubic_ref(x, sy, sx)
    assert ref.shape == (hp, wp, C)
    _, mag = W.bicubic_taps(x, hp, wp, sy, sx)
    _within(f"bicubic {s}->{hp}x{wp} C={C}", out.view(hp, wp, C), ref, 16 * U24 * mag)


# ------------------------------------------------------------------------------------------------------------ scale by device scalar
@pytest.mark.parametrize("n", [1, 255, 257, 70001])
def test_scale_by_device_scalar(n):
    g = _gen(n)
    y = torch.randn(n, generator=g)
    sc = torch.randn(1, generator=g) * 3
    got = ops.scale_by_device_scalar(y.cuda(), sc.cuda()).cpu()
    assert torch.equal(got, y * sc)
    print(f"[scale_by_device_scalar n={n}] equal to the float32 product")
