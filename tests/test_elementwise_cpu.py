"""Pins the float64 restatements of tests/elementwise_helpers.py (the references of tests/test_elementwise_gpu.py) to independent
statements of the same operations: torch autograd for the hand-written backward formulas, the oracle's rotate_half form for RoPE,
algebraic identities for the split and the counter-based dropout mask.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as R
from tests import elementwise_helpers as E


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)))


def _pre(n, seed):
    """Pre-activations: a grid over [-9, 9] plus the special points the GPU tests use."""
    x = torch.cat((torch.linspace(-9, 9, n, dtype=torch.float64), torch.tensor([0.0, 2.0 ** -20, -2.0 ** -20, -2.0 ** 0.5, 20.0, -20.0, 37.5, -60.0, 60.0], dtype=torch.float64)))
    return x[torch.randperm(x.numel(), generator=_gen(seed))]


def _close(got, want, tol=1e-13):
    err = (got - want).abs()
    assert (err <= tol * (1.0 + want.abs())).all(), err.max().item()


def test_activation_gradients_equal_autograd():
    x = _pre(400, 1)
    for act, fn in ((E.ACT_GELU, F.gelu), (E.ACT_RELU, F.relu), (E.ACT_QGELU, lambda v: v * torch.sigmoid(1.702 * v)), (E.ACT_NONE, lambda v: v)):
        xx = x.clone().requires_grad_(True)
        g, = torch.autograd.grad(fn(xx).sum(), xx)
        _close(E.act_grad(x, act), g)
    _close(E.gelu(x), F.gelu(x))


def test_geglu_and_swiglu_equal_autograd():
    g_ = _gen(2)
    pre = _pre(400, 3)
    other, d = torch.randn(pre.shape, generator=g_, dtype=torch.float64), torch.randn(pre.shape, generator=g_, dtype=torch.float64)
    a, g = other.clone().requires_grad_(True), pre.clone().requires_grad_(True)
    out = a * F.gelu(g)
    da, dg = torch.autograd.grad(out, (a, g), d)
    _close(E.geglu_fwd_ref(other, pre), out.detach())
    ra, rg = E.geglu_bwd_ref(other, pre, d)
    _close(ra, da), _close(rg, dg)
    a, g = pre.clone().requires_grad_(True), other.clone().requires_grad_(True)
    out = F.silu(a) * g
    da, dg = torch.autograd.grad(out, (a, g), d)
    _close(E.swiglu_fwd_ref(pre, other), out.detach())
    ra, rg = E.swiglu_bwd_ref(pre, other, d)
    _close(ra, da), _close(rg, dg)


def test_bounds_are_finite_and_positive_where_something_is_rounded():
    x = _pre(400, 4)
    d = torch.randn(x.shape, generator=_gen(5), dtype=torch.float64)
    for b in (E.gelu_bound(x, 2.0), E.gelu_grad_bound(x, 2.0, 2.0), E.qgelu_grad_bound(x, 2.0), E.swiglu_fwd_bound(x, d, 2.0),
              *E.swiglu_bwd_bound(x, d, d, 2.0), *E.geglu_bwd_bound(d, x, d, 2.0, 2.0)):
        assert torch.isfinite(b).all() and (b >= 0).all()
    assert (E.act_grad_mul_bound(d, x, E.ACT_RELU, 2.0, 2.0) == 0).all()


@pytest.mark.parametrize("half,ft,H", [(32, 4, 2), (4, 3, 3)])
def test_rope_ref_equals_the_rotate_half_form(half, ft, H):
    cos, sin = R.eva_rope_tables(half_head_dim=half, pt_seq_len=16, ft_seq_len=ft)
    cos, sin = cos.double(), sin.double()
    np_, d = ft * ft, 2 * half
    rows = 3 * np_
    x = torch.randn(rows, H * d + 5, generator=_gen(half, ft), dtype=torch.float64)
    got = E.rope_ref(x, cos, sin, np_, H * d, d)
    v = x[:, :H * d].view(3, np_, H, d)
    want = v * cos[None, :, None, :] + R.rotate_half(v) * sin[None, :, None, :]
    _close(got[:, :H * d], want.reshape(rows, H * d), 1e-15)
    assert torch.equal(got[:, H * d:], x[:, H * d:])


@pytest.mark.parametrize("np_,H,d", [(16, 4, 64), (5, 3, 8), (7, 2, 6)])
def test_rope_inverse_is_the_exact_transpose(np_, H, d):
    """<R x, y> == <x, R^T y> for independent random tables per column (cos[2i] != cos[2i+1])."""
    g = _gen(np_, H, d)
    rows, nc = 3 * np_ + 2, H * d
    cos, sin = torch.randn(np_, d, generator=g, dtype=torch.float64), torch.randn(np_, d, generator=g, dtype=torch.float64)
    x, y = torch.randn(rows, nc, generator=g, dtype=torch.float64), torch.randn(rows, nc, generator=g, dtype=torch.float64)
    lhs = (E.rope_ref(x, cos, sin, np_, nc, d) * y).sum()
    rhs = (x * E.rope_ref(y, cos, sin, np_, nc, d, inverse=True)).sum()
    scale = (E.rope_abs(x, cos, sin, np_, nc, d) * y.abs()).sum()
    assert abs(lhs - rhs) <= 1e-14 * scale
    assert torch.equal(E.rope_bound(x, cos, sin, np_, nc, d), 2 * E.U * (1 + 2 * E.U) * E.rope_abs(x, cos, sin, np_, nc, d))


@pytest.mark.parametrize("K", [1, 63, 64, 100, 101])
def test_split3_halves_reproduce_the_operand(K):
    x = torch.randn(5, K, generator=_gen(K)) * 3
    Kp = (K + 63) // 64 * 64
    for pattern in (0, 1):
        s = E.split3_ref(x, pattern).float().view(5, 3, Kp)
        hi, lo = s[:, 0], s[:, 2 if pattern == 0 else 1]
        assert torch.equal(s[:, 1 if pattern == 0 else 2], hi)
        assert ((hi[:, :K].double() + lo[:, :K].double() - x.double()).abs() <= 2.0 ** -16 * x.double().abs()).all()
        assert (s[:, :, K:] == 0).all()


def test_transpose_and_lora_pack_refs():
    x = torch.randn(5, 3, generator=_gen(9))
    t = E.transpose_ref(x, 8, torch.float32)
    assert torch.equal(t[:, :5], x.t()) and (t[:, 5:] == 0).all()
    A, B = torch.randn(2, 4, generator=_gen(10)), torch.randn(3, 2, generator=_gen(11))
    s = lambda *sh: torch.full(sh, -77.0)  # noqa: E731
    a, at, w, wt = E.lora_pack_ref(A, B, s(3, 6), s(5, 3), s(4, 9), s(9, 4), 5)
    assert torch.equal(a[:2, :4], A) and torch.equal(at[:4, :2], A.t()) and torch.equal(w[:3, 5:7], B) and torch.equal(wt[5:7, :3], B.t())
    assert int((a == -77).sum()) == 18 - 8 and int((at == -77).sum()) == 15 - 8 and int((w == -77).sum()) == 36 - 6 and int((wt == -77).sum()) == 36 - 6
    assert E.lora_pack_ref(A, B, s(3, 6), s(5, 3), s(4, 9), None, 5)[3] is None


def test_hash_matches_a_scalar_restatement():
    """The array arithmetic against Python integers masked to 64 bits."""
    M = (1 << 64) - 1

    def h(seed, idx):
        z = (seed + 0x9E3779B97F4A7C15 * (idx + 1)) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return (z ^ (z >> 31)) >> 32

    for seed in (0, 123, M - 5):
        idx = [0, 1, 77, (1 << 33) + 5, M - 1]
        assert [int(v) for v in E.hash_u32(seed, np.array(idx, dtype=np.uint64))] == [h(seed, i) for i in idx]


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_dropout_mask_ref_contracts(p):
    n, seed = 1 << 20, 123
    m0 = E.dropout_mask_ref(n, p, seed, 0, torch.float32)
    for a, k in ((77, 1000), (n - 3, 3)):
        assert torch.equal(E.dropout_mask_ref(k, p, seed, a, torch.float32), m0[a:a + k])
    big = (1 << 33) + 5
    assert torch.equal(E.dropout_mask_ref(64, p, seed, big + 9, torch.float32), E.dropout_mask_ref(73, p, seed, big, torch.float32)[9:])
    if p == 0.0:
        assert (m0 == 1.0).all()
    ks = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert set(m0.unique().tolist()) <= {0.0, float(ks)}
    keep = (m0 > 0).double().mean().item()
    sd = (p * (1 - p) / n) ** 0.5
    assert abs(keep - (1 - p)) <= 4 * sd, (keep, sd)
    assert not torch.equal(E.dropout_mask_ref(4096, 0.5, seed + 1, 0, torch.float32), E.dropout_mask_ref(4096, 0.5, seed, 0, torch.float32))


def test_dropout_ties_are_ties():
    """The hard-coded counters really give u == float32(p): (h >> 8) is 0 for p = 0 and 2^23 for p = 0.5; the restatement keeps them."""
    for p, ties in E.DROPOUT_TIES.items():
        for t in ties:
            assert int(E.hash_u32(E.DROPOUT_TIE_SEED, np.array([t], dtype=np.uint64))[0]) >> 8 == int(p * 2 ** 24)
            assert E.dropout_mask_ref(1, p, E.DROPOUT_TIE_SEED, t, torch.float32)[0] > 0


def test_summation_depths_never_exceed_the_number_of_terms_once_it_matters():
    """The sum bounds of the GPU tests use gamma(depth), depth = additions one term passes through in the kernel as written; that is
    never looser than gamma(number of terms) at the sizes where the two differ, and the geometry restated here is the dispatcher's."""
    assert E.colsum_geometry(5, 3) == (8, 32, 1) and E.colsum_geometry(300, 12) == (16, 16, 3)
    assert E.colsum_geometry(700, 19) == (32, 8, 11) and E.colsum_geometry(2100, 70) == (64, 4, 64)
    assert E.mask_token_geometry(1) == (1, 1) and E.mask_token_geometry(100) == (4, 25) and E.mask_token_geometry(2100) == (64, 33)
    assert E.colsum_depth(2100, 70) < 2100 and E.mask_token_depth(2100) < 2100 and E.reduce_depth(5000) < 5000
    assert E.gamma(1000) > 1000 * E.U
