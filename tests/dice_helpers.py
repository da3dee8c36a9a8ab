"""Float64 torch restatement of mmseg 1.2.2 losses/dice_loss.py as the decode heads use it (vfmseg_amd/dice_loss.py):
F.interpolate + one_hot + the three sums per image, with autograd.  The tests of tests/test_dice_*.py compare the HIP kernels, the heads
and the closed-form gradient against it.  Nothing here touches the GPU."""
import torch
import torch.nn.functional as F

from tests.loss_options_helpers import EPS, labels, rnd, upsampled  # noqa: F401  (the seeded makers are shared)

FORMS = [(False, False), (False, True), (True, False), (True, True)]   # (use_sigmoid, naive_dice)
FORM_IDS = ["softmax-plain", "softmax-naive", "sigmoid-plain", "sigmoid-naive"]


def one_hot(label, C):
    """t [B,C,H,W] float64: a label >= C (255 included) is an all-zero row, a negative label class 0."""
    return F.one_hot(torch.clamp(label, 0, C), C + 1)[..., :C].permute(0, 3, 1, 2).double()


def activate(v, use_sigmoid):
    return torch.sigmoid(v) if use_sigmoid else torch.softmax(v, dim=1)


def sums(p, t, naive, drop_class=-1):
    """(a, b, c) per image without eps: a = sum p t, b = sum p^2 (naive: sum p), c = sum t, over every class but drop_class."""
    C = p.shape[1]
    if 0 <= drop_class < C:
        keep = [c for c in range(C) if c != drop_class]
        p, t = p[:, keep], t[:, keep]
    p, t = p.flatten(1), t.flatten(1)
    return (p * t).sum(1), (p if naive else p * p).sum(1), t.sum(1)


def dice_terms(a, b, c, naive, eps):
    """(d, s) per image."""
    if naive:
        s = b + c + eps
        return (2 * a + eps) / s, s
    s = (b + eps) + (c + eps)
    return 2 * a / s, s


def coef(a, s, naive, eps):
    """(alpha, beta, gamma) [B,3] of d (1 - d_n) / d p = alpha t + beta p + gamma."""
    if naive:
        return torch.stack([-2 / s, torch.zeros_like(s), (2 * a + eps) / (s * s)], 1)
    return torch.stack([-2 / s, 4 * a / (s * s), torch.zeros_like(s)], 1)


def dice(logits_nhwc, label, use_sigmoid=True, naive=False, eps=1e-3, drop_class=-1, loss_weight=1.0, ignore_label=255):
    """The whole definition in float64 -> dict(loss, grad [d loss / d logits_nhwc], a, b, c [B], d [B], coef [B,3], hits, valid,
    grad_p [d loss / d p by autograd, B,C,H,W], p, t)."""
    C = logits_nhwc.shape[-1]
    lg = logits_nhwc.detach().double().requires_grad_(True)
    up = upsampled(lg, label.shape[1:])
    p = activate(up, use_sigmoid)
    p.retain_grad()
    t = one_hot(label, C)
    a, b, c = sums(p, t, naive, drop_class)
    d, s = dice_terms(a, b, c, naive, eps)
    loss = loss_weight * (1 - d).mean()
    loss.backward()
    valid = label != ignore_label
    return dict(loss=loss.item(), grad=lg.grad, a=a.detach(), b=b.detach(), c=c.detach(), d=d.detach(), coef=coef(a, s, naive, eps).detach(),
                hits=int(((up.argmax(1) == label) & valid).sum()), valid=int(valid.sum()), grad_p=p.grad, p=p.detach(), t=t)


def closed_form_grad_p(ref, naive, drop_class=-1, loss_weight=1.0):
    """d loss / d p from (alpha, beta, gamma): (loss_weight / B) (alpha_n t + beta_n p + gamma_n), zero in the dropped channel."""
    B = ref["p"].shape[0]
    k = ref["coef"].view(B, 3, 1, 1, 1)
    g = (loss_weight / B) * (k[:, 0] * ref["t"] + k[:, 1] * ref["p"] + k[:, 2])
    if 0 <= drop_class < g.shape[1]:
        g[:, drop_class] = 0
    return g
