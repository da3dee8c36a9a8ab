"""functional._PackCache keys an entry by the weights' storage addresses.  An entry must answer only for the parameter OBJECTS it was packed
from: a parameter that lives on in other storage (module.to(), an optimiser that moves it into its flat buffer) keeps the entry's weak
references alive while its old address is free for other tensors, and whatever lands there must not be served the old packed image."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vfmseg_amd  # noqa: E402,F401
from tests.helpers import rel_err  # noqa: E402
from vfmseg_amd import functional as Fh  # noqa: E402

DEV = "cuda"
# bf16 operands (the reference rounds the weights the same way), fp32 accumulation of K = 256 products: at most 256 * 2^-24 = 1.5e-5 of the
# sum of the terms' magnitudes; a stale image is wrong by the size of the result
TOL = 1e-4


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def test_a_recycled_address_is_not_served_the_moved_parameters_image():
    N, K = 64, 256
    x = _rnd(128, K, seed=1).to(DEV).bfloat16()
    room = torch.empty(N * K, device=DEV)                       # the address both weights sit at, one after the other
    first, second = _rnd(N, K, seed=2).to(DEV), _rnd(N, K, seed=3).to(DEV)
    room.view(N, K).copy_(first)
    p = torch.nn.Parameter(room.view(N, K), requires_grad=False)
    y = Fh.linear(x, p, "linear", out_dtype=torch.float32)
    assert rel_err(y, x.double() @ first.bfloat16().double().t()) < TOL
    p.data = first.clone()                                      # p moves away and stays alive
    w = torch.nn.Parameter(room.view(N, K), requires_grad=False)
    assert w.data_ptr() == room.data_ptr() and p.data_ptr() != room.data_ptr()
    room.view(N, K).copy_(second)
    y = Fh.linear(x, w, "linear", out_dtype=torch.float32)
    assert rel_err(y, x.double() @ second.bfloat16().double().t()) < TOL
    y = Fh.linear(x, p, "linear", out_dtype=torch.float32)     # and p is packed from where it lives now
    assert rel_err(y, x.double() @ first.bfloat16().double().t()) < TOL
