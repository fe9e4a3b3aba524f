"""One trunk layer of the training path - ``layer_forward_train`` / ``layer_backward_train`` of mmmot_amd/train_vgg.py, the
bodies of the layer loops of ``appearance_forward_train`` / ``appearance_backward`` - on the float64 emulation of the C-ABI
against float64 autograd through conv2d -> training-mode batch_norm -> relu (-> max_pool2d), to 1e-9: this pins the
reference and the launch sequence that tests/test_train_kernels_gpu.py runs through the HIP kernels, and the per-block
statement of ``TorchOps.conv3x3_first_wgrad``.

The cases, their inputs, the reference and the decision margin live here and are imported by the device test."""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from fake_ops import TorchOps
from mmmot_amd import train_vgg
from mmmot_amd.train_vgg import dgrad_weights, layer_backward_train, layer_forward_train

EPS = 1e-5
MARGIN = 3e-5  # of max |y|: distance of every BatchNorm output from the ReLU kink and between a window's two largest values

# (L, H, W, Cin, Cout, pool) -> input seed.  Seeds: the first of 0 .. 39 for which the float64 reference keeps MARGIN
# (find_seed below; 21 to 29 of the 40 qualify for each shape with these draws).
LAYER_CASES = {
    (2, 6, 5, 64, 64, 1): 1,
    (1, 5, 7, 64, 128, 1): 1,
    (2, 4, 4, 128, 64, 0): 1,
    (1, 4, 6, 128, 128, 1): 3,
    (1, 6, 8, 3, 64, 0): 2,
    (1, 6, 8, 3, 64, 1): 2,
}


def rnd64(*shape, seed=0, scale=1.0):
    """the draws of test_kernels_gpu.rnd (fp32 values), as float64"""
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).float().double()


def fake_engine(ops):
    """what the two layer functions use of an Engine: the backend, the BatchNorm epsilon and a workspace dict"""
    return types.SimpleNamespace(ops=ops, eps=EPS, ws={})


def layer_inputs(case, seed):
    """fp32-representable float64 inputs of one layer: x (crops [L][3][H][W] for the first layer, post-ReLU NHWC rows
    otherwise), w [Cout][Cin][3][3], b, gamma (both signs, 0.5 <= |gamma|), beta, dA"""
    L, H, W, cin, cout, pool = case
    first = cin == 3
    x = rnd64(L, 3, H, W, seed=seed) if first else torch.relu(rnd64(L * H * W, cin, seed=seed))
    w = rnd64(cout, cin, 3, 3, seed=seed + 100, scale=(2.0 / (9 * cin)) ** 0.5)
    b = rnd64(cout, seed=seed + 200, scale=0.1)
    gamma = rnd64(cout, seed=seed + 300).abs() * 0.5 + 0.5
    gamma[::3] *= -1.0
    beta = rnd64(cout, seed=seed + 400, scale=0.3)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    dA = rnd64(L * Ho * Wo, cout, seed=seed + 500)
    return x, w, b, gamma, beta, dA


def layer_reference(case, inputs):
    """float64 autograd: dict(y = BatchNorm output NHWC rows, A, dX (None for the first layer), dW, db, dgamma, dbeta, dZ_max
    = max |gradient at the convolution's output|)"""
    L, H, W, cin, cout, pool = case
    x, w, b, gamma, beta, dA = [t.clone() for t in inputs]
    first = cin == 3
    xi = (x if first else x.view(L, H, W, cin).permute(0, 3, 1, 2)).contiguous().requires_grad_(not first)
    leaves = [t.requires_grad_(True) for t in (w, b, gamma, beta)]
    z = F.conv2d(xi, w, b, padding=1)
    z.retain_grad()
    y = F.batch_norm(z, None, None, gamma, beta, True, 0.0, EPS)
    a = torch.relu(y)
    if pool:
        a = F.max_pool2d(a, 2, 2)
    Ho, Wo = a.shape[2], a.shape[3]
    (a * dA.view(L, Ho, Wo, cout).permute(0, 3, 1, 2)).sum().backward()
    rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    return dict(y=rows(y), A=rows(a), dX=None if first else rows(xi.grad), dW=w.grad, db=b.grad, dgamma=gamma.grad,
                dbeta=beta.grad, dZ_max=z.grad.abs().max().item(), y4=y.detach())


def decision_margin(case, ref):
    """(distance of the BatchNorm outputs from zero, smallest gap between the two largest post-ReLU values of a pool window
    with a positive maximum - inf without pooling), both as fractions of max |y|"""
    L, H, W, cin, cout, pool = case
    y = ref['y4']
    top = y.abs().max().item()
    gap = float('inf')
    if pool:
        a = torch.relu(y)[:, :, :H // 2 * 2, :W // 2 * 2]
        win = a.unfold(2, 2, 2).unfold(3, 2, 2).reshape(L, cout, H // 2, W // 2, 4)
        two = win.topk(2, dim=-1)[0]
        pos = two[..., 0] > 0
        gap = (two[..., 0] - two[..., 1])[pos].min().item() / top
    return y.abs().min().item() / top, gap


def find_seed(case, seeds=range(40)):
    ok = []
    for s in seeds:
        kink, gap = decision_margin(case, layer_reference(case, layer_inputs(case, s)))
        if min(kink, gap) >= MARGIN:
            ok.append(s)
    return ok


@functools.lru_cache(None)
def layer_case(case):
    """(inputs, reference) of a case at its seed, the margin asserted; computed once, shared by the tests, never modified"""
    inputs = layer_inputs(case, LAYER_CASES[case])
    ref = layer_reference(case, inputs)
    kink, gap = decision_margin(case, ref)
    assert kink >= MARGIN and gap >= MARGIN, (case, kink, gap)
    return inputs, ref


def run_layer(ops, case, inputs, dtype, device='cpu'):
    """the product's two functions on one layer -> (tape record, dict of A / dX / dW / db / dgamma / dbeta)"""
    L, H, W, cin, cout, pool = case
    x, w, b, gamma, beta, dA = [t.to(dtype).to(device).contiguous() for t in inputs]
    eng, plan = fake_engine(ops), types.SimpleNamespace()
    A, ly = layer_forward_train(eng, {}, x, w, b, gamma, beta, L, H, W, cin, cout, pool, cin == 3)
    dX, dW, db, dgamma, dbeta = layer_backward_train(eng, plan, ly, dA, L)
    return ly, dict(A=A, dX=dX, dW=dW, db=db, dgamma=dgamma, dbeta=dbeta)


def layer_errors(case, got, ref):
    """worst error of every output as a fraction of the reference's maximum; db - zero by cancellation in front of a
    BatchNorm - absolutely, against max |dZ| * rows"""
    L, H, W = case[:3]
    err = {}
    for k in ('A', 'dX', 'dW', 'dgamma', 'dbeta'):
        if ref[k] is None:
            assert got[k] is None
            continue
        g = got[k].detach().cpu().double()
        assert g.shape == ref[k].shape and torch.isfinite(g).all(), k
        err[k] = (g - ref[k]).abs().max().item() / ref[k].abs().max().item()
    g = got['db'].detach().cpu().double()
    assert torch.isfinite(g).all()
    err['db'] = (g - ref['db']).abs().max().item() / (ref['dZ_max'] * L * H * W)
    return err


@pytest.mark.parametrize('case', list(LAYER_CASES), ids=lambda c: 'x'.join(map(str, c)))
def test_one_layer_on_the_float64_emulation_matches_autograd(case):
    inputs, ref = layer_case(case)
    ly, got = run_layer(TorchOps(torch.float64), case, inputs, torch.float64)
    assert ly['L'].Y.dtype == torch.float64 and got['A'].dtype == torch.float64  # nothing between the operators is fp32
    y = ly['L'].Y * ly['L'].sc + ly['L'].sh
    assert (y - ref['y']).abs().max().item() < 1e-9 * ref['y'].abs().max().item()
    err = layer_errors(case, got, ref)
    assert max(err.values()) < 1e-9, err


def test_the_seeds_are_the_first_that_keep_the_margin():
    """the recorded seed of one pooled and one unpooled case is what the search gives (the whole search: find_seed)"""
    for case in [(1, 4, 6, 128, 128, 1), (1, 6, 8, 3, 64, 0)]:
        assert find_seed(case, range(LAYER_CASES[case] + 1)) == [LAYER_CASES[case]]


@pytest.mark.parametrize('mutant', ['no flip', 'no permute'])
def test_a_wrong_input_gradient_weight_layout_is_noticed(monkeypatch, mutant):
    """dgrad_weights without its flip(0), or without its permute, moves dX by O(1) of its maximum - for Cin != Cout as for
    Cin == Cout: nothing near the tolerances of the layer tests"""
    wrong = (lambda wp: wp.permute(0, 2, 1).contiguous()) if mutant == 'no flip' else (lambda wp: wp.flip(0).contiguous())
    for case in [(2, 4, 4, 128, 64, 0), (2, 6, 5, 64, 64, 1)]:
        inputs, ref = layer_case(case)
        good = layer_errors(case, run_layer(TorchOps(torch.float64), case, inputs, torch.float64)[1], ref)
        monkeypatch.setattr(train_vgg, 'dgrad_weights', wrong)
        bad = layer_errors(case, run_layer(TorchOps(torch.float64), case, inputs, torch.float64)[1], ref)
        monkeypatch.undo()
        assert good['dX'] < 1e-9 and bad['dX'] > 0.1, (mutant, case, good['dX'], bad['dX'])
        assert bad['dW'] < 1e-9  # only the input gradient goes through the flipped weights
    assert train_vgg.dgrad_weights is dgrad_weights


@pytest.mark.parametrize('L,H,W', [(3, 9, 6), (2, 4, 2), (1, 1, 1)])
def test_first_layer_weight_gradient_specification_per_block(L, H, W):
    """TorchOps.conv3x3_first_wgrad: block b holds the pixels P b // nb .. P (b + 1) // nb; whatever nb, the blocks add up to
    autograd's gradient of conv2d w.r.t. its weight (and the 28th column to the sum of dZ); empty blocks are zero"""
    emu = TorchOps(torch.float64)
    P = L * H * W
    dZ, X = rnd64(P, 64, seed=12), rnd64(L, 3, H, W, seed=13)
    w = torch.zeros(64, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad(F.conv2d(X, w, None, padding=1), w, dZ.view(L, H, W, 64).permute(0, 3, 1, 2))
    want = torch.cat([gw.permute(0, 2, 3, 1).reshape(64, 27), dZ.sum(0).view(64, 1)], 1).reshape(-1)
    for nb in (1, 5, P + 3):
        PW = torch.full((nb, 64 * 28), float('nan'), dtype=torch.float64)
        emu.conv3x3_first_wgrad(dZ, X, L, H, W, PW)
        assert (PW.sum(0) - want).abs().max().item() < 1e-12 * max(1.0, want.abs().max().item())
        for b in range(nb):
            if P * b // nb == P * (b + 1) // nb:
                assert (PW[b] == 0).all()
    one = torch.zeros(P, 64 * 28, dtype=torch.float64)  # P blocks: block p is pixel p alone
    emu.conv3x3_first_wgrad(dZ, X, L, H, W, one)
    assert torch.equal(one.view(P, 64, 28)[:, :, 27], dZ)
