"""tests/f32_ref.py against other formulations of the same operations (torch.nn.functional, einsum, autograd) on the CPU, and the
conditions under which its bounds can see one product -- so that a misreading shared between the references and the kernels of
csrc/wn_f32.hip cannot hide, and so that the GPU comparison of tests/test_hip_f32_kernels.py means what it says."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f32_ref as R


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize('shift', [0, -1, -2, -5, -9, 1, 3, 9])
def test_shifted_rows_are_zero_outside_their_own_utterance(shift):
    """A @ W with rows shifted inside each utterance == einsum over a zero-padded [B, T, K] tensor (F.pad, another mechanism)."""
    B, T, K, M = 3, 7, 5, 4
    g = _gen(1)
    x = torch.randn(B * T, K, generator=g, dtype=torch.float64); W = torch.randn(K, M, generator=g, dtype=torch.float64)
    ref, _ = R.ref_sgemm(x, W, B, T, shift=shift)
    pad = 10
    xp = F.pad(x.view(B, T, K), (0, 0, pad, pad))
    want = torch.einsum('btk,km->btm', xp[:, pad + shift:pad + shift + T], W).reshape(B * T, M)
    assert torch.allclose(ref, want, rtol=0, atol=1e-12)
    if abs(shift) >= T:
        assert float(ref.abs().max()) == 0.0


@pytest.mark.parametrize('d', [1, 2, 4])
def test_three_launches_are_a_dilated_causal_convolution_and_its_gradients(d):
    """The forward's tap launches (shift -(2 - tap) d, accumulate, bias on the first), the weight gradients (ref_wgrad with the same
    shifts, bias as column sums) and the data gradient (transposed weights, shift +(2 - tap) d) against F.conv1d and autograd."""
    B, T, Rc, G = 3, 11, 5, 6
    g = _gen(2 + d)
    x = torch.randn(B, Rc, T, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(3, Rc, G, generator=g, dtype=torch.float64, requires_grad=True)      # TF layout [tap][in][out]
    b = torch.randn(G, generator=g, dtype=torch.float64, requires_grad=True)
    z = F.conv1d(F.pad(x, (2 * d, 0)), w.permute(2, 1, 0), b, dilation=d)                # [B, G, T]
    dz = torch.randn(B, G, T, generator=g, dtype=torch.float64)
    (z * dz).sum().backward()
    xr = x.detach().permute(0, 2, 1).reshape(B * T, Rc); dzr = dz.permute(0, 2, 1).reshape(B * T, G)
    out = None
    for tap in range(3):
        out, _ = R.ref_sgemm(xr, w.detach()[tap], B, T, shift=-(2 - tap) * d, prev=out, bias=b.detach() if tap == 0 else None)
    assert torch.allclose(out, z.detach().permute(0, 2, 1).reshape(B * T, G), rtol=0, atol=1e-12)
    gx = None
    for tap in range(3):
        dW, _, cs, _ = R.ref_wgrad(xr, dzr, B, T, shift=-(2 - tap) * d)
        assert torch.allclose(dW, w.grad[tap], rtol=0, atol=1e-12)
        assert torch.allclose(cs, b.grad, rtol=0, atol=1e-12)
        gx, _ = R.ref_sgemm(dzr, w.detach()[tap].t(), B, T, shift=(2 - tap) * d, prev=gx)
    assert torch.allclose(gx, x.grad.permute(0, 2, 1).reshape(B * T, Rc), rtol=0, atol=1e-12)


def test_epilogue_order_element_by_element():
    """alpha * acc, output dropout, + prev, + bias[b], + add, * scale, relu, mask -- as a plain Python loop."""
    B, T, K, M = 2, 3, 4, 3
    g = _gen(5)
    x, W = R.real_unit(g, B * T, K), R.real_unit(g, K, M)
    prev, add, bias = R.real_unit(g, B * T, M), R.real_unit(g, B * T, M), R.real_unit(g, B, M)
    mask = torch.randint(-1, 2, (B * T, M), generator=g).double()
    keep = torch.randint(0, 2, (B * T, M), generator=g).double()
    ref, bound = R.ref_sgemm(x, W, B, T, shift=-1, alpha=0.5, scale=0.25, prev=prev, bias=bias, add=add, relu=True, mask=mask, keep_out=keep, keep_scale=2.0)
    for row in range(B * T):
        b, t = divmod(row, T)
        for m in range(M):
            acc = sum(float(x[row - 1, k]) * float(W[k, m]) for k in range(K)) if t - 1 >= 0 else 0.0
            v = 0.5 * acc
            v = v * 2.0 if keep[row, m] else 0.0
            v = (v + float(prev[row, m]) + float(bias[b, m]) + float(add[row, m])) * 0.25
            v = max(v, 0.0)
            if not mask[row, m] > 0:
                v = 0.0
            assert abs(float(ref[row, m]) - v) < 1e-14
            assert (float(bound[row, m]) == 0.0) == (not mask[row, m] > 0)


def test_dropout_on_a_is_indexed_by_the_row_that_is_read():
    B, T, K, M = 2, 6, 4, 3
    g = _gen(6)
    x, W = R.real_unit(g, B * T, K), R.real_unit(g, K, M)
    keep = torch.randint(0, 2, (B * T, K), generator=g).double()
    ref, _ = R.ref_sgemm(x, W, B, T, shift=-2, keep_a=keep, keep_scale=2.0)
    want, _ = R.ref_sgemm(x * keep * 2.0, W, B, T, shift=-2)
    assert torch.equal(ref, want)
    dW, _, _, _ = R.ref_wgrad(x, R.real_unit(g, B * T, M), B, T, shift=-2, keep_a=keep, keep_scale=2.0)
    assert dW.shape == (K, M)


def test_out_bot_layout():
    B, T, M = 2, 5, 3
    o = torch.arange(B * T * M, dtype=torch.float64).view(B * T, M)
    bot = R.to_bot(o, B, T)
    assert bot.shape == (B, M, T)
    for b in range(B):
        for m in range(M):
            for t in range(T):
                assert bot[b, m, t] == o[b * T + t, m]


def test_gate_reference_against_autograd():
    g = _gen(7)
    rows, GH = 50, 8
    Z = (torch.rand(rows, 2 * GH, generator=g, dtype=torch.float64) * 12 - 6).requires_grad_(True)
    GU = torch.randn(rows, GH, generator=g, dtype=torch.float64)
    u = torch.tanh(Z[:, :GH]) * torch.sigmoid(Z[:, GH:])
    (u * GU).sum().backward()
    U, DZ = R.ref_gate(Z.detach(), GU)
    assert torch.allclose(U, u.detach(), rtol=1e-13, atol=1e-15)
    assert torch.allclose(DZ, Z.grad, rtol=1e-11, atol=1e-15)
    U64, DZ64, ub, dzb = R.gate_bounds(Z.detach().float(), GU.float())
    assert float(ub.min()) >= 2.0 ** -22 and bool((dzb >= 2.0 ** -22 * torch.cat([GU, GU], dim=1).abs().float().double()).all())


@pytest.mark.parametrize('name', sorted(R.SGEMM_CASES))
def test_sgemm_cases_exact_inputs_stay_exact_and_real_inputs_show_one_product(name):
    """Exact run: every partial sum, in any order, is an integer multiple of 2^-6 below 2^24 2^-6 (alpha, scale in {1, 1/2, 1/4}, keep = 2), hence
    exact in fp32, and the reference itself is representable.  Real run: the bound is at most 0.01 everywhere and a single product
    (>= 0.25 keep |alpha scale|) is more than twice the bound -- on the reference alone, before any device is asked."""
    c = R.SGEMM_CASES[name]
    keep = 2.0 if c['drop'] else 1.0
    g = _gen(R.case_seed(name))
    ops = R.sgemm_operands(c, 'exact', g)
    ref, _ = R.sgemm_case_ref(c, ops)
    assert 64.0 * c['K'] * keep + 3 * 8 < 2 ** 24 / 64
    assert torch.equal(ref.to(torch.float32).to(torch.float64), ref)
    for s in (c['alpha'], c['scale']):
        assert s in (1.0, 0.5, 0.25)
    ops = R.sgemm_operands(c, 'real', g)
    ref, bound = R.sgemm_case_ref(c, ops)
    assert R.visible(bound, c['alpha'], c['scale'], keep), float(bound.max())
    assert c['K'] <= 264
    assert c['drop'] != 'out' or c['M'] <= c['drop_ld']
    assert c['drop'] != 'a' or c['K'] <= c['drop_ld']


@pytest.mark.parametrize('name', sorted(R.WGRAD_CASES))
def test_wgrad_cases_exact_inputs_stay_exact_and_real_inputs_show_one_row(name):
    c = R.WGRAD_CASES[name]
    keep = 2.0 if c['drop'] else 1.0
    g = _gen(R.case_seed(name))
    ops = R.wgrad_operands(c, 'exact', g)
    dW, _, cs, _ = R.wgrad_case_ref(c, ops)
    assert 64.0 * c['B'] * c['T'] * keep < 2 ** 24 / 4 and c['alpha'] in (1.0, 0.5)
    for r in (dW, cs):
        if r is not None:
            assert torch.equal(r.to(torch.float32).to(torch.float64), r)
    if R.wgrad_runs_real(c):
        ops = R.wgrad_operands(c, 'real', g)
        dW, bound, cs, cs_bound = R.wgrad_case_ref(c, ops)
        assert c['B'] * c['T'] <= 160
        if dW is not None:
            assert R.visible(bound, c['alpha'], 1.0, keep), float(bound.max())
        assert 2.0 * float(cs_bound.max()) < 0.5 * abs(c['alpha']) and float(cs_bound.max()) <= 0.01


def test_a_dropped_product_and_a_leaked_row_exceed_the_bound():
    """What the real-input comparison is for: drop the last k of one case, or let a tap read across the utterance start, and the
    difference exceeds the bound at the affected elements (all of them for the dropped k)."""
    c = R.SGEMM_CASES['gate_tap1']
    g = _gen(11)
    ops = R.sgemm_operands(c, 'real', g)
    ref, bound = R.sgemm_case_ref(c, ops)
    cut = dict(ops, In=ops['In'].clone()); cut['In'][:, -1] = 0.0
    bad, _ = R.sgemm_case_ref(c, cut)
    keep = R.keep_mask(c['B'] * c['T'], c['drop_ld'])[:, c['K'] - 1]
    hit = R.shift_rows(keep[:, None], c['B'], c['T'], c['shift'])[:, 0] > 0          # rows whose last product exists at all
    assert bool(((bad - ref).abs() > bound)[hit].all()) and int(hit.sum()) > 100
    T = c['T']
    leak = ops['In'] * R.keep_mask(c['B'] * T, c['drop_ld'])[:, :c['K']] * 2.0
    leaked = torch.roll(leak, 1, dims=0); leaked[0] = 0.0                            # shift -1 WITHOUT the utterance boundary
    bad2 = (leaked @ ops['W']) + ops['prev']
    d = (bad2 - ref).abs() > bound
    assert bool(d[T].any()) and bool(d[2 * T].any()) and not bool(d[1:T].any())


def test_exact_inputs_use_the_device_mask_mirror_for_p_one_half():
    m = R.keep_mask(64, 136)
    assert m.shape == (64, 136) and set(np.unique(m.numpy())) == {0.0, 1.0}
    assert 0.4 < float(m.mean()) < 0.6
