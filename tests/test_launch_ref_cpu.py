"""tests/launch_ref.py pinned to float64 autograd of the oracle (CPU, no GPU).

launch_ref restates every launch of the backward chain as an operation on stored buffers; the GPU test (test_hip_launch_local.py) holds
the device to it element by element.  Those formulas are new code and could share a misreading with the kernels, so here the fp64
oracle runs WITHOUT rounding emulation (O.step + O.training_loss on float64 leaves, dropout masks on) with retain_grad on every h_l,
z_l, the skip sum and y_hat; the oracle's own unrounded intermediates go through ref_dpre1 ... ref_wgrads in chain order (each launch
fed by the previous launch's reference output), and every output must equal autograd's to 1e-10 relative (max-abs over max-abs): both
sides are float64 evaluations of the same expression, so 1e-10 is a derived number (~1e6 ulps of slack for the different association of
sums of <= 1e3 terms), not a measured one.  Where the device stores s = sigmoid and u = tanh * sigmoid the chain gets exactly those,
and recovers tanh as u / s like the kernel.

The forward launches (second half of this file) are pinned the same way against the float64 oracle FORWARD, and each of their bounds,
without its bf16 store term, against a plain float32 evaluation of the same launch."""
import numpy as np
import pytest
import torch

import launch_ref as LR
from hip_util import SMALL, dropout_mask, make_hp, oracle_cfg, synth_batch
from oracle import mulaw as M
from oracle import wavenet_oracle as O

TOL = 1e-10

CASES = {
    'mol_plain': (dict(), 2, 64, [64, 40]),
    'mol_legacy_drop_ragged_b3': (dict(legacy=True, residual_legacy=True, wavenet_dropout=0.05), 3, 96, [96, 50, 2]),
    'mol_legacy_only': (dict(legacy=True, wavenet_dropout=0.05), 2, 64, [64, 64]),
    'mol_reslegacy_only': (dict(residual_legacy=True), 2, 64, [64, 33]),
    'gauss_subpixel_legacy': (dict(out_channels=2, upsample_type='SubPixel', legacy=True, residual_legacy=True,
                                   log_scale_min_gauss=float(np.log(1e-7))), 3, 64, [64, 17, 2]),
    'softmax': (dict(input_type='mulaw-quantize', out_channels=256, quantize_channels=256, layers=8, stacks=1,
                     upsample_activation='LeakyRelu', wavenet_dropout=0.05), 2, 64, [64, 30]),
    'mol_nobias': (dict(use_bias=False, wavenet_dropout=0.05), 3, 64, [64, 64, 9]),
    'mol_gin_embed': (dict(gin_channels=16, use_speaker_embedding=True, n_speakers=5, wavenet_dropout=0.05), 3, 64, [64, 31, 2]),
}


def _close(name, got, want):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    assert err <= TOL * scale, '%s: max |ref - autograd| = %.3e, max |autograd| = %.3e (ratio %.2e)' % (name, err, scale, err / max(scale, 1e-300))
    return err / max(scale, 1e-300)


def _bt(x):
    """oracle [B, ch, T] -> launch layout [B, T, ch]"""
    return x.detach().permute(0, 2, 1).contiguous()


@pytest.mark.parametrize('name', list(CASES))
def test_launch_ref_equals_float64_autograd(name):
    over, B, T, lengths = CASES[name]
    hp = make_hp(**dict(SMALL, **over))
    cfg = oracle_cfg(hp)
    assert T % cfg.hop == 0
    L, R, G = cfg.layers, cfg.residual_channels, cfg.gate_channels
    GH = G // 2
    params = O.init_params(cfg, seed=5339, bias_scale=0.05)
    gen = torch.Generator().manual_seed(7)
    for k in params:
        if k.startswith('local_conditioning') and k.endswith('kernel'):
            params[k] = params[k] + 0.05 * torch.randn(params[k].shape, generator=gen)
    leaf = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    wav, c = synth_batch(cfg, B, T, seed=2)
    if cfg.input_type == 'mulaw-quantize':
        ids = torch.from_numpy(M.mulaw_quantize(wav.numpy())).long()
        x_or = torch.nn.functional.one_hot(ids, 256).double().permute(0, 2, 1).contiguous()
        y_or, x_in = ids, ids
    else:
        x_or, y_or, x_in = wav.double().view(B, 1, T), wav.double().view(B, T, 1), wav.double()
    g = None
    if cfg.gin_channels > 0:
        g = torch.randint(0, cfg.n_speakers, (B,), generator=torch.Generator().manual_seed(11))
        g[-1] = g[0]                                   # two utterances of one speaker: the embedding row gets a SUM
    seed = 99
    masks_or, masks = None, [None] * L
    if cfg.wavenet_dropout > 0:
        masks = [torch.from_numpy(dropout_mask(seed, l, B * T, R, cfg.wavenet_dropout)).double().view(B, T, R) for l in range(L)]
        masks_or = [m.permute(0, 2, 1).contiguous() for m in masks]
    y_hat, aux = O.step(leaf, cfg, x_or, c.double(), dropout_masks=masks_or, return_aux=True, g=g)
    for t in aux['layer_in'] + aux['z'] + [aux['skips'], aux['c_up'], y_hat]:
        t.retain_grad()
    loss = O.training_loss(cfg, y_hat, y_or, lengths)
    loss.backward()
    assert y_hat.dtype == torch.float64 and loss.dtype == torch.float64

    W = LR.Weights({k: v.detach() for k, v in leaf.items()}, cfg, rounded=False)
    rho = W.res_scale
    worst = {}

    def chk(kind, got, want):
        worst[kind] = max(worst.get(kind, 0.0), _close('%s/%s' % (name, kind), got, want))

    # ---- the forward launches that feed the backward
    X = [_bt(h) for h in aux['layer_in']]
    U = [_bt(u) for u in aux['u']]
    TS = [torch.sigmoid(_bt(z)[..., GH:]) for z in aux['z']]
    chk('X0', LR.ref_x0(W, x_in)[0], X[0])
    for l in range(L - 1):
        chk('X_next', LR.ref_x_next(W, l, U[l], X[l])[0], X[l + 1])
    skips = _bt(aux['skips'])
    R1 = torch.relu(skips)
    H2 = torch.relu(R1 @ W.fin1 + leaf['final_convolution_1/bias'].detach())
    cbt = _bt(aux['c_up'])
    # ---- loss + head
    DY = LR.ref_dy(cfg, y_hat.detach(), y_or, lengths)
    chk('DY', DY, _bt(y_hat.grad))
    assert float(DY[1, lengths[1] - 1:].abs().max()) == 0.0          # nothing is scored past a ragged length
    DPRE1, _ = LR.ref_dpre1(W, DY, H2)
    DSKIP, _ = LR.ref_dskip(W, DPRE1, R1)
    chk('DSKIP', DSKIP, _bt(aux['skips'].grad))
    # ---- the chain, top to bottom, every launch fed by the previous launch's reference output
    GX = [None] * (L + 1)
    GX[L] = torch.zeros(B, T, R, dtype=torch.float64)
    DZ = [None] * L
    dc = None
    for l in range(L - 1, -1, -1):
        DZ[l], _ = LR.ref_dz(W, l, GX[l + 1], DSKIP, TS[l], U[l])
        chk('DZ', DZ[l], _bt(aux['z'][l].grad))
        GX[l], _ = LR.ref_gx(W, l, DZ[l], masks[l], GX[l + 1] if l < L - 1 else None)
        chk('GX', GX[l], (rho if l > 0 else 1.0) * _bt(aux['layer_in'][l].grad))
        dc = LR.ref_dc_accumulate(W, l, DZ[l], dc)
    chk('DC', dc[0], _bt(aux['c_up'].grad))
    # ---- weight gradients from the chain's buffers
    grad = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaf.items()}
    for l in range(L):
        XD = X[l] if masks[l] is None else X[l] * masks[l] * W.keep_scale
        for k, (r, _) in LR.ref_wgrads_layer(W, l, XD, cbt, DZ[l], U[l], DSKIP, GX[l + 1]).items():
            if k in grad:                              # (use_bias=False has no layer biases)
                chk('wgrad ' + k.split('/')[1], r, grad[k])
        if B > 1 and W.dil[l] == 1:                    # the leak term is a real quantity here, so a taps reference that crossed b would miss 1e-10
            assert float(LR.taps_leak(W, l, XD, DZ[l]).abs().max()) > 0
    for k, (r, _) in {**LR.ref_wgrads_head(W, R1, H2, DPRE1, DY), **LR.ref_wgrads_input(W, x_in, GX[0])}.items():
        chk('wgrad ' + k, r, grad[k])
    if g is not None:
        gvec = leaf['gc_embedding'].detach()[g]
        for k, r in LR.ref_wgrads_gin({k: v.detach() for k, v in leaf.items()}, cfg, gvec, g, [rw.sum(1) for rw in DZ]).items():
            chk('wgrad ' + k.split('/')[-2 if '/' in k else 0], r, grad[k])
    print('\n[%s] worst max|ref - autograd| / max|autograd|: ' % name + '  '.join('%s=%.1e' % kv for kv in sorted(worst.items())))


def test_rounded_weights_fold_the_legacy_skip_factor_before_the_bf16_rounding():
    """csrc/wn_pack.hip rounds W_skip * float32(c_l), not W_skip: the two differ in about half of the elements when c_l is not a power of two."""
    hp = make_hp(**dict(SMALL, legacy=True))
    cfg = oracle_cfg(hp)
    params = O.init_params(cfg, seed=5339, bias_scale=0.05)
    W = LR.Weights(params, cfg, rounded=True)
    L = cfg.layers
    assert W.skip_scale[0] == float(np.float32(LR.SQRT_HALF_F32 ** (L - 1))) and W.skip_scale[L - 1] == LR.SQRT_HALF_F32
    k = params['ResidualConv1DGLU_%d/residual_block_skip_conv/kernel' % (L - 1)][0]
    folded = (k * torch.tensor(W.skip_scale[L - 1])).bfloat16().double()
    late = k.bfloat16().double() * W.skip_scale[L - 1]
    assert torch.equal(W.w_skip[L - 1], folded) and not torch.equal(folded, late)
    assert bool(((W.w_skip[L - 1] - late).abs() <= 2.0 ** -7 * late.abs()).all())      # (never more than one bf16 ulp apart)


def test_shift_time_never_crosses_an_utterance():
    x = torch.arange(2 * 5, dtype=torch.float64).view(2, 5, 1) + 1
    assert LR.shift_time(x, 2)[:, :, 0].tolist() == [[3, 4, 5, 0, 0], [8, 9, 10, 0, 0]]
    assert LR.shift_time(x, -1)[:, :, 0].tolist() == [[0, 1, 2, 3, 4], [0, 6, 7, 8, 9]]
    assert float(LR.shift_time(x, 5).abs().max()) == 0 and float(LR.shift_time(x, -7).abs().max()) == 0


def test_bound_is_zero_where_reference_and_operands_are_zero():
    """Rows whose operands are all zero (past a ragged length) get bound 0: the device must be exactly 0 there."""
    hp = make_hp(**dict(SMALL, wavenet_dropout=0.05, residual_legacy=True))
    cfg = oracle_cfg(hp)
    W = LR.Weights(O.init_params(cfg, seed=1, bias_scale=0.05), cfg, rounded=True)
    gen = torch.Generator().manual_seed(0)
    B, T, R, G = 1, 16, cfg.residual_channels, cfg.gate_channels
    DZ = LR.bf16(torch.randn(B, T, G, generator=gen)); DZ[:, 8:] = 0
    up = LR.bf16(torch.randn(B, T, R, generator=gen)); up[:, 6:] = 0
    mask = (torch.rand(B, T, R, generator=gen) > 0.05).double()
    ref, bound = LR.ref_gx(W, 1, DZ, mask, up, want_bound=True)          # d = 2: rows >= 8 see nothing
    assert float(ref[:, 8:].abs().max()) == 0 and float(bound[:, 8:].abs().max()) == 0 and float(bound[:, :6].min()) > 0


# ------------------------------------------------------------------------------------------------------------------ forward chain
# The forward launches of launch_ref (ref_x0 -> per layer ref_gate, ref_x_next -> ref_r1 -> ref_h2 -> ref_yhat; the upsample levels; the gate
# bias) pinned twice:
#   * rounded=False, chained (each launch fed by the previous launch's reference output), against the float64 oracle forward to 1e-10;
#   * rounded=True, every bound without its bf16 store term against the SAME launch evaluated in plain float32 (float32 matmuls, the fp32
#     bias sums in the kernels' order, fast_tanh / fast_sigmoid step by step with a correctly rounded exp2 and reciprocal -- the hardware's
#     are allowed one ulp): a bound that a clean float32 evaluation violates is too tight before any GPU sees it.
FWD_CASES = dict(CASES)
FWD_CASES.update({
    'resize_odd_leaky': (dict(upsample_type='Resize', upsample_scales=[3, 5], hop_size=15, upsample_activation='LeakyRelu'), 2, 60, [60, 31]),
    'resize_even': (dict(upsample_type='Resize', upsample_scales=[2, 8]), 2, 64, [64, 64]),
    'gauss_1d': (dict(out_channels=2, upsample_type='1D', log_scale_min_gauss=float(np.log(1e-7))), 2, 64, [64, 40]),
    'gauss_cdf_nn': (dict(out_channels=2, upsample_type='NearestNeighbor', cdf_loss=True, log_scale_min_gauss=float(np.log(9.1188196e-4))), 3, 64, [64, 33, 2]),
    'gauss_gin_raw_nobias': (dict(out_channels=2, gin_channels=8, use_speaker_embedding=False, use_bias=False, log_scale_min_gauss=float(np.log(1e-7))),
                             3, 64, [64, 31, 2]),
})


def _fwd_case(name):
    over, B, T, _ = FWD_CASES[name]
    hp = make_hp(**dict(SMALL, **over))
    cfg = oracle_cfg(hp)
    assert T % cfg.hop == 0
    params = O.init_params(cfg, seed=5339, bias_scale=0.05)
    gen = torch.Generator().manual_seed(7)
    for k in params:
        if k.startswith('local_conditioning') and k.endswith('kernel'):
            params[k] = params[k] + 0.05 * torch.randn(params[k].shape, generator=gen)
    wav, c = synth_batch(cfg, B, T, seed=2)
    if cfg.input_type == 'mulaw-quantize':
        ids = torch.from_numpy(M.mulaw_quantize(wav.numpy())).long()
        x_or, x_in = torch.nn.functional.one_hot(ids, 256).double().permute(0, 2, 1).contiguous(), ids
    else:
        x_or, x_in = wav.double().view(B, 1, T), wav.double()
    g = None
    if cfg.gin_channels > 0:
        gg = torch.Generator().manual_seed(11)
        g = torch.randint(0, cfg.n_speakers, (B,), generator=gg) if cfg.use_speaker_embedding else torch.randn(B, cfg.gin_channels, generator=gg)
    masks = [None] * cfg.layers
    if cfg.wavenet_dropout > 0:
        masks = [torch.from_numpy(dropout_mask(99, l, B * T, cfg.residual_channels, cfg.wavenet_dropout)).double().view(B, T, -1) for l in range(cfg.layers)]
    return cfg, params, B, T, x_or, x_in, c, g, masks


def _level_oracle(params, cfg, i, inp):
    """O.upsample restricted to level i: the same oracle code on a one-level configuration that holds level i's kernel and bias."""
    import dataclasses
    if cfg.upsample_type == 'NearestNeighbor':
        return O.upsample(params, cfg, inp)
    sub = dataclasses.replace(cfg, upsample_scales=[cfg.upsample_scales[i]])
    p = {'local_conditioning_upsampling_1/' + k: params['local_conditioning_upsampling_%d/%s' % (i + 1, k)] for k in ('kernel', 'bias')}
    return O.upsample(p, sub, inp)


def _n_levels(cfg):
    return 1 if cfg.upsample_type == 'NearestNeighbor' else len(cfg.upsample_scales)


# (raw global features: the oracle casts them to float32 before its matvec, so its float64 forward does not take them; the embedding case pins the same formula)
@pytest.mark.parametrize('name', [n for n in FWD_CASES if n != 'gauss_gin_raw_nobias'])
def test_forward_launch_refs_equal_the_float64_oracle(name):
    cfg, params, B, T, x_or, x_in, c, g, masks = _fwd_case(name)
    L, GH = cfg.layers, cfg.gate_channels // 2
    p64 = {k: v.double() for k, v in params.items()}
    masks_or = None if masks[0] is None else [m.permute(0, 2, 1).contiguous() for m in masks]
    y_hat, aux = O.step(p64, cfg, x_or, c.double(), dropout_masks=masks_or, return_aux=True, g=g)
    assert y_hat.dtype == torch.float64
    W = LR.Weights(p64, cfg, rounded=False)
    worst = {}

    def chk(kind, got, want):
        worst[kind] = max(worst.get(kind, 0.0), _close('%s/%s' % (name, kind), got, want))

    # ---- upsample net, level by level: chained against the oracle's c_up, every level against the oracle code of that level alone
    inp = c.double()
    for i in range(_n_levels(cfg)):
        out, _ = LR.ref_cup_level(p64, cfg, i, inp, rounded=False)
        chk('CUP level', out, _level_oracle(p64, cfg, i, inp))
        inp = out
    chk('CUP', inp, aux['c_up'])
    cbt = inp.permute(0, 2, 1).contiguous()
    # ---- gate bias
    gvec = None if g is None else (p64['gc_embedding'][g] if cfg.use_speaker_embedding else g.double())
    bias, _ = LR.ref_gate_bias(W, p64, cfg, gvec)
    assert bias.shape == (L, B if g is not None else 1, cfg.gate_channels)
    # ---- the chain, every launch fed by the previous launch's reference output
    X, _ = LR.ref_x0(W, x_in)
    chk('X0', X, _bt(aux['layer_in'][0]))
    U_all = []
    for l in range(L):
        XD = X if masks[l] is None else X * masks[l] * W.keep_scale
        (TS, U), _ = LR.ref_gate(W, l, XD, cbt, (bias[l], None))
        zor = _bt(aux['z'][l])
        chk('TS', TS, torch.sigmoid(zor[..., GH:]))
        chk('U', U, _bt(aux['u'][l]))
        if B > 1 and W.dil[l] <= 2:      # the leak is a real quantity here: a gate reference that crossed b would miss 1e-10
            leak = LR.gate_start_leak(W, l, XD)
            assert float(leak[1:, :2 * W.dil[l]].abs().max()) > 0 and float(leak[0].abs().max()) == 0 and float(leak[:, 2 * W.dil[l]:].abs().max()) == 0
        U_all.append(U)
        if l < L - 1:
            X, _ = LR.ref_x_next(W, l, U, X)
            chk('X_next', X, _bt(aux['layer_in'][l + 1]))
    R1, _ = LR.ref_r1(W, iter(U_all))
    chk('R1', R1, torch.relu(_bt(aux['skips'])))
    H2, _ = LR.ref_h2(W, R1)
    chk('H2', H2, _bt(torch.relu(O._conv1x1(torch.relu(aux['skips']), p64['final_convolution_1/kernel'], p64['final_convolution_1/bias']))))
    Y, _ = LR.ref_yhat(W, H2)
    assert Y.shape == (B, cfg.out_channels, T)
    chk('YHAT', Y, y_hat)
    print('\n[%s] worst max|ref - oracle| / max|oracle|: ' % name + '  '.join('%s=%.1e' % kv for kv in sorted(worst.items())))


def _f32(t):
    return t.to(torch.float32)


def _exp2_cr(p):
    """exp2 of a float32 tensor, rounded once from float64 (to within the double rounding, 2^-29 ulp)."""
    return torch.exp2(p.double()).to(torch.float32)


def _rcp_cr(q):
    return (1.0 / q.double()).to(torch.float32)


def _fast_tanh32(x):
    e = _exp2_cr(x * torch.tensor(2.885390082, dtype=torch.float32))
    return 1.0 - 2.0 * _rcp_cr(e + 1.0)


def _fast_sigmoid32(x):
    return _rcp_cr(1.0 + _exp2_cr(x * torch.tensor(-1.442695041, dtype=torch.float32)))


def _inside(name, kind, got32, ref, bound, report):
    err = (got32.double() - ref).abs()
    assert got32.dtype == torch.float32 and bool((bound >= 0).all())
    ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    worst = float(ratio.max())
    report[kind] = max(report.get(kind, 0.0), worst)
    assert worst <= 1.0, '%s/%s: the float32 evaluation is %.3f x the bound (without the bf16 store) at flat element %d' % (name, kind, worst, int(ratio.argmax()))


@pytest.mark.parametrize('name', list(FWD_CASES))
def test_forward_bounds_hold_a_float32_evaluation(name):
    """Inputs of every launch: the bf16-emulating oracle's own intermediates (realistic magnitudes, bf16 values like the device's buffers)."""
    cfg, params, B, T, x_or, x_in, c, g, masks = _fwd_case(name)
    L, GH, R = cfg.layers, cfg.gate_channels // 2, cfg.residual_channels
    masks_or = None if masks[0] is None else [m.float().permute(0, 2, 1).contiguous() for m in masks]
    _, aux = O.step(params, cfg, x_or.float(), c, dropout_masks=masks_or, emulate_bf16=True, return_aux=True, g=g)
    W = LR.Weights(params, cfg, rounded=True)
    rep = {}
    # ---- upsample levels: float32 oracle code of that level on the same input
    inp = c
    for i in range(_n_levels(cfg)):
        ref, bound = LR.ref_cup_level(params, cfg, i, inp.double(), want_bound=True)
        out32 = _level_oracle(params, cfg, i, inp)
        _inside(name, 'CUP', out32, ref, bound, rep)
        if cfg.upsample_type == 'NearestNeighbor':
            assert float(bound.abs().max()) == 0.0
        inp = out32
    cbt = LR.ref_cbt(inp.double())
    assert torch.equal(cbt, O.bf16_round(inp).double().permute(0, 2, 1))
    # ---- gate bias: the fp32 sums in the kernels' order
    gvec = None if g is None else (params['gc_embedding'][g] if cfg.use_speaker_embedding else g.float())
    bias, ebias = LR.ref_gate_bias(W, params, cfg, gvec)
    zero = torch.zeros(cfg.gate_channels)
    bias32 = []
    for l in range(L):
        q = 'ResidualConv1DGLU_%d/' % l
        a = params.get(q + 'residual_block_causal_conv/bias', zero) + params.get(q + 'residual_block_cin_conv/bias', zero)
        if gvec is not None:
            a = (a + params.get(q + 'residual_block_gin_conv/bias', zero))[None].repeat(B, 1)
            Wg = params[q + 'residual_block_gin_conv/kernel'][0]
            for k in range(cfg.gin_channels):
                a = a + gvec[:, k:k + 1] * Wg[k][None]
        else:
            a = a[None]
        bias32.append(a)
        _inside(name, 'gate bias', a, bias[l], ebias[l], rep)
    # ---- the chain
    X = [O.bf16_round(_bt(h)).double() for h in aux['layer_in']]
    U = [O.bf16_round(_bt(u)).double() for u in aux['u']]
    for l in range(L):
        XD = LR.ref_xd(W, X[l], masks[l])
        (TS, Ur), (bTS, bU) = LR.ref_gate(W, l, XD, cbt, (bias[l], ebias[l]), want_bound=True, store=False)
        d = W.dil[l]
        z32 = _f32(cbt) @ _f32(W.w_cin[l]) + bias32[l][:, None, :]
        for j in range(3):
            z32 = z32 + _f32(LR.shift_time(XD, -(2 - j) * d)) @ _f32(W.w_dil[l][j])
        t32, s32 = _fast_tanh32(z32[..., :GH]), _fast_sigmoid32(z32[..., GH:])
        _inside(name, 'TS', s32, TS, bTS, rep)
        _inside(name, 'U', t32 * s32, Ur, bU, rep)
        _, full = LR.ref_gate(W, l, XD, cbt, (bias[l], ebias[l]), want_bound=True)
        assert bool((full[0] >= bTS + LR.BF * TS).all()) and bool((full[1] >= bU + LR.BF * Ur.abs()).all())      # the store adds 2^-8 (|ref| + e)
    sb, esb = LR.skip_bias_total(W)
    sb32 = torch.zeros(cfg.skip_out_channels)
    for l in range(L):
        bk = params.get('ResidualConv1DGLU_%d/residual_block_skip_conv/bias' % l)
        if bk is not None:
            sb32 = sb32 + torch.tensor(W.skip_scale[l], dtype=torch.float32) * bk
    _inside(name, 'skip bias', sb32, sb, esb, rep)
    R1, bR1 = LR.ref_r1(W, iter(U), want_bound=True, store=False)
    v32 = sb32[None, None, :].clone()
    for l in range(L):
        v32 = v32 + _f32(U[l]) @ _f32(W.w_skip[l])
    _inside(name, 'R1', torch.relu(v32), R1, bR1, rep)
    R1b = LR.bf16(R1)
    H2, bH2 = LR.ref_h2(W, R1b, want_bound=True, store=False)
    _inside(name, 'H2', torch.relu(_f32(R1b) @ _f32(W.fin1) + params['final_convolution_1/bias']), H2, bH2, rep)
    H2b = LR.bf16(H2)
    Y, bY = LR.ref_yhat(W, H2b, want_bound=True)
    _inside(name, 'YHAT', (_f32(H2b) @ _f32(W.fin2) + params['final_convolution_2/bias']).permute(0, 2, 1), Y, bY, rep)
    print('\n[%s] float32 evaluation / bound (no bf16 store): ' % name + '  '.join('%s=%.3f' % kv for kv in sorted(rep.items())))


def test_gate_bound_covers_saturated_and_tiny_preactivations():
    """fast_tanh / fast_sigmoid over the whole range the accumulator can reach, |z| up to 100 (saturation, exp2 overflow to inf and underflow
    to 0 included): the float32 evaluation stays inside Et / Es with dz = 0."""
    x = torch.cat([torch.linspace(-100, 100, 200001), torch.tensor([0.0, 1e-30, -1e-30, 1e-6, -1e-6, 88.7, -88.7, 43.6, -43.6])]).float()
    xd = x.double()
    t, s = torch.tanh(xd), torch.sigmoid(xd)
    omt, oms = 2.0 * torch.sigmoid(-2.0 * xd), torch.sigmoid(-xd)
    Et = LR._fast_tanh_err(xd.abs(), t.abs(), omt, 0.5 * (2.0 - omt))
    Es = LR._fast_sigmoid_err(xd.abs(), s, oms)
    et = (_fast_tanh32(x).double() - t).abs()
    es = (_fast_sigmoid32(x).double() - s).abs()
    assert bool((et <= Et).all()), float((et / Et).max())
    assert bool((es <= Es).all()), float((es / Es).max())
    assert float(Et.max()) < 8 * LR.U24 * 1.01 and float(Es.max()) < 40 * LR.U24      # (absolute errors of a few fp32 ulps of 1: far below the bf16 store)
    print('\nfast_tanh err / bound %.3f, fast_sigmoid err / bound %.3f' % (float((et / Et).max()), float((es / Es).max())))


# ------------------------------------------------------------------------------------------------------------------ the report itself
# launch_report.Report decides every launch-local GPU test.  A NaN compares false with everything, so `ratio > 1` and `rel > tol` alone
# would pass a device buffer full of them: the cases below hold the report to "a device value that is not finite is a failure, with its
# coordinates" on a synthetic [B, T, ch] triple, and to "a reference or bound that is not finite raises".
def _triple(B=2, T=160, ch=8, bound_scale=2.0 ** -8):
    g = torch.Generator().manual_seed(5)
    ref = torch.randn(B, T, ch, generator=g, dtype=torch.float64)
    bound = bound_scale * ref.abs() + 1e-6
    dev = ref + 0.25 * bound * (2 * torch.rand(B, T, ch, generator=g, dtype=torch.float64) - 1)
    return dev, ref, bound


def _report(B=2, T=160):
    from launch_report import Report
    return Report('synthetic', B, T, False)


def _expect_one_failure(rep, *words):
    assert len(rep.fail) == 1, rep.fail
    for w in words:
        assert w in rep.fail[0], (w, rep.fail[0])
    with pytest.raises(AssertionError):
        rep.finish()


def test_report_passes_a_clean_triple():
    dev, ref, bound = _triple()
    rep = _report()
    rep.elementwise('GX', 3, dev, ref, bound, d=4)
    rep.elementwise('GX edge', 3, dev, ref, bound, d=4, group=torch.ones(2, 160, 1, dtype=torch.float64))
    rep.elementwise('DY', 0, ref.clone(), ref, torch.zeros_like(bound))      # bound 0: exact
    rep.exact('XD', 3, ref.clone(), ref)
    rep.tensor('ResidualConv1DGLU_3/residual_block_causal_conv/kernel', 3, (ref * (1 + 1e-7)).float(), ref, 1e-7)
    rep.tensor('ResidualConv1DGLU_3/residual_block_out_conv/kernel', 3, torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.float64), 0.0)
    assert rep.fail == []
    rep.finish()


@pytest.mark.parametrize('value', [float('nan'), float('inf'), -float('inf')])
def test_report_fails_a_non_finite_element_under_a_positive_bound(value):
    """(The NaN case passes the Report of the commit before this one: NaN / bound > 1 is false.)"""
    dev, ref, bound = _triple()
    dev[1, 131, 5] = value
    rep = _report()
    rep.elementwise('GX', 3, dev, ref, bound, d=4)
    _expect_one_failure(rep, 'GX layer 3', 'utterance 1 t 131 channel 5', 'row 291, tile 2', '1 of 2560 elements', 'not finite')


def test_report_fails_a_nan_where_the_bound_is_zero():
    dev, ref, _ = _triple()
    dev = ref.clone()
    dev[0, 159, 0] = float('nan')
    rep = _report()
    rep.elementwise('DY', 0, dev, ref, torch.zeros_like(ref), d=4)
    _expect_one_failure(rep, 'DY layer 0', 'utterance 0 t 159 channel 0', 'within 2d of an utterance end')


def test_report_group_sees_a_nan_inside_it_and_not_one_outside():
    dev, ref, bound = _triple()
    grp = torch.zeros(2, 160, 1, dtype=torch.float64)
    grp[1:, :8] = 1.0
    inside, outside = dev.clone(), dev.clone()
    inside[1, 7, 2] = float('nan')
    outside[1, 8, 2] = float('nan')
    rep = _report()
    rep.elementwise('U start', 2, outside, ref, bound, d=4, group=grp)
    assert rep.fail == []                                    # not this call's rows ...
    rep.elementwise('U', 2, outside, ref, bound, d=4)        # ... the ungrouped call of the same buffer covers them
    _expect_one_failure(rep, '] U layer 2', 'utterance 1 t 8 channel 2')
    rep = _report()
    rep.elementwise('U start', 2, inside, ref, bound, d=4, group=grp)
    _expect_one_failure(rep, 'U start layer 2', 'utterance 1 t 7 channel 2')


def test_report_exact_fails_a_nan():
    _, ref, _ = _triple()
    dev = ref.clone()
    dev[1, 3, 1] = float('nan')
    rep = _report()
    rep.exact('cbt', 0, dev, ref)
    _expect_one_failure(rep, 'cbt layer 0', '1 elements differ', 'utterance 1 t 3 channel 1')


def test_report_fails_a_nan_in_a_weight_gradient_tensor():
    """(Passes the Report of the commit before this one: the rel-L2 is NaN and NaN > tol is false.)"""
    ref = torch.randn(3, 8, 16, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    dev = ref.float()
    dev[2, 1, 4] = float('nan')
    rep = _report()
    rep.tensor('ResidualConv1DGLU_3/residual_block_causal_conv/kernel', 3, dev, ref, 1e-7)
    _expect_one_failure(rep, 'wgrad ResidualConv1DGLU_3/residual_block_causal_conv/kernel', 'layer 3', '1 of 384 elements are not finite', 'flat index %d' % (2 * 128 + 16 + 4))


def test_report_fails_a_nan_in_a_zero_reference_tensor():
    dev = torch.zeros(4, 4)
    dev[3, 3] = float('nan')
    rep = _report()
    rep.tensor('ResidualConv1DGLU_3/residual_block_out_conv/kernel', 3, dev, torch.zeros(4, 4, dtype=torch.float64), 0.0)
    _expect_one_failure(rep, 'residual_block_out_conv/kernel', 'not finite', 'flat index 15')


def test_report_raises_on_a_non_finite_reference_or_bound():
    dev, ref, bound = _triple()
    for bad_ref, bad_bound in ((True, False), (False, True)):
        r, b = ref.clone(), bound.clone()
        (r if bad_ref else b)[0, 0, 0] = float('nan')
        rep = _report()
        with pytest.raises(AssertionError, match='mistake of the test'):
            rep.elementwise('GX', 0, dev, r, b)
        assert rep.fail == []
    r = ref.clone(); r[0, 0, 0] = float('inf')
    with pytest.raises(AssertionError, match='mistake of the test'):
        _report().exact('XD', 0, dev, r)
    with pytest.raises(AssertionError, match='mistake of the test'):
        _report().tensor('x/kernel', 0, dev, r, 1e-7)
    with pytest.raises(AssertionError, match='mistake of the test'):
        _report().tensor('x/kernel', 0, dev, ref, float('nan'))
