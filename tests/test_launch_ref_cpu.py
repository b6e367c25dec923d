"""tests/launch_ref.py pinned to float64 autograd of the oracle (CPU, no GPU).

launch_ref restates every launch of the backward chain as an operation on stored buffers; the GPU test (test_hip_launch_local.py) holds
the device to it element by element.  Those formulas are new code and could share a misreading with the kernels, so here the fp64
oracle runs WITHOUT rounding emulation (O.step + O.training_loss on float64 leaves, dropout masks on) with retain_grad on every h_l,
z_l, the skip sum and y_hat; the oracle's own unrounded intermediates go through ref_dpre1 ... ref_wgrads in chain order (each launch
fed by the previous launch's reference output), and every output must equal autograd's to 1e-10 relative (max-abs over max-abs): both
sides are float64 evaluations of the same expression, so 1e-10 is a derived number (~1e6 ulps of slack for the different association of
sums of <= 1e3 terms), not a measured one.  Where the device stores s = sigmoid and u = tanh * sigmoid the chain gets exactly those,
and recovers tanh as u / s like the kernel."""
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
