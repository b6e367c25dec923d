"""HIP path vs oracle on identical seeded inputs (run on the GPU box: pytest -m gpu).

Tolerances = (values measured on MI355X in round 2, profiles/r2f_pytest_gpu_all_verbose.log) x <= 3:
  * vs the bf16-emulating oracle (same rounding points, fp32 contraction) -- the check of kernel LOGIC: per-layer activations
    rel-L2 <= 8e-3 (measured <= 2.7e-3), y_hat <= 2.4e-2 (measured <= 7.9e-3: the 512-channel legacy config; <= 3e-3 elsewhere),
    device loss vs the oracle's loss on the device's own y_hat rtol 2e-4;
  * vs the pure fp32 oracle (the reference arithmetic): y_hat rel-L2 <= 2.6e-2 (measured <= 8.7e-3), loss rtol 5e-3 -- the stated
    price of bf16 MFMA operands;
  * gradients vs autograd of the emulating oracle: all tensors as one vector <= 7e-3 (measured <= 2.4e-3), every residual-stack /
    head tensor <= 1.4e-2 (measured <= 4.5e-3), the input convolution and the upsample-net tensors (a few hundred elements each,
    at the far end of the bf16 backward signals) <= 4.5e-2 (measured <= 1.4e-2); the mu-law / softmax configuration, whose one-hot
    input and 256-way head concentrate the signal in few elements: 4.5e-2 / 1e-1 / 1.2e-1 (measured 1.5e-2 / 3.2e-2 / 4.1e-2);
  * integer outputs (mu-law indices, argmax, categorical samples given identical logits+noise): bit-exact.
"""
import os

import numpy as np
import pytest
import torch

from hip_util import (SMALL, download_grads, make_hp, oracle_cfg, oracle_masks, rel_err, synth_batch, upload_params)
from oracle import mulaw as M
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu


def _engine(hp, B, T):
    from wavenet_vocoder import _ext
    return _ext.Engine(hp, B, T)


def _inputs(cfg, hp, B, T, seed=0):
    wav, c = synth_batch(cfg, B, T, seed)
    if hp.input_type == 'mulaw-quantize':
        ids = torch.from_numpy(M.mulaw_quantize(wav.numpy())).int()
        x_dev, y_dev = ids.cuda(), ids.cuda()
        x_or = torch.nn.functional.one_hot(ids.long(), 256).float().permute(0, 2, 1).contiguous()
        y_or = ids.long()
    else:
        if hp.input_type == 'mulaw':
            wav = torch.from_numpy(M.mulaw(wav.numpy())).float()
        x_dev, y_dev = wav.view(B, 1, T).contiguous().cuda(), wav.view(B, T, 1).contiguous().cuda()
        x_or, y_or = wav.view(B, 1, T), wav.view(B, T, 1)
    return x_dev, y_dev, x_or, y_or, c


CONFIGS = {
    'mol_2d': dict(),
    'mol_2d_legacy_drop': dict(legacy=True, residual_legacy=True, wavenet_dropout=0.05),
    'gauss_subpixel': dict(out_channels=2, upsample_type='SubPixel', legacy=True, residual_legacy=True,
                           log_scale_min_gauss=float(np.log(1e-7))),
    'gauss_cdf_nn': dict(out_channels=2, upsample_type='NearestNeighbor', cdf_loss=True,
                         log_scale_min_gauss=float(np.log(9.1188196e-4))),
    # the two upsamplers that both reference hparams files leave off (modules.py:657-733); even and odd scales
    'mol_resize': dict(upsample_type='Resize', upsample_scales=[2, 8], upsample_activation='LeakyRelu'),
    'mol_resize_odd': dict(upsample_type='Resize', upsample_scales=[3, 5], hop_size=15),
    'gauss_1d': dict(out_channels=2, upsample_type='1D', log_scale_min_gauss=float(np.log(1e-7))),
    # hparam-gated options that both reference hparams files leave off: bias-free residual layers (hparams.py:189) and global
    # conditioning with / without the speaker-embedding table (hparams.py:228-230)
    'mol_nobias': dict(use_bias=False),
    'mol_gin_embed': dict(gin_channels=16, use_speaker_embedding=True, n_speakers=5, wavenet_dropout=0.05),
    'gauss_gin_raw_nobias': dict(out_channels=2, gin_channels=8, use_speaker_embedding=False, use_bias=False,
                                 log_scale_min_gauss=float(np.log(1e-7))),
    'paper_width_gin': dict(residual_channels=256, gate_channels=512, skip_out_channels=256, cin_channels=80, num_mels=80,
                            layers=4, stacks=2, gin_channels=16, use_speaker_embedding=True, n_speakers=3),
    # Salimans & Kingma weight normalisation of every convolution (hparams.py:323): v, g are the trained variables
    'mol_weightnorm': dict(wavenet_weight_normalization=True, wavenet_dropout=0.05),
    'gauss_weightnorm_gin_nobias': dict(wavenet_weight_normalization=True, out_channels=2, use_bias=False, gin_channels=8,
                                        use_speaker_embedding=True, n_speakers=3, upsample_type='SubPixel',
                                        log_scale_min_gauss=float(np.log(1e-7))),
    'softmax_c1': dict(input_type='mulaw-quantize', out_channels=256, quantize_channels=256, layers=8, stacks=1,
                       upsample_activation='LeakyRelu'),
    'wide': dict(residual_channels=128, gate_channels=256, skip_out_channels=128, cin_channels=80, num_mels=80,
                 layers=6, stacks=2),
    # the channel widths of the benchmark configs: these (and only these) take the LDS-DMA GEMM (M % 256 == 0) and the
    # grouped ds_read_b64_tr_b16 weight-gradient kernels; T = 400 is not a multiple of the 128-row tile
    'paper_width_drop': dict(residual_channels=256, gate_channels=512, skip_out_channels=256, cin_channels=80, num_mels=80,
                             layers=6, stacks=2, wavenet_dropout=0.05),
    'c5_width_legacy': dict(residual_channels=512, gate_channels=1024, skip_out_channels=512, cin_channels=80, num_mels=80,
                            layers=3, stacks=1, out_channels=2, upsample_type='SubPixel', legacy=True, residual_legacy=True,
                            log_scale_min_gauss=float(np.log(1e-7))),
}


def _run_fwd(name, B=2, T=400, lengths=None, with_bwd=False):
    kw = dict(SMALL); kw.update(CONFIGS[name])
    hp = make_hp(**kw)
    cfg = oracle_cfg(hp)
    T = (T // cfg.hop) * cfg.hop
    eng = _engine(hp, B, T)
    params = O.init_params(cfg, seed=5339, bias_scale=0.05)
    # non-NN-init upsample kernels so that the frequency taps are exercised
    g = torch.Generator().manual_seed(7)
    for k in params:
        if k.startswith('local_conditioning') and k.endswith('kernel'):
            params[k] = params[k] + 0.05 * torch.randn(params[k].shape, generator=g)
    for k in params:
        if k.endswith('/g'):          # gains start at ||v|| (kernel == v): move them so that the normalisation is exercised
            params[k] = params[k] * (torch.rand(params[k].shape, generator=g) * 0.8 + 0.6)
    flat = upload_params(eng, params)
    eng.pack_weights(flat)
    x_dev, y_dev, x_or, y_or, c = _inputs(cfg, hp, B, T)
    g = None
    if cfg.gin_channels > 0:       # global conditioning of this batch: speaker ids or raw features
        gg = torch.Generator().manual_seed(11)
        g = (torch.randint(0, cfg.n_speakers, (B,), generator=gg).int() if cfg.use_speaker_embedding
             else torch.randn(B, cfg.gin_channels, generator=gg))
        eng.set_global_condition(g.cuda())
    lengths = lengths or [T] * B
    len_dev = torch.tensor(lengths, dtype=torch.int32).cuda()
    loss_dev = torch.zeros(1, device='cuda')
    yhat_dev = torch.empty(B, cfg.out_channels, T, device='cuda')
    seed = 1234
    eng.train_fwd(x_dev, c.cuda(), y_dev, len_dev, seed, loss_dev, yhat_dev)
    torch.cuda.synchronize()
    masks = oracle_masks(seed, cfg, B, T) if cfg.wavenet_dropout > 0 else None
    return dict(hp=hp, cfg=cfg, eng=eng, params=params, flat=flat, x_or=x_or, y_or=y_or, c=c, lengths=lengths, g=g,
                loss_dev=loss_dev, yhat_dev=yhat_dev, masks=masks, B=B, T=T, seed=seed)


@pytest.mark.parametrize('name', list(CONFIGS))
def test_train_forward(name):
    r = _run_fwd(name)
    cfg, eng, B, T = r['cfg'], r['eng'], r['B'], r['T']
    y_em, aux = O.step(r['params'], cfg, r['x_or'], r['c'], dropout_masks=r['masks'], emulate_bf16=True, return_aux=True, g=r['g'])
    y_fp = O.step(r['params'], cfg, r['x_or'], r['c'], dropout_masks=r['masks'], g=r['g'])
    rows = B * T
    rep = []
    cup = eng.debug_copy('CUP', eng.cfg.n_upsample - 1 if cfg.upsample_type != 'NearestNeighbor' else 0, B * cfg.cin_channels, T).cpu()
    rep.append(('c_up', rel_err(cup.view(B, cfg.cin_channels, T), aux['c_up'])))
    for l in range(cfg.layers):
        X = eng.debug_copy('X', l, rows, cfg.residual_channels).cpu().view(B, T, -1).permute(0, 2, 1)
        rep.append(('X%d' % l, rel_err(X, aux['layer_in'][l])))
        U = eng.debug_copy('U', l, rows, cfg.gate_channels // 2).cpu().view(B, T, -1).permute(0, 2, 1)
        rep.append(('U%d' % l, rel_err(U, aux['u'][l])))
    yh = r['yhat_dev'].cpu()
    rep.append(('y_hat(emul)', rel_err(yh, y_em)))
    rep.append(('y_hat(fp32)', rel_err(yh, y_fp)))
    loss_em = float(O.training_loss(cfg, y_em, r['y_or'], r['lengths']))
    loss_fp = float(O.training_loss(cfg, y_fp, r['y_or'], r['lengths']))
    loss_same = float(O.training_loss(cfg, yh, r['y_or'], r['lengths']))      # oracle loss on the device's own y_hat
    ld = float(r['loss_dev'].item())
    print('\n[%s] ' % name + '  '.join('%s=%.2e' % kv for kv in rep))
    print('[%s] loss dev=%.6f oracle(dev y_hat)=%.6f emul=%.6f fp32=%.6f' % (name, ld, loss_same, loss_em, loss_fp))
    assert np.isfinite(ld)
    for k, v in rep[:-2]:
        assert v < 8e-3, (k, v)                      # per-layer activations vs the emulating oracle
    assert rep[-2][1] < 2.4e-2, rep[-2]              # y_hat vs the emulating oracle
    assert rep[-1][1] < 2.6e-2, rep[-1]              # y_hat vs the fp32 oracle
    assert abs(ld - loss_same) <= 2e-4 * max(1.0, abs(loss_same)), 'loss kernel vs oracle on identical y_hat'
    # (secondary signals: a loss moves little even under a gross activation error)
    assert abs(ld - loss_em) <= 2e-3 * max(1.0, abs(loss_em))
    assert abs(ld - loss_fp) <= 5e-3 * max(1.0, abs(loss_fp))


def test_ragged_lengths_and_tail_tile():
    # T not a multiple of the 128-row tile, lengths shorter than T (mask), B=3
    r = _run_fwd('mol_2d', B=3, T=336, lengths=[336, 200, 17])
    cfg = r['cfg']
    y_em = O.step(r['params'], cfg, r['x_or'], r['c'], emulate_bf16=True)
    assert rel_err(r['yhat_dev'].cpu(), y_em) < 5e-3
    loss_same = float(O.training_loss(cfg, r['yhat_dev'].cpu(), r['y_or'], r['lengths']))
    assert abs(float(r['loss_dev'].item()) - loss_same) <= 2e-4 * max(1.0, abs(loss_same))


@pytest.mark.parametrize('name', list(CONFIGS))
def test_train_backward(name):
    r = _run_fwd(name)
    cfg, eng, B, T = r['cfg'], r['eng'], r['B'], r['T']
    grads_dev = torch.empty(eng.n_params, device='cuda')
    eng.train_bwd(grads_dev)
    torch.cuda.synchronize()
    g_dev = download_grads(eng, grads_dev)
    leaf = {k: v.clone().requires_grad_(True) for k, v in r['params'].items()}
    y = O.step(leaf, cfg, r['x_or'], r['c'], dropout_masks=r['masks'], emulate_bf16=True, g=r['g'])
    loss = O.training_loss(cfg, y, r['y_or'], r['lengths'])
    gs = torch.autograd.grad(loss, list(leaf.values()), allow_unused=True)
    g_or = {k: (g if g is not None else torch.zeros_like(leaf[k])) for k, g in zip(leaf, gs)}
    worst = []
    for k in g_or:
        n_or = float(g_or[k].norm())
        err = float((g_dev[k] - g_or[k]).norm())
        # (tensors whose true gradient vanishes -- e.g. v of a 1-element-per-channel weight-normalised kernel -- compare absolutely)
        worst.append((err / (n_or + 1e-12) if n_or > 1e-6 else err, k, n_or))
    worst.sort(reverse=True)
    print('\n[%s] worst gradient errors:' % name)
    for e, k, n in worst[:12]:
        print('   %-70s rel=%.3e |g|=%.3e' % (k, e, n))
    total = torch.cat([g_dev[k].flatten() for k in g_or]), torch.cat([g_or[k].flatten() for k in g_or])
    print('[%s] global grad rel err %.3e' % (name, rel_err(*total)))
    soft = name == 'softmax_c1'
    assert rel_err(*total) < (4.5e-2 if soft else 7e-3)
    for e, k, n in worst:
        far = k.startswith(('input_convolution', 'local_conditioning_upsampling', 'gc_embedding'))
        assert e < ((1.2e-1 if far else 1e-1) if soft else (4.5e-2 if far else 1.4e-2)), (k, e, n)


def test_optimizer_step_matches_tf_adam():
    """Whole values of p, m, v, ema against the oracle at allclose tolerances, one model, one step, ema0 = p0.  The EMA's movement here
    ((1 - decay) |dp| ~ 7e-8) is below this test's own atol + rtol |ema|: tests/test_hip_heads.py owns the increments (m - m0, v - v0, p - p0,
    ema - ema0 of every element under a derived float32 bound, ema0 != p0, five models, steps 0 / 41 / 1e6)."""
    r = _run_fwd('mol_2d')
    eng = r['eng']
    n = eng.n_params
    g = torch.Generator().manual_seed(3)
    grads = (torch.randn(n, generator=g) * 0.5)
    # one tensor with a huge norm (norm clip) and some huge values (value clip)
    k0, (sh0, off0) = list(eng.layout.items())[2]
    grads[off0:off0 + int(np.prod(sh0))] *= 400.0
    p0 = r['flat'].cpu().clone()
    m0, v0 = torch.rand(n, generator=g) * 0.01, torch.rand(n, generator=g) * 0.01
    e0 = p0.clone()
    p, m, v, e, gd = p0.cuda(), m0.cuda(), v0.cuda(), e0.cuda(), grads.cuda()
    step, lr = 41, 7.5e-4
    eng.optim_step(p, gd, m, v, e, lr, step)
    torch.cuda.synchronize()
    for name, (shape, off) in eng.layout.items():
        sl = slice(off, off + int(np.prod(shape)))
        gc = O.clip_gradient(grads[sl])
        pn, mn, vn, en = O.adam_ema_update(p0[sl], gc, m0[sl], v0[sl], e0[sl], step + 1, lr)
        assert torch.allclose(p.cpu()[sl], pn, rtol=1e-5, atol=1e-7), name
        assert torch.allclose(m.cpu()[sl], mn, rtol=1e-5, atol=1e-8), name
        assert torch.allclose(v.cpu()[sl], vn, rtol=2e-5, atol=1e-9), name
        assert torch.allclose(e.cpu()[sl], en, rtol=1e-5, atol=1e-7), name


def test_mulaw_codec_bit_exact(golden_dir):
    from wavenet_vocoder import _ext
    g = np.load(os.path.join(golden_dir, 'mulaw_golden.npz'))
    x = torch.from_numpy(g['x']).cuda()
    q = _ext.mulaw_quantize(x).cpu().numpy()
    assert np.array_equal(q, g['quantized'])                                       # bit-exact indices
    dec = _ext.inv_mulaw_quantize(torch.arange(256, dtype=torch.int32).cuda()).cpu().numpy()
    assert np.array_equal(dec, g['inv_q_all'].astype(np.float32))
    np.testing.assert_allclose(_ext.mulaw(x).cpu().numpy(), g['mulaw'], rtol=0, atol=2e-7)
    yy = torch.linspace(-1, 1, 4097).cuda()
    np.testing.assert_allclose(_ext.inv_mulaw(yy).cpu().numpy(), g['inv_mulaw'], rtol=1e-6, atol=1e-7)
    # 16M random + full-size property: quantiser is monotone and matches the numpy oracle exactly
    xr = (torch.rand(1 << 24, generator=torch.Generator().manual_seed(1)) * 2 - 1)
    qr = _ext.mulaw_quantize(xr.cuda()).cpu().numpy()
    assert np.array_equal(qr, M.mulaw_quantize(xr.numpy()))


def test_argmax_and_samplers_match_oracle(golden_dir):
    from wavenet_vocoder import _ext
    # argmax decode: bit-exact indices
    logits = torch.randn(3, 256, 500, generator=torch.Generator().manual_seed(0))
    idx = _ext.argmax_channels(logits.cuda()).cpu()
    assert torch.equal(idx.long(), logits.argmax(dim=1))
    # MoL sampler vs the reference-generated golden sample (same params + same uniforms)
    g = np.load(os.path.join(golden_dir, 'mol_golden.npz'))
    y_hat = torch.from_numpy(g['y_hat'])
    B, O3, T = y_hat.shape
    hp = make_hp(**SMALL)
    eng = _engine(hp, B, 16 * 32)
    noise = torch.cat([torch.from_numpy(g['u1']), torch.from_numpy(g['u2']).unsqueeze(-1)], dim=-1)   # [B,T,M+1]
    noise = noise.permute(1, 0, 2).contiguous()                                                          # [T,B,M+1]
    out = torch.empty(B, T, device='cuda')
    eng.sample(y_hat.cuda(), noise.cuda(), out)
    np.testing.assert_allclose(out.cpu().numpy(), g['sample'], rtol=0, atol=2e-5)
    # Gaussian
    gg = np.load(os.path.join(golden_dir, 'gaussian_golden.npz'))
    kw = dict(SMALL); kw.update(out_channels=2, log_scale_min_gauss=float(np.log(1e-7)))
    eng2 = _engine(make_hp(**kw), B, 16 * 32)
    out2 = torch.empty(B, T, device='cuda')
    eng2.sample(torch.from_numpy(gg['y_hat']).cuda(), torch.from_numpy(gg['eps']).permute(1, 0).contiguous().unsqueeze(-1).contiguous().cuda(), out2)
    np.testing.assert_allclose(out2.cpu().numpy(), gg['sample'], rtol=0, atol=2e-5)
    # categorical: identical logits + identical Gumbel uniforms -> identical indices
    kw = dict(SMALL); kw.update(input_type='mulaw-quantize', out_channels=256, quantize_channels=256)
    eng3 = _engine(make_hp(**kw), B, 16 * 32)
    lg = torch.randn(2, 256, 64, generator=torch.Generator().manual_seed(5))
    u = torch.rand(64, 2, 256, generator=torch.Generator().manual_seed(6)) * 0.98 + 0.01
    out3 = torch.empty(2, 64, dtype=torch.int32, device='cuda')
    eng3.sample(lg.cuda(), u.cuda(), out3)
    exp = torch.stack([O.sample_categorical(lg[:, :, t], u[t]) for t in range(64)], dim=1)
    assert torch.equal(out3.cpu().long(), exp)


def test_error_paths():
    from wavenet_vocoder import _ext
    with pytest.raises(_ext.WnError) as ei:
        _engine(make_hp(**dict(SMALL, layers=5, stacks=2)), 1, 64)
    assert ei.value.code == -2
    with pytest.raises(_ext.WnError):
        _engine(make_hp(**dict(SMALL, input_type='mulaw-quantize', out_channels=30)), 1, 64)   # models/__init__.py:6-9
    hp = make_hp(**SMALL)
    eng = _engine(hp, 2, 64)
    flat = upload_params(eng, O.init_params(oracle_cfg(hp)))
    x = torch.zeros(2, 1, 64, device='cuda'); c = torch.zeros(2, 16, 4, device='cuda'); y = torch.zeros(2, 64, 1, device='cuda')
    ln = torch.tensor([64, 64], dtype=torch.int32, device='cuda'); loss = torch.zeros(1, device='cuda')
    with pytest.raises(_ext.WnError) as ei:          # pack first
        eng.train_fwd(x, c, y, ln, 0, loss)
    assert ei.value.code == -5
    eng.pack_weights(flat)
    with pytest.raises(_ext.WnError) as ei:          # bwd before fwd
        eng.train_bwd(torch.zeros(eng.n_params, device='cuda'))
    assert ei.value.code == -5
    with pytest.raises(_ext.WnError) as ei:          # Tc*hop != T  (wavenet.py:699)
        eng.train_fwd(x, torch.zeros(2, 16, 3, device='cuda'), y, ln, 0, loss)
    assert ei.value.code == -2


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_training_reduces_loss_and_tracks_oracle_trajectory(dtype):
    """Several full steps (fwd + bwd + clip + TF-Adam + EMA + re-pack) on one batch: the device loss trajectory follows the
    oracle's train_step (fp32, same dropout masks) and the loss goes down.  In the fp32 training mode (mi355_compute_dtype = 'fp32',
    csrc/wn_f32.hip: the reference's arithmetic end to end) the trajectory is the oracle's to summation order."""
    kw = dict(SMALL); kw.update(wavenet_dropout=0.05, wavenet_learning_rate=1e-3, mi355_compute_dtype=dtype)
    hp = make_hp(**kw)
    cfg = oracle_cfg(hp)
    B, T = 2, 320
    eng = _engine(hp, B, T)
    params = O.init_params(cfg, seed=5339, bias_scale=0.0)
    flat = upload_params(eng, params)
    x_dev, y_dev, x_or, y_or, c = _inputs(cfg, hp, B, T)
    ln = torch.full((B,), T, dtype=torch.int32, device='cuda')
    m = torch.zeros_like(flat); v = torch.zeros_like(flat); ema = flat.clone(); grads = torch.empty_like(flat)
    loss = torch.zeros(1, device='cuda')
    state = O.init_opt_state(params)
    dev_losses, or_losses = [], []
    n_steps = 12
    for step in range(n_steps):
        seed = 100 + step
        eng.pack_weights(flat)
        eng.train_fwd(x_dev, c.cuda(), y_dev, ln, seed, loss)
        eng.train_bwd(grads)
        lr = float(O.learning_rate(step, init_lr=1e-3))
        eng.optim_step(flat, grads, m, v, ema, lr, step)
        dev_losses.append(float(loss.item()))
        masks = oracle_masks(seed, cfg, B, T)
        l, _, params, state = O.train_step(params, state, cfg, x_or, c, y_or, [T] * B, step, dropout_masks=masks)
        or_losses.append(float(l))
    print('\ndevice losses', ['%.4f' % l for l in dev_losses]); print('oracle losses', ['%.4f' % l for l in or_losses])
    assert dev_losses[-1] < dev_losses[0] - 0.05 and or_losses[-1] < or_losses[0] - 0.05
    tol_loss, tol_par = (2e-3, 2e-2) if dtype == 'bf16' else (2.5e-5, 1e-4)      # measured 2.2e-4 / 1.0e-3 and 8.2e-6 / 1.9e-5 (profiles/r4i_pytest_fp32.log)
    dl = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(dev_losses, or_losses))
    # parameters after 12 updates stay close to the oracle's
    p_or = torch.cat([params[k].reshape(-1) for k in eng.layout])
    p_dev = torch.cat([flat.cpu()[off:off + int(np.prod(shape))] for _, (shape, off) in eng.layout.items()])
    ep = rel_err(p_dev, p_or)
    print('[%s] worst loss deviation over the steps %.2e; parameters after %d updates rel-L2 %.2e' % (dtype, dl, n_steps, ep))
    assert dl <= tol_loss                   # bf16 path vs fp32 oracle, compounding over the steps (measured <= 2.5e-4)
    assert ep < tol_par
