"""Held-out validation on the device (pytest -m gpu): wn_eval_fwd (the dropout-free forward of a dropout context + per-utterance scores),
wn_score (stand-alone per-utterance / per-sample negative log-likelihood of head outputs), WaveNet.validate, and the drivers.

Per-sample parity (test_score_per_sample_values): worst |device - float64 oracle| / max(1, |nll|) over the counted positions outside the two
exclusions, next to the same oracle functions evaluated in float32 (the yardstick).  Measured on MI355X (profiles/validation_parity.json):

    head             device     float32 yardstick   bound = max(3 x device, yardstick)
    mol_65536        6.33e-4    4.00e-4             1.90e-3
    mol_256          1.89e-4    1.89e-4             5.67e-4
    gauss_pdf        2.77e-6    4.29e-7             8.32e-6
    gauss_cdf        1.81e-3    1.06e-3             5.43e-3
    softmax          3.29e-7    1.72e-7             9.88e-7

The device uses __expf where the float32 oracle uses expf; a bound is never below the yardstick the issue states for the head.
"""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from hip_util import SMALL, make_hp, oracle_cfg, synth_batch, upload_params
from oracle import wavenet_oracle as O
from test_hip_parity import CONFIGS, _inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WN_E_STATE = -5


def _bytes_equal(a, b):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _params(cfg):
    """the parameter recipe of test_hip_parity._run_fwd"""
    params = O.init_params(cfg, seed=5339, bias_scale=0.05)
    g = torch.Generator().manual_seed(7)
    for k in params:
        if k.startswith('local_conditioning') and k.endswith('kernel'):
            params[k] = params[k] + 0.05 * torch.randn(params[k].shape, generator=g)
    for k in params:
        if k.endswith('/g'):
            params[k] = params[k] * (torch.rand(params[k].shape, generator=g) * 0.8 + 0.6)
    return params


def _context(kw, B, T, **override):
    """engine + parameters + inputs as test_hip_parity._run_fwd makes them; `override` changes hparams (not the parameters)"""
    from wavenet_vocoder import _ext
    k = dict(SMALL); k.update(kw); k.update(override)
    hp = make_hp(**k)
    cfg = oracle_cfg(hp)
    T = (T // cfg.hop) * cfg.hop
    eng = _ext.Engine(hp, B, T)
    params = _params(cfg)
    flat = upload_params(eng, params)
    eng.pack_weights(flat)
    x_dev, y_dev, x_or, y_or, c = _inputs(cfg, hp, B, T)
    g = None
    if cfg.gin_channels > 0:
        gg = torch.Generator().manual_seed(11)
        g = (torch.randint(0, cfg.n_speakers, (B,), generator=gg).int() if cfg.use_speaker_embedding else torch.randn(B, cfg.gin_channels, generator=gg))
        eng.set_global_condition(g.cuda())
    return types.SimpleNamespace(hp=hp, cfg=cfg, eng=eng, params=params, flat=flat, x=x_dev, y=y_dev, x_or=x_or, y_or=y_or, c=c, cd=c.cuda(), g=g, B=B, T=T)


def _eval(r, lengths=None, want_nll=True):
    ln = torch.tensor(lengths or [r.T] * r.B, dtype=torch.int32, device='cuda')
    stats = torch.full((r.B, 3), float('nan'), device='cuda')
    nll = torch.full((r.B, r.T), float('nan'), device='cuda') if want_nll else None
    yh = torch.full((r.B, r.cfg.out_channels, r.T), float('nan'), device='cuda')
    r.eng.eval_fwd(r.x, r.cd, r.y, ln, stats, nll, yh)
    torch.cuda.synchronize()
    return stats.cpu(), None if nll is None else nll.cpu(), yh.cpu()


def _train_fwd(r, lengths=None, seed=1234, with_loss=True):
    ln = torch.tensor(lengths or [r.T] * r.B, dtype=torch.int32, device='cuda')
    loss = torch.zeros(1, device='cuda')
    yh = torch.full((r.B, r.cfg.out_channels, r.T), float('nan'), device='cuda')
    r.eng.train_fwd(r.x, r.cd, r.y, ln, seed, loss if with_loss else None, yh)
    torch.cuda.synchronize()
    return float(loss.item()), yh.cpu()


# ---- 1. the dropout-free forward of a dropout context == the forward of a dropout-0 context, bit for bit -----------------------------------------
DROP_CASES = {
    'mol_2d_legacy_drop': CONFIGS['mol_2d_legacy_drop'], 'mol_gin_embed': CONFIGS['mol_gin_embed'], 'mol_weightnorm': CONFIGS['mol_weightnorm'],
    'paper_width_drop': CONFIGS['paper_width_drop'],                                   # the LDS-DMA GEMM path
    'small_fp32_drop': dict(wavenet_dropout=0.05, mi355_compute_dtype='fp32'),
}


@pytest.mark.parametrize('name,lengths', [(n, None) for n in DROP_CASES] + [('mol_2d_legacy_drop', 'ragged')])
def test_eval_fwd_is_the_dropout_free_forward_bit_exact(name, lengths):
    B, T = 3, 400                                                                      # 400 -> 400 (hop 16): not a multiple of the 128-row tile
    rd = _context(DROP_CASES[name], B, T)
    assert rd.hp.wavenet_dropout > 0
    lens = [rd.T, 137, 2] if lengths == 'ragged' else None
    stats, nll, yh_eval = _eval(rd, lens)
    _, yh_drop = _train_fwd(rd, lens)
    assert not _bytes_equal(yh_eval, yh_drop), 'the training forward of this context does apply dropout'
    r0 = _context(DROP_CASES[name], B, T, wavenet_dropout=0.0)
    _, yh_ref = _train_fwd(r0, lens)
    assert torch.isfinite(yh_eval).all()
    diff = int((yh_eval.view(torch.int32) != yh_ref.view(torch.int32)).sum())
    assert diff == 0, '%d of %d y_hat words differ from the dropout-0 context' % (diff, yh_ref.numel())
    # the scores are those of wn_score on the same y_hat, and the counted positions follow the lengths
    st2 = torch.empty(B, 3, device='cuda'); nl2 = torch.empty(B, rd.T, device='cuda')
    ln = torch.tensor(lens or [rd.T] * B, dtype=torch.int32, device='cuda')
    r0.eng.score(yh_ref.cuda(), r0.y, ln, 1, st2, nl2)
    torch.cuda.synchronize()
    assert _bytes_equal(stats, st2) and _bytes_equal(nll, nl2)
    assert [int(v) for v in stats[:, 1]] == [max(min(n, rd.T) - 1, 0) for n in (lens or [rd.T] * B)]
    # a second evaluation repeats bit for bit, and the features are this batch's
    stats_b, nll_b, yh_b = _eval(rd, lens)
    assert _bytes_equal(stats, stats_b) and _bytes_equal(nll, nll_b) and _bytes_equal(yh_eval, yh_b)
    feats = torch.empty(B, rd.cfg.cin_channels, rd.T, device='cuda'); feats0 = torch.empty_like(feats)
    rd.eng.upsampled_features(feats); r0.eng.upsampled_features(feats0)
    torch.cuda.synchronize()
    assert _bytes_equal(feats, feats0)
    rd.eng.close(); r0.eng.close()


# ---- 2. the aggregate of the per-utterance rows against the training loss kernel ---------------------------------------------------------------------
@pytest.mark.parametrize('name', ['mol_2d', 'gauss_subpixel', 'gauss_cdf_nn', 'softmax_c1'])
def test_eval_fwd_aggregate_matches_the_loss_kernel(name):
    r = _context(CONFIGS[name], 3, 400)
    lens = [r.T, 137, 2]
    loss, yh_t = _train_fwd(r, lens)
    stats, nll, yh_e = _eval(r, lens)
    assert _bytes_equal(yh_t, yh_e)
    s = stats.double()
    den = s[:, 2].sum() if name == 'softmax_c1' else s[:, 1].sum()
    agg = float(s[:, 0].sum() / den)
    print('\n[%s] loss kernel %.7f  sum stats / count %.7f  (rel %.2e)' % (name, loss, agg, abs(agg - loss) / max(1.0, abs(loss))))
    assert abs(agg - loss) <= 2e-4 * max(1.0, abs(loss))                               # the project's bound: loss kernel vs oracle on identical y_hat
    assert [int(v) for v in stats[:, 1]] == [r.T - 1, 136, 1]
    assert abs(float(nll.double().sum()) - float(s[:, 0].sum())) <= 1e-6 * max(1.0, abs(float(s[:, 0].sum())))
    r.eng.close()


# ---- 3. per-sample values through wn_score on synthetic head outputs ------------------------------------------------------------------------------------
SCORE_B, SCORE_T = 3, 300
SCORE_HEADS = {
    'mol_65536': dict(out_channels=30, quantize_channels=65536, log_scale_min=-7.0),
    'mol_256': dict(out_channels=30, quantize_channels=256, log_scale_min=-7.0),
    'gauss_pdf': dict(out_channels=2, log_scale_min_gauss=float(np.log(1e-7))),
    'gauss_cdf': dict(out_channels=2, cdf_loss=True, log_scale_min_gauss=float(np.log(9.1188196e-4))),
    'softmax': dict(input_type='mulaw-quantize', out_channels=256, quantize_channels=256),
}
# worst |float32 oracle - float64 oracle| / max(1, |nll|) with these recipes, as the issue states them (softmax: measured with the device, below)
F32_YARDSTICK = {'mol_65536': 5.1e-4, 'mol_256': 1.2e-4, 'gauss_pdf': 6.7e-7, 'gauss_cdf': 3.0e-3, 'softmax': 1.8e-7}
# worst device error measured on MI355X (profiles/validation_parity.json); bound = max(3 x this, the yardstick)
DEVICE_MEASURED = {'mol_65536': 6.33e-4, 'mol_256': 1.89e-4, 'gauss_pdf': 2.775e-6, 'gauss_cdf': 1.81e-3, 'softmax': 3.294e-7}
MAX_EXCLUDED = 0.05


def _score_inputs(head, shift=0):
    """the issue's recipes, generator seed 2024: targets U(-1, 1) with 5 % at exactly -1 and 5 % at exactly +1, head outputs per head (the Gaussian
    means lie around the sample they are scored against: y[t + shift])"""
    kw = SCORE_HEADS[head]
    B, T = SCORE_B, SCORE_T
    g = torch.Generator().manual_seed(2024)
    y = torch.rand(B, T, generator=g, dtype=torch.float64) * 2 - 1
    edge = torch.rand(B, T, generator=g, dtype=torch.float64)
    y = torch.where(edge < 0.05, -torch.ones_like(y), torch.where(edge > 0.95, torch.ones_like(y), y)).float()
    if head.startswith('mol'):
        logits = torch.randn(B, 10, T, generator=g)
        means = torch.rand(B, 10, T, generator=g) * 2 - 1
        ls = torch.rand(B, 10, T, generator=g) * 10 - 9                              # a quarter below log_scale_min = -7
        return torch.cat([logits, means, ls], 1).contiguous(), y
    if head == 'softmax':
        return (3 * torch.randn(B, 256, T, generator=g)).contiguous(), torch.randint(0, 256, (B, T), generator=g).int()
    ls = torch.rand(B, T, generator=g) * 8 - 9
    n = torch.randn(B, T, generator=g)
    yt = torch.roll(y, -shift, dims=1)                                                # yt[t] = y[t + shift] (the wrapped tail is never counted)
    if head == 'gauss_pdf':
        mu = yt + 0.05 * n
    else:
        mu = yt + 1.5 * torch.exp(torch.clamp(ls, min=kw['log_scale_min_gauss'])) * n   # scale after the clamp
    return torch.stack([mu, ls], 1).contiguous(), y


def _oracle_nll(head, y_hat, y, shift, dtype):
    """unreduced oracle loss [B, T] (0 where the shifted target does not exist) and the mask of excluded positions, in `dtype`"""
    kw = SCORE_HEADS[head]
    B, T = y.shape
    n = T - shift
    yh = y_hat.to(dtype)[:, :, :n]
    out = torch.zeros(B, T, dtype=dtype)
    excl = torch.zeros(B, T, dtype=torch.bool)
    if head == 'softmax':
        logits = yh.transpose(1, 2)
        tgt = y[:, shift:].long()
        out[:, :n] = torch.logsumexp(logits, dim=-1) - logits.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)      # training_loss's CE expression
        return out, excl
    yt = y.to(dtype)[:, shift:].unsqueeze(-1)
    if head.startswith('mol'):
        Q, lsmin = kw['quantize_channels'], kw['log_scale_min']
        out[:, :n] = O.discretized_mix_logistic_loss(yh, yt, num_classes=Q, log_scale_min=lsmin).squeeze(-1)
        t = yh.transpose(1, 2)
        inv = torch.exp(-torch.clamp(t[:, :, 20:30], min=lsmin)); cy = yt - t[:, :, 10:20]
        cd = torch.sigmoid(inv * (cy + 1.0 / (Q - 1))) - torch.sigmoid(inv * (cy - 1.0 / (Q - 1)))
        excl[:, :n] = ((cd - 1e-5).abs() <= 0.01 * 1e-5).any(-1)                       # a component within 1 % of the branch threshold
        return out, excl
    Q, lsmin, cdf = make_hp(**dict(SMALL, **kw)).quantize_channels, kw['log_scale_min_gauss'], bool(kw.get('cdf_loss', False))
    out[:, :n] = O.gaussian_mle_loss(yh, yt, lsmin, Q, cdf).squeeze(-1)
    if cdf:
        sc = torch.exp(torch.clamp(yh[:, 1], min=lsmin))
        d = O.tf_ndtr((yt.squeeze(-1) + 1.0 / (Q - 1) - yh[:, 0]) / sc) - O.tf_ndtr((yt.squeeze(-1) - 1.0 / (Q - 1) - yh[:, 0]) / sc)
        excl[:, :n] = d < 1e-6
    return out, excl


def _engine_for(head, inference_only=False):
    from wavenet_vocoder import _ext
    return _ext.Engine(make_hp(**dict(SMALL, **SCORE_HEADS[head])), SCORE_B, 304, inference_only=inference_only)


def score_case(head, shift, lengths=(SCORE_T, 171, 64)):
    """-> dict(device error, float32 yardstick, excluded share, ...) of one head and shift; asserts the exact properties"""
    y_hat, y = _score_inputs(head, shift)
    B, T = y.shape
    eng = _engine_for(head, inference_only=True)                                       # no gradient is written: an inference-only context will do
    ln = torch.tensor(lengths, dtype=torch.int32)
    stats = torch.full((B, 3), float('nan'), device='cuda'); nll = torch.full((B, T), float('nan'), device='cuda')
    eng.score(y_hat.cuda(), y.cuda(), ln.cuda(), shift, stats, nll)
    torch.cuda.synchronize()
    stats, nll = stats.cpu(), nll.cpu()
    eng.close()
    counted = (torch.arange(T)[None, :] + shift) < torch.minimum(ln, torch.tensor(T))[:, None]
    ref64, excl = _oracle_nll(head, y_hat, y, shift, torch.float64)
    ref32, _ = _oracle_nll(head, y_hat, y, shift, torch.float32)
    keep = counted & ~excl
    share = float((counted & excl).sum()) / float(counted.sum())
    den = torch.clamp(ref64.abs(), min=1.0)
    dev_err = float(((nll.double() - ref64).abs() / den)[keep].max())
    f32_err = float(((ref32.double() - ref64).abs() / den)[keep].max())
    assert torch.isfinite(nll).all() and torch.isfinite(stats).all()
    assert float(nll[~counted].abs().max()) == 0.0 if (~counted).any() else True       # uncounted elements are exactly 0
    for b in range(B):
        s64 = float(nll[b].double().sum())
        assert abs(float(stats[b, 0]) - s64) <= 1e-6 * max(1.0, abs(s64)), (b, float(stats[b, 0]), s64)
        assert int(stats[b, 1]) == int(counted[b].sum())                               # the mask count, exactly
        assert int(stats[b, 2]) == int((nll[b][counted[b]] != 0).sum())
    return dict(head=head, shift=shift, device=dev_err, float32=f32_err, excluded=share)


@pytest.mark.parametrize('shift', [0, 1])
@pytest.mark.parametrize('head', list(SCORE_HEADS))
def test_score_per_sample_values(head, shift):
    r = score_case(head, shift)
    bound = max(3.0 * DEVICE_MEASURED[head], F32_YARDSTICK[head])
    print('\n[%s shift %d] device %.3e  float32 yardstick %.3e  bound %.3e  excluded %.2f %%' % (head, shift, r['device'], r['float32'], bound, 100 * r['excluded']))
    assert r['excluded'] <= MAX_EXCLUDED
    assert r['device'] <= bound


# ---- 4. determinism and row independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('head', ['mol_65536', 'softmax'])
def test_score_is_deterministic_and_row_independent(head):
    y_hat, y = _score_inputs(head)
    eng = _engine_for(head)
    B, T = y.shape

    def run(order, lengths, shift=1):
        idx = torch.tensor(order)
        st = torch.full((len(order), 3), float('nan'), device='cuda'); nl = torch.full((len(order), T), float('nan'), device='cuda')
        eng.score(y_hat[idx].contiguous().cuda(), y[idx].contiguous().cuda(), torch.tensor([lengths[i] for i in order], dtype=torch.int32).cuda(), shift, st, nl)
        torch.cuda.synchronize()
        return st.cpu(), nl.cpu()
    lens = [T, 257, 31]
    a = run([0, 1, 2], lens); b = run([0, 1, 2], lens)
    assert _bytes_equal(a[0], b[0]) and _bytes_equal(a[1], b[1])                        # run to run
    p = run([2, 0, 1], lens)
    assert _bytes_equal(p[0], a[0][[2, 0, 1]]) and _bytes_equal(p[1], a[1][[2, 0, 1]])  # permuted utterances give the permuted rows
    one = run([1], lens)
    assert _bytes_equal(one[0], a[0][1:2]) and _bytes_equal(one[1], a[1][1:2])          # a row does not depend on its batch
    z = run([0, 1, 2], [1, T, 0])
    assert z[0][0].tolist() == [0.0, 0.0, 0.0] and z[0][2].tolist() == [0.0, 0.0, 0.0] and float(z[1][0].abs().max()) == 0.0      # nothing counted: zeros, never NaN
    assert _bytes_equal(z[0][1:2], run([1], [1, T, 0])[0])
    eng.close()


# ---- 5. WaveNet.validate against the fp32 oracle, end to end ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_validate_matches_the_oracle_without_dropout(dtype):
    from wavenet_vocoder.models import create_model
    hp = make_hp(**dict(SMALL, wavenet_dropout=0.05, mi355_compute_dtype=dtype))
    cfg = oracle_cfg(hp)
    T = 400 // cfg.hop * cfg.hop
    model = create_model('WaveNet', hp)
    params = _params(cfg)
    model.build(2, T)
    model.params.copy_(upload_params(model.engine, params)); model._dirty = True
    wav, c = synth_batch(cfg, 3, T, seed=5)
    lens = [T, 281, T]

    def batch(b0, b1):
        w = wav[b0:b1]
        return (w.view(-1, 1, T).contiguous().cuda(), w.view(-1, T, 1).contiguous().cuda(), torch.tensor(lens[b0:b1], dtype=torch.int32).cuda(),
                c[b0:b1].contiguous().cuda(), None)
    res = model.validate(iter([batch(0, 2), batch(2, 3)]))
    y_or = O.step(params, cfg, wav.view(3, 1, T), c, dropout_masks=None)
    l_or = float(O.training_loss(cfg, y_or, wav.view(3, T, 1), lens))
    tol = (5e-3 if dtype == 'bf16' else 2.5e-5) * max(1.0, abs(l_or))                  # the existing bounds: bf16 path / fp32 mode against the fp32 oracle
    print('\n[%s] validate %.6f  oracle %.6f' % (dtype, res['loss'], l_or))
    assert len(res['utterances']) == 3 and [u[1] for u in res['utterances']] == [n - 1 for n in lens] and res['count'] == sum(lens) - 3
    assert abs(res['loss'] - l_or) <= tol
    # per utterance too: each row against the oracle on that utterance alone
    for b in range(3):
        lb = float(O.training_loss(cfg, y_or[b:b + 1], wav[b:b + 1].view(1, T, 1), lens[b:b + 1]))
        s, n, _ = res['utterances'][b]
        assert abs(s / n - lb) <= (5e-3 if dtype == 'bf16' else 2.5e-5) * max(1.0, abs(lb))
    # dropout really is off: the training forward of the same context, same batch, gives another loss
    x, y, ln, cc, _ = batch(0, 2)
    model.initialize(y, cc, None, ln, x=x)
    torch.cuda.synchronize()
    l_train = float(model._loss_dev.item())
    two = model.validate([batch(0, 2)])['loss']
    assert np.isfinite(l_train) and abs(l_train - two) > 1e-4, (l_train, two)
    model.engine.close()


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------------------------------
def test_eval_fwd_and_score_leave_the_training_state_as_documented():
    from wavenet_vocoder import _ext
    B, T = 3, 400
    # the benchmark widths: their weight gradients come from the grouped ordered-sum kernels, so the backward repeats bit for bit (narrow models keep
    # the float-atomics weight-gradient kernel, whose sums depend on the order of arrival)
    r = _context(CONFIGS['paper_width_drop'], B, T)
    fresh = _context(CONFIGS['paper_width_drop'], B, T)
    grads = torch.empty(r.eng.n_params, device='cuda'); want = torch.empty_like(grads)
    _train_fwd(fresh); fresh.eng.train_bwd(want)
    again = torch.empty_like(want)
    _train_fwd(fresh); fresh.eng.train_bwd(again)
    torch.cuda.synchronize()
    assert _bytes_equal(again, want), 'premise: the backward of this model is bit-reproducible'
    # train_fwd -> eval_fwd -> train_bwd: nothing was saved for a backward
    _train_fwd(r); _eval(r)
    with pytest.raises(_ext.WnError) as ei:
        r.eng.train_bwd(grads)
    assert ei.value.code == WN_E_STATE
    # a full step after an evaluation: the gradients of a fresh context, byte for byte
    _train_fwd(r); r.eng.train_bwd(grads)
    torch.cuda.synchronize()
    assert _bytes_equal(grads, want)
    # wn_score between forward and backward changes nothing
    _, yh = _train_fwd(r)
    st = torch.empty(B, 3, device='cuda')
    r.eng.score(yh.cuda(), r.y, torch.full((B,), r.T, dtype=torch.int32, device='cuda'), 1, st)
    r.eng.train_bwd(grads)
    torch.cuda.synchronize()
    assert _bytes_equal(grads, want) and torch.isfinite(st).all()
    # inference-only contexts: wn_score works, wn_eval_fwd is refused
    inf = _ext.Engine(r.hp, B, r.T, inference_only=True)
    inf.pack_weights(r.flat)
    st2 = torch.empty(B, 3, device='cuda')
    inf.score(yh.cuda(), r.y, torch.full((B,), r.T, dtype=torch.int32, device='cuda'), 1, st2)
    torch.cuda.synchronize()
    assert _bytes_equal(st, st2)
    with pytest.raises(_ext.WnError) as ei:
        inf.eval_fwd(r.x, r.cd, r.y, torch.full((B,), r.T, dtype=torch.int32, device='cuda'), st2)
    assert ei.value.code == WN_E_STATE
    # argument checks as wn_train_fwd: Tc * hop != T is WN_E_SHAPE, and a shape the scratch was not reserved for is refused
    with pytest.raises(_ext.WnError) as ei:
        r.eng.eval_fwd(r.x, r.cd[:, :, :-1].contiguous(), r.y, torch.full((B,), r.T, dtype=torch.int32, device='cuda'), st)
    assert ei.value.code == -2
    with pytest.raises(_ext.WnError) as ei:
        r.eng.score(torch.zeros(B + 1, r.cfg.out_channels, 16, device='cuda'), torch.zeros(B + 1, 16, device='cuda'), torch.full((B + 1,), 16, dtype=torch.int32, device='cuda'), 1,
                    torch.empty(B + 1, 3, device='cuda'))
    assert ei.value.code == -2
    for e in (r.eng, fresh.eng, inf):
        e.close()


@pytest.mark.parametrize('spg', [0, 8])
def test_eval_fwd_between_stream_pushes_does_not_disturb_the_stream(spg):
    from test_hip_synth import _setup
    from test_hip_synth_stream import _same, _stream
    B, Tc = 2, 16
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc, wavenet_dropout=0.05)
    ref = _stream(eng, cfg, c, [8, 8], seed=31, spg=spg)
    wav2, c2 = synth_batch(cfg, B, T, seed=8)
    x = wav2.view(B, 1, T).contiguous().cuda(); y = wav2.view(B, T, 1).contiguous().cuda(); c2 = c2.cuda()
    ln = torch.full((B,), T, dtype=torch.int32, device='cuda'); st = torch.empty(B, 3, device='cuda')
    got = _stream(eng, cfg, c, [8, 8], seed=31, spg=spg, between=lambda i: eng.eval_fwd(x, c2, y, ln, st))
    _same(got, ref)
    assert torch.isfinite(st).all() and [int(v) for v in st[:, 1].cpu()] == [T - 1] * B
    eng.close()


# ---- 7. drivers -------------------------------------------------------------------------------------------------------------------------------------------
def test_train_writes_validation_lines_and_the_scorer_reproduces_them(tmp_path):
    import hparams as H
    from test_hip_drivers import _dataset
    from wavenet_vocoder.train import wavenet_train
    root = str(tmp_path)
    meta = _dataset(root)
    spec = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
            'upsample_scales=[4,4],max_time_steps=512,wavenet_batch_size=4,wavenet_test_batches=1,wavenet_learning_rate=1e-3,wavenet_dropout=0.05')
    hp = H._build().parse(spec + ',mi355_validation_interval=2')
    log_dir = os.path.join(root, 'logs-WaveNet'); os.makedirs(log_dir, exist_ok=True)
    args = types.SimpleNamespace(base_dir=root, model='WaveNet', restore=False, wavenet_train_steps=4, checkpoint_interval=4, summary_interval=100,
                                 eval_interval=100, embedding_interval=100, eval_max_time=0)
    save_dir = wavenet_train(args, log_dir, hp, meta)
    assert save_dir is not None, 'the driver returns None when training raised'
    rows = [json.loads(l) for l in open(os.path.join(log_dir, 'wavenet_events', 'scalars.jsonl'))]
    key = 'Wavenet_eval_model/eval_stats/wavenet_validation_loss'
    val = [r for r in rows if key in r]
    assert [r['step'] for r in val] == [2, 4] and all(np.isfinite(r[key]) for r in val)
    assert all(r['wavenet_validation_utterances'] == 4 for r in val)                   # the test split: wavenet_test_batches x wavenet_batch_size
    out_json = os.path.join(root, 'scores.json')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'tacotron-2_amd'), ROOT]))
    p = subprocess.run([sys.executable, '-m', 'wavenet_vocoder.validate', '--checkpoint', save_dir, '--input', meta, '--base_dir', root, '--split', 'test',
                        '--json', out_json, '--hparams', spec], env=env, cwd=os.path.join(ROOT, 'tacotron-2_amd'), capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert 'Validation loss:' in p.stdout and 'Worst utterances' in p.stdout
    res = json.load(open(out_json))
    last = val[-1][key]
    assert len(res['utterances']) == 4 and res['count'] == val[-1]['wavenet_validation_samples']
    assert abs(res['loss'] - last) <= 5e-3 * max(1.0, abs(last)), (res['loss'], last)  # same parameters, same crops: the bf16 loss bound
