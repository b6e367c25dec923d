"""tests/head_ref.py pinned on the CPU (no GPU): the float64 references of the loss heads and of the optimiser against the oracle, the recipes
against what they are meant to drive, the float32 evaluation of both references against the bounds that tests/test_hip_heads.py holds the device
to, and five seeded faults of that float32 stand-in, each of which must break the bound and be named by the group that fails."""
import dataclasses

import numpy as np
import pytest
import torch

import head_ref as HR
from hip_util import SMALL, make_hp, oracle_cfg
from oracle import wavenet_oracle as O

B, T = HR.HEAD_B, HR.HEAD_T
RTOL = 1e-12                                     # two float64 evaluations of the same expressions
_CACHE = {}


def head_cfg(head):
    return oracle_cfg(make_hp(**dict(SMALL, **HR.HEADS[head])))


def head_case(head, shift, lens):
    """(cfg, y_hat, y, float64 reference, float32 evaluation) of one recipe, computed once"""
    key = (head, shift, lens)
    if key not in _CACHE:
        cfg = head_cfg(head)
        y_hat, y = HR.head_inputs(cfg, B, T, shift)
        _CACHE[key] = (cfg, y_hat, y, HR.ref_heads(cfg, y_hat, y, lens, shift), HR.ref_heads(cfg, y_hat, y, lens, shift, torch.float32))
    return _CACHE[key]


def _same(name, got, want, rtol=RTOL, whole=False):
    """element by element; whole: against the largest magnitude of the tensor (test_launch_ref_cpu's measure), for gradients that autograd sums from
    cancelling contributions in an order of its own"""
    err = (got - want).abs()
    tol = rtol * (want.abs().max() if whole else torch.maximum(got.abs(), want.abs()))
    assert bool((err <= tol).all()), '%s: worst |a - b| / max(|a|, |b|) = %.3e' % (name, float((err / torch.clamp(torch.maximum(got.abs(), want.abs()), min=1e-300)).max()))


def _oracle(cfg, y_hat, y, lens, dtype):
    """O.training_loss and its autograd gradient [B, T, O] in `dtype`, the clamp constants as float32 holds them"""
    cfg = dataclasses.replace(cfg, log_scale_min=HR._f32(cfg.log_scale_min), log_scale_min_gauss=HR._f32(cfg.log_scale_min_gauss))
    yh = y_hat.to(dtype).clone().requires_grad_(True)
    yy = y.long() if cfg.input_type == 'mulaw-quantize' else y.to(dtype).unsqueeze(-1)
    loss = O.training_loss(cfg, yh, yy, list(lens))
    (g,) = torch.autograd.grad(loss, [yh])
    return loss.detach(), g.permute(0, 2, 1).contiguous()


def _special(y, shift):
    """[B, T] bool: the target is exactly float32(-0.999) or float32(+0.999)"""
    yt = HR.shifted_target(y, shift)
    return (yt == torch.tensor(-0.999, dtype=torch.float32)) | (yt == torch.tensor(0.999, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------------------ loss heads
@pytest.mark.parametrize('lens', HR.HEAD_LENGTHS)
@pytest.mark.parametrize('head', list(HR.HEADS))
def test_ref_heads_equals_the_float64_oracle(head, lens):
    """shift 1 (what training_loss computes), value and gradient.  MoL: with the oracle's F.softplus calls, at every position whose target is not
    exactly float32(+-0.999); the default (exact log-sigmoid forms) then moves the result by no more than F.softplus's own error exp(-20)."""
    cfg, y_hat, y, r64, _ = head_case(head, 1, lens)
    l_or, g_or = _oracle(cfg, y_hat, y, lens, torch.float64)
    if r64.kind == 'softmax':      # the oracle counts the float64 non-zero losses: the positions whose float32 loss is exactly 0 are in its denominator
        zero32 = int(((r64.branch == 2) & r64.counted).sum())
        n64 = r64.denominator + zero32
        assert zero32 > 0 and n64 == int(r64.counted.sum())
        _same('loss', r64.loss * r64.denominator, l_or * n64)
        _same('dy', r64.dy * r64.denominator, g_or * n64, whole=True)      # (softmax - 1 in a confident row's target column cancels, in float64 too)
        return
    if r64.kind == 'gauss':
        _same('loss', r64.loss, l_or)
        _same('dy', r64.dy, g_or)
        return
    ro = HR.ref_heads(cfg, y_hat, y, lens, 1, oracle_softplus=True)
    ok = ~_special(y, 1)
    assert int((~ok & r64.counted).sum()) > 0
    M = cfg.out_channels // 3
    for part, sl in (('logit', slice(0, M)), ('mean', slice(M, 2 * M)), ('log-scale', slice(2 * M, 3 * M))):      # each part against its own largest element
        _same('dy ' + part, ro.dy[..., sl][ok], g_or[..., sl][ok], whole=True)
    ocfg = dataclasses.replace(cfg, log_scale_min=HR._f32(cfg.log_scale_min))
    nll_or = O.discretized_mix_logistic_loss(y_hat.double()[:, :, :-1], y.double()[:, 1:].unsqueeze(-1), num_classes=ocfg.quantize_channels, log_scale_min=ocfg.log_scale_min).squeeze(-1)
    keep = (ok & r64.counted)[:, :-1]
    _same('nll', ro.nll[:, :-1][keep], nll_or[keep])
    # the exact forms against the oracle's: F.softplus(x) = x above 20 is exp(-20) = 2.1e-9 off in the value and in the derivative; log_pdf_mid has it twice,
    # d / d mean multiplies it by exp(-log_scale) <= exp(-log_scale_min), d / d log_scale by |p| <= 300 (less), and the responsibilities move by as much
    e20 = float(np.exp(-20.0))
    assert float((r64.nll - ro.nll).abs().max()) <= 2 * e20 * 1.01
    assert float(((r64.dy - ro.dy).abs() * r64.denominator).max()) <= 8 * e20 * float(np.exp(-HR._f32(cfg.log_scale_min)))


@pytest.mark.parametrize('head', ['mol_65536', 'mol_256'])
def test_edge_decision_is_made_on_float32_values(head):
    """A target equal to float32(-0.999) or float32(+0.999): the float64 oracle (widened target against a double constant) takes the edge branch, the
    float32 oracle and the device (-0.999f) the middle one.  ref_heads follows float32: within the validation suite's float32 yardstick of the
    float32 oracle there, and at least 20 yardsticks away from the float64 oracle."""
    yardstick = {'mol_65536': 5.1e-4, 'mol_256': 1.2e-4}[head]
    cfg, y_hat, y, r64, _ = head_case(head, 1, HR.HEAD_LENGTHS[0])
    sp = (_special(y, 1) & r64.counted)[:, :-1]
    assert int(sp.sum()) >= 20
    assert bool((r64.branch[:, :-1][sp] >= HR.BR_QUOT).all())
    n32 = O.discretized_mix_logistic_loss(y_hat[:, :, :-1], y[:, 1:].unsqueeze(-1), num_classes=cfg.quantize_channels, log_scale_min=HR._f32(cfg.log_scale_min)).squeeze(-1).double()
    n64 = O.discretized_mix_logistic_loss(y_hat.double()[:, :, :-1], y.double()[:, 1:].unsqueeze(-1), num_classes=cfg.quantize_channels, log_scale_min=HR._f32(cfg.log_scale_min)).squeeze(-1)
    ref = r64.nll[:, :-1]
    near = ((ref - n32).abs() / torch.clamp(ref.abs(), min=1.0))[sp]
    away = ((ref - n64).abs() / torch.clamp(ref.abs(), min=1.0))[sp]
    print('\n[%s] %d positions at float32(+-0.999): |ref - float32 oracle| <= %.2e, |ref - float64 oracle| in [%.2e, %.2e] (both over max(1, |ref|))'
          % (head, int(sp.sum()), float(near.max()), float(away.min()), float(away.max())))
    assert float(near.max()) <= yardstick
    assert float(away.min()) > 20 * yardstick                                        # (5 - 11 nats at 65536 classes, 0.1 - 5 at 256)


@pytest.mark.parametrize('head', list(HR.HEADS))
def test_float32_evaluation_stays_inside_the_loss_gradient_bound(head):
    """the condition that the reference alone stays inside the bound and excludes (next to) nothing, on every recipe; and the recipes drive what they
    are meant to drive"""
    print()
    for shift in (0, 1):
        for lens in HR.HEAD_LENGTHS:
            cfg, y_hat, y, r64, r32 = head_case(head, shift, lens)
            rec = HR.heads_check(r32.dy, r64, r32, what='%s float32' % head)
            print('[%s shift %d lengths %s] excluded %.2f %%  ' % (head, shift, lens, 100 * rec['excluded'])
                  + '  '.join('%s r32=%.1e n=%d' % (k, v['r32'], v['n']) for k, v in rec.items() if k != 'excluded'))
            assert rec['excluded'] <= HR.MAX_EXCLUDED
            assert torch.isfinite(r64.dy).all() and torch.isfinite(r32.dy).all()
            assert float(r64.dy[~r64.counted].abs().max()) == 0.0
            c3 = r64.counted.unsqueeze(-1)
            if r64.kind == 'mol':
                M = cfg.out_channels // 3
                dls = r64.dy[..., 2 * M:]
                share = {k: float(((r64.branch == k) & c3).sum()) / float(c3.sum() * M) for k in range(4)}
                assert min(share.values()) >= 0.05, share                           # every branch of wn_mol_position is well populated
                mid = (r64.branch >= HR.BR_QUOT) & c3
                q = float(((r64.branch == HR.BR_QUOT) & c3).sum()) / float(mid.sum())
                assert 0.25 <= q <= 0.55, q
                assert 0.15 <= float((r64.clamped & c3).sum()) / float(c3.sum() * M) <= 0.35
                assert float(dls[r64.clamped].abs().max()) == 0.0                    # tf.maximum passes nothing below the minimum ...
                at = r64.at_min & c3
                assert int(at.sum()) > 0.03 * float(c3.sum() * M) and float((dls[at] != 0).float().mean()) > 0.9      # ... and everything at it
            elif hasattr(r64, 'diff'):
                far = (r64.branch == HR.BR_FAR) & r64.counted
                assert int(far.sum()) >= 0.1 * int(r64.counted.sum()) and float(r64.dy[far].abs().max()) == 0.0 and float(r32.dy[far].abs().max()) == 0.0
                assert int(((r64.branch == HR.BR_NEG) & r64.counted).sum()) >= 0.1 * int(r64.counted.sum())
                assert not ((r64.branch == HR.BR_POS) & r64.counted).any()           # (the ill-conditioned 2 - erfc side is not in the recipe)
            elif r64.kind == 'softmax':
                n = int(r64.counted.sum())
                assert 0.07 * n <= int(((r64.branch == 2) & r64.counted).sum()) == n - r64.denominator <= 0.13 * n
                assert int(((r64.branch == 1) & r64.counted).sum()) >= 0.07 * n
            if r64.kind == 'gauss':
                at = r64.at_min & r64.counted & ((r64.branch != HR.BR_FAR) if hasattr(r64, 'diff') else True)
                assert int(at.sum()) > 0 and bool((r64.dy[..., 1][at] != 0).all())
                if (r64.clamped & r64.counted).any():
                    assert float(r64.dy[..., 1][r64.clamped].abs().max()) == 0.0


def test_mol_recipe_needs_few_redraws():
    for head, most in (('mol_65536', 8), ('mol_256', 4)):
        cfg = head_cfg(head)
        for shift in (0, 1):
            assert HR.mol_inputs(cfg, B, T, shift)[2] <= most


# ------------------------------------------------------------------------------------------------------------------ optimiser
def cpu_layout():
    """a layout in the engine's format {name: (shape, offset)}, offsets multiples of 8: a bias, an odd-sized tensor (padding after it), a one-element
    tensor, a kernel of 6 spans, the paper-width dilated kernel of 96 spans (the second stage's lanes take two partials), and eight more small ones so
    that every gradient pattern meets small and large tensors"""
    shapes = [(64,), (7,), (1,), (3, 64, 128), (3, 256, 512), (1, 16, 30), (30,), (128,), (1, 64, 64), (5,), (2, 3, 5), (4097,), (8,)]
    layout, off = {}, 0
    for i, sh in enumerate(shapes):
        layout['t%02d' % i] = (sh, off)
        off = (off + int(np.prod(sh)) + 7) // 8 * 8
    return layout, off + 3                        # (a buffer that ends in a few more padding floats)


OPTIM_MODELS = {
    'small': dict(),
    'no_clip': dict(wavenet_clip_gradients=False),
    'tight_clip': dict(wavenet_gradient_max_norm=1.0, wavenet_gradient_max_value=0.01),
}


@pytest.mark.parametrize('step,zero_moments', [(0, False), (41, False), (10 ** 6, False), (0, True)])
@pytest.mark.parametrize('model', list(OPTIM_MODELS))
def test_ref_optim_equals_the_oracle_and_its_float32_evaluation_stays_inside_the_bound(model, step, zero_moments):
    hp = make_hp(**dict(SMALL, **OPTIM_MODELS[model]))
    layout, n = cpu_layout()
    g, pattern = HR.optim_gradients(layout, n, hp)
    st = HR.optim_state(layout, n, zero_moments=zero_moments)
    lr = 7.5e-4
    ref = HR.ref_optim(layout, st['p'], g, st['m'], st['v'], st['ema'], lr, step, hp)
    h = ref.hp
    assert set(pattern.values()) == set(range(6))
    for name, off, numel, end in HR.tensor_slices(layout, n):
        sl = slice(off, off + numel)
        g64 = g[sl].double()
        gc = O.clip_gradient(g64, h['max_norm'], h['max_value']) if h['clip'] else g64
        pn, mn, vn, en = O.adam_ema_update(st['p'][sl].double(), gc, st['m'][sl].double(), st['v'][sl].double(), st['ema'][sl].double(), step + 1, HR._f32(lr),
                                           beta1=h['beta1'], beta2=h['beta2'], eps=h['eps'], ema_decay=h['ema_decay'])
        _same(name + ' m', ref.m[sl], mn)
        _same(name + ' v', ref.v[sl], vn)
        # the oracle keeps lr_t in double, the reference rounds it to float32 as the kernel's argument is: 2^-24 of the increment
        dp, de = ref.p[sl] - st['p'][sl].double(), ref.ema[sl] - st['ema'][sl].double()
        noise = 2.0 ** -50 * (st['p'][sl].double().abs() + st['ema'][sl].double().abs())      # (the increments are differences of float64 values of that size)
        assert bool(((dp - (pn - st['p'][sl].double())).abs() <= 1.01 * HR.U24 * dp.abs() + noise).all()), name
        assert bool(((de - (en - st['ema'][sl].double())).abs() <= 1.01 * HR.U24 * dp.abs() + noise).all()), name
    if h['clip']:      # the patterns do what they are named for
        by = {k: [nm for nm, p in pattern.items() if p == k] for k in range(6)}
        assert all(ref.norms[nm] < h['max_norm'] for nm in by[0] + by[5]) and all(ref.norms[nm] > h['max_norm'] for nm in by[1] + by[2] + by[4])
        assert all(ref.norms[nm] == 0.0 for nm in by[3])
    r32 = HR.ref_optim(layout, st['p'], g, st['m'], st['v'], st['ema'], lr, step, hp, dtype=torch.float32)
    worst = HR.optim_check({k: getattr(r32, k) for k in ('p', 'm', 'v', 'ema')}, st, ref, layout, what='%s step %d float32' % (model, step))
    print('\n[%s step %d] float32 evaluation, worst increment err / bound: ' % (model, step) + '  '.join('%s=%.3f' % kv for kv in worst.items()))
    # the bound resolves what the old whole-value tolerance could not: it is a small part of the EMA's movement
    inside = ref.bound['ema'] > 0
    move = (ref.ema - st['ema'].double()).abs()
    assert float((ref.bound['ema'][inside] / torch.clamp(move[inside], min=1e-30)).median()) < 0.02


def test_zero_gradient_and_zero_moments_leave_p_bit_identical():
    hp = make_hp(**SMALL)
    layout, n = cpu_layout()
    g, pattern = HR.optim_gradients(layout, n, hp)
    st = HR.optim_state(layout, n, zero_moments=True)
    for dt in (torch.float64, torch.float32):
        r = HR.ref_optim(layout, st['p'], g, st['m'], st['v'], st['ema'], 7.5e-4, 0, hp, dtype=dt)
        for name, off, numel, end in HR.tensor_slices(layout, n):
            if pattern[name] == 3:
                sl = slice(off, off + numel)
                assert torch.equal(r.p[sl], st['p'][sl].to(dt)) and float(r.m[sl].abs().max()) == 0 and float(r.v[sl].abs().max()) == 0


# ------------------------------------------------------------------------------------------------------------------ seeded faults
def _head_fault(head, fault):
    cfg, y_hat, y, r64, r32 = head_case(head, 1, HR.HEAD_LENGTHS[0])
    bad = HR.ref_heads(cfg, y_hat, y, HR.HEAD_LENGTHS[0], 1, torch.float32, fault=fault)
    with pytest.raises(AssertionError) as ei:
        HR.heads_check(bad.dy, r64, r32, what='%s %s' % (head, fault))
    return str(ei.value)


def _optim_fault(fault, step=41, model='small'):
    hp = make_hp(**dict(SMALL, **OPTIM_MODELS[model]))
    layout, n = cpu_layout()
    g, _ = HR.optim_gradients(layout, n, hp)
    st = HR.optim_state(layout, n)
    ref = HR.ref_optim(layout, st['p'], g, st['m'], st['v'], st['ema'], 7.5e-4, step, hp)
    bad = HR.ref_optim(layout, st['p'], g, st['m'], st['v'], st['ema'], 7.5e-4, step, hp, dtype=torch.float32, fault=fault)
    with pytest.raises(AssertionError) as ei:
        HR.optim_check({k: getattr(bad, k) for k in ('p', 'm', 'v', 'ema')}, st, ref, layout, what=fault)
    return str(ei.value)


def _failed(msg):
    """the groups / quantities a failure message names"""
    return {line.strip().split(':')[0] for line in msg.splitlines()[1:]}


def test_seeded_faults_break_the_bound_and_are_named():
    """Five faults of the float32 stand-in, of the kind a hand-derived derivative or an `if` ladder produces; each fails exactly where it sits."""
    table = []
    for head in ('mol_65536', 'mol_256'):
        f = _failed(_head_fault(head, 'right_edge_gs_sign'))
        table.append((head, 'right-edge gs sign', f))
        assert f == {'right_edge'}, f
        f = _failed(_head_fault(head, 'no_clamp_gate'))
        table.append((head, 'clamp gate removed', f))
        assert 'middle_log_scale' in f and not f & {'middle_logit', 'middle_mean'}, f      # d / d log-scale alone (the edges carry clamped components too)
    f = _failed(_head_fault('gauss_cdf', 'no_clamp_gate'))      # (the pdf head's recipe has no log-scale below its minimum of log 1e-7)
    table.append(('gauss_cdf', 'clamp gate removed', f))
    assert f and f <= {'cdf_near', 'cdf_negative'}, f
    f = _failed(_optim_fault('ema_decay_0.999'))
    table.append(('optimiser', 'EMA decay 0.999', f))
    assert f == {'ema'}, f
    f = _failed(_optim_fault('value_clip_first'))
    table.append(('optimiser', 'value clip before norm clip', f))
    assert f == {'m', 'v', 'p', 'ema'}, f
    f = _failed(_optim_fault('bias_correction_t_is_step'))
    table.append(('optimiser', 'bias correction at t = step', f))
    assert f == {'p', 'ema'}, f                                                          # the moments do not see lr_t
    assert _failed(_optim_fault('value_clip_first', model='tight_clip')) == {'m', 'v', 'p', 'ema'}
    print()
    for row in table:
        print('%-10s %-28s fails: %s' % (row[0], row[1], ', '.join(sorted(row[2]))))
