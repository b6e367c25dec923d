"""The two ends of the training step on the device (pytest -m gpu), element by element against the float64 references of tests/head_ref.py.

Loss gradient: Engine.loss (wn_loss) on crafted head outputs that drive every branch of wn_mol_position<true>, wn_gauss_position and wn_ce_loss --
left edge, right edge, the cdf_delta > 1e-5 quotient form, the density form, the log-scale clamp gate (below, at and above the minimum), the
diff < 1e-12 branch of the Gaussian cdf head, a float32 loss of exactly 0 in the softmax head -- and DY read back with debug_copy.  Per branch group
    |DY - ref64| <= 2^-8 |ref64| + 8 r32(group) rowmax |ref64|        (head_ref.heads_check; r32: the float32 evaluation of the same reference)
rows that are not counted and the padding columns exactly 0, also right after a call that filled them.  The scalar loss: 8 x the float32
evaluation's own error (the worst of the head's four cases, torch's sum and a running float32 accumulator) + 2^-24 |loss|, the store of the float32
result -- the float32 evaluation's own error alone can be a fraction of that store by luck (6e-8 on a loss of 3.3 in one Gaussian case, whose rounding alone may be 1.2e-7).

Optimiser: Engine.optim_step on five models x {step 0, 41, 10^6, step 0 from zero moments}; the increments m - m0, v - v0, p - p0, ema - ema0 of every
element against head_ref.ref_optim under the bound derived in its docstring (the whole-value allclose of test_optimizer_step_matches_tf_adam cannot
see the EMA move at all).

With WN_PARITY_REPORT_DIR set the last test writes heads_parity.json (profiles/heads_parity.json is that file from an MI355X)."""
import json
import os

import numpy as np
import pytest
import torch

import head_ref as HR
from hip_util import SMALL, make_hp, oracle_cfg

pytestmark = pytest.mark.gpu

B, T = HR.HEAD_B, HR.HEAD_T
WN_E_UNSUPPORTED = -4
RECORDS = {'loss_gradient': {}, 'loss_scalar': {}, 'optimiser': {}}
_CACHE = {}


def _head_cases(head):
    """{(shift, lengths): (y_hat, y, float64 reference, float32 evaluation)} of a head, computed once, and the scalar loss's float32 yardstick"""
    if head not in _CACHE:
        cfg = oracle_cfg(make_hp(**dict(SMALL, **HR.HEADS[head])))
        cases = {}
        for shift in (0, 1):
            y_hat, y = HR.head_inputs(cfg, B, T, shift)
            for lens in HR.HEAD_LENGTHS:
                cases[(shift, lens)] = (y_hat, y, HR.ref_heads(cfg, y_hat, y, lens, shift), HR.ref_heads(cfg, y_hat, y, lens, shift, torch.float32))
        _CACHE[head] = (cfg, cases, max(HR.loss_yardstick(c[2], c[3]) for c in cases.values()))
    return _CACHE[head]


def test_heads_are_those_of_the_validation_suite():
    from test_hip_validation import MAX_EXCLUDED, SCORE_HEADS
    assert {k: HR.HEADS[k] for k in SCORE_HEADS} == SCORE_HEADS and MAX_EXCLUDED == HR.MAX_EXCLUDED


@pytest.mark.parametrize('head', list(HR.HEADS))
def test_loss_gradient_every_branch(head):
    from wavenet_vocoder import _ext
    cfg, cases, yard = _head_cases(head)
    O = cfg.out_channels
    ld = (O + 15) // 16 * 16
    eng = _ext.Engine(make_hp(**dict(SMALL, **HR.HEADS[head])), B, 304)               # 912 rows of workspace >= the 900 used
    loss = torch.zeros(1, device='cuda')
    full = torch.full((B,), T, dtype=torch.int32, device='cuda')
    print()
    for (shift, lens), (y_hat, y, r64, r32) in cases.items():
        what = '%s shift %d lengths %s' % (head, shift, lens)
        yh_d, y_d = y_hat.cuda(), y.cuda()
        eng.loss(yh_d, y_d, full, shift, loss)                                        # every row the case leaves uncounted holds a gradient now
        filled = eng.debug_copy('DY', 0, B * T, ld).cpu().view(B, T, ld)
        unc = ~r64.counted
        unc[:, T - shift:] = False
        assert float(filled[unc].abs().max()) > 0, what
        loss.fill_(float('nan'))
        eng.loss(yh_d, y_d, torch.tensor(lens, dtype=torch.int32, device='cuda'), shift, loss)
        dy = eng.debug_copy('DY', 0, B * T, ld).cpu().view(B, T, ld)
        torch.cuda.synchronize()
        assert torch.isfinite(dy).all(), what
        rec = HR.heads_check(dy, r64, r32, what=what)
        l_dev, l_ref = float(loss.item()), float(r64.loss)
        l_bound = HR.FACTOR * yard + HR.U24 * abs(l_ref)
        print('[%s] excluded %.2f %%  loss %.7f (ref %.7f, err / bound %.3f)  ' % (what, 100 * rec['excluded'], l_dev, l_ref, abs(l_dev - l_ref) / l_bound)
              + '  '.join('%s %.3f (r32 %.1e, n %d)' % (k, v['worst'], v['r32'], v['n']) for k, v in rec.items() if k != 'excluded'))
        assert rec['excluded'] <= HR.MAX_EXCLUDED
        assert abs(l_dev - l_ref) <= l_bound, '%s: loss %.9g, reference %.9g, bound %.3g' % (what, l_dev, l_ref, l_bound)
        RECORDS['loss_gradient']['%s/shift%d/%s' % (head, shift, 'ragged' if lens == HR.HEAD_LENGTHS[0] else 'clamped_1_0')] = rec
        RECORDS['loss_scalar'][what] = dict(device=l_dev, reference=l_ref, err_over_bound=abs(l_dev - l_ref) / l_bound, float32_yardstick=yard)
        if hasattr(r64, 'diff'):      # diff < 1e-12: both gradients exactly 0
            far = (r64.branch == HR.BR_FAR) & r64.counted
            assert int(far.sum()) > 0 and float(dy[far].abs().max()) == 0.0, what
        if r64.kind == 'mol':         # below the clamp the log-scale gradient is exactly 0
            M = O // 3
            assert float(dy[..., 2 * M:3 * M][r64.clamped].abs().max()) == 0.0, what
        if r64.kind == 'softmax':     # the scale of DY proves the denominator: the float32 non-zero count, which wn_score reports too
            stats = torch.full((B, 3), float('nan'), device='cuda')
            eng.score(yh_d, y_d, torch.tensor(lens, dtype=torch.int32, device='cuda'), shift, stats)
            torch.cuda.synchronize()
            n_all = int(r64.counted.sum())
            assert int(stats[:, 2].sum().item()) == r64.denominator < n_all == int(stats[:, 1].sum().item()), what
            rows = dy[..., :O].double()[r64.counted]
            ref_rows = r64.dy[r64.counted]
            # a row of softmax - onehot sums to 0: what remains is the bf16 store of each column, and the probabilities' own sum (each divided by a
            # sum of O exponentials accumulated one by one: O roundings at the worst, and a few for exponential, quotient and difference)
            assert bool((rows.sum(-1).abs() <= HR.BF * ref_rows.abs().sum(-1) + (O + 4) * HR.U24 / r64.denominator).all()), what
    eng.close()


def test_more_than_16_mixture_components_are_refused_by_wn_loss():
    from wavenet_vocoder import _ext
    eng = _ext.Engine(make_hp(**dict(SMALL, out_channels=51)), 1, 64)
    loss = torch.zeros(1, device='cuda')
    with pytest.raises(_ext.WnError) as ei:
        eng.loss(torch.zeros(1, 51, 64, device='cuda'), torch.zeros(1, 64, device='cuda'), torch.full((1,), 64, dtype=torch.int32, device='cuda'), 1, loss)
    assert ei.value.code == WN_E_UNSUPPORTED
    eng.close()


# ------------------------------------------------------------------------------------------------------------------ optimiser
OPTIM_MODELS = {
    'small': dict(),
    'weightnorm': dict(wavenet_weight_normalization=True),                              # v and g are separate clipped variables
    'paper_width': dict(residual_channels=256, gate_channels=512, skip_out_channels=256, cin_channels=80, num_mels=80, layers=2, stacks=1),
    'no_clip': dict(wavenet_clip_gradients=False),
    'tight_clip': dict(wavenet_gradient_max_norm=1.0, wavenet_gradient_max_value=0.01),
}
OPTIM_CASES = [(0, False), (41, False), (10 ** 6, False), (0, True)]                    # (step, start from zero moments)
LR = 7.5e-4


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('step,zero_moments', OPTIM_CASES)
@pytest.mark.parametrize('model', list(OPTIM_MODELS))
def test_optimizer_step_every_element(model, step, zero_moments):
    from wavenet_vocoder import _ext
    hp = make_hp(**dict(SMALL, **OPTIM_MODELS[model]))
    eng = _ext.Engine(hp, 1, 256)                                                     # (no forward is needed)
    n, layout = eng.n_params, eng.layout
    sizes = [int(np.prod(sh)) for sh, _ in layout.values()]
    if model == 'paper_width':      # the i += 64 loop of the second norm stage: more than 64 spans of 4096 floats
        assert max(sizes) == 3 * 256 * 512 and -(-max(sizes) // HR.NORM_SPAN) == 96
    if model == 'weightnorm':
        assert sum(k.endswith('/g') for k in layout) >= int(hp.layers)
    g, pattern = HR.optim_gradients(layout, n, hp)
    st = HR.optim_state(layout, n, zero_moments=zero_moments)
    assert set(pattern.values()) == set(range(6))

    def run():
        d = {k: v.cuda() for k, v in st.items()}
        eng.optim_step(d['p'], g.cuda(), d['m'], d['v'], d['ema'], LR, step)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in d.items()}
    out = run()
    ref = HR.ref_optim(layout, st['p'], g, st['m'], st['v'], st['ema'], LR, step, hp)
    what = '%s step %d%s' % (model, step, ' zero moments' if zero_moments else '')
    assert all(torch.isfinite(v).all() for v in out.values()), what
    worst = HR.optim_check(out, st, ref, layout, what=what)
    print('\n[%s] worst increment err / bound: ' % what + '  '.join('%s=%.3f' % kv for kv in worst.items()))
    RECORDS['optimiser'][what] = worst
    again = run()
    assert all(_bits_equal(out[k], again[k]) for k in out), what + ': two calls from the same state differ'
    assert not _bits_equal(out['ema'], st['ema']) and not _bits_equal(out['p'], st['p'])
    if zero_moments:      # an all-zero gradient on zero moments moves nothing
        for name, off, numel, end in HR.tensor_slices(layout, n):
            if pattern[name] == 3:
                sl = slice(off, off + numel)
                assert _bits_equal(out['p'][sl], st['p'][sl]) and float(out['m'][sl].abs().max()) == 0.0 and float(out['v'][sl].abs().max()) == 0.0, name
    eng.close()


def test_write_the_parity_report():
    want = ['%s/shift%d/%s' % (h, s, l) for h in HR.HEADS for s in (0, 1) for l in ('ragged', 'clamped_1_0')]
    missing = [k for k in want if k not in RECORDS['loss_gradient']] + [m for m in OPTIM_MODELS if not any(k.startswith(m + ' ') for k in RECORDS['optimiser'])]
    assert not missing, 'cases without a passing element-wise check in this session (run the whole file): %s' % missing
    d = os.environ.get('WN_PARITY_REPORT_DIR')
    if d:
        groups = {}
        for case, rec in RECORDS['loss_gradient'].items():
            head = case.split('/')[0]
            for k, v in rec.items():
                if k != 'excluded':
                    w = groups.setdefault(head, {}).setdefault(k, dict(worst_err_over_bound=0.0, r32=0.0))
                    w['worst_err_over_bound'], w['r32'] = max(w['worst_err_over_bound'], v['worst']), max(w['r32'], v['r32'])
        optim = {}
        for case, rec in RECORDS['optimiser'].items():
            for k, v in rec.items():
                optim[k] = max(optim.get(k, 0.0), v)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, 'heads_parity.json'), 'w') as f:
            json.dump({'factor': HR.FACTOR, 'loss_gradient_worst_err_over_bound_per_head_and_group': groups,
                       'excluded_share_worst': max(r['excluded'] for r in RECORDS['loss_gradient'].values()),
                       'loss_scalar_worst_err_over_bound': max(r['err_over_bound'] for r in RECORDS['loss_scalar'].values()),
                       'optimiser_worst_increment_err_over_bound': optim, 'cases': RECORDS}, f, indent=1)
