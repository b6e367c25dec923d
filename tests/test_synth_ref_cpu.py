"""tests/synth_ref.py on the CPU: the float64 reference of teacher-forced synthesis pinned to the oracle, the per-step check applied to a
stand-in of a correct device (the path's own storage rounding evaluated in float32 arithmetic), and seeded faults of the kind a kernel
edge produces -- each must fail the check, named as the failure message names it.  tests/test_hip_synth_steps.py applies the same check
to the device."""
import pytest
import torch

import synth_ref as SR
from oracle import wavenet_oracle as O

B, T = 3, 320                                   # 20 frames of hop 16; 320 is no multiple of 7
VARIANTS = (('bf16', 'pipeline'), ('fp16', 'pipeline'), ('bf16', 'launch'), ('fp32', 'f32'))      # (storage type, the path whose rounding points are mirrored)

_CACHE = {}


def _case(name):
    """(cfg, params, inputs, c, g, ref) of a model, the float64 reference computed once."""
    if name not in _CACHE:
        hp, cfg, params, inputs, wav, c, g = SR.make_case(name, B, T)
        with torch.no_grad():
            ref = SR.synth_ref(params, cfg, inputs, c, g)
        _CACHE[name] = (cfg, params, inputs, c, g, ref)
    return _CACHE[name]


@pytest.mark.parametrize('name', list(SR.MODELS))
def test_reference_equals_the_oracle_step_in_float64(name):
    cfg, params, inputs, c, g, ref = _case(name)
    p64 = SR.f64_params(params)
    with torch.no_grad():
        x = SR.shifted_input(cfg, inputs).transpose(1, 2).contiguous()
        want = O.step(p64, cfg, x, c.double(), g=g if g is None or cfg.use_speaker_embedding else g.double())
    assert want.dtype == torch.float64
    err = float((ref - want).abs().max()) / float(want.abs().max())
    print('\n%s: max |synth_ref - O.step| / max |O.step| = %.2e' % (name, err))
    assert err <= 1e-12


@pytest.mark.parametrize('name', ['s6', 's6_gauss', 's6_softmax', 's6_gin', 's6_gin_raw_1d'])
def test_reference_equals_the_incremental_loop_from_step_0(name):
    """O.incremental(formulation='reference') in float32 -- zero queues, the silence start frame, one step at a time -- within 8 x the
    float32 yardstick on every element."""
    cfg, params, inputs, c, g, ref = _case(name)
    ti = inputs.unsqueeze(-1) if cfg.scalar_input else torch.nn.functional.one_hot(inputs.long(), cfg.quantize_channels).float()
    noise = {'gumbel_u': torch.full((T, B, cfg.quantize_channels), 0.5)} if not cfg.scalar_input else (
        {'eps': torch.zeros(T, B)} if cfg.out_channels == 2 else {'u1': torch.full((T, B, cfg.out_channels // 3), 0.5), 'u2': torch.full((T, B), 0.5)})
    with torch.no_grad():
        _, raw = O.incremental(params, cfg, c, noise=noise, test_inputs=ti, formulation='reference', g=g)
        emul = SR.synth_ref(params, cfg, inputs, c, g, store='fp32', path='f32')
    rec = SR.check_steps(raw, ref, emul, SR.F_FP32, cfg, 'f32', what=name + ' O.incremental fp32')
    print('\n%s: O.incremental (fp32) worst err / Y = %.2f at stream %d step %d' % (name, rec['worst_ratio'], rec['stream'], rec['step']))


def _standin(name, store, path, fault=None):
    cfg, params, inputs, c, g, ref = _case(name)
    key = (name, store, path)
    with torch.no_grad():
        if key not in _CACHE:
            _CACHE[key] = SR.synth_ref(params, cfg, inputs, c, g, store=store, path=path)
        dev = SR.synth_ref(params, cfg, inputs, c, g, store=store, path=path, arith=torch.float32, fault=fault, ksplit=4 if store == 'fp32' else 1)
    return cfg, ref, _CACHE[key], dev


def standin_ratios():
    """{model: {variant: worst err / Y of the float32-arithmetic stand-in}} (also written beside the device's figures)."""
    out = {}
    for name in SR.MODELS:
        for store, path in VARIANTS:
            cfg, ref, emul, dev = _standin(name, store, path)
            rec = SR.check_steps(dev, ref, emul, SR.FACTOR[store], cfg, path, what='%s stand-in %s' % (name, store))
            out.setdefault(name, {})['%s/%s' % (path, store)] = rec['worst_ratio']
    return out


def test_standin_of_a_correct_device_passes_the_check():
    """The condition that the reference alone stays inside the bound: the emulation in float32 arithmetic at F = 4 (16-bit) / F = 8 (fp32)."""
    r = standin_ratios()
    print()
    for name, v in r.items():
        print('%-14s ' % name + '  '.join('%s %.2f' % kv for kv in v.items()))
    assert max(max(v.values()) for v in r.values()) < SR.F_16BIT


# ---- seeded faults ------------------------------------------------------------------------------------------------------------------
def _faults(cfg, path, ref):
    """One stream, one step each; named as check_steps names the step.  The neighbour fault sits where stream 1's output moves by its MEDIAN
    amount from one step to the next (neither the easiest nor the hardest place to see it)."""
    move = (ref[1, :, 1:] - ref[1, :, :-1]).abs().amax(dim=0)
    tn = 1 + int(torch.argsort(move)[move.numel() // 2])
    dil = cfg.dilations()
    l = max(range(len(dil)), key=lambda i: (dil[i], i))               # the last layer of the largest dilation
    d, s = dil[l], SR.ring_slots(path, dil[l])
    f = {'neighbour': (dict(kind='neighbour', stream=1, step=tn), tn, None),
         'zero_tap_at_2d': (dict(kind='zero_tap2', layer=l, stream=1, step=2 * d), 2 * d, 'layer %d (d=%d, %d slots): t=2d' % (l, d, s)),
         'zero_tap_after_wrap': (dict(kind='zero_tap2', layer=l, stream=1, step=s), s, 'layer %d (d=%d, %d slots): t=slots' % (l, d, s)),
         'prev_cond_at_hop': (dict(kind='prev_cond', stream=1, step=10 * cfg.hop), 10 * cfg.hop, 'hop boundary (frame 10)')}
    if cfg.gin_channels > 0:
        f['gbias_of_another_stream'] = (dict(kind='gbias_swap', stream=1, other=0), None, None)
    return f


# {model: {fault: [path/store, ...]}}: the combinations the 16-bit noise HIDES; every other combination must be caught.  At the sites of _faults
# none is hidden on these models (the table the test prints is the record: the mildest is the neighbour fault on the Gaussian `legacy` model,
# whose residuals shrink by sqrt(.5) per layer -- 5.2 x the bf16 yardstick against F = 4, 17 x in fp16; the mildest dropped tap is 15 x).
HIDDEN = {
}


def _run_fault(name, store, path, fname):
    cfg, ref = _case(name)[0], _case(name)[5]
    fault, step, label = _faults(cfg, path, ref)[fname]
    cfg, ref, emul, dev = _standin(name, store, path, fault)
    try:
        rec = SR.check_steps(dev, ref, emul, SR.FACTOR[store], cfg, path, what='%s %s' % (name, fname))
        return False, rec['worst_ratio'], ''
    except AssertionError as e:
        msg = str(e)
        first = msg.splitlines()[1]
        assert 'stream 1 ' in first, msg                             # the worst offender is the faulted stream ...
        if step is not None:
            assert 'stream 1 step %d ' % step in msg, msg            # ... the faulted step is listed ...
        if label is not None:
            assert label in msg, msg                                 # ... and named
        return True, float(first.split('= ')[1].split(' x F')[0]) * SR.FACTOR[store], first.strip()


def test_seeded_faults_fail_the_check_by_name():
    table, caught, hidden = [], set(), set()
    for name in SR.MODELS:
        for store, path in VARIANTS:
            for fname in _faults(_case(name)[0], path, _case(name)[5]):
                hit, ratio, line = _run_fault(name, store, path, fname)
                (caught if hit else hidden).add((name, fname, path + '/' + store))
                table.append((name, fname, path + '/' + store, 'CAUGHT' if hit else 'hidden', ratio))
    print('\n%-14s %-24s %-14s %-7s %s' % ('model', 'fault', 'path/store', '', 'worst err / Y'))
    for row in table:
        print('%-14s %-24s %-14s %-7s %.2f' % row)
    want_hidden = {(m, f, v) for m, fs in HIDDEN.items() for f, vs in fs.items() for v in vs}
    assert hidden == want_hidden, 'hidden but expected caught: %s; caught but expected hidden: %s' % (sorted(hidden - want_hidden), sorted(want_hidden - hidden))
    assert caught
