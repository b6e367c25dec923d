"""Synthesis parity step by step: raw [B, O, T] of ONE eng.synthesize run, every element against the float64 reference of
tests/synth_ref.py under F x the path's own storage-rounding yardstick (F = 4 on the 16-bit paths, 8 in the fp32 mode; Y is computed from
the reference inside each test, nothing here was taken from a device run).  A whole-run rel-L2 cannot see one wrong step of one stream;
this can, and names the step by the kernel edges it sits on (tap validity, ring wrap, hop boundary, head CU, instance).

Every case asserts that the library ran the variant the case is meant to cover (path, storage type, instances, batched pre-multiplication,
width specialisation) -- a case that did not run its variant fails.  The slot instantiations and the stream pushes are not repeated: their
suites pin them bit for bit to the one-shot runs checked here.  With WN_PARITY_REPORT_DIR set the last test writes synth_steps_parity.json."""
import json
import os

import pytest
import torch

import synth_ref as SR
from hip_util import upload_params
from oracle import wavenet_oracle as O
from test_hip_synth import _noise

pytestmark = pytest.mark.gpu

T_DEFAULT = 320                                  # 20 frames of hop 16; no multiple of 7
PIPE_SWITCHES = ('WN_PIPE_BATCHPRE', 'WN_PIPE_SPEC', 'WN_PIPE_EARLY_FROM', 'WN_PIPE_INSTANCES', 'WN_PIPE_ABORT_EVERY', 'WN_PIPE_DTYPE', 'WN_PIPE_HEADS', 'WN_SYNTH_MODE')
SPEC_OF = {'w128': 2, 'w256': 1}                 # width specialisation of wn_synth_pipe_kernel (0: the generic kernel)

_REF = {}                                        # (model, B, T) -> (case tuple, float64 reference), (model, B, T, store, path) -> emulation
RECORDS = {}                                     # case id -> record (worst ratio, where, configuration)

# path id -> (steps_per_graph, storage type, rounding points of synth_ref, hparams overrides, synth_path)
PATHS = {
    'pipe_fp16': (0, 'fp16', 'pipeline', {}, 'pipeline'),
    'pipe_bf16': (0, 'bf16', 'pipeline', {}, 'pipeline'),
    'launch': (7, 'bf16', 'launch', {}, 'graph'),              # 320 = 45 x 7 + 5: a partial last span
    'fp32': (7, 'fp32', 'f32', dict(mi355_compute_dtype='fp32'), 'graph-fp32'),
}


def _case(model, B, T):
    if (model, B, T) not in _REF:
        _REF[(model, B, T)] = SR.make_case(model, B, T)
    return _REF[(model, B, T)]


def _reference(model, B, T, store, path, inputs=None):
    """(ref, emul): the float64 reference once per (model, B, T), the emulation once per path and storage type (teacher-forced cases; a
    free-running case passes the device's samples and is not cached)."""
    key = (model, B, T)
    hp, cfg, params, ti, wav, c, g = _case(model, B, T)
    with torch.no_grad():
        if inputs is not None:
            return SR.synth_ref(params, cfg, inputs, c, g), SR.synth_ref(params, cfg, inputs, c, g, store=store, path=path)
        if key + ('ref',) not in _REF:
            _REF[key + ('ref',)] = SR.synth_ref(params, cfg, ti, c, g)
        if key + (store, path) not in _REF:
            _REF[key + (store, path)] = SR.synth_ref(params, cfg, ti, c, g, store=store, path=path)
    return _REF[key + ('ref',)], _REF[key + (store, path)]


def _run(case_id, model, path_id, B=3, T=T_DEFAULT, expect=None, free=False):
    from wavenet_vocoder import _ext
    spg, store, rpath, extra, want_path = PATHS[path_id]
    hp0, cfg, params, ti, wav, c, g = _case(model, B, T)
    hp = SR.make_case(model, B, T, extra)[0] if extra else hp0
    eng = _ext.Engine(hp, B, T)
    eng.pack_weights(upload_params(eng, params))
    if g is not None:
        eng.set_global_condition(g.cuda())
    if rpath == 'pipeline':
        assert eng.pipeline_eligible(B), '%s does not fit the pipeline: the case cannot cover its variant' % model
        eng.pipeline_dtype(store == 'fp16')
    nz_dev, nz_or = _noise(cfg, T, B, seed=4 if free else 0)
    out = torch.empty(B, T, dtype=torch.float32 if cfg.scalar_input else torch.int32, device='cuda')
    raw = torch.empty(B, cfg.out_channels, T, device='cuda')
    ti_dev = None if free else ti.contiguous().cuda()
    # 1. one run, 2. its abort word
    eng.synthesize(c.cuda(), nz_dev.cuda(), out, raw, ti_dev, steps_per_graph=spg)
    torch.cuda.synchronize()
    eng.synth_check()
    # 3. the variant the library ran
    conf = eng.synth_config() if rpath == 'pipeline' else {}
    assert eng.synth_path == want_path, (case_id, eng.synth_path)
    want = {}
    if rpath == 'pipeline':
        want = dict(path='pipeline', half_storage=int(store == 'fp16'), instances=1, kernel_spec=SPEC_OF.get(model, 0),
                    batched_premultiplication=int(model == 'w256'), head_cus=2)
        want.update(expect or {})
        got = {k: conf.get(k) for k in want}
        assert got == want, '%s ran %s, meant to cover %s' % (case_id, got, want)
        assert eng.lib.wn_synth_last_instances(eng.h) == want['instances'] and eng.lib.wn_synth_last_batched(eng.h) == want['batched_premultiplication']
    raw_c, out_c = raw.cpu(), out.cpu()
    eng.close()
    # 4. every element against the reference
    ref, emul = _reference(model, B, T, store, rpath, inputs=out_c if free else None)
    variant = ('%s %s' % (want_path, store)) + (' inst=%(instances)d batchpre=%(batched_premultiplication)d spec=%(kernel_spec)d heads=%(head_cus)d early_from=%(early_from)d' % conf
                                                 if rpath == 'pipeline' else ' steps_per_graph=%d' % spg)
    try:
        rec = SR.check_steps(raw_c, ref, emul, SR.FACTOR[store], cfg, rpath, head_cus=conf.get('head_cus', 1) if rpath == 'pipeline' else 1,
                             instances=conf.get('instances', 1) if rpath == 'pipeline' else 1, what=case_id)
    except AssertionError as e:
        print('\n%-28s %s\n%s' % (case_id, variant, e))
        raise
    rec.update(case=case_id, model=model, B=B, T=T, store=store, variant=variant, free_running=free,
               config={k: v for k, v in conf.items()} if rpath == 'pipeline' else {'path': want_path, 'steps_per_graph': spg})
    RECORDS[case_id] = rec
    print('\n%-28s %s: worst err / Y = %.2f (F = %g) at stream %d step %d channel %d [%s]; rel-L2 %.2e' % (
        case_id, variant, rec['worst_ratio'], rec['factor'], rec['stream'], rec['step'], rec['channel'], '; '.join(rec['where']), rec['rel_l2']))
    # the sampler ran on those raw outputs (the existing sampler assertions, repeated)
    if not cfg.scalar_input:
        exp = torch.stack([O.sample_categorical(raw_c[:, :, t], nz_or['gumbel_u'][t]) for t in range(T)], 1)
        assert torch.equal(out_c.long(), exp)                                        # class ids exact
    elif cfg.out_channels == 2:
        assert torch.allclose(out_c, O.sample_from_gaussian(raw_c, nz_or['eps'].t(), cfg.log_scale_min_gauss), atol=2e-5)
    else:
        assert torch.allclose(out_c, O.sample_from_discretized_mix_logistic(raw_c, nz_or['u1'].permute(1, 0, 2), nz_or['u2'].t(), cfg.log_scale_min), atol=2e-5)
    return rec


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in PIPE_SWITCHES:
        monkeypatch.delenv(k, raising=False)


# ---- every path at B = 3 on every model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path_id', list(PATHS))
@pytest.mark.parametrize('model', list(SR.MODELS))
def test_teacher_forced_every_step(model, path_id):
    _run('%s-%s' % (model, path_id), model, path_id)


# ---- pipeline geometry on w256 (and the generic kernel on w128), T = 160 ---------------------------------------------------------------
GEOMETRY = {      # id -> (model, B, switches, expected configuration beyond the defaults of _run)
    'w256-b2': ('w256', 2, {}, {}),
    'w256-b9-two-instances': ('w256', 9, {}, dict(instances=2, head_cus=1)),                                        # the MULTI instantiations, is0 offsets
    'w256-b18-one-run-early': ('w256', 18, {'WN_PIPE_INSTANCES': '1'}, dict(instances=1, head_cus=2, early_from=18)),      # early requests on, both head CUs
    'w256-b3-no-batchpre': ('w256', 3, {'WN_PIPE_BATCHPRE': '0'}, dict(batched_premultiplication=0)),
    'w256-b3-generic': ('w256', 3, {'WN_PIPE_SPEC': '0'}, dict(kernel_spec=0)),
    'w128-b3-generic': ('w128', 3, {'WN_PIPE_SPEC': '0'}, dict(kernel_spec=0)),
    # (one case more than the plan asked for: the per-stream gate bias is indexed by is0 + s, and no other case has global conditioning on a second instance)
    's6_gin-b9-two-instances': ('s6_gin', 9, {}, dict(instances=2, head_cus=1)),
}


@pytest.mark.parametrize('gid', list(GEOMETRY))
def test_pipeline_geometry_every_step(gid, monkeypatch):
    model, B, env, expect = GEOMETRY[gid]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rec = _run(gid, model, 'pipe_fp16', B=B, T=160, expect=expect)
    if gid == 'w256-b18-one-run-early':
        assert B >= rec['config']['early_from']                                      # the early-request mode was on


# ---- free-running: the reference is fed the device's own samples -----------------------------------------------------------------------
@pytest.mark.parametrize('path_id', ['pipe_fp16', 'launch'])
@pytest.mark.parametrize('model', ['s6', 's6_softmax'])
def test_free_running_every_step(model, path_id):
    _run('%s-%s-free' % (model, path_id), model, path_id, B=2, free=True)


# ---- coverage of the kernel's template axes, and the report ----------------------------------------------------------------------------
def test_every_template_axis_was_exercised_both_ways():
    """wn_synth_pipe_kernel<H, MULTI, BP, SPEC>: the cases above ran under an element-wise check with both storage types, one and several
    instances, the batched and the per-stream pre-multiplication, and all three width specialisations."""
    want = ['%s-%s' % (m, p) for m in SR.MODELS for p in PATHS] + list(GEOMETRY) + ['%s-%s-free' % (m, p) for m in ('s6', 's6_softmax') for p in ('pipe_fp16', 'launch')]
    missing = [k for k in want if k not in RECORDS]
    assert not missing, 'cases without a passing element-wise check in this session (run the whole file): %s' % missing
    pipe = [r['config'] for r in RECORDS.values() if r['config'].get('path') == 'pipeline']
    axes = {'H (storage type)': {c['half_storage'] for c in pipe}, 'MULTI': {int(c['instances'] > 1) for c in pipe},
            'BP': {c['batched_premultiplication'] for c in pipe}, 'SPEC': {c['kernel_spec'] for c in pipe}}
    inst = sorted({(c['half_storage'], int(c['instances'] > 1), c['batched_premultiplication'], c['kernel_spec']) for c in pipe})
    print('\ntemplate axes exercised: %s\ninstantiations <H, MULTI, BP, SPEC> run: %s' % (axes, inst))
    assert axes['H (storage type)'] == {0, 1} and axes['MULTI'] == {0, 1} and axes['BP'] == {0, 1} and axes['SPEC'] == {0, 1, 2}
    assert any(c['head_cus'] == 2 and c['streams_per_instance'] >= c['early_from'] for c in pipe)      # early requests, streams alternating between two head CUs
    d = os.environ.get('WN_PARITY_REPORT_DIR')
    if d:
        from test_synth_ref_cpu import standin_ratios
        worst = {}
        for r in RECORDS.values():
            k = r['variant'].split(' inst=')[0].split(' steps_per_graph')[0]
            worst[k] = max(worst.get(k, 0.0), r['worst_ratio'])
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, 'synth_steps_parity.json'), 'w') as f:
            json.dump({'factor': SR.FACTOR, 'floor': SR.FLOOR, 'worst_ratio_per_path': worst, 'instantiations_H_MULTI_BP_SPEC': inst,
                       'cpu_standin_worst_ratio': standin_ratios(), 'cases': list(RECORDS.values())}, f, indent=1)
