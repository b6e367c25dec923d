"""The weight path on the device against the float64 references of tests/wnorm_ref.py, element by element (pytest -m gpu).

  * wn_weightnorm_apply_kernel: the context's effective parameter copy (wn_debug_copy 'PARAMS') after wn_pack_weights against ref_effective on
    every element, |dev - ref| <= (K/2 + 2 + 2 rho) 2^-24 |ref|; a column of zeros gives exact zeros; copies and gaps are bit-exact.
  * wn_weightnorm_grad_kernel: the raw gradients wn_train_bwd returns against ref_raw_grads(raw, the device's own 'DEFF') under the bound of
    wnorm_ref's docstring; the alignment gaps of a NaN-prefilled buffer come back as exact zeros.
  * wn_pack_kernel: every pack of every layer bit-equal to ref_pack of the device's own effective parameters, padding included; 'B1SUM' and
    'SKIPB' within their bounds and bit-equal where the arithmetic is a single rounding or exact.
  * the error codes of the read hooks.
Nothing is fitted: every number is a bound derived in wnorm_ref.py or bit equality.  The float32 evaluation of the same expressions
(wnorm_ref.f32_*) is printed beside the device as a yardstick; the ratios are records, not thresholds.  With WN_PARITY_REPORT_DIR set the last
test writes wnorm_parity.json (profiles/wnorm_parity.json is that file from an MI355X).  The effective-kernel gradients themselves ('DEFF') are
held to the float64 contraction of the device's own buffers in test_hip_launch_local.py."""
import ctypes
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import wnorm_ref as WR
from hip_util import SMALL, make_hp, oracle_cfg, upload_params
from oracle import wavenet_oracle as O
from test_hip_parity import _inputs
from wnorm_ref import CONFIGS, CRAFT_TENSOR, craft_columns, wn_params

pytestmark = pytest.mark.gpu

RECORDS = OrderedDict()      # 'config/kind' -> dict(worst_err_over_bound, f32_err_over_bound, tensor, index)
E_ARG, E_STATE = -1, -5


def _engine(hp, B, T, **kw):
    from wavenet_vocoder import _ext
    return _ext.Engine(hp, B, T, **kw)


def _record(case, kind, worst, f32, tensor, index):
    r = RECORDS.setdefault('%s/%s' % (case, kind), dict(worst_err_over_bound=0.0, f32_err_over_bound=0.0, tensor=None, index=0))
    r['f32_err_over_bound'] = max(r['f32_err_over_bound'], float(f32))
    if worst >= r['worst_err_over_bound']:
        r.update(worst_err_over_bound=float(worst), tensor=tensor, index=int(index))


def _device_effective(eng):
    """(name -> fp32 array, flat array) of the context's effective parameter copy."""
    lay, n = WR.effective_layout(eng.layout)
    flat = eng.debug_copy('PARAMS', 0, 1, n).cpu().numpy().reshape(-1)
    return WR.split_flat(flat, lay), flat, lay


def check_effective(case, eng, cfg, params):
    eff, flat, lay = _device_effective(eng)
    ref = WR.ref_effective(params, cfg)
    bound = WR.bound_effective(params, cfg, ref)
    f32 = WR.f32_effective(params, cfg)
    assert set(eff) == set(ref) and len(eff) == len(ref)      # (the engine's table and the oracle's dict order the tensors of a layer differently)
    fails = []
    for k in ref:
        if cfg.wavenet_weight_normalization and WR.is_normalised(params, k):
            w, i, msg = WR.compare('effective', k, eff[k], ref[k], bound[k])
            _record(case, 'effective', w, WR.compare('effective', k, f32[k], ref[k], bound[k])[0], k, i)
        else:
            _, _, msg = WR.compare_bits('copy', k, eff[k], ref[k])
        if msg:
            fails.append(msg)
    assert not fails, '[%s]\n' % case + '\n'.join(fails[:20])
    assert not flat[WR.gap_mask(lay, flat.size)].view(np.uint32).any(), '[%s] alignment gaps of the effective copy must be zero bits' % case
    return eff


EFFECTIVE_CASES = list(CONFIGS) + ['mol_weightnorm/inference_only']


@pytest.mark.parametrize('case', EFFECTIVE_CASES)
def test_effective_kernels_every_element(case):
    name = case.split('/')[0]
    hp = make_hp(**dict(SMALL, **CONFIGS[name]))
    cfg = oracle_cfg(hp)
    params = wn_params(cfg)
    eng = _engine(hp, 1, 4 * cfg.hop, inference_only=case.endswith('inference_only'))
    try:
        eng.pack_weights(upload_params(eng, params))
        torch.cuda.synchronize()
        check_effective(case, eng, cfg, params)
    finally:
        eng.close()


def test_effective_kernels_crafted_columns():
    """One kernel with a column of zeros (exact zeros out), columns with ss = 0.99e-12 and 1.01e-12 (either side of the clamp), one of magnitude
    1e3 and one negative gain."""
    hp = make_hp(**dict(SMALL, **CONFIGS['mol_weightnorm']))
    cfg = oracle_cfg(hp)
    params = craft_columns(wn_params(cfg))
    eng = _engine(hp, 1, 4 * cfg.hop)
    try:
        eng.pack_weights(upload_params(eng, params))
        torch.cuda.synchronize()
        eff = check_effective('mol_weightnorm/crafted', eng, cfg, params)
        col = eff[CRAFT_TENSOR].reshape(-1, eff[CRAFT_TENSOR].shape[-1])
        assert not col[:, 0].view(np.uint32).any()
        v = params[CRAFT_TENSOR].numpy().reshape(col.shape)
        g = params[CRAFT_TENSOR[:-6] + 'g'].numpy()
        assert np.array_equal(np.sign(col[:, 4]), -np.sign(v[:, 4])) and g[4] < 0
        # below the clamp the scale is g * 1e6, not g / ||v||: the two differ by 0.5 %, hundreds of bounds
        assert abs(float(np.abs(col[:, 1]).max() / (abs(g[1]) * 1e6 * np.abs(v[:, 1]).max())) - 1.0) < 1e-5
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ d v, d g
GRAD_CASES = list(CONFIGS) + ['mol_weightnorm/crafted', 'mol_weightnorm/fp32']


@pytest.mark.parametrize('case', GRAD_CASES)
def test_raw_gradients_from_the_device_deff(case):
    """One train_fwd + train_bwd at B = 3, T = 144, lengths [144, 129, 2] into a NaN-prefilled buffer: d v, d g of every element against
    ref_raw_grads(raw, DEFF) under the derived bound, copies bit-exact, gaps exactly 0."""
    name, _, variant = case.partition('/')
    over = dict(CONFIGS[name])
    if variant == 'fp32':
        over['mi355_compute_dtype'] = 'fp32'
    hp = make_hp(**dict(SMALL, **over))
    cfg = oracle_cfg(hp)
    B, T, lengths = 3, 144, [144, 129, 2]
    assert T % cfg.hop == 0
    params = wn_params(cfg)
    if variant == 'crafted':
        params = craft_columns(params)
    eng = _engine(hp, B, T)
    try:
        eng.pack_weights(upload_params(eng, params))
        x_dev, y_dev, _, _, c = _inputs(cfg, hp, B, T)
        if cfg.gin_channels > 0:
            eng.set_global_condition(torch.randint(0, cfg.n_speakers, (B,), generator=torch.Generator().manual_seed(11)).int().cuda())
        loss = torch.zeros(1, device='cuda')
        eng.train_fwd(x_dev, c.cuda(), y_dev, torch.tensor(lengths, dtype=torch.int32).cuda(), 1234, loss)
        grads = torch.full((eng.n_params,), float('nan'), device='cuda')
        eng.train_bwd(grads)
        torch.cuda.synchronize()
        assert np.isfinite(float(loss.item()))
        lay, n_eff = WR.effective_layout(eng.layout)
        deff = WR.split_flat(eng.debug_copy('DEFF', 0, 1, n_eff).cpu().numpy().reshape(-1), lay)
        flat = grads.cpu().numpy()
    finally:
        eng.close()
    gaps = WR.gap_mask(eng.layout, flat.size)
    assert gaps.any() and not flat[gaps].view(np.uint32).any(), '[%s] alignment gaps of the raw gradient must be exact zeros (a NaN-prefilled buffer)' % case
    dev = WR.split_flat(flat, eng.layout)
    assert sum(float(np.abs(d).sum()) for d in deff.values()) > 0
    ref, bound = WR.ref_raw_grads(params, deff, want_bound=True)
    f32 = WR.f32_raw_grads(params, deff)
    fails = []
    for k in ref:
        if k.endswith('/g') or WR.is_normalised(params, k):
            kind = 'd g' if k.endswith('/g') else 'd v (K = 1)' if params[k].numel() == params[k].shape[-1] else 'd v'
            w, i, msg = WR.compare(kind, k, dev[k], ref[k], bound[k])
            _record(case, kind, w, WR.compare(kind, k, f32[k], ref[k], bound[k])[0], k, i)
            if kind == 'd v (K = 1)':      # the cancellation residue of a gradient that is 0: recorded beside Adam's epsilon
                RECORDS['%s/%s' % (case, kind)].update(max_abs_residue=float(np.abs(dev[k]).max()), max_abs_d_g=float(np.abs(dev[k[:-6] + 'g']).max()),
                                                       adam_epsilon=float(hp.wavenet_adam_epsilon))
        else:
            _, _, msg = WR.compare_bits('d copy', k, dev[k], ref[k])
        if msg:
            fails.append(msg)
    print('[%s] err / bound: %s' % (case, '  '.join('%s %.3f (f32 %.3f)' % (k[len(case) + 1:], v['worst_err_over_bound'], v['f32_err_over_bound'])
                                                    for k, v in RECORDS.items() if k.startswith(case + '/d '))))
    assert not fails, '[%s]\n' % case + '\n'.join(fails[:20])


# ------------------------------------------------------------------------------------------------------------------ packs
WIDE = dict(residual_channels=256, gate_channels=512, skip_out_channels=256)
PACK_CASES = {
    'small': (dict(), None),                                     # w1 kil = 32 (G = 128), w1T kil = 0; out_channels = 30 -> K tail; C = 16 -> wcT padded to 96 rows
    'g192': (dict(gate_channels=192), None),                     # w1 kil = 0 (G % 128 != 0)
    'legacy': (dict(legacy=True), None),                         # non-trivial skip scale, layer 0's exponent L - 1
    'nobias': (dict(use_bias=False), None),                      # the zero tail
    'cin80': (dict(cin_channels=80, num_mels=80), None),         # 96-row wcT
    'cin128': (dict(cin_channels=128, num_mels=128), None),      # 128-row wcT
    'r128_g256': (dict(residual_channels=128, gate_channels=256, skip_out_channels=128), None),      # kil = 32 for w1 and w1T
    'r256_g512': (WIDE, None),                                   # kil = 32, WN_GEMM8P unset
    'r256_g512_gemm8p': (WIDE, '3'),                             # kil = 64 for w1 and w1T
    'mol_weightnorm': (CONFIGS['mol_weightnorm'], None),         # packs of the device's own effective kernels
}


def check_packs(case, eng, cfg, uploaded, gemm8p, NT):
    """Every pack, B1SUM and SKIPB of a packed context against the references of the device's own effective parameters.  case: the record's
    name (both pack_weights calls of a configuration add to the same records)."""
    eff, _, _ = _device_effective(eng)
    if not cfg.wavenet_weight_normalization:
        for k, t in uploaded.items():
            assert WR.compare_bits('copy', k, eff[k], t.numpy())[2] is None, k
    L = cfg.layers
    fails, n = [], 0
    for kind in WR.PACK_KINDS:
        for layer in (range(L) if kind in WR.LAYER_PACKS else (0,)):
            geo = WR.pack_geometry(cfg, kind, gemm8p, NT)
            assert eng.pack_info(kind, layer) == geo, (case, kind, layer, eng.pack_info(kind, layer), geo)
            dev = eng.pack_copy(kind, layer).cpu().numpy()
            nbad, _, msg = WR.compare_bits('pack ' + kind, 'layer %d (M %d K %d kil %d)' % ((layer,) + geo[:3]), dev, WR.ref_pack(eff, cfg, kind, layer, geo[2]))
            r = RECORDS.setdefault('%s/packs' % case, dict(packs=0, elements=0, differing=0))      # (all kinds and layers of the configuration)
            r['packs'] += 1; r['elements'] += dev.size; r['differing'] += nbad
            if msg:
                fails.append(msg)
            n += 1
    assert n == 5 * L + 6
    b1, b1_bound, b1_f32 = WR.ref_b1sum(eff, cfg)
    dev = eng.debug_copy('B1SUM', 0, L, cfg.gate_channels).cpu().numpy()
    w, i, msg = WR.compare('bias sum', 'B1SUM', dev, b1, b1_bound)
    _record(case, 'B1SUM', w, WR.compare('bias sum', 'B1SUM', b1_f32, b1, b1_bound)[0], 'B1SUM', i)
    fails += [m for m in (msg, WR.compare_bits('bias sum', 'B1SUM', dev, b1_f32)[2]) if m]
    sb, sb_bound, sb_f32, sb_exact = WR.ref_skipb(eff, cfg)
    dev = eng.debug_copy('SKIPB', 0, 1, cfg.skip_out_channels).cpu().numpy().reshape(-1)
    w, i, msg = WR.compare('bias sum', 'SKIPB', dev, sb, sb_bound)
    _record(case, 'SKIPB', w, WR.compare('bias sum', 'SKIPB', sb_f32, sb, sb_bound)[0], 'SKIPB', i)
    fails += [m for m in (msg, WR.compare_bits('bias sum', 'SKIPB', dev, sb_f32)[2] if sb_exact else None) if m]
    if not cfg.use_bias:
        assert not dev.any() and not b1.any()
    assert not fails, '[%s]\n' % case + '\n'.join(fails[:20])


@pytest.mark.parametrize('case', list(PACK_CASES))
def test_packs_bit_equal_after_pack_weights_alone(case, monkeypatch):
    over, gemm8p = PACK_CASES[case]
    if gemm8p is None:
        monkeypatch.delenv('WN_GEMM8P', raising=False)
    else:
        monkeypatch.setenv('WN_GEMM8P', gemm8p)
    hp = make_hp(**dict(SMALL, **over))
    cfg = oracle_cfg(hp)
    B, T = 1, 4 * cfg.hop
    eng = _engine(hp, B, T)
    try:
        mask = int(gemm8p or 0)
        assert eng.lib.wn_test_gemm8p_mask(eng.h) == mask
        params = wn_params(cfg) if cfg.wavenet_weight_normalization else O.init_params(cfg, seed=5339, bias_scale=0.05)
        eng.pack_weights(upload_params(eng, params))
        check_packs(case, eng, cfg, params, mask, B * T)
        if case == 'r256_g512_gemm8p':
            assert eng.pack_info('w1', 0)[2] == 64 and eng.pack_info('w1T', 0)[2] == 64
        # a second pack_weights with other parameters: the packs follow, the padding stays zero
        g = torch.Generator().manual_seed(99)
        params2 = OrderedDict((k, (v * (torch.rand(v.shape, generator=g) + 0.5) * (-1.0 if i % 2 else 1.0))) for i, (k, v) in enumerate(params.items()))
        first = eng.pack_copy('wh2T', 0).cpu()
        eng.pack_weights(upload_params(eng, params2))
        assert not torch.equal(first, eng.pack_copy('wh2T', 0).cpu())
        check_packs(case, eng, cfg, params2, mask, B * T)
        M, K, _, _ = eng.pack_info('wcT', 0)
        assert not WR.unfragment(eng.pack_copy('wcT', 0).cpu().numpy(), M, K)[cfg.cin_channels:].any()
        M, K, _, _ = eng.pack_info('wh2T', 0)
        assert not WR.unfragment(eng.pack_copy('wh2T', 0).cpu().numpy(), M, K)[:, cfg.out_channels:].any()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ hooks
def test_read_hooks_validate_their_arguments():
    hp = make_hp(**SMALL)
    cfg = oracle_cfg(hp)
    eng = _engine(hp, 1, 4 * cfg.hop)
    hpw = make_hp(**dict(SMALL, **CONFIGS['mol_weightnorm']))
    engw = _engine(hpw, 1, 4 * cfg.hop)
    try:
        buf = torch.zeros(1 << 20, device='cuda')
        info = (ctypes.c_int32 * 4)()
        dbg = lambda e, name, n: e.lib.wn_debug_copy(e.h, name, 0, ctypes.c_void_p(buf.data_ptr()), ctypes.c_int64(n), None)      # noqa: E731
        cpy = lambda e, kind, layer, n: e.lib.wn_test_pack_copy(e.h, kind, layer, ctypes.c_void_p(buf.data_ptr()), ctypes.c_int64(n))      # noqa: E731
        # before wn_pack_weights
        for name in (b'PARAMS', b'B1SUM', b'SKIPB'):
            assert dbg(eng, name, 8) == E_STATE, name
        assert eng.lib.wn_test_pack_info(eng.h, b'w1', 0, info) == E_STATE and cpy(eng, b'w1', 0, buf.numel()) == E_STATE
        assert eng.lib.wn_test_pack_info(eng.h, b'nope', 0, info) == E_ARG
        eng.pack_weights(upload_params(eng, O.init_params(cfg, seed=1)))
        engw.pack_weights(upload_params(engw, wn_params(oracle_cfg(hpw))))
        n_eff = WR.effective_layout(eng.layout)[1]
        assert n_eff == eng.n_params and WR.effective_layout(engw.layout)[1] < engw.n_params
        assert dbg(eng, b'PARAMS', n_eff) == 0 and dbg(eng, b'PARAMS', n_eff + 1) == E_ARG
        assert dbg(eng, b'B1SUM', cfg.layers * cfg.gate_channels + 1) == E_ARG and dbg(eng, b'SKIPB', cfg.skip_out_channels + 1) == E_ARG
        assert dbg(eng, b'DEFF', 8) == E_STATE                 # no weight normalisation
        assert dbg(engw, b'DEFF', 8) == E_STATE                # weight normalisation, but no wn_train_bwd yet
        assert dbg(eng, b'NOPE', 8) == E_ARG
        for kind in WR.PACK_KINDS:
            assert eng.lib.wn_test_pack_info(eng.h, kind.encode(), 0, info) == 0, kind
            M, K = info[0], info[1]
            assert cpy(eng, kind.encode(), 0, M * K - 1) == E_ARG and cpy(eng, kind.encode(), 0, M * K) == 0
        for kind in WR.LAYER_PACKS:
            assert eng.lib.wn_test_pack_info(eng.h, kind.encode(), cfg.layers, info) == E_ARG
            assert eng.lib.wn_test_pack_info(eng.h, kind.encode(), -1, info) == E_ARG and cpy(eng, kind.encode(), cfg.layers, buf.numel()) == E_ARG
        assert eng.lib.wn_test_pack_info(eng.h, b'W1', 0, info) == E_ARG and cpy(eng, b'wcT ', 0, buf.numel()) == E_ARG
        assert eng.lib.wn_test_pack_info(eng.h, b'w1', 0, None) == E_ARG and eng.lib.wn_test_pack_info(None, b'w1', 0, info) == E_ARG
        torch.cuda.synchronize()
    finally:
        eng.close(); engw.close()


def test_write_the_parity_report():
    want = ['%s/effective' % c for c in EFFECTIVE_CASES + ['mol_weightnorm/crafted']] + ['%s/d v' % c for c in GRAD_CASES] + \
           ['%s/d g' % c for c in GRAD_CASES] + ['%s/%s' % (c, k) for c in PACK_CASES for k in ('packs', 'B1SUM', 'SKIPB')] + \
           ['%s/d v (K = 1)' % c for c in GRAD_CASES if CONFIGS[c.split('/')[0]].get('input_type', 'raw') != 'mulaw-quantize']
    missing = [k for k in want if k not in RECORDS]
    assert not missing, 'cases without a passing check in this session (run the whole file): %s' % missing
    assert all(v['differing'] == 0 and v['packs'] == 2 * (5 * oracle_cfg(make_hp(**dict(SMALL, **PACK_CASES[k.split('/')[0]][0]))).layers + 6)
               for k, v in RECORDS.items() if k.endswith('/packs'))
    d = os.environ.get('WN_PARITY_REPORT_DIR')
    if d:
        with open(os.path.join(d, 'wnorm_parity.json'), 'w') as f:
            head = dict(rho_ulps=WR.RHO, note='err / bound per configuration and kind, every element; f32 = numpy float32 with a sequential accumulator; '
                                              'packs: all kinds and layers, both pack_weights calls; records, not thresholds')
            f.write('{\n' + ''.join(' %s: %s,\n' % (json.dumps(k), json.dumps(v)) for k, v in head.items()) + ' "records": {\n' +
                    ',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in RECORDS.items()) + '\n }\n}\n')
