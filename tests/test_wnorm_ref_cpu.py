"""tests/wnorm_ref.py pinned on the CPU (no GPU): the float64 references of weight normalisation against the oracle and float64 autograd, their
bounds against a plain float32 evaluation with a sequential accumulator (the arithmetic of the kernels), ref_pack against the inverse fragment
formula and against a second, segment-by-segment construction of the same packs, and five seeded faults that every check must name."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import wnorm_ref as WR
from hip_util import SMALL, make_hp, oracle_cfg
from oracle import wavenet_oracle as O

CONFIGS, CRAFT_TENSOR, wn_params, craft_columns, random_deff = WR.CONFIGS, WR.CRAFT_TENSOR, WR.wn_params, WR.craft_columns, WR.random_deff


def _cfg(name):
    return oracle_cfg(make_hp(**dict(SMALL, **CONFIGS[name])))


@pytest.mark.parametrize('name', list(CONFIGS))
def test_ref_effective_equals_the_oracle(name):
    """1e-12 relative (max-abs over max-abs): two float64 evaluations of v g / ||v||, ~1e4 ulps of slack for the association of <= 768 terms."""
    cfg = _cfg(name)
    params = wn_params(cfg)
    ref = WR.ref_effective(params, cfg)
    want = O.effective_params(OrderedDict((k, v.double()) for k, v in params.items()), cfg)
    assert list(ref) == list(want)
    for k in want:
        w = want[k].numpy()
        assert ref[k].shape == w.shape
        if not k.endswith('/kernel'):
            assert np.array_equal(np.asarray(ref[k], dtype=np.float64), w), k
        assert float(np.abs(ref[k] - w).max()) <= 1e-12 * float(np.abs(w).max()), k


@pytest.mark.parametrize('name', list(CONFIGS))
def test_ref_raw_grads_equal_float64_autograd(name):
    """d v, d g against float64 autograd through O.effective_params for a random d W, 1e-10 relative per tensor.  The scale of a K = 1 kernel
    (d v is pure cancellation, autograd's own answer is a rounding residue) is that of the operands, |g / n| (|dW| + |v| |b|)."""
    cfg = _cfg(name)
    params = wn_params(cfg)
    deff = random_deff(params)
    leaf = OrderedDict((k, v.double().clone().requires_grad_(True)) for k, v in params.items())
    eff = O.effective_params(leaf, cfg)
    loss = sum((eff[k] * deff[k].double()).sum() for k in eff)
    gs = torch.autograd.grad(loss, list(leaf.values()))
    ref = WR.ref_raw_grads(params, deff)
    assert list(ref) == list(params)
    for k, g in zip(leaf, gs):
        g = g.numpy()
        scale = float(np.abs(g).max())
        if k.endswith('/kernel') and params[k].numel() == params[k].shape[-1]:
            v, gain, dW = params[k].double().numpy(), params[k[:-6] + 'g'].double().numpy(), deff[k].double().numpy()
            scale = float((np.abs(gain / np.abs(v)) * 2 * np.abs(dW)).max())
            assert float(np.abs(g).max()) <= 1e-10 * scale, (k, 'autograd: d v of a K = 1 kernel is not ~0')
        assert float(np.abs(ref[k] - g).max()) <= 1e-10 * scale, (k, float(np.abs(ref[k] - g).max()), scale)


F32_RATIOS = {}


def _check_f32(cfg, params, deff, fault=None):
    """The float32 stand-in (optionally with a fault) against the float64 references: list of failure messages, worst ratios per kind."""
    fails, worst = [], {}
    ref = WR.ref_effective(params, cfg)
    bound = WR.bound_effective(params, cfg, ref)
    got = WR.f32_effective(params, cfg, fault)
    for k in ref:
        if WR.is_normalised(params, k):
            r, _, msg = WR.compare('effective', k, got[k], ref[k], bound[k])
            worst['effective'] = max(worst.get('effective', 0.0), r)
        else:
            _, _, msg = WR.compare_bits('copy', k, got[k], ref[k])
        if msg:
            fails.append(msg)
    rg, bg = WR.ref_raw_grads(params, deff, want_bound=True)
    gg = WR.f32_raw_grads(params, deff, fault)
    for k in rg:
        kind = 'd g' if k.endswith('/g') else 'd v' if WR.is_normalised(params, k) else 'd copy'
        r, _, msg = WR.compare(kind, k, gg[k], rg[k], bg[k])
        if WR.is_normalised(params, k) and params[k].numel() == params[k].shape[-1]:
            kind = 'd v (K = 1)'
        worst[kind] = max(worst.get(kind, 0.0), r)
        if msg:
            fails.append(msg)
    return fails, worst


@pytest.mark.parametrize('name', list(CONFIGS))
def test_float32_evaluation_stays_inside_every_bound(name):
    """numpy float32, one sequential accumulator over k: inside every bound, the crafted columns (zeros, both sides of the clamp, 1e3, a negative gain)
    and the K = 1 column included.  The printed worst ratios are records."""
    cfg = _cfg(name)
    params = craft_columns(wn_params(cfg))
    fails, worst = _check_f32(cfg, params, random_deff(params))
    F32_RATIOS[name] = worst
    print('[%s] float32 err / bound: %s' % (name, '  '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert not fails, '\n'.join(fails[:20])
    eff = WR.f32_effective(params, cfg)[CRAFT_TENSOR]
    assert not eff.reshape(-1, eff.shape[-1])[:, 0].any()                               # the zero column: exactly 0
    if cfg.scalar_input:
        assert 'd v (K = 1)' in worst


# ------------------------------------------------------------------------------------------------------------------ packs
PACK_CONFIGS = {
    'small': dict(),                                          # out_channels = 30 -> K tail of wh2T, C = 16 -> wcT padded to 96 rows
    'legacy': dict(legacy=True),
    'nobias_cin80': dict(use_bias=False, cin_channels=80, num_mels=80),
    'cin128_r128': dict(cin_channels=128, num_mels=128, residual_channels=128, gate_channels=256, skip_out_channels=128),
}


def standin_pack(eff, cfg, kind, layer, kil, fault=None):
    """A second construction of a pack, element by element the way the device does it: segments (tensor, offset, k0, nk, stride_k, stride_m,
    scale) over the flat tensors as wn_build_packs lists them, the gate-row permutation, and the storage formula applied per storage index."""
    L, R, G, S, Oc, C = cfg.layers, cfg.residual_channels, cfg.gate_channels, cfg.skip_out_channels, cfg.out_channels, cfg.cin_channels
    GH = G // 2
    sc = WR.skip_scales(cfg)
    q = lambda l, s: 'ResidualConv1DGLU_%d/residual_block_%s/kernel' % (l, s)      # noqa: E731
    segs = []
    if kind == 'w1':
        m_valid = G
        if kil:
            for kb in range(R // kil):
                for j in range(3):
                    segs.append((q(layer, 'causal_conv'), (j * R + kb * kil) * G, (kb * 3 + j) * kil, kil, G, 1, 1.0))
        else:
            for j in range(3):
                segs.append((q(layer, 'causal_conv'), j * R * G, j * R, R, G, 1, 1.0))
        segs.append((q(layer, 'cin_conv'), 0, 3 * R, C, G, 1, 1.0))
    elif kind == 'wo':
        m_valid, segs = R, [(q(layer, 'out_conv'), 0, 0, GH, R, 1, 1.0)]
    elif kind == 'ws':
        m_valid, segs = S, [(q(layer, 'skip_conv'), 0, 0, GH, S, 1, sc[layer])]
    elif kind == 'w2T':
        m_valid, segs = GH, [(q(layer, 'out_conv'), 0, 0, R, 1, R, 1.0), (q(layer, 'skip_conv'), 0, R, S, 1, S, sc[layer])]
    elif kind == 'w1T':
        m_valid = R
        if kil:
            for kb in range(G // kil):
                for j in range(3):
                    segs.append((q(layer, 'causal_conv'), j * R * G + kb * kil, (kb * 3 + j) * kil, kil, 1, G, 1.0))
        else:
            for j in range(3):
                segs.append((q(layer, 'causal_conv'), j * R * G, j * G, G, 1, G, 1.0))
    elif kind == 'wskip':
        m_valid, segs = S, [(q(l, 'skip_conv'), 0, l * GH, GH, S, 1, sc[l]) for l in range(L)]
    elif kind == 'wh1':
        m_valid, segs = S, [('final_convolution_1/kernel', 0, 0, S, S, 1, 1.0)]
    elif kind == 'wh2':
        m_valid, segs = Oc, [('final_convolution_2/kernel', 0, 0, S, Oc, 1, 1.0)]
    elif kind == 'wh2T':
        m_valid, segs = S, [('final_convolution_2/kernel', 0, 0, Oc, 1, Oc, 1.0)]
    elif kind == 'wh1T':
        m_valid, segs = S, [('final_convolution_1/kernel', 0, 0, S, 1, S, 1.0)]
    else:
        m_valid, segs = C, [(q(l, 'cin_conv'), 0, l * G, G, 1, G, 1.0) for l in range(L)]
    M, K, _, il = WR.pack_geometry(cfg, kind)
    i = np.arange(M * K)
    j, lane, rest = i % 8, (i // 8) % 64, i // 512
    ks, mtile = rest % (K // 16), rest // (K // 16)
    m, k = mtile * 32 + (lane & 31), ks * 16 + 8 * (lane >> 5) + j
    mm = m
    if il:
        grp = 32 if fault == 'interleave32' else 64
        blk, w = m // grp, m % grp
        mm = np.where(w < grp // 2, blk * (grp // 2) + w, GH + blk * (grp // 2) + (w - grp // 2))
    out = np.zeros(M * K, dtype=np.float32)
    for name, off, k0, nk, stride_k, stride_m, scale in segs:
        flat = WR.np32(eff[name]).reshape(-1)
        sel = (k >= k0) & (k < k0 + nk) & (mm < m_valid)
        src = flat[off + (k[sel] - k0) * stride_k + mm[sel] * stride_m]
        if fault == 'scale_after_rounding':
            out[sel] = WR.bf16_round(np.float32(scale) * WR.bf16_round(src))
        else:
            out[sel] = WR.bf16_round(np.float32(scale) * src)
    return out


def _pack_cases(cfg):
    for kind in WR.PACK_KINDS:
        for layer in (range(cfg.layers) if kind in WR.LAYER_PACKS else (0,)):
            for kil in ((0, 32, 64) if kind in ('w1', 'w1T') else (0,)):
                yield kind, layer, kil


def _f32_eff(cfg, seed=5339):
    params = O.init_params(cfg, seed=seed, bias_scale=0.05)
    return OrderedDict((k, v.float().numpy()) for k, v in params.items())


@pytest.mark.parametrize('name', list(PACK_CONFIGS))
def test_ref_pack_unshuffles_to_the_logical_matrix_and_equals_the_second_construction(name):
    """All eleven kinds, every layer, kil = 0 / 32 / 64: the inverse fragment formula recovers the bf16-rounded logical matrix, whose valid block
    holds exactly the rounded parameters it is documented to hold and whose padding is zero; and the pack is bit-equal to the segment-wise
    construction (which shares no index arithmetic with ref_pack)."""
    cfg = oracle_cfg(make_hp(**dict(SMALL, **PACK_CONFIGS[name])))
    eff = _f32_eff(cfg)
    R, G, S, Oc, C, L = cfg.residual_channels, cfg.gate_channels, cfg.skip_out_channels, cfg.out_channels, cfg.cin_channels, cfg.layers
    valid = {'w1': (G, 3 * R + C), 'wo': (R, G // 2), 'ws': (S, G // 2), 'w2T': (G // 2, R + S), 'w1T': (R, 3 * G), 'wskip': (S, L * G // 2),
             'wh1': (S, S), 'wh2': (Oc, S), 'wh2T': (S, Oc), 'wh1T': (S, S), 'wcT': (C, L * G)}
    n = 0
    for kind, layer, kil in _pack_cases(cfg):
        M, K, _, _ = WR.pack_geometry(cfg, kind)
        assert M % 32 == 0 and K % 16 == 0 and (kind != 'wcT' or M == (96 if C <= 96 else 128))
        W = WR.logical_matrix(eff, cfg, kind, layer, kil)
        p = WR.ref_pack(eff, cfg, kind, layer, kil)
        assert p.shape == (M * K,) and np.array_equal(WR.unfragment(p, M, K), W), (kind, layer, kil)
        mv, kv = valid[kind]
        assert not W[mv:].any() and not W[:, kv:].any(), (kind, 'padding must be zero')
        assert np.count_nonzero(W[:mv, :kv]) > 0.99 * mv * kv
        _, _, msg = WR.compare_bits('pack ' + kind, 'layer %d kil %d' % (layer, kil), standin_pack(eff, cfg, kind, layer, kil), p)
        assert msg is None, msg
        n += 1
    assert n == L * (3 + 1 + 1 + 1 + 3) + 6
    # spot values straight from the documentation of the sources: W1[row 32 of group 0] is sigmoid partner GH + 0, W1T[r][tap j block kb] ...
    dil = eff['ResidualConv1DGLU_1/residual_block_causal_conv/kernel']
    W1 = WR.logical_matrix(eff, cfg, 'w1', 1, 0)
    assert W1[32, R + 5] == WR.bf16_round(dil[1:2, 5, G // 2])[0] and W1[64 + 3, 2 * R + 7] == WR.bf16_round(dil[2:3, 7, 32 + 3])[0]
    W1T = WR.logical_matrix(eff, cfg, 'w1T', 1, 32)
    assert W1T[9, (1 * 3 + 2) * 32 + 4] == WR.bf16_round(dil[2:3, 9, 32 + 4])[0]


def test_pack_geometry_thresholds():
    """kil from the configuration: 0 below the tile engine's widths, 32 at them, 64 only with the 8-phase bit and its own widths."""
    small = oracle_cfg(make_hp(**SMALL))
    # (SMALL has G = 128, R = 64: its w1 already takes the tile engine's 32-channel interleave; G = 192 is the width that does not)
    assert WR.pack_geometry(small, 'w1')[2:] == (32, 1) and WR.pack_geometry(small, 'w1T')[2] == 0 and WR.pack_geometry(small, 'wcT')[0] == 96
    g192 = oracle_cfg(make_hp(**dict(SMALL, gate_channels=192)))
    assert WR.pack_geometry(g192, 'w1')[2:] == (0, 1) and WR.pack_geometry(g192, 'w1T')[2] == 0
    assert WR.pack_geometry(small, 'wh2T')[:2] == (64, 32) and WR.pack_geometry(small, 'wh2')[:2] == (32, 64)
    mid = oracle_cfg(make_hp(**dict(SMALL, residual_channels=128, gate_channels=256, skip_out_channels=128)))
    assert WR.pack_geometry(mid, 'w1')[2] == 32 and WR.pack_geometry(mid, 'w1T')[2] == 32
    assert WR.pack_geometry(mid, 'w1', gemm8p=3, NT=1000)[2] == 64 and WR.pack_geometry(mid, 'w1T', gemm8p=3, NT=1000)[2] == 32      # (G % 256 == 0, but R % 256 != 0)
    big = oracle_cfg(make_hp(**dict(SMALL, residual_channels=256, gate_channels=512, skip_out_channels=256, cin_channels=128, num_mels=128)))
    assert WR.pack_geometry(big, 'w1')[2] == 32 and WR.pack_geometry(big, 'wcT')[0] == 128
    assert WR.pack_geometry(big, 'w1', gemm8p=3, NT=1000)[2] == 64 and WR.pack_geometry(big, 'w1T', gemm8p=3, NT=1000)[2] == 64
    assert WR.pack_geometry(big, 'w1', gemm8p=2, NT=1000)[2] == 32 and WR.pack_geometry(big, 'w1T', gemm8p=1, NT=1000)[2] == 32
    assert WR.pack_geometry(big, 'w1', gemm8p=3, NT=2 ** 22)[2] == 32          # NT * R * 2 reaches 2^31: the 8-phase kernel is refused


# ------------------------------------------------------------------------------------------------------------------ seeded faults
def test_five_seeded_faults_fail_and_are_named():
    cfg = _cfg('mol_weightnorm')
    params = craft_columns(wn_params(cfg))
    deff = random_deff(params)
    clean, _ = _check_f32(cfg, params, deff)
    assert not clean
    # 1. gain omitted: every normalised kernel fails, forward and d v
    fails, _ = _check_f32(cfg, params, deff, 'gain_omitted')
    assert any(m.startswith('effective input_convolution/kernel:') for m in fails) and any(m.startswith('d v ' + CRAFT_TENSOR) for m in fails)
    # 2. the clamp on sqrt(ss) instead of ss: only the column below the clamp (index 1 of the crafted tensor) moves, by 0.5 %
    fails, _ = _check_f32(cfg, params, deff, 'clamp_on_sqrt')
    assert fails and all(CRAFT_TENSOR[:-6] in m for m in fails), fails[:5]
    assert any(m.startswith('effective ' + CRAFT_TENSOR) for m in fails) and any(m.startswith('d g ' + CRAFT_TENSOR[:-6] + 'g') for m in fails)
    # 3. d v without the projection term: d v fails by name, d g and the forward do not
    fails, _ = _check_f32(cfg, params, deff, 'no_projection')
    assert fails and all(m.startswith('d v ') for m in fails) and any('input_convolution/kernel' in m for m in fails)
    # 4. / 5. the packs
    leg = oracle_cfg(make_hp(**dict(SMALL, legacy=True)))
    eff = _f32_eff(leg)
    named = {}
    for fault in ('scale_after_rounding', 'interleave32'):
        for kind, layer, kil in _pack_cases(leg):
            _, _, msg = WR.compare_bits('pack ' + kind, 'layer %d kil %d' % (layer, kil), standin_pack(eff, leg, kind, layer, kil, fault), WR.ref_pack(eff, leg, kind, layer, kil))
            if msg:
                named.setdefault(fault, set()).add(msg.split(':')[0].split(' layer')[0])
    assert named['scale_after_rounding'] == {'pack ws', 'pack w2T', 'pack wskip'}
    assert named['interleave32'] == {'pack w1'}
