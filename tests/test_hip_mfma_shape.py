"""Both MFMA shapes of the LDS-DMA ring kernel (csrc/wn_tile.h, WN_MFMA16 at wn_create), whatever the library's default is: mask 0 (every launch kind on
v_mfma_f32_32x32x16_bf16) and mask 15 (every kind the library knows on v_mfma_f32_16x16x32_bf16; the hook reports the bits it kept) on the smallest
geometries at which the tile engine can go wrong -- B 1 - 7, T 64 - 656, ragged lengths, partial 128-row tiles, dilations up to 512 that reach across tiles
and behind the utterance start into the zero page.  Every element of every launch is checked by test_hip_launch_local.check_step against fp64 inside
2^-8 |ref| + K 2^-23 A + E (bounds that do not depend on the order of summation), nothing excluded; two runs of one step give the same bytes (y_hat, gradients); and the
row-local tensors are the same bytes whether the batch runs as one part or as two."""
import pytest
import torch

from test_hip_launch_local import check_step
from test_hip_parity import CONFIGS, _inputs, _run_fwd
from test_hip_round6 import GEOMETRIES

pytestmark = pytest.mark.gpu

KNOWN_BITS = 7          # gate, d x, the other 32-channel-chunk launches
DEEP = dict(CONFIGS['paper_width_drop'], layers=10, stacks=1)          # dilations 1 ... 512


def _x_in(r):
    return r['y_or'] if r['cfg'].input_type == 'mulaw-quantize' else r['x_or'].view(r['B'], r['T'])


def _step_twice_and_check(name, mask, B, T, lengths):
    r = _run_fwd(name, B=B, T=T, lengths=lengths)
    cfg, eng = r['cfg'], r['eng']
    try:
        assert r['T'] == T
        assert eng.lib.wn_test_mfma16_mask(eng.h) == mask & KNOWN_BITS
        grads = torch.empty(eng.n_params, device='cuda')
        eng.train_bwd(grads)
        torch.cuda.synchronize()
        check_step('%s mfma16=%d B=%d T=%d' % (name, mask, B, T), eng, cfg, r['params'], B, T, lengths, r['seed'], _x_in(r), r['y_or'], r['c'], grads, g=r['g'])
        # the same step again: same bytes in everything the tile engine feeds -- y_hat and every gradient.  (The loss SCALAR is summed with float atomics over
        # its workgroups, DESIGN 3.3: its last bit depends on the order in which they retire, whatever the GEMMs do; the gradients do not read it.)
        first = (r['yhat_dev'].cpu(), grads.cpu())
        x_dev, y_dev, _, _, c = _inputs(cfg, r['hp'], B, T)
        loss2 = torch.zeros(1, device='cuda'); yhat2 = torch.empty_like(r['yhat_dev']); grads2 = torch.empty_like(grads)
        eng.train_fwd(x_dev, c.cuda(), y_dev, torch.tensor(lengths, dtype=torch.int32).cuda(), r['seed'], loss2, yhat2)
        eng.train_bwd(grads2)
        torch.cuda.synchronize()
        assert torch.isfinite(loss2).all() and abs(float(loss2) - float(r['loss_dev'])) <= 1e-5 * abs(float(loss2))
        for a, b, what in zip(first, (yhat2.cpu(), grads2.cpu()), ('y_hat', 'gradients')):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), '%s differ between two runs of the same step' % what
    finally:
        eng.close()


@pytest.mark.parametrize('mask', [0, 15])
@pytest.mark.parametrize('name', ['paper_width_drop', 'wide'])
def test_both_mfma_shapes_over_the_tile_boundary_geometries(name, mask, monkeypatch):
    """R 256 / G 512 (the 256-channel tiles: two m-tiles per wave, multi-A weight gradients) and 128 channels (one m-tile per wave) x the six geometries of
    the tile-boundary sweep."""
    monkeypatch.setenv('WN_MFMA16', str(mask))
    for B, T, lengths in GEOMETRIES:
        _step_twice_and_check(name, mask, B, T, lengths)


@pytest.mark.parametrize('mask', [0, 15])
@pytest.mark.parametrize('B,T,lengths', [(2, 656, [656, 513]), (3, 144, [144, 129, 2])])
def test_both_mfma_shapes_with_dilations_across_tiles(B, T, lengths, mask, monkeypatch):
    """One stack of 10 layers: taps 1 ... 512 rows back, across 128-row tiles and behind the start of the utterance (the zero page)."""
    monkeypatch.setenv('WN_MFMA16', str(mask))
    monkeypatch.setitem(CONFIGS, 'paper_width_drop_deep', DEEP)
    _step_twice_and_check('paper_width_drop_deep', mask, B, T, lengths)


def test_mfma16_batch_parts_give_the_same_bytes(monkeypatch):
    """A launch kind has one shape for every part of the batch: with every kind on 16x16x32 the row-local tensors of a step -- y_hat, every layer's input,
    gate output, d z and d x -- are the same bytes on one stream (1 part) and on two (2 parts)."""
    monkeypatch.setenv('WN_MFMA16', '15')
    B, T, lengths = 3, 144, [144, 129, 2]
    got = {}
    for parts in (1, 2):
        monkeypatch.setitem(CONFIGS, 'paper_width_drop_parts', CONFIGS['paper_width_drop'])
        r = _run_fwd('paper_width_drop_parts', B=B, T=T, lengths=lengths)
        cfg, eng = r['cfg'], r['eng']
        try:
            assert eng.lib.wn_test_mfma16_mask(eng.h) == KNOWN_BITS
            eng.set_batch_parts(parts)
            x_dev, y_dev, _, _, c = _inputs(cfg, r['hp'], B, T)
            loss = torch.zeros(1, device='cuda'); yhat = torch.empty_like(r['yhat_dev']); grads = torch.empty(eng.n_params, device='cuda')
            eng.train_fwd(x_dev, c.cuda(), y_dev, torch.tensor(lengths, dtype=torch.int32).cuda(), r['seed'], loss, yhat)
            eng.train_bwd(grads)
            torch.cuda.synchronize()
            R, G = cfg.residual_channels, cfg.gate_channels
            t = {'y_hat': yhat.cpu()}
            for l in range(cfg.layers):
                t['X%d' % l] = eng.debug_copy('X', l, B * T, R).cpu()
                t['U%d' % l] = eng.debug_copy('U', l, B * T, G // 2).cpu()
                t['DZ%d' % l] = eng.debug_copy('DZ', l, B * T, G).cpu()
                t['GX%d' % l] = eng.debug_copy('GX', l, B * T, R).cpu()
            got[parts] = t
        finally:
            eng.close()
    for k in got[1]:
        assert torch.equal(got[1][k].view(torch.int32), got[2][k].view(torch.int32)), '%s differs between 1 and 2 batch parts' % k
