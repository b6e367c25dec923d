"""Streaming synthesis, host side (no GPU): the upsample halo wn_synth_stream_lookahead declares for all five upsample types, checked against
the oracle's upsample net in float64 (with the declared halo a window reproduces the full upsample over its interior; for 'SubPixel' and
'Resize' one frame less does not), and the frames-in -> samples-out schedule of the façade's SynthesisStream."""
import numpy as np
import pytest
import torch

from hip_util import make_hp, oracle_cfg
from oracle import wavenet_oracle as O

TYPES = ['NearestNeighbor', '2D', 'SubPixel', '1D', 'Resize']
SCALES = [[5, 5, 11], [11, 25], [4, 4], [15, 20]]


def _model(utype, scales):
    hp = make_hp(upsample_type=utype, upsample_scales=scales, hop_size=int(np.prod(scales)), cin_channels=16, num_mels=16,
                 residual_channels=64, gate_channels=128, skip_out_channels=64, layers=4, stacks=2, out_channels=30)
    cfg = oracle_cfg(hp)
    params = {k: v.double() for k, v in O.init_params(cfg, seed=7, bias_scale=0.1).items()}
    g = torch.Generator().manual_seed(3)
    for k in params:                       # random upsample kernels (the NN initialisation would make every frame's rows alike)
        if k.startswith('local_conditioning_upsampling') and k.endswith('kernel'):
            params[k] = torch.randn(params[k].shape, generator=g, dtype=torch.float64) * 0.5
    return hp, cfg, params


def _expected(utype, scales):
    if utype == 'SubPixel':
        hop, h, later = int(np.prod(scales)), 0, 1
        for s in reversed(scales):
            later *= s; h += later
        return -(-h // hop), -(-h // hop)
    if utype == 'Resize':
        hop, hl, hr, later = int(np.prod(scales)), 0, 0, 1
        for s in reversed(scales):
            p = (s - 1) // 2
            hl += p * later; hr += (s - 1 - p) * later; later *= s
        return -(-hl // hop), -(-hr // hop)
    return 0, 0


@pytest.mark.parametrize('utype', TYPES)
@pytest.mark.parametrize('scales', SCALES, ids=lambda s: 'x'.join(map(str, s)))
def test_lookahead_is_the_exact_upsample_halo(utype, scales):
    from wavenet_vocoder import _ext
    hp, cfg, params = _model(utype, scales)
    left, right = _ext.stream_lookahead(_ext.config_from_hparams(hp, 1, cfg.hop))
    assert (left, right) == _expected(utype, scales)
    if utype == 'Resize':
        assert (left, right) == (1, 1)                    # sum_i p_i prod(later scales) < hop / 2 for every list here
    if utype == 'SubPixel':
        assert (left, right) == (2, 2)                    # [5, 5, 11]: 341 samples of context at hop 275; two layers: hop + s_last
    hop, Tc, a, b = cfg.hop, 14, 2, 12
    g = torch.Generator().manual_seed(1)
    c = torch.randn(2, cfg.cin_channels, Tc, generator=g, dtype=torch.float64)
    with torch.no_grad():
        full = O.upsample(params, cfg, c)
        win = O.upsample(params, cfg, c[:, :, a:b].contiguous())
    # frames [a + left, b - right) of the window are exact
    lo, hi = a + left, b - right
    d = (win[:, :, (lo - a) * hop:(hi - a) * hop] - full[:, :, lo * hop:hi * hop]).abs().max().item()
    assert d < 1e-12, d
    if left > 0:                                          # tight: the frame one short of the halo differs by O(1)
        f = lo - 1
        d1 = (win[:, :, (f - a) * hop:(f - a + 1) * hop] - full[:, :, f * hop:(f + 1) * hop]).abs().max().item()
        assert d1 > 1e-3, d1
    if right > 0:
        f = hi
        d1 = (win[:, :, (f - a) * hop:(f - a + 1) * hop] - full[:, :, f * hop:(f + 1) * hop]).abs().max().item()
        assert d1 > 1e-3, d1
    # a window edge at the utterance's own start / end is no artificial edge
    with torch.no_grad():
        head = O.upsample(params, cfg, c[:, :, :b].contiguous())
    assert (head[:, :, :(b - right) * hop] - full[:, :, :(b - right) * hop]).abs().max().item() < 1e-12


def test_lookahead_rejects_bad_configurations():
    from wavenet_vocoder import _ext
    hp, cfg, _ = _model('SubPixel', [4, 4])
    cc = _ext.config_from_hparams(hp, 1, cfg.hop)
    cc.upsample_scales[1] = 0
    with pytest.raises(_ext.WnError):
        _ext.stream_lookahead(cc)


def test_stream_schedule_frames_in_samples_out():
    from wavenet_vocoder.models.wavenet import stream_schedule
    # right = 2 frames held back; (pushed frames, final) -> generated frame spans
    pushes = [(0, False), (1, False), (3, False), (0, False), (1, False), (5, False), (0, True)]
    got, done, pushed = [], 0, 0
    for k, final in pushes:
        pushed += k
        s, e = stream_schedule(done, pushed, right=2, final=final)
        got.append((s, e)); done = e
    assert got == [(0, 0), (0, 0), (0, 2), (2, 2), (2, 3), (3, 8), (8, 10)]
    assert stream_schedule(4, 4, right=0, final=True) == (4, 4)          # final with nothing pending
    assert stream_schedule(0, 1, right=3, final=False) == (0, 0)         # a push shorter than the lookahead
    assert stream_schedule(0, 1, right=3, final=True) == (0, 1)
