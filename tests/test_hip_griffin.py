"""Griffin-Lim on the device (csrc/wn_griffin.hip) under the STAGED rule of tests/griffin_ref.py -- the spectrum before the projection against float64 STFT of
the device's input, the output of an iteration against float64 projection + ISTFT of the device's OWN spectrum, the magnitudes from a mel against float64,
each within 8 x max(float32 yardstick, 2^-23 x the largest value), no element left out -- over (64, 48, 12), (96, 80, 20), (64, 64, 16) and one case of
(2048, 1100, 275); ragged rows of 2, 31, 32, 33 and 65 frames in batches of 1 and 3 with a sentinel beyond every row; five kinds of signal; whole runs by
their properties (the spectral convergence does not increase, and the device after 2 k iterations is at least as converged as float64 after k); and the
bit-for-bit identities.  WN_GRIFFIN_PARITY_OUT=<file> makes the session write the worst error / bound per stage and geometry there
(profiles/griffin_parity.json is such a file)."""
import json
import os

import numpy as np
import pytest
import torch

import griffin_ref as R

pytestmark = pytest.mark.gpu
PARITY = {}
SENTINEL = -7.25
BATCHES = ([65], [2], [31, 65, 2], [33, 32, 31])      # B = 1 and B = 3, frame counts around the 32-frame tile


@pytest.fixture(scope='module', autouse=True)
def parity_record():
    yield
    path = os.environ.get('WN_GRIFFIN_PARITY_OUT')
    if path and PARITY:
        with open(path, 'w') as f:
            json.dump({'what': 'wn_griffin_run on an MI355X against the float64 reference of tests/griffin_ref.py, stage by stage: worst error / bound over every '
                               'element, bound = 8 x max(float32 yardstick, 2^-23 x the largest value) per frame (spectrum, magnitudes) or row (output, start); '
                               'yardstick_scale = the worst yardstick / floor', 'cases': PARITY}, f, indent=1, sort_keys=True)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _handle(name, rows, max_frames, **level):
    from wavenet_vocoder import _ext
    geo = R.GEOMETRIES[name]
    return _ext.GriffinLim(None, rows, max_frames, cfg=_ext.griffin_config(*geo, **level))


def _case(kind, frames, geo, seed, pad=3):
    """S [B, F_max + pad, bins] (NaN beyond a row's frames), y0 [B, pitch] (NaN beyond a row's samples), u likewise"""
    B, Fm, nb = len(frames), max(frames) + pad, 1 + geo[0] // 2
    S = np.full((B, Fm, nb), np.nan, np.float32)
    u = np.full((B, Fm, nb), np.nan, np.float32)
    y0 = np.full((B, geo[2] * (Fm - 1) + 5), np.nan, np.float32)
    for b, F in enumerate(frames):
        S[b, :F], x = R.target(kind, F, seed + 7 * b, geo)
        u[b, :F] = R.uniforms(F, geo, seed + 100 + b)
        y0[b, :len(x)] = 0.0 if kind == 'zeros' else R.signal('noise', len(x), seed + 50 + b, geo[0])
    return S, u, y0


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _sentinel(frames, geo, extra=9):
    return torch.full((len(frames), geo[2] * (max(frames) - 1) + extra), SENTINEL, device='cuda')


def _record(key, geo, stage, worst, scale):
    PARITY.setdefault(key, {'n_fft': geo[0], 'win_size': geo[1], 'hop': geo[2]})[stage] = {'worst_error_over_bound': worst, 'yardstick_scale': scale}


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('name', ['A', 'B', 'C'])
def test_spectrum_output_and_start_stage_by_stage(name, kind):
    geo = R.GEOMETRIES[name]
    g = _handle(name, 3, 70)
    g.store_spectrum(True)
    ws = wo = wst = ss = so = sst = 0.0
    for i, frames in enumerate(BATCHES):
        S, u, y0 = _case(kind, frames, geo, 10 * i + 1)
        out = g.run_magnitude(_dev(S), frames, iters=1, y0=_dev(y0), out=_sentinel(frames, geo))
        got, X = _np(out), g.spectrum(S.shape[1])
        st = _np(g.run_magnitude(_dev(S), frames, iters=0, u=_dev(u), out=_sentinel(frames, geo)))
        for b, F in enumerate(frames):
            n = R.num_samples(F, geo[2])
            assert np.all(got[b, n:] == SENTINEL) and np.all(st[b, n:] == SENTINEL), (frames, b)      # nothing beyond a row's samples is written
            if kind == 'zeros':
                assert np.all(got[b, :n] == 0.0) and np.all(st[b, :n] == 0.0)
            a, sa = R.check_spectrum(X[b, :F], y0[b, :n], F, geo)
            c, sc = R.check_output(got[b, :n], X[b, :F], S[b, :F], F, geo)
            e, se = R.check_start(st[b, :n], S[b, :F], u[b, :F], F, geo)
            print('%s %-8s frames %r row %d: spectrum %.3f output %.3f start %.3f (error / bound)' % (name, kind, frames, b, a, c, e))
            ws, wo, wst, ss, so, sst = max(ws, a), max(wo, c), max(wst, e), max(ss, sa), max(so, sc), max(sst, se)
    key = '%s/%s' % (name, kind)
    _record(key, geo, 'spectrum', ws, ss); _record(key, geo, 'output', wo, so); _record(key, geo, 'start', wst, sst)
    g.close()
    assert ws <= 1.0 and wo <= 1.0 and wst <= 1.0, (ws, wo, wst)


def test_production_geometry_two_rows():
    geo = R.GEOMETRIES['P']
    frames = [40, 33]
    g = _handle('P', 2, 40)
    g.store_spectrum(True)
    S, u, y0 = _case('tones', frames, geo, 3, pad=0)
    got = _np(g.run_magnitude(_dev(S), frames, iters=1, y0=_dev(y0), out=_sentinel(frames, geo)))
    X = g.spectrum(S.shape[1])
    st = _np(g.run_magnitude(_dev(S), frames, iters=0, u=_dev(u), out=_sentinel(frames, geo)))
    worst = [0.0, 0.0, 0.0]
    scale = [0.0, 0.0, 0.0]
    for b, F in enumerate(frames):
        n = R.num_samples(F, geo[2])
        assert np.all(got[b, n:] == SENTINEL) and np.all(st[b, n:] == SENTINEL)
        for j, (w, s) in enumerate((R.check_spectrum(X[b, :F], y0[b, :n], F, geo), R.check_output(got[b, :n], X[b, :F], S[b, :F], F, geo),
                                    R.check_start(st[b, :n], S[b, :F], u[b, :F], F, geo))):
            worst[j], scale[j] = max(worst[j], w), max(scale[j], s)
    print('P tones frames %r: spectrum %.3f output %.3f start %.3f (error / bound)' % (frames, *worst))
    for j, stage in enumerate(('spectrum', 'output', 'start')):
        _record('P/tones', geo, stage, worst[j], scale[j])
    g.close()
    assert max(worst) <= 1.0, worst


def _mel_case(name, variant, frames, seed, num_mels=12):
    from wavenet_vocoder import _ext
    geo = R.GEOMETRIES[name]
    lv = R.mel_level(variant)
    basis = R.mel_basis(num_mels, geo[0])
    pinv = R.pinv_of(basis)
    Fm = max(frames) + 2
    mel = np.full((len(frames), Fm, num_mels), np.nan, np.float32)
    for b, F in enumerate(frames):
        S, _ = R.target('tones' if b % 2 == 0 else 'noise', F, seed + b, geo)
        mel[b, :F] = R.normalised_mel(S, basis, lv)
    if lv['clip']:
        mel[0, 0, :3] = (9.0, -9.0, 4.0)      # beyond the clipping range on both sides
    cfg = _ext.griffin_config(*geo, num_mels=num_mels, magnitude_power=lv['magnitude_power'], power=lv['power'], min_level_db=lv['lo'], ref_level_db=lv['ref'],
                              max_abs_value=lv['maxabs'], signal_normalization=lv['norm'], allow_clipping=lv['clip'], symmetric_mels=lv['sym'])
    return geo, lv, pinv, mel, _ext.GriffinLim(None, len(frames), Fm, cfg=cfg, pinv=pinv)


@pytest.mark.parametrize('variant', sorted(R.MEL_VARIANTS))
@pytest.mark.parametrize('name', ['A', 'B'])
def test_magnitudes_from_a_mel_against_float64(name, variant):
    frames = [33, 2, 65]
    geo, lv, pinv, mel, g = _mel_case(name, variant, frames, 5)
    Fm = mel.shape[1]
    out_a = _np(g.run_mel(_dev(mel), frames, iters=2, seed=4))
    mag = g.magnitudes(Fm)
    out_b = _np(g.run_mel(_dev(np.ascontiguousarray(mel.transpose(0, 2, 1))), frames, iters=2, seed=4, channels_first=True))
    mag_cf = g.magnitudes(Fm)
    worst = scale = 0.0
    for b, F in enumerate(frames):
        assert np.array_equal(mag[b, :F], mag_cf[b, :F])      # both layouts: the same bits
        w, s = R.check_magnitudes(mag[b, :F], mel[b, :F], pinv, lv)
        print('%s %-9s row %d: magnitudes %.3f (error / bound)' % (name, variant, b, w))
        worst, scale = max(worst, w), max(scale, s)
    assert np.array_equal(out_a, out_b)
    _record('%s/mel_%s' % (name, variant), geo, 'magnitudes', worst, scale)
    g.close()
    assert worst <= 1.0


@pytest.mark.parametrize('name', ['A', 'B'])
def test_whole_runs_converge_like_float64(name):
    """c(k) = || |STFT(y_k)| - S || / || S || on the device's y_k: non-increasing in k (Griffin and Lim's theorem for this window-normalised inverse), and
    c_device(2 k) <= c_float64(k)"""
    geo = R.GEOMETRIES[name]
    frames = [65, 33, 40]
    S, u, _ = _case('tones', frames, geo, 21, pad=0)
    g = _handle(name, 3, 70)
    ks = (1, 2, 4, 8, 16, 32)
    dev = {}
    y = g.run_magnitude(_dev(S), frames, iters=1, u=_dev(u))
    dev[1] = _np(y).copy()
    for k in ks[1:]:
        dev[k] = _np(g.continue_(k // 2)).copy()
    for b, F in enumerate(frames):
        n = R.num_samples(F, geo[2])
        c_dev = {k: R.convergence(dev[k][b, :n], S[b, :F], F, geo) for k in ks}
        y64, c64 = R.start(S[b, :F], u[b, :F], F, geo), {}
        done = 0
        for k in ks[:-1]:
            y64 = R.iterate(y64, np.asarray(S[b, :F], np.float64), F, geo, k - done); done = k
            c64[k] = R.convergence(y64, S[b, :F], F, geo)
        print('%s row %d: device %s float64 %s' % (name, b, ['%.4f' % c_dev[k] for k in ks], ['%.4f' % c64[k] for k in ks[:-1]]))
        for a, c in zip(ks[:-1], ks[1:]):
            assert c_dev[c] <= c_dev[a], (b, a, c, c_dev)
            assert c_dev[c] <= c64[a], (b, a, c_dev[c], c64[a])
    g.close()


def test_all_zero_magnitudes_give_exact_zeros():
    geo = R.GEOMETRIES['A']
    frames = [33, 2]
    g = _handle('A', 2, 40)
    S = np.zeros((2, 33, 33), np.float32)
    u = np.stack([R.uniforms(33, geo, 1), R.uniforms(33, geo, 2)])
    out = _np(g.run_magnitude(_dev(S), frames, iters=3, u=_dev(u), out=_sentinel(frames, geo)))
    for b, F in enumerate(frames):
        n = R.num_samples(F, geo[2])
        assert np.all(out[b, :n] == 0.0) and np.all(out[b, n:] == SENTINEL)
    g.close()


# ---- the bit-for-bit identities
def test_two_runs_agree_and_the_hook_changes_no_bit():
    geo = R.GEOMETRIES['B']
    frames = [33, 65, 2]
    S, u, _ = _case('tones', frames, geo, 2)
    g = _handle('B', 3, 70)
    a = _np(g.run_magnitude(_dev(S), frames, iters=5, u=_dev(u), out=_sentinel(frames, geo)))
    b = _np(g.run_magnitude(_dev(S), frames, iters=5, u=_dev(u), out=_sentinel(frames, geo)))
    g.store_spectrum(True)
    c = _np(g.run_magnitude(_dev(S), frames, iters=5, u=_dev(u), out=_sentinel(frames, geo)))
    g.store_spectrum(False)
    d = _np(g.run_magnitude(_dev(S), frames, iters=5, u=_dev(u), out=_sentinel(frames, geo)))
    g.close()
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)
    assert not np.all(a[0, :geo[2] * 32] == 0.0)


def test_zero_phase_start_is_the_start_from_zero_uniforms():
    geo = R.GEOMETRIES['A']
    frames = [33, 31]
    S, u, _ = _case('noise', frames, geo, 6)
    g = _handle('A', 2, 40)
    a = _np(g.run_magnitude(_dev(S), frames, iters=2, seed=None, out=_sentinel(frames, geo)))
    b = _np(g.run_magnitude(_dev(S), frames, iters=2, u=_dev(np.where(np.isnan(u), np.nan, 0.0).astype(np.float32)), out=_sentinel(frames, geo)))
    g.close()
    assert np.array_equal(a, b)


def test_a_row_alone_equals_the_row_in_any_batch():
    """at any row index, under other pitches (F_max of the source, out_pitch) and, from a mel, both layouts"""
    geo = R.GEOMETRIES['A']
    frames = [65, 33, 31]
    S, u, _ = _case('tones', frames, geo, 9)
    g = _handle('A', 3, 70)
    full = _np(g.run_magnitude(_dev(S), frames, iters=4, u=_dev(u), out=_sentinel(frames, geo)))
    for b, F in enumerate(frames):
        n = R.num_samples(F, geo[2])
        alone = _np(g.run_magnitude(_dev(S[b:b + 1, :F]), [F], iters=4, u=_dev(u[b:b + 1, :F]), out=_sentinel([F], geo, extra=2)))
        assert np.array_equal(alone[0, :n], full[b, :n]), b
        order = [(b + 1) % 3, b]      # the row at index 1 of another batch
        two = _np(g.run_magnitude(_dev(S[order]), [frames[i] for i in order], iters=4, u=_dev(u[order]), out=_sentinel([frames[i] for i in order], geo, extra=1)))
        assert np.array_equal(two[1, :n], full[b, :n]), b
    g.close()
    mframes = [33, 2, 65]
    geo, lv, pinv, mel, gm = _mel_case('A', 'clip_sym', mframes, 5)
    full = _np(gm.run_mel(_dev(mel), mframes, iters=3, seed=8))
    uu = torch.rand((3, mel.shape[1], 33), generator=torch.Generator(device='cuda').manual_seed(8), device='cuda')
    for b, F in enumerate(mframes):
        n = R.num_samples(F, geo[2])
        cf = np.ascontiguousarray(mel[b:b + 1, :F].transpose(0, 2, 1))
        alone = _np(gm.run_mel(_dev(cf), [F], iters=3, u=uu[b:b + 1, :F].contiguous(), channels_first=True))
        assert np.array_equal(alone[0, :n], full[b, :n]), b
    gm.close()


def test_run_then_continue_equals_one_run():
    geo = R.GEOMETRIES['B']
    frames = [33, 65]
    S, u, _ = _case('noise', frames, geo, 4)
    g = _handle('B', 2, 70)
    whole = _np(g.run_magnitude(_dev(S), frames, iters=7, u=_dev(u), out=_sentinel(frames, geo)))
    g.run_magnitude(_dev(S), frames, iters=3, u=_dev(u))
    part = _np(g.continue_(4, out=_sentinel(frames, geo)))
    same = _np(g.continue_(0, out=_sentinel(frames, geo)))
    g.close()
    assert np.array_equal(whole, part) and np.array_equal(whole, same)


def test_hparams_handle_runs_a_default_mel():
    """_ext.GriffinLim from the default hparams (2048 / 1100 / 275, 80 mels, power 1.5): a tone's mel comes back as a signal with the tone's pitch"""
    import hparams as H
    from datasets import audio
    from wavenet_vocoder import _ext
    hp = H._build()
    sr, hop = hp.sample_rate, audio.get_hop_size(hp)
    F = 40
    t = np.arange(hop * (F - 1))
    x = (0.5 * np.sin(2 * np.pi * 440.0 * t / sr)).astype(np.float32)
    mel = audio.melspectrogram(x, hp).astype(np.float32)      # [num_mels, F]
    g = _ext.GriffinLim(hp, 1, F)
    y = _np(g.run_mel(_dev(mel[None]), [F], iters=30, channels_first=True, seed=1))[0]
    g.close()
    assert np.all(np.isfinite(y))
    lo, hi = R.mel_band(hp, 440.0)
    peak = R.spectral_peak(y, sr)
    print('peak %.1f Hz in the band [%.1f, %.1f] of the mel filter that holds 440 Hz' % (peak, lo, hi))
    assert lo <= peak <= hi, (peak, lo, hi)
