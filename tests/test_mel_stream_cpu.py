"""Streaming mel analysis without a GPU: the ABI symbols; wn_mel_stream_ready against the rule written out in Python; the plan hook wn_test_mel_stream_plan against
tests/mel_stream_ref.py over seeded cut schedules; every validation code, and that a refused push leaves the counters alone; tests/host/mel_stream_main.cpp under
ASAN + UBSAN as an ordinary program; LiveVocoder's bookkeeping on a stub model; and that mi355_synthesis_live_chunk_ms = 0 constructs nothing."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import mel_stream_ref as M
import mel_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
WN_E_ARG, WN_E_SHAPE, WN_E_UNSUPPORTED, WN_E_STATE = -1, -2, -4, -5
SYMBOLS = ['wn_mel_stream_create', 'wn_mel_stream_destroy', 'wn_mel_stream_last_error', 'wn_mel_stream_ready', 'wn_mel_stream_push', 'wn_test_mel_stream_plan']


def _hp(name):
    n_fft, win, hop = M.GEOMETRIES[name]
    return mel_util.mel_hparams(n_fft=n_fft, win_size=win, hop_size=hop)


def _stream(name, rows=0, max_push=4000, **kw):
    from wavenet_vocoder import _ext
    return _ext.MelStream(_hp(name), rows, max_push, **kw)


def test_abi_symbols_are_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    hooks = text[text.index('#ifndef WN_NO_TEST_HOOKS'):]
    for s in SYMBOLS:
        assert re.search(r'\b%s\(' % s, text), s
        assert s in _ext.exported_symbols() and hasattr(_ext.load_library(), s)
    assert 'wn_test_mel_stream_plan(' in hooks and 'wn_test_mel_stream_plan(' not in text[:text.index('#ifndef WN_NO_TEST_HOOKS')]
    assert 'wn_mel_stream_push(' not in hooks and 'wn_mel_stream_ready(' not in hooks
    assert re.search(r'#define WN_ABI_VERSION\s+4\b', text) and _ext.WN_ABI_VERSION == 4      # additions only: the version stays


@pytest.mark.parametrize('name', sorted(M.GEOMETRIES))
def test_ready_against_the_rule(name):
    n_fft, win, hop = M.GEOMETRIES[name]
    Hl, Hr = M.geometry(n_fft, win, hop)
    assert Hl + Hr == win and (name != 'default' or (n_fft - win) // 2 != 0)
    ms = _stream(name)
    assert (ms.hop, ms.lag_samples, ms.lead_samples) == (hop, Hr, Hl)
    around = sorted(set(max(0, s + d) for s in (0, Hr - 1, Hr, Hr + hop - 1, Hr + hop, 7 * hop, Hr + 31 * hop, 2 ** 31 - 1 - hop) for d in (-1, 0, 1)))
    for S in around:
        for final in (False, True):
            want = (1 + S // hop) if final else ((S - Hr) // hop + 1 if S >= Hr else 0)
            assert ms.ready(S, final) == want, (S, final)
            if S < 10 ** 6:
                assert want == M.ready(n_fft, win, hop, S, final)
        assert ms.ready(S, False) <= ms.ready(S, True) == 1 + S // hop
    assert [ms.ready(S) for S in (0, Hr - 1, Hr, Hr + hop - 1, Hr + hop)] == [0, 0, 1, 1, 2]
    lib = ms.lib
    assert lib.wn_mel_stream_ready(None, 0, 0) == WN_E_ARG and lib.wn_mel_stream_ready(ms.h, -1, 0) == WN_E_ARG and lib.wn_mel_stream_ready(ms.h, 2 ** 31, 1) == WN_E_ARG
    ms.close()


@pytest.mark.parametrize('seed', range(4))
@pytest.mark.parametrize('name', sorted(M.GEOMETRIES))
def test_plan_hook_against_the_python_counters(name, seed):
    from wavenet_vocoder import _ext
    geom = M.GEOMETRIES[name]
    n_fft, win, hop = geom
    max_push = 5 * win + 3
    cuts = M.fixed_cuts(*geom, max_push)
    rs = np.random.RandomState(100 + seed)
    lens = [int(v) for v in rs.randint(0, 9 * win, size=5)] + [0, 1, hop, max_push]
    pushes = M.random_schedule(rs, lens, max_push, cuts, restart_mid={1: lens[1] // 2, 3: 1})
    # rows that ended are restarted with a second recording: restart after final
    again = M.random_schedule(rs, lens[::-1], max_push, cuts)
    pushes = pushes + again
    assert any(sum(n) == 0 for n, r, f in pushes) or any(0 in n for n, r, f in pushes)
    assert any(f[b] and n[b] == 0 for n, r, f in pushes for b in range(len(lens)))      # a final with n = 0
    ms = _stream(name, max_push=max_push)
    got = _ext.mel_stream_plan(ms, pushes, in_pitch=max_push, out_pitch=max_push // hop + 4)
    rows = [M.Row(*geom) for _ in lens]
    total = [0] * len(lens)
    for p, (n, r, f) in enumerate(pushes):
        assert got['status'][p] == 0
        for b, row in enumerate(rows):
            st, n_out, first = row.push(n[b], bool(r[b]), bool(f[b]))
            assert st == 'ok'
            if r[b]:
                total[b] = 0
            total[b] += n_out
            assert (got['n_out'][p, b], got['first_frame'][p, b], got['S'][p, b], got['F'][p, b], got['tail_len'][p, b]) == (n_out, first, row.S, row.F, row.tail_len), (p, b)
            assert 0 <= got['tail_len'][p, b] < win
            if f[b]:
                assert total[b] == 1 + row.S // hop == row.F      # summed n_out over the row
    assert all(row.ended for row in rows)
    ms.close()


def test_every_validation_code_and_a_refused_push_changes_nothing():
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    vp = ctypes.c_void_p
    hp = _hp('default')
    mb = np.zeros((hp.num_mels, 1 + hp.n_fft // 2), np.float32)

    def create(rows=0, max_push=8, basis=True, **over):
        cfg = _ext.mel_config_from_hparams(hp, 7, 9)      # (max_batch / max_samples are ignored)
        for k, v in over.items():
            setattr(cfg, k, v)
        h = vp()
        rc = lib.wn_mel_stream_create(ctypes.byref(cfg), mb.ctypes.data_as(vp) if basis else None, rows, max_push, ctypes.byref(h))
        if rc == 0:
            lib.wn_mel_stream_destroy(h)
        return rc, (lib.wn_mel_stream_last_error(None) or b'').decode() if rc else ''
    assert create()[0] == 0
    for kw, code, word in ((dict(abi_version=5), WN_E_ARG, 'abi_version'), (dict(basis=False), WN_E_ARG, 'mel_basis'), (dict(rows=-1), WN_E_ARG, 'max_rows'),
                           (dict(max_push=0), WN_E_ARG, 'max_push'), (dict(n_fft=1023), WN_E_SHAPE, 'n_fft'), (dict(win_size=4096), WN_E_SHAPE, 'win_size'),
                           (dict(hop_size=0), WN_E_SHAPE, 'hop_size'), (dict(num_mels=0), WN_E_SHAPE, 'num_mels'), (dict(num_mels=129), WN_E_UNSUPPORTED, 'num_mels'),
                           (dict(magnitude_power=0.0), WN_E_ARG, 'magnitude_power'), (dict(n_fft=1 << 17, win_size=1024), WN_E_UNSUPPORTED, 'n_fft'),
                           (dict(n_fft=4096, win_size=4096, hop_size=2048), WN_E_UNSUPPORTED, 'LDS')):
        rc, text = create(**kw)
        assert rc == code and word in text, (kw, rc, text)
    assert lib.wn_mel_stream_create(None, None, 0, 1, None) == WN_E_ARG
    # a geometry-only handle refuses every push before it looks at a row
    ms = _stream('default', max_push=8)
    x = np.zeros(8, np.float32)
    xp, one, no = x.ctypes.data_as(vp), (ctypes.c_int32 * 1)(4), (ctypes.c_int32 * 1)(-9)
    push = lambda *a: lib.wn_mel_stream_push(ms.h, *a)
    assert push(xp, 8, one, None, None, None, 1, xp, 8, 1, no, None) == WN_E_SHAPE and b'max_rows' in lib.wn_mel_stream_last_error(ms.h)
    assert push(xp, 8, None, None, None, None, 1, xp, 8, 1, no, None) == WN_E_ARG and push(xp, 8, one, None, None, None, 1, None, 8, 1, no, None) == WN_E_ARG
    assert push(xp, 8, one, None, None, None, 1, xp, 8, 1, None, None) == WN_E_ARG and push(xp, 8, one, None, None, None, 0, xp, 8, 1, no, None) == WN_E_ARG
    assert lib.wn_mel_stream_push(None, xp, 8, one, None, None, None, 1, xp, 8, 1, no, None) == WN_E_ARG and no[0] == -9
    # the plan of a push on the hook: every status of the header, and the counters after a refused push are those before it
    hop = ms.hop
    ok1, ok2, then = ([6, 3], [1, 1], None), ([0, 0], None, [0, 1]), ([2, 0], None, None)      # row 1 ends at the second push
    for bad, code in ((([9, 0], None, None), WN_E_SHAPE), (([-1, 0], None, None), WN_E_ARG), (([0, 1], None, None), WN_E_STATE), (([0, 0], None, [0, 1]), WN_E_STATE)):
        got = _ext.mel_stream_plan(ms, [ok1, ok2, bad, then], in_pitch=8, out_pitch=4)
        assert got['status'].tolist() == [0, 0, code, 0], (bad, got['status'])
        for key in ('S', 'F', 'tail_len'):
            assert (got[key][2] == got[key][1]).all(), (bad, key)
        assert (got['n_out'][2] == 0).all() and got['S'][1].tolist() == [6, 3] and got['F'][1].tolist() == [0, 1] and got['S'][3].tolist() == [8, 3]
    first = ([6, 0], [1, 1], None)
    for seq, kw, want, S0 in (([first, ([8, 0], None, None), ([1, 0], None, None)], dict(in_pitch=7, out_pitch=4), [0, WN_E_SHAPE, 0], [6, 6, 7]),
                              ([first, ([0, 0], None, [1, 0]), ([1, 0], None, None)], dict(in_pitch=8, out_pitch=0), [0, WN_E_SHAPE, 0], [6, 6, 7]),
                              ([([0, 0], [1, 1], None), ([1, 0], None, None)], dict(in_pitch=8, out_pitch=4, have_in=False), [0, WN_E_ARG], [0, 0]),
                              ([first, first], dict(in_pitch=-1, out_pitch=4), [WN_E_ARG, WN_E_ARG], [0, 0]),
                              ([first, first], dict(in_pitch=8, out_pitch=-1), [WN_E_ARG, WN_E_ARG], [0, 0])):
        got = _ext.mel_stream_plan(ms, seq, **kw)
        assert got['status'].tolist() == want and got['S'][:, 0].tolist() == S0, (kw, got['status'], got['S'])
    # a row beyond 2^31 - 1 samples since its restart
    ms2 = _stream('default', max_push=2 ** 30)
    got = _ext.mel_stream_plan(ms2, [([2 ** 30], [1], None), ([2 ** 30 - 1], None, None), ([1], None, None), ([0], None, [1])], in_pitch=2 ** 30, out_pitch=2 ** 23)
    assert got['status'].tolist() == [0, 0, WN_E_SHAPE, 0] and got['S'][:, 0].tolist() == [2 ** 30, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1]
    assert got['F'][3, 0] == 1 + (2 ** 31 - 1) // hop
    with pytest.raises(_ext.WnError):
        _ext.mel_stream_plan(_StubHandle(), [ok1])
    ms.close(); ms2.close()


class _StubHandle:
    h, hop = None, 275


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/host/mel_stream_main.cpp built with ASAN + UBSAN, run once as an ordinary child process"""
    exe = str(tmp_path_factory.mktemp('mel_stream') / 'mel_stream_main')
    r = subprocess.run(['hipcc', '-std=c++20', '-O1', '-g', '-Wall', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        '-I', os.path.join(ROOT, 'tacotron-2_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'mel_stream_main.cpp'), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    return subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)


def test_host_plan_under_address_and_ub_sanitizers(host_program):
    r = host_program
    assert r.returncode == 0 and 'mel stream ok' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    codes = dict(re.findall(r'^code (\w+) (-?\d+)$', r.stdout, re.M))
    want = {'sizes_ok': 0, 'sizes_rows': WN_E_ARG, 'sizes_push': WN_E_ARG, 'push_ok': 0, 'push_in_null': WN_E_ARG, 'push_n_null': WN_E_ARG, 'push_out_null': WN_E_ARG,
            'push_n_out_null': WN_E_ARG, 'push_b_zero': WN_E_ARG, 'push_n_negative': WN_E_ARG, 'push_pitch_negative': WN_E_ARG, 'push_b_over': WN_E_SHAPE,
            'push_max_push': WN_E_SHAPE, 'push_in_pitch': WN_E_SHAPE, 'push_out_pitch': WN_E_SHAPE, 'push_gain_not_finite': WN_E_ARG, 'push_ended': WN_E_STATE,
            'push_ended_restarted': 0, 'push_row_too_long': WN_E_SHAPE}
    assert {k: int(v) for k, v in codes.items()} == want


# ---- LiveVocoder's bookkeeping on a stub model (no device)
class _StubMel:
    def __init__(self, geom, rows, max_push):
        self.geom, self.rows, self.max_push, self.hop, self.num_mels = geom, rows, max_push, geom[2], 4
        self.lead_samples, self.lag_samples = M.geometry(*geom)
        self.row = [M.Row(*geom) for _ in range(rows)]
        self.calls, self.closed = [], False

    def push(self, samples, n=None, restart=None, final=None, gain=None, channels_first=True, out=None):
        assert channels_first and max(n) <= self.max_push
        res = [self.row[b].push(n[b], bool(restart[b]), bool(final[b])) for b in range(self.rows)]
        assert all(r[0] == 'ok' for r in res)
        n_out = [r[1] for r in res]
        mel = torch.zeros(self.rows, self.num_mels, max(n_out) + 2)
        for b in range(self.rows):
            mel[b, :, :n_out[b]] = torch.arange(res[b][2], res[b][2] + n_out[b], dtype=torch.float32)      # every frame carries its index
        self.calls.append((list(n), list(restart), list(final), list(gain)))
        return mel, n_out

    def close(self):
        self.closed = True


class _StubSession:
    lookahead = (2, 3)

    def __init__(self, rows, wide):
        self.rows, self.wide, self.opened, self.pushes, self.closed = rows, wide, [], [], False

    def open(self, slot, g=None, seed=None):
        self.opened.append((slot, g, seed))

    def push(self, items, **kw):
        self.pushes.append(({b: (fr.clone(), fin) for b, (fr, fin) in items.items()}, kw))
        return {b: torch.zeros(int(fr.shape[-1]) * 16) for b, (fr, fin) in items.items()}

    def check(self):
        pass

    def close(self):
        self.closed = True


class _StubModel:
    device = 'cpu'

    def __init__(self, geom):
        self.geom = geom
        self._hparams = mel_util.mel_hparams(clip_for_wavenet=False, normalize_for_wavenet=False)
        self.made = []

    def mel_stream(self, rows, max_push, preemphasis=None):
        self.mel = _StubMel(self.geom, rows, max_push)
        self.made.append('mel')
        return self.mel

    def slots(self, rows, steps_per_graph=None):
        self.session = _StubSession(rows, False)
        self.made.append('slots')
        return self.session

    def wide_slots(self, rows, steps_per_graph=None):
        self.session = _StubSession(rows, True)
        self.made.append('wide_slots')
        return self.session


def test_live_vocoder_forwards_n_out_frames_and_final():
    from wavenet_vocoder.live import LiveVocoder
    geom = M.GEOMETRIES['fft800']
    hop = geom[2]
    model = _StubModel(geom)
    voc = LiveVocoder(model, 3, 700)
    assert model.made == ['mel', 'slots'] and voc.lag_samples == M.geometry(*geom)[1] + 3 * hop
    voc.open(0, seed=5, gain=2.0); voc.open(2, seed=7)
    with pytest.raises(ValueError):
        voc.open(0)
    with pytest.raises(ValueError):
        voc.push(np.zeros((3, 700), np.float32), [0, 10, 0], None)      # row 1 is idle
    lens, pos, frames = {0: 9 * hop + 3, 2: 14 * hop}, {0: 0, 2: 0}, {0: [], 2: []}
    k = 0
    while voc._open[0] or voc._open[2]:
        n, fin = [0, 0, 0], [False] * 3
        for b in (0, 2):
            if voc._open[b]:
                n[b] = min(700, lens[b] - pos[b]); pos[b] += n[b]; fin[b] = pos[b] == lens[b]
        res = voc.push(np.zeros((3, 700), np.float32), n, fin)
        items, kw = model.session.pushes[-1]
        call = model.mel.calls[-1]
        assert call[1] == [int(k == 0), 0, int(k == 0)] and call[3][0] == 2.0 and call[3][2] == 1.0      # restart at the first push only; the gains travel
        for b in (0, 2):
            if n[b] == 0 and not fin[b]:
                assert b not in items and b not in res
                continue
            fr, f = items[b]
            assert f == fin[b] and int(fr.shape[-1]) == int(res[b].frames.shape[-1])      # final reaches the session in the push that flushes the row
            frames[b] += [int(v) for v in fr[0]]
        k += 1
    for b in (0, 2):
        assert frames[b] == list(range(1 + lens[b] // hop)) and voc.frames_in[b] == 1 + lens[b] // hop      # every frame once, in order: n_out per push
    assert model.session.opened == [(0, None, 5), (2, None, 7)]
    voc.open(0, seed=9)                                                                    # the row is free again, and restarts
    voc.push(np.zeros((3, 700), np.float32), [5, 0, 0], [True, False, False])
    assert model.mel.calls[-1][1] == [1, 0, 0] and model.session.pushes[-1][0][0][1] is True
    voc.close()
    assert model.mel.closed and model.session.closed
    wide = _StubModel(geom)
    LiveVocoder(wide, 33, 700)
    assert wide.made == ['mel', 'wide_slots']


def test_live_gain_is_the_float32_gain_of_the_device_route():
    from wavenet_vocoder import live
    hp = mel_util.mel_hparams()
    x = mel_util.make_signal('harmonic', 5000, 3)
    k = np.float32(0.97)
    whole = np.max(np.abs(x - k * np.concatenate([[np.float32(0)], x[:-1]]).astype(np.float32)))
    for cut in (1, 7, 1000, 5000):
        assert np.float32(live.chunked_peak([x[i:i + cut] for i in range(0, len(x), cut)], 0.97)) == whole
    assert live.peak_gain(hp, whole) == float((float(hp.rescaling_max) / torch.tensor([float(whole)]).clamp_min(1e-30))[0])      # analyse_wavs' expression
    assert abs(live.peak_gain(hp, whole) * float(whole) - hp.rescaling_max) < 1e-6 and np.isfinite(live.peak_gain(hp, 0.0))


def test_live_chunk_ms_zero_constructs_nothing(monkeypatch, tmp_path):
    import hparams as H
    from wavenet_vocoder import synthesize as S
    hp = H._build()
    assert hp.mi355_synthesis_live_chunk_ms == 0
    called = []
    monkeypatch.setattr(S, 'run_live_wav_synthesis', lambda *a, **k: called.append('live'))
    monkeypatch.setattr(S, 'analyse_wavs', lambda paths, hparams: [np.zeros((3, hp.num_mels), np.float32) for _ in paths])

    class Synth:
        def load(self, *a):
            pass

        def synthesize(self, mels, speakers, names, wav_dir, plot_dir):
            called.append('whole')
            return ['w-%s' % n for n in names]
    monkeypatch.setattr(S, 'Synthesizer', Synth)
    monkeypatch.delitem(sys.modules, 'wavenet_vocoder.live', raising=False)
    wavs = tmp_path / 'in'
    mel_util.write_wav_folder(str(wavs), hp.sample_rate, 275)

    class Args:
        wavs_dir = str(wavs)
    S.run_wav_synthesis(Args, None, str(tmp_path / 'out'), hp)
    assert called == ['whole'] and 'wavenet_vocoder.live' not in sys.modules
    hp.mi355_synthesis_live_chunk_ms = 50
    S.run_wav_synthesis(Args, None, str(tmp_path / 'out2'), hp)
    assert called == ['whole', 'live']
