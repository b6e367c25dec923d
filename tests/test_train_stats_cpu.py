"""Training summaries, host side (no GPU): the C ABI names, every validation code, the bucket table, the statistics evaluated on the host through
wn_test_stats_hist_host / wn_test_stats_tensors_host (the very element steps, cuts and joins the kernels inline, csrc/wn_stats.h) against the numpy
reference of tests/stats_util.py -- counts, extremes and non-finite counters equal, sums inside the derived any-order bound -- their invariance to what
lies beyond a row's length and in the pitch gap, the TensorFlow encoding, the host functions under ASAN + UBSAN in a stand-alone program, the training
loop's plumbing against a stand-in TrainStats, and five faults seeded into the numpy reference, each of which the comparison must catch."""
import ctypes
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import stats_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
WN_E_ARG, WN_E_SHAPE, WN_E_HIP, WN_E_STATE = -1, -2, -3, -5
INT_NAMES = ('wn_stats_create', 'wn_stats_hist_limits', 'wn_stats_histogram', 'wn_stats_set_tensors', 'wn_stats_tensors', 'wn_test_stats_hist_host',
             'wn_test_stats_tensors_host')


def _raw_hist(x, pitch, lengths, B, T):
    """the hook on a [B, pitch] array, T <= pitch"""
    from wavenet_vocoder import _ext
    x = np.ascontiguousarray(x, np.float32)
    ln = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
    bucket, summary = np.full(SU.N_BUCKETS, -1, np.int64), np.full(8, np.nan)
    vp = ctypes.c_void_p
    rc = _ext.load_library().wn_test_stats_hist_host(x.ctypes.data_as(vp), pitch, None if ln is None else ln.ctypes.data_as(vp), B, T, bucket.ctypes.data_as(vp),
                                                     summary.ctypes.data_as(vp))
    assert rc == 0, rc
    return _ext._hist_dict(bucket, summary)


def test_symbols_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    declared = set(re.findall(r'\bint\s+(wn_\w+)\s*\(', text))
    lib = _ext.load_library()
    for name in INT_NAMES + ('wn_stats_destroy', 'wn_stats_last_error'):
        assert name in _ext.exported_symbols() and hasattr(lib, name), name
    for name in INT_NAMES:
        assert name in declared, name
    assert 'void wn_stats_destroy(' in text and 'const char* wn_stats_last_error(' in text
    assert '#define WN_ABI_VERSION 4' in text and _ext.WN_ABI_VERSION == 4
    assert '#define WN_HIST_BUCKETS 1551' in text and _ext.WN_HIST_BUCKETS == 1551
    hooks = text[text.index('#ifndef WN_NO_TEST_HOOKS'):]
    assert 'wn_test_stats_hist_host(' in hooks and 'wn_test_stats_tensors_host(' in hooks and 'wn_stats_create(' not in hooks      # the hooks alone are fenced
    assert ctypes.sizeof(_ext.WnStatsConfig) == 16


def _create(**kw):
    from wavenet_vocoder import _ext
    cfg = _ext.stats_config(kw.pop('max_rows', 0), kw.pop('max_time', 8), kw.pop('max_tensors', 3))
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    rc = _ext.load_library().wn_stats_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc == 0:
        _ext.load_library().wn_stats_destroy(h)
    return rc


def test_create_validates_before_any_device_call():
    """every configuration error is WN_E_ARG with a text, on a machine without a device too; a validation-only handle (max_rows = 0) needs no device; a real
    one gets as far as the device (WN_E_HIP without one)"""
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    h = ctypes.c_void_p()
    assert lib.wn_stats_create(None, ctypes.byref(h)) == WN_E_ARG
    assert lib.wn_stats_create(ctypes.byref(_ext.stats_config()), None) == WN_E_ARG
    for kw in (dict(abi_version=5), dict(max_rows=-1), dict(max_rows=65536), dict(max_time=-1), dict(max_rows=2, max_time=0), dict(max_tensors=-1), dict(max_tensors=65536)):
        assert _create(**kw) == WN_E_ARG, kw
        assert (lib.wn_stats_last_error(None) or b'').startswith(b'wn_stats_create: '), kw
    for kw in (dict(), dict(max_time=0), dict(max_tensors=0)):
        assert _create(**kw) == 0, kw                                                          # max_rows = 0: no device is touched
    assert _create(max_rows=2) == (0 if torch.cuda.is_available() else WN_E_HIP)
    lib.wn_stats_destroy(None)


def test_every_validation_code_of_a_call_through_a_validation_only_handle():
    """max_rows = 0: every run is refused -- argument errors as WN_E_ARG first, then WN_E_SHAPE -- and nothing touches a device"""
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    cfg = _ext.stats_config(0, 8, 3)
    h = ctypes.c_void_p()
    assert lib.wn_stats_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    hist = lib.wn_stats_histogram
    assert hist(None, p, 8, None, 1, 8, p, p, None) == WN_E_ARG
    assert hist(h, None, 8, None, 1, 8, p, p, None) == WN_E_ARG
    assert hist(h, p, 8, None, 1, 8, None, p, None) == WN_E_ARG
    assert hist(h, p, 8, None, 1, 8, p, None, None) == WN_E_ARG
    assert hist(h, p, 8, None, 0, 8, p, p, None) == WN_E_ARG
    assert b'B (0)' in lib.wn_stats_last_error(h)
    assert hist(h, p, 8, None, 1, 0, p, p, None) == WN_E_ARG
    assert hist(h, p, 8, None, 1, 8, p, p, None) == WN_E_SHAPE
    assert b'max_rows = 0' in lib.wn_stats_last_error(h)
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    st = lib.wn_stats_set_tensors
    assert lib.wn_stats_tensors(h, p, p, None) == WN_E_STATE                       # no table yet
    assert st(None, i64(0), i64(4), 1) == WN_E_ARG
    assert st(h, None, i64(4), 1) == WN_E_ARG and st(h, i64(0), None, 1) == WN_E_ARG
    assert st(h, i64(0), i64(4), 0) == WN_E_ARG
    assert st(h, i64(0, 4), i64(4, 0), 2) == WN_E_ARG and b'counts[1]' in lib.wn_stats_last_error(h)
    assert st(h, i64(0, -4), i64(4, 4), 2) == WN_E_ARG
    assert st(h, i64(8, 0), i64(4, 9), 2) == WN_E_ARG and b'overlap' in lib.wn_stats_last_error(h)
    assert st(h, i64(0, 4, 8, 12), i64(4, 4, 4, 4), 4) == WN_E_SHAPE and b'max_tensors = 3' in lib.wn_stats_last_error(h)
    assert st(h, i64(8, 0), i64(4, 8), 2) == 0                                       # unsorted and touching is fine
    assert lib.wn_stats_tensors(h, None, p, None) == WN_E_ARG and lib.wn_stats_tensors(h, p, None, None) == WN_E_ARG
    assert lib.wn_stats_tensors(h, p, p, None) == WN_E_SHAPE and b'validation-only' in lib.wn_stats_last_error(h)
    lib.wn_stats_destroy(h)
    assert lib.wn_stats_hist_limits(None, 0) == 1551 and lib.wn_stats_hist_limits(None, 4) == WN_E_ARG and lib.wn_stats_hist_limits(p, -1) == WN_E_ARG
    # the hooks validate the same calls (no size limits of a handle)
    TS = _ext.TrainStats
    with pytest.raises(_ext.WnError) as ei:
        TS.tensor_stats_host(np.zeros(8, np.float32), [(0, 5), (4, 4)])
    assert ei.value.code == WN_E_ARG
    with pytest.raises(_ext.WnError) as ei:
        TS.tensor_stats_host(np.zeros(8, np.float32), [])
    assert ei.value.code == WN_E_ARG
    with pytest.raises(_ext.WnError) as ei:
        TS.histogram_host(np.zeros((0, 4), np.float32))
    assert ei.value.code == WN_E_ARG
    x = np.zeros((1, 4), np.float32)
    vp = ctypes.c_void_p
    assert lib.wn_test_stats_hist_host(x.ctypes.data_as(vp), 3, None, 1, 4, p, p) == WN_E_SHAPE


def test_the_table_is_the_loop_bit_for_bit():
    from wavenet_vocoder import _ext
    lim = _ext.hist_limits()
    assert lim.dtype == np.float64 and lim.shape == (1551,) and lim.tobytes() == SU.LIMITS.tobytes()
    assert np.all(np.diff(lim) > 0) and lim[775] == 0.0 and lim[776] == 1e-12 and lim[0] == -lim[-1] == -np.finfo(np.float64).max
    part = np.zeros(3)
    assert _ext.load_library().wn_stats_hist_limits(part.ctypes.data_as(ctypes.c_void_p), 3) == 1551 and part.tobytes() == lim[:3].tobytes()
    with np.errstate(over='ignore'):
        assert int(np.sum(lim.astype(np.float32).astype(np.float64) == lim)) == 1          # only 0.0 is a float32 value: a float32 table misplaces neighbours


def test_named_edge_values_land_where_the_issue_says():
    from wavenet_vocoder import _ext
    fm = np.finfo(np.float32).max
    h = _ext.TrainStats.histogram_host(np.array([[0.0, 1e-12, -fm, -0.0, fm, np.nan, np.inf, -np.inf]], np.float32))
    assert h['bucket'][776] == 3 and h['bucket'][1] == 1 and h['bucket'][1550] == 1 and h['bucket'].sum() == h['num'] == 5
    assert (h['n_nan'], h['n_pos_inf'], h['n_neg_inf']) == (1, 1, 1) and h['min'] == -float(fm) and h['max'] == float(fm)
    e = _ext.TrainStats.histogram_host(np.array([[np.nan, np.inf]], np.float32))
    assert e['num'] == 0 and e['min'] == 0.0 and e['max'] == 0.0 and e['sum'] == 0.0 and e['bucket'].sum() == 0


def _edge_input():
    e = SU.edge_values()
    return np.random.RandomState(5).permutation(e).reshape(1, -1).astype(np.float32)


@pytest.mark.parametrize('name', ['edges', 'audio', 'log_scales'])
@pytest.mark.parametrize('B,T,pitch', SU.SHAPES)
def test_hook_against_numpy(B, T, pitch, name):
    """ragged rows (one of length 0) at a pitch, the gap and the tails poisoned: the exact parts equal numpy, the sums inside gamma * sum |terms|"""
    x = SU.value_sets(B, T)[name]
    ln = SU.ragged_lengths(B, T)
    got = _raw_hist(SU.with_pitch(x, pitch, ln), pitch, ln, B, T)
    SU.check_hist(got, SU.reference_hist(x, ln), 'hook %s %s' % ((B, T, pitch), name))
    assert got['num'] + got['n_nan'] + got['n_pos_inf'] + got['n_neg_inf'] == int(ln.sum())


def test_hook_on_every_edge_value_at_once():
    """all neighbours of all limits, +-0, the denormals, +-FLT_MAX, NaN and +-inf in one row, and in two segments of a longer one"""
    from wavenet_vocoder import _ext
    x = _edge_input()
    SU.check_hist(_ext.TrainStats.histogram_host(x), SU.reference_hist(x), 'hook all edges')
    x2 = np.concatenate([x, x[:, ::-1]], 1)
    assert x2.shape[1] > 2 * 4096
    SU.check_hist(_ext.TrainStats.histogram_host(x2), SU.reference_hist(x2), 'hook all edges twice')


def test_poison_and_layout_change_nothing():
    """poison beyond lengths and in the pitch gap, another pitch, and a channel view of [B, 2, T] against the same data laid out densely: bit for bit"""
    from wavenet_vocoder import _ext
    B, T = 3, 4500
    x = SU.value_sets(B, T)['audio']
    ln = SU.ragged_lengths(B, T)
    base = _raw_hist(SU.with_pitch(x, T, ln, poison=0.0), T, ln, B, T)
    for pitch, poison in ((T, np.nan), (T + 7, np.inf), (2 * T, 1e30)):
        assert SU.same_hist(base, _raw_hist(SU.with_pitch(x, pitch, ln, poison=poison), pitch, ln, B, T)), (pitch, poison)
    other = SU.value_sets(B, T, seed=1)['log_scales']
    both = np.stack([x, other], 1)
    assert SU.same_hist(_ext.TrainStats.histogram_host(both, ln, channel=0), base)
    assert SU.same_hist(_ext.TrainStats.histogram_host(both, ln, channel=1), _ext.TrainStats.histogram_host(other, ln))
    full = _ext.TrainStats.histogram_host(x)
    assert SU.same_hist(full, _ext.TrainStats.histogram_host(x, np.full(B, T, np.int32))) and full['num'] == B * T


@pytest.mark.parametrize('inside', [False, True])
def test_tensor_hook_against_numpy(inside):
    """tensors of 1 ... 24576 elements (one, two and six segments) with NaN-poisoned gaps, magnitudes 1e-20 ... 1e15; inside: non-finite values in three"""
    from wavenet_vocoder import _ext
    flat, table = SU.tensor_table(inside=inside)
    ref, bound = SU.reference_tensors(flat, table)
    got = _ext.TrainStats.tensor_stats_host(flat, table)
    SU.check_tensors(got, ref, bound, 'hook tensors')
    assert int(got[:, 2].sum()) == (3 if inside else 0)
    order = [4, 0, 8, 2, 6, 1, 3, 7, 5]                                              # a permuted table: each tensor's bits are its own
    perm = _ext.TrainStats.tensor_stats_host(flat, [table[i] for i in order])
    assert perm.tobytes() == got[order].tobytes()


def test_encode_collapses_empty_runs_and_decodes():
    from wavenet_vocoder import _ext
    TS, lim = _ext.TrainStats, SU.LIMITS
    h = TS.histogram_host(np.array([[0.5, 0.5, 0.9, -2.0, 3.0e30]], np.float32))
    e = TS.encode(h)
    nz = np.flatnonzero(h['bucket'])
    assert len(nz) == 4 and h['bucket'][nz].tolist() == [1, 2, 1, 1]
    # a zero entry with the limit just below every non-empty bucket (the end of the empty run), then the bucket; nothing behind the last bucket
    want_lim, want_cnt = [], []
    for i in nz:
        want_lim += [lim[i - 1], lim[i]]; want_cnt += [0, int(h['bucket'][i])]
    assert nz[-1] == 1550                                                              # 3e30 lies above the last limit below DBL_MAX: no empty run behind it
    assert e['bucket_limit'] == want_lim and e['bucket'] == want_cnt
    assert e['num'] == 5 and e['min'] == -2.0 and e['max'] == float(np.float32(3.0e30)) and e['n_nan'] == 0
    assert np.array_equal(TS.decode(json.loads(json.dumps(e))), h['bucket'])          # through a JSON row and back
    adj = dict(h, bucket=np.zeros(1551, np.int64)); adj['bucket'][[0, 1, 2, 1550]] = [1, 0, 2, 4]      # neighbours, and both ends non-empty
    ea = TS.encode(adj)
    assert ea['bucket_limit'] == [lim[0], lim[1], lim[2], lim[1549], lim[1550]] and ea['bucket'] == [1, 0, 2, 0, 4]
    assert np.array_equal(TS.decode(ea), adj['bucket'])
    empty = TS.encode(TS.histogram_host(np.array([[np.nan]], np.float32)))
    assert empty['bucket_limit'] == [lim[-1]] and empty['bucket'] == [0] and empty['n_nan'] == 1
    for name, x in SU.value_sets(3, 257).items():
        hh = TS.histogram_host(x)
        assert np.array_equal(TS.decode(TS.encode(hh)), hh['bucket']), name


@pytest.mark.parametrize('fault', SU.FAULTS)
def test_seeded_fault_in_the_reference_is_caught(fault):
    """each fault makes the numpy stand-in wrong the way a careless implementation would be; the comparison that passes above must fail, by name"""
    from wavenet_vocoder import _ext
    B, T = 2, 4700
    e = _edge_input()[0]
    x = np.stack([np.resize(e, T), SU.value_sets(1, T)['audio'][0]]).astype(np.float32)
    ln = np.array([T, T - 900], np.int32)
    got = _ext.TrainStats.histogram_host(SU.with_pitch(x, T, ln), ln)
    SU.check_hist(got, SU.reference_hist(x, ln), 'no fault')
    with pytest.raises(AssertionError) as ei:
        SU.check_hist(got, SU.reference_hist(x, ln, fault=fault), fault)
    what = {'side_left': 'bucket counts', 'float32_table': 'bucket counts', 'padding_counted': 'bucket counts', 'nonfinite_binned': 'bucket counts',
            'float32_squares': 'sum_squares'}[fault]
    assert what in str(ei.value), (fault, str(ei.value)[:200])


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/host/stats_main.cpp built with ASAN + UBSAN, run once as an ordinary child process"""
    exe = str(tmp_path_factory.mktemp('stats') / 'stats_main')
    r = subprocess.run(['hipcc', '-std=c++20', '-O1', '-g', '-Wall', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        '-I', os.path.join(ROOT, 'tacotron-2_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'stats_main.cpp'), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    return subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)


def test_host_functions_under_address_and_ub_sanitizers(host_program):
    """the table, the search, the histogram over the GPU test's shapes and the segment edges (4096, 4097, more than 64 segments) in heap blocks that end with
    the last row's last element, the tensor statistics in blocks of exactly the tensor; the program checks the bits across pitches itself"""
    r = host_program
    assert r.returncode == 0 and 'stats ok' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_every_validation_code_through_the_host_program(host_program):
    got = dict(l.split()[1:] for l in host_program.stdout.splitlines() if l.startswith('code '))
    got = {k: int(v) for k, v in got.items()}
    A, S = WN_E_ARG, WN_E_SHAPE
    want = dict(cfg_null=A, cfg_ok=0, cfg_abi=A, cfg_rows_neg=A, cfg_rows_over=A, cfg_rows_zero=0, cfg_time_neg=A, cfg_time_zero=A, cfg_time_zero_validation_only=0,
                cfg_tensors_neg=A, cfg_tensors_over=A, cfg_tensors_zero=0,
                hist_ok=0, hist_x_null=A, hist_bucket_null=A, hist_summary_null=A, hist_b_zero=A, hist_t_zero=A, hist_b_over=S, hist_t_over=S, hist_pitch=S,
                tensors_ok_unsorted=0, tensors_off_null=A, tensors_cnt_null=A, tensors_nt_zero=A, tensors_count_zero=A, tensors_offset_neg=A, tensors_overlap=A,
                tensors_nt_over=S)
    assert got == want


# ---- hparams and the training loop's plumbing
def test_hparams_key_is_off_by_default():
    import hparams as H
    hp = H._build()
    assert hp.mi355_train_stats is False
    hp.parse('mi355_train_stats=True')
    assert hp.mi355_train_stats is True


class _Stats(object):
    """stands in for _ext.TrainStats: records the calls; tensor t has sum of squares (t + 1)^2, so its norm is t + 1"""
    names = ['a/kernel', 'a/bias', 'b/kernel']

    def __init__(self):
        self.calls = []

    def tensor_stats(self, flat):
        self.calls.append(('tensor_stats', tuple(flat.shape)))
        return np.array([[1.0, 0.5, 0, 4], [4.0, 1.5, 2, 4], [9.0, 2.5, 0, 8]])

    def histogram(self, x, lengths=None, channel=None):
        self.calls.append(('histogram', tuple(x.shape), None if lengths is None else [int(v) for v in lengths], channel))
        from wavenet_vocoder import _ext
        return _ext.TrainStats.histogram_host(x.numpy(), None if lengths is None else lengths.numpy(), channel)

    def histogram_host(self, x, lengths=None, channel=None):
        self.calls.append(('histogram_host', tuple(x.shape)))
        from wavenet_vocoder import _ext
        return _ext.TrainStats.histogram_host(x, lengths, channel)

    def encode(self, hist):
        from wavenet_vocoder import _ext
        return _ext.TrainStats.encode(hist)


class _Model(object):
    """what wavenet_vocoder.train.train() touches of WaveNet, on CPU tensors"""
    def __init__(self, hp):
        self.device = torch.device('cpu'); self.global_step = 0; self.learning_rate = 1e-3; self.embedding_table = None
        self.stats, self.kept, self.made = _Stats(), [], 0

    def build(self, B, T):
        self.params = torch.zeros(16); self.grads = torch.zeros(16)
        return self

    def initialize(self, y, c, g, lengths, x=None, **kw):
        self.kept.append((self.global_step + 1, dict(kw)))
        self._y_hat_train = torch.stack([x[:, 0], x[:, 0] - 7.0], 1) if kw.get('keep_y_hat') else None
        self._x = x

    def add_loss(self, flags=None):
        self.reduced_flags = flags
        return self._x.mean().reshape(1)

    def add_optimizer(self, step):
        self.grads.fill_(0.25 * (step + 1)); self.global_step = step + 1
        return self.global_step

    def train_stats(self):
        self.made += 1
        return self.stats

    def train_outputs(self, y, step):
        assert self._y_hat_train is not None
        return self._y_hat_train[:, 0].contiguous(), y.reshape(y.shape[0], -1).float().contiguous()

    def state_dict(self):
        return {'params': self.params.clone(), 'global_step': self.global_step}


class _Feeder(object):
    def __init__(self, hp, B, T):
        self.i = 0; self.test_steps = 1

    def start_threads(self, session=None):
        pass

    def next_train_batch(self):
        self.i += 1
        x = torch.linspace(-0.9, 0.9, 16).reshape(2, 1, 8) * (0.5 + 0.1 * self.i)
        return x, x.reshape(2, 8, 1).clone(), torch.tensor([8, 5], dtype=torch.int32), torch.zeros(2, 4, 2), None


def _run_loop(tmp_path, monkeypatch, on, out_channels=2):
    import hparams as H
    from wavenet_vocoder import train as T
    box = []
    monkeypatch.setattr(T, 'create_model', lambda name, hp: (box.append(_Model(hp)) or box[-1]))
    monkeypatch.setattr(T, 'SyntheticFeeder', _Feeder)
    monkeypatch.setattr(T, 'save_log', lambda *a, **k: None)
    monkeypatch.setattr(T, 'eval_step', lambda *a, **k: 0.0)
    hp = H._build()
    hp.parse('mi355_synthetic_data=True,wavenet_batch_size=2,max_time_steps=8,hop_size=4,upsample_scales=[2,2],input_type=raw,out_channels=%d,wavenet_gradient_max_norm=1.5,mi355_train_stats=%s' % (out_channels, on))
    args = types.SimpleNamespace(base_dir=str(tmp_path), model='WaveNet', restore=False, wavenet_train_steps=4, checkpoint_interval=100, summary_interval=2,
                                 eval_interval=100, embedding_interval=100, eval_max_time=0)
    log_dir = os.path.join(str(tmp_path), 'logs_%s_%d' % (on, out_channels)); os.makedirs(log_dir)
    assert T.wavenet_train(args, log_dir, hp, 'no_such_map.txt') is not None
    ev = os.path.join(log_dir, 'wavenet_events')
    rows = [json.loads(l) for l in open(os.path.join(ev, 'scalars.jsonl'))]
    return box[0], ev, rows


OLD_KEYS = {'step', 'wavenet_loss', 'wavenet_learning_rate', 'wavenet_max_gradient_norm', 'audio_samples_per_sec'}


def test_training_loop_with_the_key_off_makes_no_stats_call_and_writes_no_new_file(tmp_path, monkeypatch):
    m, ev, rows = _run_loop(tmp_path, monkeypatch, False)
    assert m.made == 0 and m.stats.calls == [] and all(kw == {} for _, kw in m.kept) and len(m.kept) == 4
    assert sorted(os.listdir(ev)) == ['scalars.jsonl']
    assert [set(r) for r in rows] == [OLD_KEYS, OLD_KEYS] and [r['step'] for r in rows] == [2, 4]


def test_training_loop_with_the_key_on_writes_the_rows_and_keys(tmp_path, monkeypatch):
    from wavenet_vocoder import _ext
    m, ev, rows = _run_loop(tmp_path, monkeypatch, True)
    assert [(s, kw) for s, kw in m.kept] == [(1, {}), (2, {'keep_y_hat': True}), (3, {}), (4, {'keep_y_hat': True})]      # y_hat is asked for at summary steps only
    assert sorted(os.listdir(ev)) == ['gradient_norms.jsonl', 'histograms.jsonl', 'scalars.jsonl']
    new = {'wavenet_stats/max_gradient_norm', 'wavenet_stats/max_gradient_norm_tensor', 'wavenet_stats/global_gradient_norm', 'wavenet_stats/clipped_tensors',
           'wavenet_stats/nonfinite_gradients'}
    assert [set(r) for r in rows] == [OLD_KEYS | new] * 2
    r = rows[1]
    assert r['wavenet_stats/max_gradient_norm'] == 3.0 and r['wavenet_stats/max_gradient_norm_tensor'] == 'b/kernel'
    assert r['wavenet_stats/global_gradient_norm'] == pytest.approx(14.0 ** 0.5) and r['wavenet_stats/clipped_tensors'] == 2 and r['wavenet_stats/nonfinite_gradients'] == 2
    assert r['wavenet_max_gradient_norm'] == 1.0                                         # today's key, today's value: the largest |element| (0.25 * 4)
    g = [json.loads(l) for l in open(os.path.join(ev, 'gradient_norms.jsonl'))]
    assert [x['step'] for x in g] == [2, 4] and g[0]['names'] == _Stats.names and g[0]['norm'] == [1.0, 2.0, 3.0] and g[0]['max_abs'] == [0.5, 1.5, 2.5] and g[0]['nonfinite'] == [0, 2, 0]
    h = [json.loads(l) for l in open(os.path.join(ev, 'histograms.jsonl'))]
    tags = ['gradient_norm', 'wav_outputs 0', 'wav_targets 0', 'gaussian_means 0', 'gaussian_log_scales 0']
    assert [(x['step'], x['tag']) for x in h] == [(s, t) for s in (2, 4) for t in tags]
    by = {x['tag']: x for x in h if x['step'] == 4}
    assert by['gradient_norm']['num'] == 3 and by['gradient_norm']['min'] == 1.0 and by['gradient_norm']['max'] == 3.0
    for t in tags[1:]:
        assert by[t]['num'] == 13 and sum(by[t]['bucket']) == 13, t                        # lengths 8 + 5: the padding is not counted
        assert _ext.TrainStats.decode(by[t]).sum() == 13
    assert by['gaussian_log_scales 0']['max'] < -6.0 < by['gaussian_means 0']['min']      # channel 1 and channel 0 of the kept y_hat
    calls = [c for c in m.stats.calls if c[0] == 'histogram']
    assert [c[3] for c in calls] == [None, None, 0, 1] * 2 and all(c[2] == [8, 5] for c in calls)
    assert ('tensor_stats', (16,)) in m.stats.calls and ('histogram_host', (1, 3)) in m.stats.calls


def test_training_loop_other_heads_write_no_gaussian_rows_and_a_failure_is_logged(tmp_path, monkeypatch):
    m, ev, rows = _run_loop(tmp_path, monkeypatch, True, out_channels=30)
    h = [json.loads(l) for l in open(os.path.join(ev, 'histograms.jsonl'))]
    assert [x['tag'] for x in h if x['step'] == 2] == ['gradient_norm', 'wav_outputs 0', 'wav_targets 0']
    # a failing summary never kills the run: the scalars row keeps today's keys
    monkeypatch.setattr(_Stats, 'tensor_stats', lambda self, flat: (_ for _ in ()).throw(RuntimeError('injected')))
    (tmp_path / 'second').mkdir()
    m2, ev2, rows2 = _run_loop(tmp_path / 'second', monkeypatch, True, out_channels=30)
    assert [set(r) for r in rows2] == [OLD_KEYS, OLD_KEYS] and m2.global_step == 4
