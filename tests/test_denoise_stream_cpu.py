"""Streaming denoiser without a GPU: the ABI symbols and every validation code on a geometry-only handle; wn_denoise_stream_ready against a brute-force
statement of the emit rule; the host hook wn_test_denoise_stream_host streamed through every cutting against wn_test_denoise_host of the whole row, BIT FOR
BIT, and against float64 under the rule of tests/denoise_ref.py; nothing read beyond n[b] or written beyond n_out[b]; tests/host/denoise_stream_main.cpp under
ASAN + UBSAN as an ordinary program; the Python plumbing of SynthesisStream.push / SlotSession.push with stub handles; and five faults seeded into a numpy
statement of the state machine, each caught by name."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import denoise_stream_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
WN_E_ARG, WN_E_SHAPE, WN_E_UNSUPPORTED, WN_E_STATE = -1, -2, -4, -5
SYMBOLS = ['wn_denoise_stream_create', 'wn_denoise_stream_destroy', 'wn_denoise_stream_last_error', 'wn_denoise_stream_set_profile',
           'wn_denoise_stream_take_profile', 'wn_denoise_stream_ready', 'wn_denoise_stream_push', 'wn_test_denoise_stream_host']


def test_abi_symbols_are_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    hooks = text[text.index('#ifndef WN_NO_TEST_HOOKS'):]
    for s in SYMBOLS:
        assert re.search(r'\b%s\(' % s, text), s
        assert s in _ext.exported_symbols()
    assert 'wn_test_denoise_stream_host(' in hooks and 'wn_denoise_stream_push(' not in hooks
    assert re.search(r'#define WN_ABI_VERSION\s+4\b', text) and _ext.WN_ABI_VERSION == 4      # no existing struct changed: the version stays


def _create(n_fft, hop, rows=0, max_push=64, in_type=0, abi=None):
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    cfg = _ext.denoise_stream_config(n_fft, hop, rows, max_push, in_type)
    if abi is not None:
        cfg.abi_version = abi
    h = ctypes.c_void_p()
    return lib.wn_denoise_stream_create(ctypes.byref(cfg), ctypes.byref(h)), h, lib


def test_every_validation_code_on_a_geometry_only_handle():
    from wavenet_vocoder import _ext
    vp = ctypes.c_void_p
    for args, code in (((1023, 8), WN_E_SHAPE), ((6, 1), WN_E_SHAPE), ((64, 0), WN_E_SHAPE), ((64, 17), WN_E_SHAPE), ((100, 25), WN_E_UNSUPPORTED),
                       ((8192, 2048), WN_E_UNSUPPORTED), ((1024, 256), 0), ((2048, 512), 0), ((64, 16), 0)):
        rc, h, lib = _create(*args)
        assert rc == code, (args, rc)
        if rc == 0:
            lib.wn_denoise_stream_destroy(h)
        else:
            assert lib.wn_denoise_stream_last_error(None)
    assert _create(64, 16, abi=5)[0] == WN_E_ARG and _create(64, 16, rows=-1)[0] == WN_E_ARG and _create(64, 16, max_push=0)[0] == WN_E_ARG
    assert _create(64, 16, in_type=3)[0] == WN_E_ARG
    rc, _, lib = _create(1024, 256, rows=4096, max_push=1 << 20)      # the reserve limit, checked before any device is touched
    assert rc == WN_E_UNSUPPORTED and b'limit' in lib.wn_denoise_stream_last_error(None)
    assert lib.wn_denoise_stream_create(None, None) == WN_E_ARG
    rc, h, lib = _create(64, 16)
    assert rc == 0
    assert lib.wn_denoise_stream_ready(h, 100, 0) == 48 and lib.wn_denoise_stream_ready(h, 100, 1) == 100
    assert lib.wn_denoise_stream_ready(h, -1, 0) == WN_E_ARG and lib.wn_denoise_stream_ready(None, 1, 0) == WN_E_ARG
    x = np.zeros(8, np.float32)
    xp = x.ctypes.data_as(vp)
    one, neg, no = (ctypes.c_int32 * 1)(4), (ctypes.c_int32 * 1)(-1), (ctypes.c_int32 * 1)(-9)
    prof = np.ones(33, np.float32)
    push = lambda *a: lib.wn_denoise_stream_push(h, *a)
    assert push(xp, 8, one, None, None, 1, 1.0, xp, 8, no, None) == WN_E_STATE                      # before any profile
    assert b'profile' in lib.wn_denoise_stream_last_error(h)
    bad = prof.copy()
    for v in (-1.0, np.nan, np.inf):
        bad[5] = v
        assert lib.wn_denoise_stream_set_profile(h, bad.ctypes.data_as(vp), None) == WN_E_ARG
    assert lib.wn_denoise_stream_set_profile(h, None, None) == WN_E_ARG
    assert lib.wn_denoise_stream_take_profile(h, None, None) == WN_E_ARG
    # the profile of a wn_denoise: none yet (WN_E_STATE), another n_fft (WN_E_SHAPE), then taken
    src = _ext.SpectralDenoiser(64, 16, 0, 0)
    assert lib.wn_denoise_stream_take_profile(h, src.h, None) == WN_E_STATE
    other = _ext.SpectralDenoiser(96, 20, 0, 0)
    other.profile = np.ones(49, np.float32)
    assert lib.wn_denoise_stream_take_profile(h, other.h, None) == WN_E_SHAPE and b'n_fft' in lib.wn_denoise_stream_last_error(h)
    src.profile = prof
    assert lib.wn_denoise_stream_take_profile(h, src.h, None) == 0
    assert push(None, 8, one, None, None, 1, 1.0, xp, 8, no, None) == WN_E_ARG
    assert push(xp, 8, None, None, None, 1, 1.0, xp, 8, no, None) == WN_E_ARG
    assert push(xp, 8, one, None, None, 1, 1.0, None, 8, no, None) == WN_E_ARG
    assert push(xp, 8, one, None, None, 1, 1.0, xp, 8, None, None) == WN_E_ARG
    assert push(xp, 8, one, None, None, 0, 1.0, xp, 8, no, None) == WN_E_ARG
    assert push(xp, 8, neg, None, None, 1, 1.0, xp, 8, no, None) == WN_E_ARG and b'n[0]' in lib.wn_denoise_stream_last_error(h)
    assert push(xp, -1, one, None, None, 1, 1.0, xp, 8, no, None) == WN_E_ARG and b'in_pitch' in lib.wn_denoise_stream_last_error(h)
    for s in (-0.5, float('nan'), float('inf')):
        assert push(xp, 8, one, None, None, 1, s, xp, 8, no, None) == WN_E_ARG
    assert push(xp, 8, one, None, None, 1, 1.0, xp, 8, no, None) == WN_E_SHAPE and b'max_rows' in lib.wn_denoise_stream_last_error(h)      # a geometry-only handle refuses every B
    assert no[0] == -9                                                                              # a failed call writes no n_out
    assert lib.wn_denoise_stream_push(None, xp, 8, one, None, None, 1, 1.0, xp, 8, no, None) == WN_E_ARG
    lib.wn_denoise_stream_destroy(h)
    # the shapes and states of a push that need rows, through the host hook (no max_rows there)
    blk = np.zeros((1, 80), np.float32)

    def code(pushes, **kw):
        with pytest.raises(_ext.WnError) as e:
            _ext.denoise_stream_host(64, 16, pushes, prof, 1.0, **kw)
        return e.value.code, str(e.value)
    c, text = code([(blk, [65], None, None)], max_push=64)
    assert c == WN_E_SHAPE and 'max_push' in text
    c, text = code([(blk, [10], None, [1]), (blk, [10], None, None)])
    assert c == WN_E_STATE and 'restart' in text and 'push 1' in text                               # an ended row must be restarted
    assert len(_ext.denoise_stream_host(64, 16, [(blk, [10], None, [1]), (blk, [10], [1], None), (blk, [0], None, None)], prof, 1.0)) == 3
    lib = _ext.load_library()
    cfg = _ext.denoise_stream_config(64, 16, 0, 80)
    n, n_out, out = np.array([[80]], np.int32), np.zeros((1, 1), np.int32), np.zeros((1, 40), np.float32)
    hook = lambda ip, op: lib.wn_test_denoise_stream_host(ctypes.byref(cfg), prof.ctypes.data_as(vp), 1.0, blk.ctypes.data_as(vp), ip, n.ctypes.data_as(vp), None, None, 1, 1,
                                                          out.ctypes.data_as(vp), op, n_out.ctypes.data_as(vp))
    assert hook(79, 40) == WN_E_SHAPE and b'in_pitch' in lib.wn_denoise_stream_last_error(None)
    assert hook(80, 31) == WN_E_SHAPE and b'out_pitch' in lib.wn_denoise_stream_last_error(None)     # 80 given, not final: 4 x 16 - 32 = 32 go out
    assert hook(80, 32) == 0 and n_out[0, 0] == 32


@pytest.mark.parametrize('geo', [(64, 16), (96, 20), (1024, 256)])
def test_ready_against_a_brute_force_statement_of_the_rule(geo):
    from wavenet_vocoder import _ext
    n_fft, hop = geo
    rc, h, lib = _create(n_fft, hop)
    assert rc == 0
    for s in range(0, 4 * n_fft + 1):
        e = lib.wn_denoise_stream_ready(h, s, 0)
        assert e == S.ready_brute(n_fft, hop, s, False) == _ext.denoise_stream_ready(n_fft, hop, s), s
        assert lib.wn_denoise_stream_ready(h, s, 1) == S.ready_brute(n_fft, hop, s, True) == s
        if e > 0:
            assert s - n_fft < e <= s - n_fft + hop, s      # the lag stays below n_fft
        else:
            assert s < n_fft
    lib.wn_denoise_stream_destroy(h)


# ---- the host hook streamed == the host hook one-shot, bit for bit
_ONE_SHOT = {}


def one_shot(name, kind, strength):
    """wn_test_denoise_host of the whole rows, once per (geometry, signal, strength): the reference every cutting shares (never modified)"""
    from wavenet_vocoder import _ext
    key = (name, kind, strength)
    if key not in _ONE_SHOT:
        n_fft, hop = R.GEOMETRIES[name]
        lens = R.lengths_of(n_fft, hop)
        wav = R.batch(kind, lens, 300, n_fft)
        ref, _ = _ext.denoise_host(n_fft, hop, wav, lens, strength, profile=R.noise_profile(n_fft, hop))
        ref.setflags(write=False)
        _ONE_SHOT[key] = (wav, lens, ref)
    return _ONE_SHOT[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize('cut', S.CUTTINGS)
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('name', ['A', 'B'])
def test_host_hook_streamed_equals_one_shot_bit_for_bit(name, kind, cut):
    from wavenet_vocoder import _ext
    n_fft, hop = R.GEOMETRIES[name]
    prof = R.noise_profile(n_fft, hop)
    for strength in (0.0, 1.0, 4.0):
        wav, lens, ref = one_shot(name, kind, strength)
        sched = S.schedule(lens, cut, n_fft, hop)
        assert cut == 'all_final' or len({k for k, (n, fin) in enumerate(sched) for b in range(len(lens)) if fin[b]}) > 1      # rows of one batch end at different pushes
        res = _ext.denoise_stream_host(n_fft, hop, S.blocks(wav, sched), prof, strength)
        rows = S.gather(res, len(lens))
        for b, n in enumerate(lens):
            assert same_bits(rows[b], ref[b, :n]), (strength, b, n)
        for (out, n_out), (nn, fin) in zip(res, sched):      # input beyond n[b] is NaN and was not read (no NaN came out); output beyond n_out[b] kept its fill
            for b in range(len(lens)):
                assert np.all(np.isnan(out[b, n_out[b]:])) and not np.any(np.isnan(out[b, :n_out[b]]))


@pytest.mark.parametrize('name', ['A', 'B'])
def test_a_row_restarted_mid_utterance_runs_the_second_signal_alone(name):
    from wavenet_vocoder import _ext
    n_fft, hop = R.GEOMETRIES[name]
    prof = R.noise_profile(n_fft, hop)
    n1, n2, c = 5 * hop + 3, 40 * hop + 3, hop + 1
    first = R.signal('above', n1, 11, n_fft)
    second = np.stack([R.signal('tone', n2, 12, n_fft), R.signal('straddle', n2, 13, n_fft)])
    ref, _ = _ext.denoise_host(n_fft, hop, second, [n2, n2], 1.0, profile=prof)
    pushes, pos = [], 0
    for k in range(0, n1, c):      # row 0 starts another utterance and is cut off; row 1 waits
        blk = np.full((2, c), np.nan, np.float32)
        m = min(c, n1 - k)
        blk[0, :m] = first[k:k + m]
        pushes.append((blk, [m, 0], [int(k == 0), 0], None))
    cut_off = len(pushes)
    while pos < n2:
        m = min(c, n2 - pos)
        blk = np.full((2, c), np.nan, np.float32)
        blk[:, :m] = second[:, pos:pos + m]
        pushes.append((blk, [m, m], [int(pos == 0), int(pos == 0)], [int(pos + m == n2)] * 2))
        pos += m
    res = _ext.denoise_stream_host(n_fft, hop, pushes, prof, 1.0)
    rows = S.gather(res[cut_off:], 2)
    assert same_bits(rows[0], ref[0]) and same_bits(rows[1], ref[1])
    assert sum(int(m[0]) for _, m in res[:cut_off]) == _ext.denoise_stream_ready(n_fft, hop, n1)      # what the cut-off utterance had emitted: the rule's, no more


@pytest.mark.parametrize('name', ['A', 'B'])
def test_host_hook_streamed_against_float64(name):
    from wavenet_vocoder import _ext
    n_fft, hop = R.GEOMETRIES[name]
    prof = R.noise_profile(n_fft, hop)
    wav, lens, _ = one_shot(name, 'tone', 1.0)
    res = _ext.denoise_stream_host(n_fft, hop, S.blocks(wav, S.schedule(lens, 'ragged', n_fft, hop)), prof, 1.0)
    got = np.full(wav.shape, np.nan, np.float32)
    for b, row in enumerate(S.gather(res, len(lens))):
        got[b, :len(row)] = row
    assert R.check_rows(got, wav, lens, prof, 1.0, n_fft, hop)[0] <= 1.0


@pytest.mark.parametrize('in_type', [1, 2])
def test_host_hook_decodes_as_the_output_stage_does(in_type):
    from wavenet_vocoder import _ext
    n_fft, hop = R.GEOMETRIES['A']
    prof = R.noise_profile(n_fft, hop)
    rs = np.random.RandomState(3)
    n = 20 * hop + 5
    x = rs.randint(0, 256, (2, n)).astype(np.int32) if in_type == 2 else rs.uniform(-1, 1, (2, n)).astype(np.float32)
    dec = np.stack([_ext.post_host(x[b], in_type)[0] for b in range(2)])
    ref, _ = _ext.denoise_host(n_fft, hop, dec, [n, n], 1.0, profile=prof)
    res = _ext.denoise_stream_host(n_fft, hop, S.blocks(x, S.schedule([n, n], 'hop+1', n_fft, hop)), prof, 1.0, in_type=in_type)
    rows = S.gather(res, 2)
    assert same_bits(rows[0], ref[0]) and same_bits(rows[1], ref[1])


# ---- the stand-alone host program
@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/host/denoise_stream_main.cpp built with ASAN + UBSAN, run once as an ordinary child process"""
    exe = str(tmp_path_factory.mktemp('denoise_stream') / 'denoise_stream_main')
    r = subprocess.run(['hipcc', '-std=c++20', '-O1', '-g', '-Wall', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        '-I', os.path.join(ROOT, 'tacotron-2_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'denoise_stream_main.cpp'), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    return subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)


def test_host_state_machine_under_address_and_ub_sanitizers(host_program):
    r = host_program
    assert r.returncode == 0 and 'denoise stream ok' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_every_validation_code_through_the_host_program(host_program):
    got = {l.split()[1]: int(l.split()[2]) for l in host_program.stdout.splitlines() if l.startswith('code ')}
    want = {'cfg_null': WN_E_ARG, 'cfg_ok': 0, 'cfg_abi': WN_E_ARG, 'cfg_rows_neg': WN_E_ARG, 'cfg_rows_zero': 0, 'cfg_push_zero': WN_E_ARG, 'cfg_in_type': WN_E_ARG,
            'cfg_in_type_2': 0, 'cfg_fft_odd': WN_E_SHAPE, 'cfg_hop_over': WN_E_SHAPE, 'cfg_fft_not_32': WN_E_UNSUPPORTED, 'cfg_reserve': WN_E_UNSUPPORTED,
            'push_ok': 0, 'push_n_null': WN_E_ARG, 'push_out_null': WN_E_ARG, 'push_n_out_null': WN_E_ARG, 'push_in_null': WN_E_ARG, 'push_in_null_all_zero': 0,
            'push_b_zero': WN_E_ARG, 'push_in_pitch_negative': WN_E_ARG, 'push_out_pitch_negative': WN_E_ARG, 'push_n_negative': WN_E_ARG, 'push_strength_nan': WN_E_ARG,
            'push_no_profile': WN_E_STATE, 'push_b_over': WN_E_SHAPE, 'push_n_over_max_push': WN_E_SHAPE, 'push_in_pitch_short': WN_E_SHAPE,
            'push_out_pitch_short': WN_E_SHAPE, 'push_out_pitch_exact': 0, 'push_ended_row': WN_E_STATE, 'push_ended_row_final': WN_E_STATE,
            'push_ended_row_restarted': 0, 'push_ended_row_left_alone': 0, 'push_row_too_long': WN_E_SHAPE}
    assert got == want


# ---- Python plumbing with stub handles
class _StubEngine:
    hop = 4

    def __init__(self):
        self.slot = {}

    def stream_lookahead(self):
        return (0, 1)

    def stream_begin(self, B, seed=0, steps_per_graph=0):
        self.done = self.pushed = 0

    def stream_push(self, cc, out, raw, noise, ti, final=False):
        from wavenet_vocoder.models.wavenet import stream_schedule
        self.pushed += 0 if cc is None else int(cc.shape[-1])
        first, end = stream_schedule(self.done, self.pushed, 1, final)
        self.done = end
        out.fill_(1.0)
        return (end - first) * self.hop

    def slots_begin(self, B, steps_per_graph=0):
        self.B = B
    wide_slots_begin = slots_begin

    def slot_open(self, slot, seed=None, g=None):
        self.slot[slot] = [0, 0]

    def slot_temperature(self, slot, *pair):
        pass

    def slot_abandon(self, slot):
        del self.slot[slot]

    def slots_push(self, cc, frames, final, out, raw):
        from wavenet_vocoder.models.wavenet import stream_schedule
        n = [0] * self.B
        for b, st in list(self.slot.items()):
            st[1] += frames[b]
            first, end = stream_schedule(st[0], st[1], 1, final[b])
            st[0] = end
            n[b] = (end - first) * self.hop
            if final[b]:
                del self.slot[b]
        return n


class _StubModel:
    device, scalar_input = 'cpu', True

    def __init__(self, extra=''):
        import hparams as H
        self._hparams = H._build().parse('mi355_output_denoise=0.75' + extra)
        self.engine = _StubEngine()

    def _ensure_packed(self):
        pass

    def global_conditioning_enabled(self):
        return False


class _StubDenoise:
    """counts like a DenoiseStream of (n_fft, hop) = (32, 8) and logs every push"""
    n_fft, hop = 32, 8

    def __init__(self, rows):
        self.S, self.E, self.log = [0] * rows, [0] * rows, []

    def push(self, samples, n=None, restart=None, final=None, strength=0.0):
        import torch
        from wavenet_vocoder import _ext
        B = samples.shape[0]
        restart = [1] * B if restart is True else [0] * B if restart is None else list(restart)
        final = [0] * B if final is None else [int(bool(f)) for f in final]
        n_out = []
        for b in range(B):
            if restart[b]:
                self.S[b] = self.E[b] = 0
            self.S[b] += n[b]
            e = _ext.denoise_stream_ready(self.n_fft, self.hop, self.S[b], final[b]) if (n[b] or final[b]) else self.E[b]
            n_out.append(e - self.E[b])
            self.E[b] = e
        self.log.append((list(n), restart, final, float(strength), n_out))
        return torch.full((B, max(n) + self.n_fft), 2.0), n_out


class _StubPost:
    def __init__(self, in_type):
        self.in_type, self.log = in_type, []

    def push(self, samples, n=None, restart=None, pcm=True, float_out=False):
        self.log.append((list(n), restart if restart is None or restart is True else list(restart), float(samples[0, 0])))
        return samples * 3


def test_synthesis_stream_push_plumbing_with_stub_handles():
    import torch
    from wavenet_vocoder.models.wavenet import SynthesisStream
    m = _StubModel()
    cin = m._hparams.cin_channels
    st = SynthesisStream(m, 2)
    ds, post = _StubDenoise(2), _StubPost(0)
    lens, S_, E_ = [], 0, 0
    for k, (frames, final) in enumerate([(3, False), (5, False), (0, False), (4, True)]):
        out, chunk = st.push(torch.zeros(2, cin, frames), final=final, post=post, post_output='float', denoise=ds)
        n = out.shape[1]
        S_ += n
        from wavenet_vocoder import _ext
        e = _ext.denoise_stream_ready(32, 8, S_, final)
        assert chunk.shape == (2, e - E_) and (chunk.numel() == 0 or float(chunk[0, 0]) == 6.0)      # the denoiser's output through the stage
        assert ds.log[-1][:4] == ([n, n], [1, 1] if k == 0 else [0, 0], [int(final)] * 2, 0.75)      # restarted at the first push; strength from the hparams
        assert post.log[-1][0] == [e - E_] * 2 and post.log[-1][2] == 2.0                             # the stage is given what the denoiser emitted
        E_ = e
        lens.append(n)
    assert E_ == S_ == 48 and lens == [8, 20, 0, 20]                                                      # the final push flushed the rest
    st2 = SynthesisStream(m, 2)
    out, chunk = st2.push(torch.zeros(2, cin, 12), denoise=_StubDenoise(2), denoise_strength=0.25)      # without post: the denoised float chunk
    assert chunk.shape == (2, 16) and float(chunk[0, 0]) == 2.0 and out.shape == (2, 44)      # 44 samples: 4 x 8 - 16 go out
    with pytest.raises(ValueError, match="in_type='raw'"):
        SynthesisStream(m, 2).push(torch.zeros(2, cin, 3), post=_StubPost(2), denoise=_StubDenoise(2))
    plain = SynthesisStream(m, 2).push(torch.zeros(2, cin, 3), post=_StubPost(2))                      # without denoise any stage is taken, as before
    assert plain[1].shape == (2, 8)


@pytest.mark.parametrize('wide', [False, True])
def test_slot_session_push_plumbing_with_stub_handles(wide):
    import torch
    from wavenet_vocoder.models.wavenet import SlotSession
    m = _StubModel()
    cin = m._hparams.cin_channels
    ss = SlotSession(m, 3, wide=wide)
    ds, post = _StubDenoise(3), _StubPost(0)
    fr = lambda k: torch.zeros(cin, k)
    ss.open(0); ss.open(2)
    r = ss.push({0: fr(12), 2: fr(5)}, post=post, post_output='float', denoise=ds, denoise_strength=1.5)
    assert ds.log[-1] == ([44, 0, 16], [1, 0, 1], [0, 0, 0], 1.5, [16, 0, 0]) and post.log[-1][:2] == ([16, 0, 0], [1, 0, 1])
    assert r[0][0].shape == (44,) and r[0][1].shape == (16,) and r[2][1].shape == (0,)      # 44 samples: 4 frames complete, 4 x 8 - 16 go out
    ss.open(1)
    r = ss.push({0: (fr(1), True), 1: fr(6), 2: None}, post=post, post_output='float', denoise=ds, denoise_strength=1.5)
    assert ds.log[-1] == ([8, 20, 0], [0, 1, 0], [1, 0, 0], 1.5, [36, 0, 0]) and r[0][1].shape == (36,)      # slot 0 ends: 52 samples in all, the rest flushed
    ss.abandon(2)
    ss.open(0); ss.open(2)                                                                                  # slot 0 reopened after its end, slot 2 after being abandoned
    r = ss.push({0: fr(2), 2: (fr(3), True)}, post=post, post_output='float', denoise=ds, denoise_strength=1.5)
    assert ds.log[-1] == ([4, 0, 12], [1, 0, 1], [0, 0, 1], 1.5, [0, 0, 12]) and post.log[-1][:2] == ([0, 0, 12], [1, 0, 1])
    r = ss.push({0: fr(1), 1: fr(4)}, denoise=ds)                                                           # no post: float chunks; strength from the hparams
    assert ds.log[-1][1] == [0, 0, 0] and ds.log[-1][3] == 0.75 and r[1][1].shape == (8,) and float(r[1][1][0]) == 2.0
    with pytest.raises(ValueError, match="in_type='raw'"):
        ss.push({0: fr(1)}, post=_StubPost(1), denoise=ds)


def test_stream_denoiser_takes_geometry_and_type_from_the_hparams(monkeypatch):
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.wavenet import WaveNet
    made = []

    class Stub:
        def __init__(self, *a):
            made.append(a)

        def take_profile(self, src):
            made.append(('take', src))
    monkeypatch.setattr(_ext, 'DenoiseStream', Stub)
    m = WaveNet.__new__(WaveNet)
    m._hparams = _StubModel(',mi355_output_denoise_fft=2048,mi355_output_denoise_hop=512,input_type=mulaw-quantize')._hparams
    m.stream_denoiser(20, 2200)
    src = object()
    m.stream_denoiser(4, 100, source=src)
    assert made == [(2048, 512, 20, 2200, 'mulaw-quantize'), (2048, 512, 4, 100, 'mulaw-quantize'), ('take', src)]


# ---- five faults seeded into a numpy statement of the state machine
def _numpy_streamed(n_fft, hop, prof, fault):
    """two utterances through one row: the first is cut off after a few pushes by the restart of the second; returns (second signal, its streamed output)"""
    first, second = R.signal('above', 9 * hop + 1, 21, n_fft), R.signal('tone', 12 * hop + 3, 22, n_fft)
    ns = S.NumpyStream(n_fft, hop, prof, 1.0, fault=fault)
    for k in range(0, len(first), hop + 1):
        ns.push(first[k:k + hop + 1])
    ns.restart()
    out = [ns.push(second[k:k + hop + 1], final=k + hop + 1 >= len(second)) for k in range(0, len(second), hop + 1)]
    return second, np.concatenate(out)


@pytest.mark.parametrize('fault', (None,) + S.FAULTS)
def test_a_fault_seeded_into_the_state_machine_is_caught(fault):
    for name in ('A', 'B'):
        n_fft, hop = R.GEOMETRIES[name]
        prof = R.noise_profile(n_fft, hop)
        x, got = _numpy_streamed(n_fft, hop, prof, fault)
        ref = R.denoise(x, prof, 1.0, n_fft, hop)
        ok = got.shape == ref.shape and bool(np.all(np.abs(got - ref) <= 1e-12))      # float64 against float64: streaming changes nothing but the order of a few sums
        assert ok == (fault is None), (name, fault)
