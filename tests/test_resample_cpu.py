"""Sample-rate conversion without a GPU: the ABI symbols and every validation code on a geometry-only handle; num_out / ready against brute force; the float64
statement of tests/resample_ref.py against an independent scipy.signal.upfirdn construction and its two algebraic forms against each other; its frequency
response at the default design; the host hook wn_test_resample_host against float64 under the bound of a T-term fmaf chain and against a numpy float32
emulation of that chain BIT FOR BIT; zeros, identity and split invariance of the hook's pushes; tests/host/resample_main.cpp under ASAN + UBSAN as an ordinary
program; five faults seeded into the numpy stand-in, each caught by name; the Python plumbing of resample= with stub handles; and the input side: load_wav
still refuses a foreign rate, preprocessing with mi355_resample_input on and no GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import resample_ref as R
from hip_util import make_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
WN_E_ARG, WN_E_SHAPE, WN_E_UNSUPPORTED, WN_E_STATE = -1, -2, -4, -5
SYMBOLS = ['wn_resample_create', 'wn_resample_destroy', 'wn_resample_last_error', 'wn_resample_num_out', 'wn_resample_ready', 'wn_resample_taps', 'wn_resample_run',
           'wn_resample_push', 'wn_test_resample_host', 'wn_test_resample_table']
# (sr_in, sr_out, Z)
CASES = [(3, 2, 4), (2, 3, 4), (2, 1, 4), (1, 2, 4), (7, 5, 3), (5, 7, 3), (320, 147, 4), (147, 320, 4), (48000, 22050, 64), (22050, 8000, 64)]
RATE_PAIRS = [(48000, 22050), (22050, 48000), (22050, 8000), (16000, 22050)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_abi_symbols_are_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    hooks = text[text.index('#ifndef WN_NO_TEST_HOOKS'):]
    for s in SYMBOLS:
        assert re.search(r'\b%s\(' % s, text), s
        assert s in _ext.exported_symbols()
    assert 'wn_test_resample_host(' in hooks and 'wn_test_resample_table(' in hooks and 'wn_resample_push(' not in hooks and 'wn_resample_run(' not in hooks
    assert re.search(r'#define WN_ABI_VERSION\s+4\b', text) and _ext.WN_ABI_VERSION == 4      # no existing struct changed: the version stays


def _create(sr_in=48000, sr_out=22050, rows=0, max_in=0, zeros=64, beta=R.BETA, rolloff=R.ROLLOFF, abi=None):
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    cfg = _ext.resample_config(sr_in, sr_out, rows, max_in, zeros, beta, rolloff)
    if abi is not None:
        cfg.abi_version = abi
    h = ctypes.c_void_p()
    rc = lib.wn_resample_create(ctypes.byref(cfg), ctypes.byref(h))
    return rc, h, lib, (lib.wn_resample_last_error(None) or b'').decode() if rc else ''


def test_every_validation_code_on_a_geometry_only_handle():
    from wavenet_vocoder import _ext
    vp = ctypes.c_void_p
    for kw, code, field in ((dict(abi=5), WN_E_ARG, 'abi_version'), (dict(rows=-1), WN_E_ARG, 'max_rows'), (dict(max_in=-1), WN_E_ARG, 'max_in'),
                            (dict(sr_in=0), WN_E_ARG, 'sr_in'), (dict(sr_out=0), WN_E_ARG, 'sr_out'), (dict(sr_out=-8000), WN_E_ARG, 'sr_out'),
                            (dict(zeros=0), WN_E_ARG, 'zeros'), (dict(rolloff=0.0), WN_E_ARG, 'rolloff'), (dict(rolloff=1.01), WN_E_ARG, 'rolloff'),
                            (dict(rolloff=float('nan')), WN_E_ARG, 'rolloff'), (dict(beta=-0.5), WN_E_ARG, 'beta'), (dict(beta=float('inf')), WN_E_ARG, 'beta'),
                            (dict(beta=float('nan')), WN_E_ARG, 'beta'), (dict(beta=300.0), WN_E_UNSUPPORTED, 'limit'),
                            (dict(sr_in=44101, sr_out=44100), WN_E_UNSUPPORTED, 'limit of 4194304'), (dict(sr_in=1000000, sr_out=1, zeros=1), WN_E_UNSUPPORTED, 'limit')):
        rc, h, lib, text = _create(**kw)
        assert rc == code and field in text, (kw, rc, text)
    assert _ext.load_library().wn_resample_create(None, None) == WN_E_ARG
    for kw in (dict(), dict(rolloff=1.0, beta=0.0), dict(sr_in=22050, sr_out=8000), dict(sr_in=16000, sr_out=16000)):
        rc, h, lib, _ = _create(**kw)
        assert rc == 0, kw
        lib.wn_resample_destroy(h)
    rc, h, lib, _ = _create(22050, 8000)
    L, M, W = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    assert lib.wn_resample_taps(h, ctypes.byref(L), ctypes.byref(M), ctypes.byref(W)) == 0 and (L.value, M.value, W.value) == (160, 441, 177)
    assert L.value * 2 * W.value == 56640
    assert lib.wn_resample_taps(None, None, None, None) == WN_E_ARG and lib.wn_resample_taps(h, None, None, None) == 0
    assert lib.wn_resample_num_out(h, 441) == 160 and lib.wn_resample_num_out(h, 442) == 161 and lib.wn_resample_num_out(h, 0) == 0
    assert lib.wn_resample_num_out(h, -1) == WN_E_ARG and lib.wn_resample_num_out(None, 1) == WN_E_ARG and lib.wn_resample_num_out(h, 1 << 31) == WN_E_ARG
    assert lib.wn_resample_ready(h, 177, 0) == 0 and lib.wn_resample_ready(h, 178, 0) == 1 and lib.wn_resample_ready(h, 178, 1) == 65
    assert lib.wn_resample_ready(h, -1, 0) == WN_E_ARG and lib.wn_resample_ready(None, 1, 0) == WN_E_ARG
    x = np.zeros(8, np.float32)
    xp = x.ctypes.data_as(vp)
    one, neg, no = (ctypes.c_int32 * 1)(4), (ctypes.c_int32 * 1)(-1), (ctypes.c_int32 * 1)(-9)
    err = lambda: lib.wn_resample_last_error(h)
    run = lambda *a: lib.wn_resample_run(h, *a)
    assert run(None, 8, one, 1, xp, 8, None) == WN_E_SHAPE          # (a geometry-only handle refuses every B before it looks at a row)
    assert run(xp, 8, None, 1, xp, 8, None) == WN_E_ARG and run(xp, 8, one, 1, None, 8, None) == WN_E_ARG and run(xp, 8, one, 0, xp, 8, None) == WN_E_ARG
    assert run(xp, 8, one, 1, xp, 8, None) == WN_E_SHAPE and b'max_rows' in err()      # (negative lengths and pitches: the stand-alone host program, and the hook below)
    assert lib.wn_resample_run(None, xp, 8, one, 1, xp, 8, None) == WN_E_ARG
    push = lambda *a: lib.wn_resample_push(h, *a)
    assert push(xp, 8, None, None, None, 1, xp, 8, no, None) == WN_E_ARG and push(xp, 8, one, None, None, 1, None, 8, no, None) == WN_E_ARG
    assert push(xp, 8, one, None, None, 1, xp, 8, None, None) == WN_E_ARG and push(xp, 8, one, None, None, 0, xp, 8, no, None) == WN_E_ARG
    assert push(xp, 8, one, None, None, 1, xp, 8, no, None) == WN_E_SHAPE and b'max_rows' in err()
    assert no[0] == -9                                                # a failed call writes no n_out
    assert lib.wn_resample_push(None, xp, 8, one, None, None, 1, xp, 8, no, None) == WN_E_ARG
    lib.wn_resample_destroy(h)
    # the shapes and states that need rows, through the host hook (no max_rows there)
    blk = np.zeros((1, 80), np.float32)

    def code(pushes, **kw):
        with pytest.raises(_ext.WnError) as e:
            _ext.resample_host(pushes, 3, 2, 4, **kw)
        return e.value.code, str(e.value)
    c, text = code([(blk, [65], None, None)], max_in=64)
    assert c == WN_E_SHAPE and 'max_in' in text
    c, text = code([(blk, [-1], None, None)])
    assert c == WN_E_ARG and 'n[0]' in text
    c, text = code([(blk, [10], None, [1]), (blk, [10], None, None)])
    assert c == WN_E_STATE and 'restart' in text and 'push 1' in text      # an ended row must be restarted
    assert len(_ext.resample_host([(blk, [10], None, [1]), (blk, [10], [1], None), (blk, [0], None, None)], 3, 2, 4)) == 3
    cfg = _ext.resample_config(3, 2, 0, 0, 4)
    n, n_out, out = np.array([[80]], np.int32), np.zeros((1, 1), np.int32), np.zeros((1, 60), np.float32)
    lib = _ext.load_library()
    hook = lambda ip, op: lib.wn_test_resample_host(ctypes.byref(cfg), blk.ctypes.data_as(vp), ip, n.ctypes.data_as(vp), None, None, 1, 1, out.ctypes.data_as(vp), op,
                                                    n_out.ctypes.data_as(vp))
    assert hook(79, 60) == WN_E_SHAPE and b'in_pitch' in lib.wn_resample_last_error(None)
    assert hook(-1, 60) == WN_E_ARG and b'in_pitch' in lib.wn_resample_last_error(None) and hook(80, -1) == WN_E_ARG and b'out_pitch' in lib.wn_resample_last_error(None)
    assert hook(80, 49) == WN_E_SHAPE and b'out_pitch' in lib.wn_resample_last_error(None)      # 80 given, not final, W = 6: ceil(74 x 2 / 3) = 50 go out
    assert hook(80, 50) == 0 and n_out[0, 0] == 50
    assert lib.wn_test_resample_table(ctypes.byref(cfg), out.ctypes.data_as(vp), 23) == WN_E_ARG      # L x T = 2 x 12


@pytest.mark.parametrize('sr_in,sr_out,Z', [(3, 2, 4), (2, 3, 4), (1, 2, 4), (7, 5, 3), (48000, 22050, 64), (22050, 8000, 64)])
def test_num_out_and_ready_against_brute_force(sr_in, sr_out, Z):
    from wavenet_vocoder import _ext
    L, M, W, T = R.plan(sr_in, sr_out, Z)
    rs = _ext.Resampler(sr_in, sr_out, 0, 0, zeros=Z)
    assert (rs.L, rs.M, rs.W) == (L, M, W)
    for S in range(3 * W + 6):
        n_out = 0
        while n_out * M < S * L:                    # the smallest n_out with n_out M >= S L
            n_out += 1
        e = 0
        while e * M // L + W <= S - 1:              # output e is ready once its last tap k0 + W lies below S
            e += 1
        assert rs.num_out(S) == n_out == R.num_out(S, L, M) and rs.ready(S, True) == n_out
        assert rs.ready(S) == e == R.ready(S, L, M, W), S
        assert S - (e * M // L) <= 2 * W if e else True
    rs.close()


@pytest.mark.parametrize('sr_in,sr_out,Z', CASES)
def test_reference_against_the_upfirdn_construction(sr_in, sr_out, Z):
    L, M, W, T = R.plan(sr_in, sr_out, Z)
    x = np.random.default_rng(5).standard_normal(3 * W + 40)
    y, bs = R.polyphase(x, sr_in, sr_out, Z, return_bound_sum=True)
    u = R.upfirdn_reference(x, sr_in, sr_out, Z)
    assert u.shape == y.shape
    bound = 2 * (T + 2) * 2.0 ** -53 * bs
    print('%d -> %d: worst difference %.2e' % (sr_in, sr_out, np.abs(u - y).max()))
    assert np.all(np.abs(u - y) <= bound)


@pytest.mark.parametrize('sr_in,sr_out,Z', CASES[:8])
def test_the_two_algebraic_forms_agree(sr_in, sr_out, Z):
    L, M, W, T = R.plan(sr_in, sr_out, Z)
    x = np.random.default_rng(6).standard_normal(2 * W + 23)
    y, bs = R.polyphase(x, sr_in, sr_out, Z, return_bound_sum=True)
    d = R.direct(x, sr_in, sr_out, Z)
    assert d.shape == y.shape and np.all(np.abs(d - y) <= 2 * (len(x) + 2) * 2.0 ** -53 * np.maximum(bs, np.abs(x).sum() * 1e-3))


def _interior(n, L, M, W):
    m = np.arange(R.num_out(n, L, M))
    k0 = m * M // L
    return m[(k0 - W + 1 >= 0) & (k0 + W <= n - 1)]


@pytest.mark.parametrize('sr_in,sr_out', RATE_PAIRS)
def test_frequency_response_at_the_defaults(sr_in, sr_out):
    L, M, W, T = R.plan(sr_in, sr_out)
    low = min(sr_in, sr_out)
    n = 2 * W + int(900 * M / L)
    k = np.arange(n)
    C = R.table(sr_in, sr_out)
    m = _interior(n, L, M, W)
    assert len(m) >= 800
    worst = 0.0
    for frac in (0.05, 0.25, 0.40, 0.43):                          # the passband: a tone comes out as the same tone
        for phase in (0.0, 0.7, 2.1):
            f = frac * low
            y = R.polyphase(np.sin(2 * np.pi * f * k / sr_in + phase), sr_in, sr_out, m=m, C=C)
            worst = max(worst, float(np.abs(y - np.sin(2 * np.pi * f * m / sr_out + phase)).max()))
    print('%d -> %d: worst passband error %.2e' % (sr_in, sr_out, worst))
    assert worst <= 2e-7
    f = R.ROLLOFF / 2 * low                                         # the -6 dB point
    y = R.polyphase(np.sin(2 * np.pi * f * k / sr_in + 0.3), sr_in, sr_out, m=m, C=C)
    full = np.zeros(int(m[-1]) + 1); full[m] = y
    amp = R.tone_fit(full, [f / sr_out, (sr_in - f) / sr_out] if sr_out > sr_in else [f / sr_out], int(m[0]), int(m[-1]) + 1)[0]
    print('%d -> %d: gain at rolloff / 2: %.3f dB' % (sr_in, sr_out, 20 * np.log10(amp)))
    assert abs(20 * np.log10(amp) + 6.02) <= 0.05
    for frac in (0.52, 0.55, 0.6, 0.8):                             # the stopband: what would alias (down) or what images (up) is 140 dB down
        if sr_out < sr_in:
            y = R.polyphase(np.sin(2 * np.pi * frac * low * k / sr_in + 0.3), sr_in, sr_out, m=m, C=C)
            gain = float(np.abs(y).max())
        else:
            f = (1.0 - frac) * low                                  # its first image lies at frac x sr_in
            y = R.polyphase(np.sin(2 * np.pi * f * k / sr_in + 0.3), sr_in, sr_out, m=m, C=C)
            full = np.zeros(int(m[-1]) + 1); full[m] = y
            gain = float(R.tone_fit(full, [f / sr_out, (sr_in - f) / sr_out], int(m[0]), int(m[-1]) + 1)[1])
        print('%d -> %d: gain at %.2f: %.1f dB' % (sr_in, sr_out, frac, 20 * np.log10(max(gain, 1e-300))))
        assert 20 * np.log10(max(gain, 1e-300)) <= -140.0


@pytest.mark.parametrize('sr_in,sr_out,Z', CASES)
def test_hook_against_float64_and_a_float32_emulation_bit_for_bit(sr_in, sr_out, Z):
    from wavenet_vocoder import _ext
    L, M, W, T = R.plan(sr_in, sr_out, Z)
    rng = np.random.default_rng(7)
    C32 = _ext.resample_table(sr_in, sr_out, Z)
    C = R.table(sr_in, sr_out, Z)
    assert C32.shape == C.shape and np.all(np.abs(C32 - C) <= 2.0 ** -24 * 1.0001 * np.abs(C) + 1e-45)      # rounded once
    worst = 0.0
    for n in (1, W, 2 * W + 1, 3 * W + 29):
        x = rng.standard_normal(n).astype(np.float32)
        y, = _ext.resample_rows_host([x], sr_in, sr_out, Z)
        ref, bs = R.polyphase(x, sr_in, sr_out, Z, return_bound_sum=True)
        bound = R.bound32(bs, T)
        assert y.shape == ref.shape and np.all(np.abs(y - ref) <= bound), n      # every output, no element excused
        worst = max(worst, float((np.abs(y - ref) / np.maximum(bound, 1e-300)).max()))
        assert np.array_equal(_bits(R.emulate32(x, C32, L, M, W)), _bits(y)), n
    print('%d -> %d, Z = %d: worst error / bound %.3f' % (sr_in, sr_out, Z, worst))


def test_zeros_give_zeros_and_equal_rates_are_the_identity():
    from wavenet_vocoder import _ext
    from datasets import audio
    for sr_in, sr_out in RATE_PAIRS:
        y = audio.resample_host(np.zeros(700, np.float32), sr_in, sr_out)
        assert y.shape[0] == -(-700 * sr_out // sr_in) and not np.any(_bits(y))      # exact +0.0
    x = np.random.default_rng(8).standard_normal(333).astype(np.float32)
    x[5] = -0.0
    assert np.array_equal(_bits(audio.resample_host(x, 22050, 22050)), _bits(x))
    rs = _ext.Resampler(8000, 8000, 0, 0)
    assert (rs.L, rs.M, rs.W) == (1, 1, 0) and rs.ready(7) == 7 and rs.num_out(7) == 7
    outs = _ext.resample_host([(x[None, :100], [100], None, None), (x[None, 100:], [233], None, [1])], 8000, 8000)
    assert [int(k[0]) for _, k in outs] == [100, 233] and np.array_equal(_bits(np.concatenate([o[0, :k[0]] for o, k in outs])), _bits(x))


def _cut(n, kind, W, seed):
    if kind == 'random':
        rng = np.random.default_rng(seed)
        c = []
        while sum(c) < n:
            c.append(int(rng.integers(0, 2 * W + 3)))
    elif kind == 0:
        c = [0, n]
    else:
        c = [kind] * (n // kind + 1)
    out, pos = [], 0
    for v in c:
        v = min(v, n - pos)
        out.append(v); pos += v
        if pos == n and kind != 0:
            break
    return out


@pytest.mark.parametrize('sr_in,sr_out,Z', [(3, 2, 4), (2, 3, 4), (7, 5, 3), (320, 147, 4), (22050, 8000, 64)])
def test_the_hooks_pushes_do_not_depend_on_the_cutting(sr_in, sr_out, Z):
    """two rows cut differently in one call -- row 0 by the cutting under test, row 1 at random -- against the rows pushed whole; then a mid-row restart"""
    from wavenet_vocoder import _ext
    L, M, W, T = R.plan(sr_in, sr_out, Z)
    lens = [3 * W + 11, 2 * W + 5]
    rng = np.random.default_rng(9)
    x = [rng.standard_normal(n).astype(np.float32) for n in lens]
    whole = _ext.resample_rows_host(x, sr_in, sr_out, Z)
    for kind in (1, W - 1, W, W + 1, 0, 'random'):
        cuts = [_cut(lens[0], kind, W, 1), _cut(lens[1], 'random', W, 2)]
        K = max(len(c) for c in cuts)
        pushes, pos = [], [0, 0]
        for k in range(K):
            nn = [c[k] if k < len(c) else 0 for c in cuts]
            blk = np.full((2, max(max(nn), 1)), np.nan, np.float32)
            for b in range(2):
                blk[b, :nn[b]] = x[b][pos[b]:pos[b] + nn[b]]
                pos[b] += nn[b]
            pushes.append((blk, nn, [int(k == 0)] * 2, [int(k == len(c) - 1) for c in cuts]))
        outs = _ext.resample_host(pushes, sr_in, sr_out, Z)
        S = [0, 0]
        for (o, n_out), (_, nn, _, fin) in zip(outs, pushes):
            for b in range(2):
                if nn[b] or fin[b]:
                    assert n_out[b] == R.ready(S[b] + nn[b], L, M, W, fin[b]) - R.ready(S[b], L, M, W), (kind, b)
                    S[b] += nn[b]
                else:
                    assert n_out[b] == 0
                assert np.all(np.isnan(o[b, n_out[b]:]))             # nothing is written beyond n_out[b]
        for b in range(2):
            got = np.concatenate([o[b, :k[b]] for o, k in outs])
            assert np.array_equal(_bits(got), _bits(whole[b])), (kind, b)
    # row 0 is cut off after W + 3 samples without a final push and restarted with another signal
    a, b2 = x[0][:W + 3], x[1]
    outs = _ext.resample_host([(a[None], [len(a)], [1], None), (b2[None], [len(b2)], [1], [1])], sr_in, sr_out, Z)
    assert outs[0][1][0] == R.ready(W + 3, L, M, W) and np.array_equal(_bits(outs[1][0][0, :outs[1][1][0]]), _bits(whole[1]))


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/host/resample_main.cpp built with ASAN + UBSAN, run once as an ordinary child process"""
    exe = str(tmp_path_factory.mktemp('resample') / 'resample_main')
    r = subprocess.run(['hipcc', '-std=c++20', '-O1', '-g', '-Wall', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        '-I', os.path.join(ROOT, 'tacotron-2_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'resample_main.cpp'), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    return subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)


def test_host_functions_under_address_and_ub_sanitizers(host_program):
    """the plan, the table, the row loop and the push state machine over rows of 0, 1, W, 2 W + 1 and 3 W + 7 samples in heap blocks of exactly the row's size,
    cut into pushes of 1, W - 1, W, W + 1, 0 and 2 W + 3; the program checks the bits against the whole row and the emit rule against brute force itself"""
    r = host_program
    assert r.returncode == 0 and 'resample ok' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_every_validation_code_of_a_call(host_program):
    """wn_resample_run / wn_resample_push run rs_check_run / rs_plan_push (csrc/wn_resample.h) before any device call; a handle with rows needs a device, so
    the functions are exercised in the stand-alone host program (B <= max_rows = 4, max_in = 8 there)"""
    got = {l.split()[1]: int(l.split()[2]) for l in host_program.stdout.splitlines() if l.startswith('code ')}
    A, S, U = WN_E_ARG, WN_E_SHAPE, WN_E_UNSUPPORTED
    want = dict(cfg_null=A, cfg_ok=0, cfg_abi=A, cfg_rows=A, cfg_max_in_neg=A, cfg_max_in_zero=A, cfg_sr_in=A, cfg_sr_out=A, cfg_zeros=A, cfg_rolloff_zero=A,
                cfg_rolloff_hi=A, cfg_rolloff_nan=A, cfg_rolloff_one=0, cfg_beta_neg=A, cfg_beta_inf=A, cfg_beta_nan=A, cfg_beta_zero=0, cfg_beta_big=U, cfg_table=U,
                cfg_span=U, cfg_identity=0,
                run_ok=0, run_in_null=A, run_n_null=A, run_out_null=A, run_b_zero=A, run_n_negative=A, run_pitch_negative=A, run_b_over=S, run_max_in=S,
                run_in_pitch=S, run_out_pitch=S,
                push_ok=0, push_in_null=A, push_n_null=A, push_out_null=A, push_n_out_null=A, push_b_zero=A, push_n_negative=A, push_b_over=S, push_max_in=S,
                push_in_pitch=S, push_out_pitch=S, push_ended=WN_E_STATE, push_ended_restarted=0, push_row_too_long=S)
    assert got == want


def _stream_against_whole(fault, sr_in=3, sr_out=2, Z=4):
    """the stand-in push loop with a seeded fault against the unfaulted definition: the names of the checks that notice"""
    L, M, W, T = R.plan(sr_in, sr_out, Z)
    x = np.random.default_rng(10).standard_normal(3 * W + 10)
    good = R.upfirdn_reference(x, sr_in, sr_out, Z)
    st = R.Stream(sr_in, sr_out, Z, fault=fault)
    parts, S, caught = [], 0, set()
    for c, fin in ((W + 2, False), (1, False), (W, False), (len(x) - 2 * W - 3, True)):
        y = st.push(x[S:S + c], restart=(S == 0), final=fin)
        e0, e1 = R.ready(S, L, M, W), R.ready(S + c, L, M, W, fin)
        if len(y) != e1 - e0:
            caught.add('emit_count')
        S += c
        parts.append(y)
    y = np.concatenate(parts)
    if len(y) != len(good):
        caught.add('length')
    k = min(len(y), len(good))
    if np.abs(y[:k] - good[:k]).max() > 1e-12:
        caught.add('values')
    if k and abs(np.abs(y[:k]).sum() / np.abs(good[:k]).sum() - 1.0) > 0.2:
        caught.add('gain')
    return caught


def test_five_seeded_faults_are_each_caught():
    assert _stream_against_whole(None) == set()
    assert 'values' in _stream_against_whole('phase_off_by_one')
    assert _stream_against_whole('one_tap_short') == {'values'}
    assert _stream_against_whole('s_dropped') >= {'values', 'gain'}
    assert _stream_against_whole('s_dropped', 2, 3) == set()          # (upsampling has s = 1: nothing to drop)
    assert _stream_against_whole('floor_n_out') >= {'length'}
    assert 'emit_count' in _stream_against_whole('early_emit')
    assert set(R.FAULTS) == {'phase_off_by_one', 'one_tap_short', 's_dropped', 'floor_n_out', 'early_emit'}


# ---- the Python plumbing of resample= with stub handles
class _Engine(object):
    hop = 4

    def __init__(self):
        self.calls = []

    def stream_lookahead(self):
        return (0, 0)

    def stream_push(self, cc, out, raw, noise, ti, final=False):
        return 0 if cc is None else int(cc.shape[-1]) * self.hop

    def slots_push(self, cc, frames, final, out, raw):
        return [f * self.hop for f in frames]

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
        return call


class _Stage(object):
    in_type = 0

    def __init__(self):
        self.pushes = []

    def push(self, samples, n=None, restart=None, pcm=True, float_out=False, clipped=False):
        self.pushes.append((list(n), restart if restart in (None, True) else list(restart), pcm, float_out))
        q, y = torch.full(samples.shape, 7, dtype=torch.int16), torch.full(samples.shape, 0.5)
        res = tuple(t for t, on in ((q, pcm), (y, float_out)) if on)
        return res[0] if len(res) == 1 else res


class _Resampler(object):
    """stands in for WaveNet.output_resampler's handle: two outputs for every three inputs, whatever is left at a final push"""

    def __init__(self):
        self.pushes, self.tail, self.S, self.E = [], _Stage(), {}, {}

    def push(self, samples, n=None, restart=None, final=None, out=None):
        B = samples.shape[0]
        rs = [1] * B if restart is True else [0] * B if restart is None else list(restart)
        fin = [0] * B if final is None else [int(f) for f in final]
        self.pushes.append((list(n), rs, fin, samples.dtype))
        n_out = []
        for b in range(B):
            if rs[b]:
                self.S[b] = self.E[b] = 0
            self.S[b] = self.S.get(b, 0) + n[b]
            e = -(-self.S[b] * 2 // 3) if fin[b] else self.S[b] * 2 // 3
            n_out.append(e - self.E.get(b, 0)); self.E[b] = e
        return torch.full((B, max(n_out) + 3), 0.25), n_out


def _model(**kw):
    from wavenet_vocoder.models.wavenet import WaveNet
    m = WaveNet(make_hp(**dict(dict(out_channels=30, cin_channels=16, num_mels=16, hop_size=4, upsample_scales=[2, 2]), **kw)))
    m.engine, m._dirty, m.device = _Engine(), False, torch.device('cpu')
    return m


def test_stream_push_with_resample_returns_the_chunk_at_the_output_rate():
    m = _model()
    st, post, rs = m.stream(2, seed=1), _Stage(), _Resampler()
    c = torch.zeros(2, 16, 3)
    out, chunk = st.push(c, post=post, resample=rs)                  # 12 samples -> 8
    assert out.shape == (2, 12) and chunk.shape == (2, 8) and chunk.dtype == torch.int16
    out, (q, y) = st.push(c[:, :, :1], post=post, post_output='both', resample=rs)      # 16 -> 10
    assert q.shape == (2, 2) and y.shape == (2, 2) and y.dtype == torch.float32
    out, y = st.push(c[:, :, :1], final=True, post=post, post_output='float', resample=rs)      # 20 -> ceil(40 / 3) = 14
    assert y.shape == (2, 4)
    assert [(p[0], p[1], p[3]) for p in post.pushes] == [([12, 12], True, True), ([4, 4], None, True), ([4, 4], None, True)]      # the stage in front always hands floats on
    assert [p[2] for p in post.pushes] == [False] * 3
    assert [(p[0], p[1], p[2]) for p in rs.pushes] == [([12, 12], [1, 1], [0, 0]), ([4, 4], [0, 0], [0, 0]), ([4, 4], [0, 0], [1, 1])]
    assert [(p[0], p[1]) for p in rs.tail.pushes] == [([8, 8], True), ([2, 2], None)]      # the int16 cast behind the conversion; none for 'float'
    with pytest.raises(ValueError, match='post='):
        m.stream(2, seed=1).push(c, resample=rs)                     # nothing in front of it that decodes
    assert isinstance(m.stream(2, seed=1).push(c), torch.Tensor)     # without it the call is what it was


def test_slot_session_forwards_restart_and_final_to_the_resampler():
    m = _model()
    sess, post, rs = m.slots(3), _Stage(), _Resampler()
    sess.open(0, seed=1); sess.open(2, seed=2)
    c = torch.zeros(16, 3)
    r = sess.push({0: c}, post=post, resample=rs)
    assert r[0][0].shape == (12,) and r[0][1].shape == (8,) and r[0][1].dtype == torch.int16
    r = sess.push({0: (c[:, :1], True), 2: c[:, :1]}, post=post, post_output='float', resample=rs)
    assert r[0][1].shape == (3,) and r[2][1].shape == (2,) and r[2][1].dtype == torch.float32      # slot 0 ends: ceil(32 / 3) - 8; slot 2: 4 -> 2
    sess.open(0, seed=3)
    r = sess.push({0: c, 2: (c, True)}, post=post, resample=rs)
    assert r[0][1].shape == (8,) and r[2][1].shape == (9,)           # slot 0 afresh; slot 2 ends: ceil(32 / 3) - 2
    assert [(p[0], p[1], p[2]) for p in rs.pushes] == [([12, 0, 0], [1, 0, 0], [0, 0, 0]), ([4, 0, 4], [0, 0, 1], [1, 0, 0]), ([12, 0, 12], [1, 0, 0], [0, 0, 1])]


def test_output_resampler_takes_the_rates_from_the_hparams():
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.wavenet import WaveNet
    seen = []

    class Probe(WaveNet):
        def output_stage(self, rows, **kw):
            seen.append((rows, kw))
            return None
    real = _ext.Resampler
    try:
        _ext.Resampler = lambda sr_in, sr_out, rows, max_in: real(sr_in, sr_out, 0, max_in)      # geometry only: no GPU here
        rs = Probe(make_hp(out_channels=30, cin_channels=16, num_mels=16, hop_size=4, upsample_scales=[2, 2])).output_resampler(3, 2200, 8000)
    finally:
        _ext.Resampler = real
    assert (rs.sr_in, rs.sr_out, rs.L, rs.M, rs.W, rs.max_in) == (22050, 8000, 160, 441, 177, 2200)
    assert seen == [(3, dict(in_type='raw', deemphasis=0.0))] and rs.tail is None
    rs.close()


# ---- the input side
def _write_tone(path, rate, seconds=0.4, f=440.0):
    from scipy.io import wavfile
    t = np.arange(int(rate * seconds)) / rate
    wavfile.write(path, rate, np.round(0.5 * 32767 * np.sin(2 * np.pi * f * t)).astype(np.int16))
    return len(t)


def test_load_wav_still_refuses_a_foreign_rate(tmp_path):
    import hparams as H
    from datasets import audio
    assert H._build().mi355_resample_input is False and H._build().mi355_output_sample_rate == 0
    p = str(tmp_path / 'a.wav')
    n = _write_tone(p, 48000)
    with pytest.raises(ValueError, match='resample the file first'):
        audio.load_wav(p, 22050)
    rate, x = audio.read_wav(p)
    assert rate == 48000 and x.dtype == np.float32 and len(x) == n and np.array_equal(x, audio.load_wav(p, 48000))
    from datasets import wavenet_preprocessor as P
    hp = H._build(); hp.parse('mi355_device_mel=False')
    os.makedirs(str(tmp_path / 'o'))
    with pytest.raises(ValueError, match='resample the file first'):      # the key is off: preprocessing fails exactly as before
        P.build_from_path(hp, str(tmp_path), str(tmp_path / 'o'), str(tmp_path / 'o'), n_jobs=1)


def test_preprocessing_accepts_an_off_rate_file_with_the_key_on(tmp_path):
    import hparams as H
    from datasets import audio, wavenet_preprocessor as P
    only, both = tmp_path / 'only', tmp_path / 'both'
    for d in (only, both, tmp_path / 'out_off', tmp_path / 'out_on'):
        os.makedirs(str(d))
    _write_tone(str(only / 'a.wav'), 22050)
    _write_tone(str(both / 'a.wav'), 22050)
    n48 = _write_tone(str(both / 'b.wav'), 48000)
    base = 'mi355_device_mel=False,trim_silence=False,input_type=raw'
    off = H._build(); off.parse(base)
    on = H._build(); on.parse(base + ',mi355_resample_input=True')
    rows_off = P.build_from_path(off, str(only), str(tmp_path / 'out_off'), str(tmp_path / 'out_off'), n_jobs=1)
    conv = P.resample_off_rate([str(both / 'a.wav'), str(both / 'b.wav')], on)
    assert list(conv) == [str(both / 'b.wav')]                       # the file at sample_rate never passes through the resampler
    n_res = len(conv[str(both / 'b.wav')])
    assert n_res == -(-n48 * 147 // 320)
    assert np.array_equal(_bits(conv[str(both / 'b.wav')]), _bits(audio.resample_host(audio.read_wav(str(both / 'b.wav'))[1], 48000, 22050)))
    rows_on = P.build_from_path(on, str(both), str(tmp_path / 'out_on'), str(tmp_path / 'out_on'), n_jobs=1)
    assert len(rows_off) == 1 and len(rows_on) == 2
    for col in (0, 1):                                               # the first file: byte-identical to the run with the key off
        assert open(rows_off[0][col], 'rb').read() == open(rows_on[0][col], 'rb').read()
    assert rows_on[0][4:] == rows_off[0][4:]
    hop = audio.get_hop_size(on)
    assert rows_on[1][5] == 1 + n_res // hop and rows_on[1][4] == rows_on[1][5] * hop      # lengths follow ceil(n 147 / 320), then the usual padding
    mel_a, mel_b = np.load(rows_on[0][1]), np.load(rows_on[1][1])
    assert mel_a.shape[1] == mel_b.shape[1] and int(mel_a.mean(0).argmax()) == int(mel_b.mean(0).argmax())      # the same tone: the same strongest band
