"""Alignment check, host side (no GPU): the C ABI names, the validation of a configuration and of a call, the float64 reference of tests/align_ref.py against
a brute-force recursion, the whole chain evaluated on the host through wn_test_align_host (the very functions the kernels inline, csrc/wn_align.h) against that
reference inside the bounds derived there, exact integer costs and constructed warps through wn_test_align_dp_host, the band, the invariance of a row's bits,
the host functions under ASAN + UBSAN in a stand-alone program, the Python surface (hparams, the float64 dtw helper, score_host, the Synthesizer's plumbing, the
TSV helpers, the command line in --host mode), and five faults seeded into a numpy stand-in, each caught by the check that is there for it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import align_ref as R
from hip_util import make_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
WN_E_ARG, WN_E_SHAPE, WN_E_UNSUPPORTED = -1, -2, -4
T = 64
SHAPES = [(1, 1), (1, 7), (7, 1), (T - 1, T), (T, T + 1), (T + 1, T - 1), (2 * T + 1, 40), (40, 2 * T + 1)]
FA, FB = [s[0] for s in SHAPES], [s[1] for s in SHAPES]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_symbols_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    declared = set(re.findall(r'\bint\s+(wn_\w+)\s*\(', text))
    lib = _ext.load_library()
    names = ('wn_align_create', 'wn_align_tile', 'wn_align_run', 'wn_test_align_host', 'wn_test_align_dp_host', 'wn_test_align_dp', 'wn_test_align_store_matrix', 'wn_test_align_copy')
    for name in names + ('wn_align_destroy', 'wn_align_last_error'):
        assert name in _ext.exported_symbols() and hasattr(lib, name), name
    for name in names:
        assert name in declared, name
    assert 'void wn_align_destroy(' in text and 'const char* wn_align_last_error(' in text
    assert '#define WN_ABI_VERSION 4' in text and _ext.WN_ABI_VERSION == 4
    hooks = text[text.index('#ifndef WN_NO_TEST_HOOKS'):]
    assert all(n + '(' in hooks for n in names[3:]) and 'wn_align_run(' not in hooks and 'wn_align_create(' not in hooks          # the hooks alone are fenced
    assert ctypes.sizeof(_ext.WnAlignConfig) == 32


def _create(**kw):
    from wavenet_vocoder import _ext
    cfg = _ext.align_config(80, 13, 1.0, 0, 0, 0, 0)          # validation-only: no device
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    lib = _ext.load_library()
    rc = lib.wn_align_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = (lib.wn_align_last_error(None) or b'').decode()
    if rc == 0:
        lib.wn_align_destroy(h)
    return rc, msg


def test_create_validates_before_any_device_call():
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    h = ctypes.c_void_p()
    assert lib.wn_align_create(None, ctypes.byref(h)) == WN_E_ARG and b'null argument' in lib.wn_align_last_error(None)
    assert lib.wn_align_create(ctypes.byref(_ext.align_config(80)), None) == WN_E_ARG
    nan, inf = float('nan'), float('inf')
    bad = [(dict(abi_version=5), 'abi_version'), (dict(num_mels=0), 'num_mels'), (dict(num_mels=129), 'num_mels'), (dict(n_cep=0), 'n_cep'), (dict(n_cep=80), 'n_cep'),
           (dict(unit_db=0.0), 'unit_db'), (dict(unit_db=-1.0), 'unit_db'), (dict(unit_db=nan), 'unit_db'), (dict(unit_db=inf), 'unit_db'), (dict(band=-1), 'band'),
           (dict(band=(1 << 20) + 1), 'band'), (dict(max_batch=-1), 'max_batch'), (dict(max_frames_a=-1), 'max_frames_a'), (dict(max_frames_b=-2), 'max_frames_b')]
    for kw, field in bad:
        rc, msg = _create(**kw)
        assert rc == WN_E_ARG and msg.startswith('wn_align_create: ') and field in msg, (kw, rc, msg)
    for kw in (dict(max_frames_a=4097), dict(max_frames_b=5000)):          # the reserve limit, stated in the header: 4096 frames a side ...
        rc, msg = _create(**kw)
        assert rc == WN_E_UNSUPPORTED and '4096' in msg, (kw, rc, msg)
    for kw in (dict(), dict(n_cep=79), dict(num_mels=2, n_cep=1), dict(band=1 << 20), dict(max_frames_a=4096, max_frames_b=4096)):
        assert _create(**kw)[0] == 0, kw
    lib.wn_align_destroy(None)
    assert lib.wn_align_tile(None) == WN_E_ARG


def test_every_validation_code_of_a_call_on_a_validation_only_handle():
    """argument errors as WN_E_ARG first, each with its message; then WN_E_SHAPE: a validation-only handle takes no row at all.  Nothing touches a device.  (The
    other shape codes: test_every_validation_code_through_the_host_program and the host hook below.)"""
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    cfg = _ext.align_config(80, 13, 1.0, 0, 0, 0, 0)
    h = ctypes.c_void_p()
    assert lib.wn_align_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    assert lib.wn_align_tile(h) == T
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    i2 = ctypes.c_int32 * 2
    f, zero = i2(5, 6), i2(5, 0)
    run, err = lib.wn_align_run, lambda: lib.wn_align_last_error(h)
    tail = (p, 20, p, 10, p, 10, p, None)
    assert run(None, p, 1, 10, p, 1, 10, f, f, 2, *tail) == WN_E_ARG
    for a, b, fa, fb, sm in ((None, p, f, f, p), (p, None, f, f, p), (p, p, None, f, p), (p, p, f, None, p), (p, p, f, f, None)):
        assert run(h, a, 1, 10, b, 1, 10, fa, fb, 2, p, 20, p, 10, p, 10, sm, None) == WN_E_ARG and b'null argument' in err()
    assert run(h, p, 1, 10, p, 1, 10, f, f, 0, *tail) == WN_E_ARG and b'B (0)' in err()
    assert run(h, p, 1, 10, p, 1, 10, zero, f, 2, *tail) == WN_E_ARG and b'frames_a[1] = 0' in err()
    assert run(h, p, 1, 10, p, 1, 10, f, zero, 2, *tail) == WN_E_ARG and b'frames_b[1] = 0' in err()
    assert run(h, p, 1, 10, p, 1, 10, f, f, 2, *tail) == WN_E_SHAPE and b'max_batch = 0' in err()
    assert lib.wn_test_align_store_matrix(h, 1) == WN_E_SHAPE and lib.wn_test_align_copy(h, 0, p, 4, None) == WN_E_SHAPE
    lib.wn_align_destroy(h)
    # the shape codes of the pitches, through the hook (whose capacity is the call's own)
    a, b = np.zeros((1, 4, 9), np.float32), np.zeros((1, 4, 9), np.float32)
    for kw, text in ((dict(frames_a=[10]), 'a_pitch'), (dict(frames_b=[10]), 'b_pitch'), (dict(path_pitch=13), 'path_pitch'), (dict(map_a_pitch=6), 'map_a_pitch'),
                     (dict(map_b_pitch=6), 'map_b_pitch')):
        args = dict(frames_a=[7], frames_b=[8], n_cep=3, b_channels_first=True)
        args.update(kw)
        with pytest.raises(_ext.WnError) as ei:
            _ext.align_host(a, b, args.pop('frames_a'), args.pop('frames_b'), **args)
        assert ei.value.code == WN_E_SHAPE and text in str(ei.value), kw
    with pytest.raises(_ext.WnError) as ei:
        _ext.align_dp_host(np.zeros((1, 3, 3), np.float32), [4], [2])
    assert ei.value.code == WN_E_SHAPE


def test_reference_against_a_brute_force_recursion():
    rng = np.random.RandomState(1)
    for Fa, Fb in ((1, 1), (1, 4), (5, 1), (2, 2), (4, 6), (6, 5), (7, 7)):
        for band in (0, 1, 2):
            cost = rng.rand(Fa, Fb)
            dm = R.recurrence(cost, band)
            assert abs(dm[-1, -1] - R.brute_force(cost, band)) <= 1e-12 * dm[-1, -1], (Fa, Fb, band)
            path = R.backtrace(dm, band)
            assert R.is_valid_path(path, Fa, Fb) and abs(R.path_cost(path, cost) - dm[-1, -1]) <= 1e-12 * dm[-1, -1]
            assert all(R.admissible(i, j, Fa, Fb, band) for i, j in path)


def _mels(M, seed=3):
    rng = np.random.RandomState(seed)
    a, b = np.full((len(SHAPES), M, 140), np.nan, np.float32), np.full((len(SHAPES), 133, M), np.nan, np.float32)
    for r, (Fa, Fb) in enumerate(SHAPES):
        x = np.cumsum(rng.randn(Fa, M), axis=0).astype(np.float32) * 0.3
        pos = np.clip(np.round(np.linspace(0, Fa - 1, Fb) + 2.0 * np.sin(np.arange(Fb) / 9.0)).astype(int), 0, Fa - 1)
        a[r, :, :Fa] = x.T
        b[r, :Fb] = x[pos] + 0.1 * rng.randn(Fb, M).astype(np.float32) + 0.7
    return a, b


def check_against_reference(h, a_rows, b_rows, unit, K, band, who):
    """the assertions of tests/test_hip_align.py on one evaluation `h` (a dict with the stages): every stage against float64 of the previous one"""
    for r, (x, y) in enumerate(zip(a_rows, b_rows)):
        Fa, Fb = len(x), len(y)
        for side, z, c in (('a', x, h['cep_a'][r, :Fa]), ('b', y, h['cep_b'][r, :Fb])):
            c64, bound = R.cepstra(z, unit, K)
            assert np.all(np.abs(c - c64) <= bound), (who, r, side, 'cepstra')
        k64, rel = R.cost_matrix(h['cep_a'][r, :Fa], h['cep_b'][r, :Fb])
        cost = h['cost'][r, :Fa, :Fb]
        assert np.all(np.abs(cost - k64) <= rel * k64), (who, r, 'cost')
        d64, d = R.recurrence(cost, band), h['dm'][r, :Fa, :Fb]
        assert np.array_equal(np.isinf(d), np.isinf(d64)) and not np.any(np.isnan(d)), (who, r, 'band cells')
        fin = np.isfinite(d64)
        assert np.all(np.abs(d[fin] - d64[fin]) <= R.recurrence_bound(d64)[fin]), (who, r, 'recurrence')
        path = R.backtrace(d, band)
        n = int(h['summary'][r, 2])
        assert n == len(path) and np.array_equal(h['path'][r, :, :n].T, path), (who, r, 'path')
        tc, lim = R.near_optimal(path, cost, d64[-1, -1])
        assert tc <= lim, (who, r, 'near-optimality')
        mab, mba = R.maps(path, Fa, Fb)
        assert np.array_equal(h['map_ab'][r, :Fa], mab) and np.array_equal(h['map_ba'][r, :Fb], mba), (who, r, 'maps')
        s64 = R.summary(path, cost, d[-1, -1])
        assert np.array_equal(h['summary'][r, :4], s64[:4].astype(np.float32)) and np.all(np.abs(h['summary'][r, 4:] - s64[4:]) <= 2.0 ** -23 * np.abs(s64[4:])), (who, r, 'summary')
        assert np.all(h['path'][r, :, n:] == -7) and np.all(h['map_ab'][r, Fa:] == -7) and np.all(h['map_ba'][r, Fb:] == -7), (who, r, 'sentinels')


@pytest.mark.parametrize('M,K,band', [(16, 13, 0), (16, 1, 1), (80, 13, 4), (80, 1, 0), (16, 13, 1)])
def test_host_hook_against_the_reference(M, K, band):
    from wavenet_vocoder import _ext
    a, b = _mels(M)
    h = _ext.align_host(a, b, FA, FB, n_cep=K, unit_db=2.5, band=band, b_channels_first=False, stages=True, path_pitch=300, map_a_pitch=150, map_b_pitch=151)
    check_against_reference(h, [a[r, :, :Fa].T for r, Fa in enumerate(FA)], [b[r, :Fb] for r, Fb in enumerate(FB)], 2.5, K, band, 'hook')


@pytest.mark.parametrize('band', [0, 1, 4])
def test_exact_integer_costs_pin_the_tie_order(band):
    """small non-negative integer costs, every sum below 2^24: Dm equals float64 in every cell and the path equals float64's, ties included"""
    from wavenet_vocoder import _ext
    rng = np.random.RandomState(7 + band)
    cost = rng.randint(0, 4, size=(len(SHAPES), 130, 131)).astype(np.float32)
    h = _ext.align_dp_host(cost, FA, FB, band=band)
    ties = 0
    for r, (Fa, Fb) in enumerate(SHAPES):
        d64 = R.recurrence(cost[r, :Fa, :Fb], band)
        assert np.array_equal(h['dm'][r, :Fa, :Fb].astype(np.float64), d64), r
        p64 = R.backtrace(d64, band)
        n = int(h['summary'][r, 2])
        assert n == len(p64) and np.array_equal(h['path'][r, :, :n].T, p64), r
        for i, j in p64[1:]:
            if i > 0 and j > 0:
                ties += len({d64[i - 1, j - 1], d64[i - 1, j], d64[i, j - 1]}) < 3
    assert ties > 50          # the cases do decide ties


def test_constructed_warps_are_recovered():
    """b is a with frame i repeated r_i in {1, 2, 3} times: the total is 0 and map_ba recovers the warp"""
    from wavenet_vocoder import _ext
    rng = np.random.RandomState(11)
    for Fa in (1, 5, T, T + 3):
        x = rng.randn(Fa, 16).astype(np.float32)
        rep = rng.randint(1, 4, size=Fa)
        src = np.repeat(np.arange(Fa), rep)
        h = _ext.align_host(x.T[None], x[src][None], [Fa], [len(src)], n_cep=13, b_channels_first=False)
        assert h['summary'][0, 3] == 0.0 and h['summary'][0, 4] == 0.0 and np.array_equal(h['map_ba'][0], src)
        assert np.array_equal(h['map_ab'][0], np.cumsum(rep) - 1) and h['summary'][0, 2] == len(src)          # every frame of b on the path once


def test_band_one_always_connects_the_corners():
    """every (Fa, Fb) in 1 ... 40 squared at band = 1, zero costs: the total is finite (0), the path is valid and no cell of it lies outside the band; the
    admissible cells are exactly those of the inequality (Dm is +inf elsewhere)"""
    from wavenet_vocoder import _ext
    fa, fb = [a for a in range(1, 41) for _ in range(40)], [b for _ in range(40) for b in range(1, 41)]
    h = _ext.align_dp_host(np.zeros((1600, 40, 40), np.float32), fa, fb, band=1)
    assert np.all(h['summary'][:, 3] == 0.0)
    for r, (Fa, Fb) in enumerate(zip(fa, fb)):
        n = int(h['summary'][r, 2])
        path = h['path'][r, :, :n].T
        assert R.is_valid_path(path, Fa, Fb) and np.all(np.abs(path[:, 0] * Fb - path[:, 1] * Fa) <= max(Fa, Fb)), (Fa, Fb)
        i, j = np.arange(Fa)[:, None], np.arange(Fb)[None, :]
        adm = np.abs(i * Fb - j * Fa) <= max(Fa, Fb)
        assert np.array_equal(np.isfinite(h['dm'][r, :Fa, :Fb]), adm), (Fa, Fb)


def test_inadmissible_cells_never_lie_on_the_path():
    """a cost matrix whose cheap cells all lie OUTSIDE the band: the path stays inside it and pays"""
    from wavenet_vocoder import _ext
    Fa, Fb = 50, 70
    i, j = np.arange(Fa)[:, None], np.arange(Fb)[None, :]
    for band in (1, 2):
        adm = np.abs(i * Fb - j * Fa) <= band * max(Fa, Fb)
        cost = np.where(adm, 5.0, 0.0).astype(np.float32)
        h = _ext.align_dp_host(cost[None], [Fa], [Fb], band=band)
        n = int(h['summary'][0, 2])
        path = h['path'][0, :, :n].T
        assert np.all(adm[path[:, 0], path[:, 1]]) and h['summary'][0, 3] == 5.0 * n
        free = _ext.align_dp_host(cost[None], [Fa], [Fb], band=0)
        assert free['summary'][0, 3] < 5.0 * n


def test_a_rows_bits_do_not_depend_on_layout_pitch_or_batch():
    from wavenet_vocoder import _ext
    M, K = 16, 13
    a, b = _mels(M)
    base = _ext.align_host(a, b, FA, FB, n_cep=K, band=4, b_channels_first=False, stages=True)
    order = [7, 3, 0, 5]
    a2, b2 = np.full((len(order), 170, M), np.nan, np.float32), np.full((len(order), M, 190), np.nan, np.float32)
    for q, r in enumerate(order):
        a2[q, :FA[r]] = a[r, :, :FA[r]].T
        b2[q, :, :FB[r]] = b[r, :FB[r]].T
    moved = _ext.align_host(a2, b2, [FA[r] for r in order], [FB[r] for r in order], n_cep=K, band=4, a_channels_first=False, b_channels_first=True, stages=True,
                            path_pitch=400, map_a_pitch=200, map_b_pitch=201)
    for q, r in enumerate(order):
        n = int(base['summary'][r, 2])
        assert np.array_equal(_bits(moved['summary'][q]), _bits(base['summary'][r])) and np.array_equal(moved['path'][q, :, :n], base['path'][r, :, :n])
        assert np.array_equal(_bits(moved['dm'][q, :FA[r], :FB[r]]), _bits(base['dm'][r, :FA[r], :FB[r]]))
        assert np.array_equal(moved['map_ab'][q, :FA[r]], base['map_ab'][r, :FA[r]]) and np.array_equal(moved['map_ba'][q, :FB[r]], base['map_ba'][r, :FB[r]])
        alone = _ext.align_host(a[r:r + 1], b[r:r + 1], [FA[r]], [FB[r]], n_cep=K, band=4, b_channels_first=False)
        assert np.array_equal(_bits(alone['summary'][0]), _bits(base['summary'][r]))


def test_non_finite_inputs_give_a_valid_path():
    from wavenet_vocoder import _ext
    a, b = _mels(16)
    r = 4
    a[r, :, 10:20] = np.nan; b[r, 30:33] = np.inf; a[r, 3, 40] = -np.inf
    h = _ext.align_host(a[r:r + 1], b[r:r + 1], [FA[r]], [FB[r]], n_cep=13, band=1, b_channels_first=False)
    n = int(h['summary'][0, 2])
    assert 1 <= n <= FA[r] + FB[r] - 1 and R.is_valid_path(h['path'][0, :, :n].T, FA[r], FB[r])
    nan_cost = np.full((1, 9, 11), np.nan, np.float32)
    h = _ext.align_dp_host(nan_cost, [9], [11])
    assert R.is_valid_path(h['path'][0, :, :int(h['summary'][0, 2])].T, 9, 11)


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/host/align_main.cpp built with ASAN + UBSAN, run once as an ordinary child process"""
    exe = str(tmp_path_factory.mktemp('align') / 'align_main')
    r = subprocess.run(['hipcc', '-std=c++20', '-O1', '-g', '-Wall', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        '-I', os.path.join(ROOT, 'tacotron-2_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'align_main.cpp'), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    return subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)


def test_host_functions_under_address_and_ub_sanitizers(host_program):
    """the whole chain over num_mels in {2, 16} x band in {0, 1, 3} x both layouts x eight shapes, rows in heap blocks of exactly their size, with and without
    the optional outputs, the recurrence alone on the same costs, and non-finite frames; the program checks every path itself"""
    r = host_program
    assert r.returncode == 0 and 'align ok' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_every_validation_code_through_the_host_program(host_program):
    got = dict(l.split()[1:] for l in host_program.stdout.splitlines() if l.startswith('code '))
    got = {k: int(v) for k, v in got.items()}
    A, S, N = WN_E_ARG, WN_E_SHAPE, WN_E_UNSUPPORTED
    want = dict(cfg_null=A, cfg_ok=0, cfg_abi=A, cfg_mels_zero=A, cfg_mels_over=A, cfg_cep_zero=A, cfg_cep_over=A, cfg_cep_most=0, cfg_unit_zero=A, cfg_unit_nan=A,
                cfg_unit_inf=A, cfg_band_neg=A, cfg_band_seven=0, cfg_batch_neg=A, cfg_validation_only=0, cfg_frames_zero=A, cfg_frames_neg=A, cfg_frames_most=0,
                cfg_frames_over=N, cfg_cells_over=N, run_ok=0, run_ok_no_outputs=0, run_a_null=A, run_b_null=A, run_frames_a_null=A, run_frames_b_null=A,
                run_summary_null=A, run_b_zero=A, run_frames_a_zero=A, run_frames_b_zero=A, run_b_over=S, run_frames_a_over=S, run_frames_b_over=S, run_path_short=S,
                run_map_a_short=S, run_map_b_short=S, run_a_pitch_short=S, run_b_pitch_short=S)
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


# ---- the Python surface
def test_hparams_keys_keep_todays_behaviour_by_default(tmp_path):
    """both keys off by default; with them off the Synthesizer's hook returns at once: no handle, no file"""
    import hparams as H
    from wavenet_vocoder.synthesizer import Synthesizer
    hp = H._build()
    assert hp.mi355_alignment_reference_dir == '' and hp.mi355_alignment_band == 0
    hp2 = H._build().parse('mi355_alignment_reference_dir=/data/rec dir/x,mi355_alignment_band=3')
    assert hp2.mi355_alignment_reference_dir == '/data/rec dir/x' and hp2.mi355_alignment_band == 3

    class _Model(object):
        device = torch.device('cpu')

        def alignment_check(self, rows, max_samples, band=None):
            raise AssertionError('no handle may be made with the key off')

    s = Synthesizer(); s._hparams = make_hp(); s.model = _Model(); s._align_chk = None
    assert s._alignment(None, [np.zeros(160, np.float32)], [10], ['a'], str(tmp_path)) is None and os.listdir(str(tmp_path)) == [] and s._align_chk is None


def test_dtw_helper_equals_the_reference():
    from wavenet_vocoder import alignment as AL
    rng = np.random.RandomState(0)
    for Fa, Fb in ((1, 1), (1, 5), (6, 1), (13, 9), (9, 14), (30, 30)):
        for band in (0, 1, 2):
            c = rng.randint(0, 3, (Fa, Fb)).astype(np.float64) + (rng.rand(Fa, Fb) if band == 2 else 0)
            total, path = AL.dtw(c, band)
            d = R.recurrence(c, band)
            assert total == d[-1, -1] and np.array_equal(path, R.backtrace(d, band)), (Fa, Fb, band)


HP16 = dict(sample_rate=8000, hop_size=100, n_fft=400, win_size=400, num_mels=16, fmin=50, fmax=3800, mi355_pitch_window=400)


def _tone(f, n, sr=8000):
    k = np.arange(n)
    return sum(a * np.sin(2 * np.pi * h * f * k / sr) for h, a in ((1, 0.3), (2, 0.15), (3, 0.1))).astype(np.float32)


def test_synthesizer_scores_the_utterances_that_have_a_recording(tmp_path):
    """the key on: the utterances whose basename -- or basename without mel- -- has a wav in the directory are scored, the others are not; one tsv row each;
    a failure logs one line and never fails the run"""
    from scipy.io import wavfile
    from wavenet_vocoder import alignment as AL
    from wavenet_vocoder.synthesizer import Synthesizer
    rec, out = str(tmp_path / 'rec'), str(tmp_path / 'out')
    os.makedirs(rec); os.makedirs(out)
    wavfile.write(os.path.join(rec, 'u0.wav'), 8000, (_tone(150.0, 900) * 32767).astype(np.int16))
    wavfile.write(os.path.join(rec, 'mel-u1.wav'), 8000, (_tone(180.0, 1200) * 32767).astype(np.int16))
    assert AL.reference_for(rec, 'mel-u0').endswith('u0.wav') and AL.reference_for(rec, 'mel-u1').endswith('mel-u1.wav') and AL.reference_for(rec, 'u2') is None
    calls = []

    class _Check(object):
        def __init__(self, rows, max_samples):
            self.rows, self.max_samples = rows, max_samples

        def score(self, gen, gl, ref, rl):
            calls.append((tuple(gen.shape), list(gl), tuple(ref.shape), list(rl)))
            return np.arange(len(gl) * 13, dtype=np.float32).reshape(len(gl), 13)

        def close(self):
            pass

    class _Model(object):
        device = torch.device('cpu')
        made = []

        def alignment_check(self, rows, max_samples, band=None):
            self.made.append((rows, max_samples))
            return _Check(rows, max_samples)

    hp = make_hp(mi355_alignment_reference_dir=rec, **HP16)
    s = Synthesizer(); s._hparams = hp; s.model = _Model(); s._align_chk = None
    wavs = [np.zeros(1000, np.float32), np.zeros(700, np.float32), np.zeros(800, np.float32)]
    t = s._alignment(None, wavs, [10, 7, 8], ['mel-u0', 'u2', 'mel-u1'], out)
    assert t.shape == (2, 13) and s.model.made == [(2, 1200)] and calls == [((2, 1000), [1000, 800], (2, 1200), [900, 1200])]
    assert [r['name'] for r in AL.read_tsv(os.path.join(out, 'alignment.tsv'))] == ['mel-u0', 'mel-u1']
    assert s._alignment(None, wavs[1:2], [7], ['u2'], out) is None and len(calls) == 1          # no recording: nothing runs
    s._alignment(torch.zeros(3, 1600), None, [16, 16, 16], ['u0', 'x', 'y'], out)              # the device path: the rows with a recording are picked; outgrown
    assert s.model.made == [(2, 1200), (2, 1600)] and calls[-1] == ((1, 1600), [1600], (1, 900), [900])
    assert len(AL.read_tsv(os.path.join(out, 'alignment.tsv'))) == 3
    s.model.alignment_check = None                                                              # a failure logs one line
    s._align_chk = None
    assert s._alignment(None, wavs, [10, 7, 8], ['mel-u0', 'u2', 'mel-u1'], out) is None


def test_score_host_and_the_command_line_in_host_mode(tmp_path, capsys):
    """a recording against itself scores zero on a diagonal path; against a copy whose middle is repeated the path stretches, the MCD-DTW stays near zero and
    the F0 error along the path stays small; a wav without a recording is skipped, and said so"""
    from scipy.io import wavfile
    from wavenet_vocoder import alignment as AL
    gen, ref = str(tmp_path / 'gen'), str(tmp_path / 'ref')
    os.makedirs(gen); os.makedirs(ref)
    x = np.concatenate([_tone(160.0, 1600), _tone(240.0, 1600), _tone(200.0, 1600)])
    y = np.concatenate([x[:1600], _tone(240.0, 3200), x[3200:]])          # the middle note twice as long (160, 240 and 200 Hz divide 8000: hop-periodic notes)

    def pcm(z):
        return (z * 32767).astype(np.int16)

    wavfile.write(os.path.join(ref, 'u0.wav'), 8000, pcm(x)); wavfile.write(os.path.join(gen, 'wavenet-audio-u0.wav'), 8000, pcm(x))
    wavfile.write(os.path.join(ref, 'u1.wav'), 8000, pcm(x)); wavfile.write(os.path.join(gen, 'u1.wav'), 8000, pcm(y))
    wavfile.write(os.path.join(gen, 'orphan.wav'), 8000, pcm(x))
    over = ','.join('%s=%s' % kv for kv in HP16.items())
    names, table = AL.main(['--generated', gen, '--reference', ref, '--host', '--band', '0', '--hparams', over, '--tsv', str(tmp_path / 't.tsv')])
    text = capsys.readouterr().out.splitlines()
    t = {n: dict(zip(AL.COLUMNS, row)) for n, row in zip(names, table)}
    assert 'skipped 1 generated wav file(s)' in text[0] and text[1].split('\t') == list(AL.TSV_HEADER) and text[-1].startswith('Alignment check: 2 utterance(s)')
    assert t['u0']['frames_ref'] == 49 and t['u0']['n_path'] == 49 and t['u0']['mcd_dtw'] == 0.0 and t['u0']['stretch'] == 0.0 and t['u0']['f0_rmse_cents'] == 0.0
    assert t['u0']['both'] > 40
    assert t['u1']['frames_gen'] == 65 and t['u1']['stretch'] > 0.15 and t['u1']['mcd_dtw'] < 0.5 and t['u1']['gpe'] == 0.0 and t['u1']['f0_rmse_cents'] < 5.0
    rows = AL.read_tsv(str(tmp_path / 't.tsv'))
    assert sorted(r['name'] for r in rows) == ['u0', 'u1'] and rows[0]['mcd_dtw'] == '%.4f' % table[0][4]


# ---- five faults seeded into a numpy stand-in of the device code, each caught by the check that is there for it
def standin(cost, band, fault=None):
    """float32 recurrence, directions and back-trace like csrc/wn_align.h, with one fault: 'tie' (tie order swapped), 'diag' (the diagonal predecessor dropped),
    'band' (the band inequality made strict), 'edge' (a block's boundary column taken from the wrong diagonal: the left neighbour of a block's first column is
    read one row up).  -> (Dm float32, path)"""
    Fa, Fb = cost.shape
    W = band * max(Fa, Fb)

    def adm(i, j):
        e = abs(i * Fb - j * Fa)
        return band == 0 or (e < W if fault == 'band' else e <= W)

    dm = np.full((Fa, Fb), np.inf, np.float32)
    dirs = np.full((Fa, Fb), 3, np.int8)
    for i in range(Fa):
        for j in range(Fb):
            if not adm(i, j):
                continue
            if i == 0 and j == 0:
                dm[0, 0] = cost[0, 0]
                continue
            cands = []
            if i > 0 and j > 0 and adm(i - 1, j - 1) and fault != 'diag':
                cands.append((dm[i - 1, j - 1], 0))
            if i > 0 and adm(i - 1, j):
                cands.append((dm[i - 1, j], 1))
            if j > 0 and adm(i, j - 1):
                cands.append((dm[max(i - 1, 0), j - 1] if fault == 'edge' and j % T == 0 else dm[i, j - 1], 2))
            if fault == 'tie':
                cands = cands[::-1]
            if cands:
                best, w = cands[0]
                for v, d in cands[1:]:
                    if v < best:
                        best, w = v, d
                dm[i, j], dirs[i, j] = np.float32(cost[i, j]) + best, w
    i, j, rev = Fa - 1, Fb - 1, []
    while i > 0 or j > 0:
        rev.append((i, j))
        w = 2 if i == 0 else 1 if j == 0 else 0 if dirs[i, j] == 3 else dirs[i, j]
        i, j = i - (w != 2), j - (w != 1)
    rev.append((0, 0))
    return dm, np.array(rev[::-1], np.int64)


def _standin_checks(fault):
    """the names of the exact-integer checks (test_exact_integer_costs_pin_the_tie_order and its device twin) that fail on a stand-in with `fault`"""
    failed = set()
    rng = np.random.RandomState(5)
    Fa, Fb = T + 6, T + 9
    cost = rng.randint(0, 4, size=(Fa, Fb)).astype(np.float32)
    for band in (0, 1):
        dm, path = standin(cost, band, fault)
        d64 = R.recurrence(cost, band)
        if not np.array_equal(np.isinf(dm), np.isinf(d64)):
            failed.add('band cells')
        elif not np.array_equal(dm.astype(np.float64), d64):
            failed.add('exact integer Dm')
        elif not np.array_equal(path, R.backtrace(d64, band)):
            failed.add('exact integer path')
    return sorted(failed)


def test_seeded_faults_are_caught_by_name():
    assert _standin_checks(None) == []
    assert _standin_checks('tie') == ['exact integer path']
    assert _standin_checks('diag') == ['exact integer Dm']
    assert _standin_checks('band') == ['band cells']
    assert _standin_checks('edge') == ['exact integer Dm']
    # the square root or the 0.5 dropped: the cost stage's bound
    rng = np.random.RandomState(6)
    ca, cb = rng.randn(9, 13).astype(np.float32), rng.randn(11, 13).astype(np.float32)
    k64, rel = R.cost_matrix(ca, cb)
    e = ca[:, None, :] - cb[None, :, :]
    good = np.sqrt(np.float32(0.5) * np.sum(e * e, axis=2, dtype=np.float32)).astype(np.float32)
    assert np.all(np.abs(good - k64) <= 8 * rel * k64)          # (numpy's pairwise float32 sum is not the fused chain: a few of its bounds)
    for bad in (np.sqrt(np.sum(e * e, axis=2, dtype=np.float32)), np.float32(0.5) * np.sum(e * e, axis=2, dtype=np.float32)):
        assert not np.all(np.abs(bad - k64) <= 8 * rel * k64)
