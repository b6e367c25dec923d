"""The fp32 training mode's kernels (csrc/wn_f32.hip: wn_f32_sgemm_kernel, wn_f32_wgrad_kernel + wn_f32_wgrad_reduce, wn_f32_gate,
wn_f32_gate_bwd) ONE launch at a time on operands this module owns, element by element against float64 (tests/f32_ref.py).

Every sgemm / wgrad case (f32_ref.SGEMM_CASES / WGRAD_CASES: the argument patterns of wn_f32_forward / wn_f32_backward and, beside them,
the smallest shapes at which each run-time branch is reached -- 16-byte or scalar loads, K / M / time tails, transposed weights, the ones
row in a k block of its own, a second 2048-row slab) runs twice through the same launch (wn_test_f32_sgemm / wn_test_f32_wgrad, which
call the chain's own sgemm() / wgrad32()):

  * exact inputs: integers in [-8, 8], alpha / scale / keep_scale powers of two.  Every product and partial sum is exact in fp32 in any
    order, so the device must EQUAL the float64 reference, every element, no tolerance (the sign of a zero is not compared).  The whole
    output buffer is compared, guards included: what the launch must not write (columns >= M of a wider pitch, rows beyond B * T, the
    floats before and after) keeps its sentinel.  This sees every indexing fault; it cannot see a reduced-precision product.
  * real inputs: magnitudes in [0.5, 1], random signs; |dev - ref| <= the worst-case bound of f32_ref (derived there, nothing fitted),
    at most 0.01 while one product is >= 0.25: test_f32_ref_cpu.py asserts that condition on the reference alone.

Input buffers carry NaN in every float a launch has no business reading (pad columns, guard rows before and after): a stray read
poisons the output.  The gate kernels are held to 8 x the error of the same formula in float32 on the CPU.  One live train_fwd then checks
the wiring of the forward chain from the device's own buffers.  With WN_PARITY_REPORT_DIR set the last test writes
f32_kernels_parity.json (profiles/f32_kernels_parity.json is that file from an MI355X)."""
import json
import os

import numpy as np
import pytest
import torch

import f32_ref as R
import launch_ref as LR
from hip_util import SMALL, layer_key, make_hp, oracle_cfg, synth_batch, upload_params
from oracle import wavenet_oracle as O

pytestmark = pytest.mark.gpu

SENT = 777.25                      # what an output float holds before the launch
NAN = float('nan')
MAXB, MAXT = 3, 2080               # the hook engine's capacity (2080 = 130 hops >= 2072)
HOOK_HP = dict(SMALL, layers=2, stacks=1, residual_channels=128, gate_channels=256, skip_out_channels=128, wavenet_dropout=R.DROP_P, mi355_compute_dtype='fp32')
RECORDS = {'sgemm': {}, 'wgrad': {}, 'gate': {}, 'live_forward': {}}
_ENG = {}


def hook_engine():
    """one fp32-mode context for every hook launch: partial-sum buffer 6 slabs x 129 x 256 floats."""
    if 'e' not in _ENG:
        from wavenet_vocoder import _ext
        _ENG['e'] = _ext.Engine(make_hp(**HOOK_HP), MAXB, MAXT)
    return _ENG['e']


def place(mat, ld, off=0, before=0, after=0, fill=NAN, pad=None):
    """mat [rows, cols] (float64, or None: rows x cols of `fill`) into a flat float32 device buffer: `before` guard floats (rounded up to a
    multiple of 4: the buffer itself is 256-byte aligned), `off` more floats (1: the operand loses its 16-byte alignment), rows of pitch ld
    (pad columns = pad, default fill), `after` guard floats.  Returns (buffer, view from the operand's first float, index of that float)."""
    rows, cols = mat.shape
    before = (before + 3) // 4 * 4
    start = before + off
    buf = torch.full((start + rows * max(ld, cols) + after + 8,), fill, dtype=torch.float32)
    body = torch.full((rows, max(ld, cols)), fill if pad is None else pad, dtype=torch.float32)
    body[:, :cols] = mat.to(torch.float32)
    buf[start:start + body.numel()] = body.reshape(-1)
    buf = buf.cuda()
    return buf, buf[start:], start


def worst(dev, ref, bound):
    """(max err / bound, [row, col]) with 0 / 0 = 0 and x / 0 = inf."""
    err = (dev.double() - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    ratio = torch.where(torch.isnan(dev.double()), torch.full_like(ratio, float('inf')), ratio)
    i = int(ratio.argmax())
    return float(ratio.reshape(-1)[i]), [i // ratio.shape[-1], i % ratio.shape[-1]]


# ------------------------------------------------------------------------------------------------------------------ sgemm
def run_sgemm(case, ops, in_off=0, w_off=0):
    """One launch of the case on the operands `ops`; returns (out buffer on the host, expected-untouched buffer, index map of the logical
    output [N, M] into the buffer)."""
    c = case
    eng = hook_engine()
    B, T, K, M = c['B'], c['T'], c['K'], c['M']
    N = B * T
    g = 160 * max(c['ld_in'], 1)      # guard rows on both sides of In: no shift of a case reaches further
    _, In, _ = place(ops['In'], c['ld_in'], in_off, before=g, after=g)
    if c['wm']:        # transposed: W[k][m] at m * wm + k
        _, W, _ = place(ops['W'].t(), c['wm'], w_off, before=64, after=64)
        wk, wm = 1, c['wm']
    else:
        _, W, _ = place(ops['W'], c['ldw'], w_off, before=64, after=64)
        wk, wm = c['ldw'], 1
    if c['out_bot']:
        init = torch.full((B, M, T), SENT, dtype=torch.float64)
        if ops['prev'] is not None:
            init = R.to_bot(ops['prev'], B, T)
        obuf, Out, start = place(init.reshape(1, -1), B * M * T, before=4096, after=4096, fill=SENT)
        idx = start + ((torch.arange(B)[:, None, None] * M + torch.arange(M)[None, None, :]) * T + torch.arange(T)[None, :, None]).reshape(N, M)
    else:
        init = ops['prev'] if ops['prev'] is not None else torch.full((N, M), SENT, dtype=torch.float64)
        obuf, Out, start = place(init, c['ld_out'], before=4096, after=4096, fill=SENT)
        idx = start + torch.arange(N)[:, None] * c['ld_out'] + torch.arange(M)[None, :]
    before = obuf.cpu().clone()
    kw = {}
    if ops['bias'] is not None:
        kw['bias'] = place(ops['bias'].reshape(1, -1), ops['bias'].numel(), before=8, after=256)[1]
        kw['bias_bstride'] = M if ops['bias'].dim() == 2 else 0
    if ops['add'] is not None:
        kw['add'] = place(ops['add'], M, before=256, after=256)[1]; kw['ld_add'] = M
    if ops['mask'] is not None:
        kw['mask'] = place(ops['mask'], M, before=256, after=256)[1]; kw['ld_mask'] = M
    if c['drop']:
        kw.update(key=layer_key(R.DROP_SEED, R.DROP_LAYER), thresh16=int(np.rint(np.float32(R.DROP_P) * np.float32(65536.0))), keep_scale=2.0,
                  drop_ld=c['drop_ld'], drop_on_out=int(c['drop'] == 'out'))
    eng.f32_sgemm(B, T, In, c['ld_in'], W, wk, wm, K, M, Out, c['ld_out'], shift=c['shift'], accumulate=c['accumulate'], alpha=c['alpha'], scale=c['scale'],
                  relu=c['relu'], out_bot=c['out_bot'], **kw)
    torch.cuda.synchronize()
    return obuf.cpu(), before, idx


def check_sgemm(name, case, kind, in_off=0, w_off=0):
    gen = torch.Generator().manual_seed(R.case_seed(name))
    if kind == 'real':
        R.sgemm_operands(case, 'exact', gen)      # (the draws of the CPU test: exact first, then real, from one generator)
    ops = R.sgemm_operands(case, kind, gen)
    ref, bound = R.sgemm_case_ref(case, ops)
    out, before, idx = run_sgemm(case, ops, in_off, w_off)
    dev = out[idx.reshape(-1)].reshape(ref.shape)
    untouched = torch.ones(out.numel(), dtype=torch.bool); untouched[idx.reshape(-1)] = False
    stray = int((out[untouched] != before[untouched]).sum())
    if kind == 'exact':
        bad = dev.double() != ref
        n = int(bad.sum())
        where = [int(v) for v in bad.nonzero()[0]] if n else None
        print('\n  sgemm %-20s exact: %d of %d elements differ%s; %d floats outside the output written' % (name, n, ref.numel(), ' (first at %s: dev %r ref %r)' % (
            where, float(dev[tuple(where)]), float(ref[tuple(where)])) if n else '', stray))
        rec = dict(differ=n, first=where, stray=stray)
        ok = n == 0 and stray == 0
    else:
        w, at = worst(dev, ref, bound)
        print('\n  sgemm %-20s real : worst |dev - ref| / bound = %.3g at %s (bound max %.2e); %d floats outside the output written' % (name, w, at, float(bound.max()), stray))
        rec = dict(worst_err_over_bound=w, at=at, bound_max=float(bound.max()), stray=stray)
        ok = w <= 1.0 and stray == 0
    return ok, rec, dev


@pytest.mark.parametrize('name', sorted(R.SGEMM_CASES))
def test_sgemm_launch_equals_float64_on_exact_inputs_and_stays_in_bound_on_real_inputs(name):
    case = R.SGEMM_CASES[name]
    ok_e, rec_e, _ = check_sgemm(name, case, 'exact')
    ok_r, rec_r, _ = check_sgemm(name, case, 'real')
    RECORDS['sgemm'][name] = dict(exact=rec_e, real=rec_r)
    assert ok_e, rec_e
    assert ok_r, rec_r


@pytest.mark.parametrize('name', ['gate_tap1', 'gate_tap0', 'drop_a_kept_tail', 'd_skips', 'd_h_tap1', 'fin2_o30', 'k2_ld16'])
def test_sgemm_bits_do_not_depend_on_operand_alignment(name):
    """In or W displaced by one float: the 16-byte paths fall back to scalar loads of the same values into the same places, so the output
    must be the aligned run's, bit for bit, on real inputs -- and still equal float64 on exact inputs."""
    case = R.SGEMM_CASES[name]
    _, _, base = check_sgemm(name, case, 'real')
    for in_off, w_off in ((1, 0), (0, 1), (1, 1)):
        ok, rec, dev = check_sgemm(name, case, 'real', in_off, w_off)
        assert ok, rec
        assert torch.equal(dev.view(torch.int32), base.view(torch.int32)), (name, in_off, w_off, int((dev.view(torch.int32) != base.view(torch.int32)).sum()))
        ok, rec, _ = check_sgemm(name, case, 'exact', in_off, w_off)
        assert ok, rec


# ------------------------------------------------------------------------------------------------------------------ wgrad
def run_wgrad(case, ops, a_off=0, b_off=0):
    c = case
    eng = hook_engine()
    B, T, K, M = c['B'], c['T'], c['K'], c['M']
    ga, gb = 2200 * c['lda'], 2200 * c['ldb']      # guard rows: a slab is 2048 rows whatever T is
    A = None if ops['A'] is None else place(ops['A'], c['lda'], a_off, before=160 * c['lda'], after=ga)[1]
    Bm = place(ops['Bm'], c['ldb'], b_off, before=160 * c['ldb'], after=gb)[1]
    outs = {}
    if A is not None:
        outs['out'] = place(torch.full((K, M), SENT, dtype=torch.float64), c['ldo'], before=1024, after=1024, fill=SENT)
    for i in range(c['biases']):
        outs['bias%d' % i] = place(torch.full((1, M), SENT, dtype=torch.float64), M, before=256, after=256, fill=SENT)
    before = {k: v[0].cpu().clone() for k, v in outs.items()}
    eng.f32_wgrad(B, T, A, c['lda'], K, Bm, c['ldb'], M, outs['out'][1] if A is not None else None, c['ldo'], shift=c['shift'], alpha=c['alpha'],
                  drop_layer=R.DROP_LAYER if c['drop'] else -1, seed=R.DROP_SEED, bias_out=outs['bias0'][1] if c['biases'] > 0 else None,
                  bias_out2=outs['bias1'][1] if c['biases'] > 1 else None)
    torch.cuda.synchronize()
    return {k: (v[0].cpu(), before[k], v[2]) for k, v in outs.items()}


def check_wgrad(name, case, kind, a_off=0, b_off=0):
    gen = torch.Generator().manual_seed(R.case_seed(name))
    if kind == 'real':
        R.wgrad_operands(case, 'exact', gen)
    ops = R.wgrad_operands(case, kind, gen)
    dW, bound, cs, cs_bound = R.wgrad_case_ref(case, ops)
    got = run_wgrad(case, ops, a_off, b_off)
    K, M = case['K'], case['M']
    ok, rec, devs = True, {}, {}
    for key, (out, before, start) in sorted(got.items()):
        if key == 'out':
            idx = start + torch.arange(K)[:, None] * case['ldo'] + torch.arange(M)[None, :]
            ref, bnd = dW, bound
        else:
            idx = start + torch.arange(M)[None, :]
            ref, bnd = cs[None, :], cs_bound[None, :]
        dev = out[idx.reshape(-1)].reshape(ref.shape)
        devs[key] = dev
        untouched = torch.ones(out.numel(), dtype=torch.bool); untouched[idx.reshape(-1)] = False
        stray = int((out[untouched] != before[untouched]).sum())
        if kind == 'exact':
            bad = dev.double() != ref
            n = int(bad.sum())
            where = [int(v) for v in bad.nonzero()[0]] if n else None
            print('\n  wgrad %-18s %-5s exact: %d of %d elements differ%s; %d floats outside written' % (name, key, n, ref.numel(), ' (first at %s: dev %r ref %r)' % (
                where, float(dev[tuple(where)]), float(ref[tuple(where)])) if n else '', stray))
            rec[key] = dict(differ=n, first=where, stray=stray)
            ok = ok and n == 0 and stray == 0
        else:
            w, at = worst(dev, ref, bnd)
            print('\n  wgrad %-18s %-5s real : worst |dev - ref| / bound = %.3g at %s (bound max %.2e); %d floats outside written' % (name, key, w, at, float(bnd.max()), stray))
            rec[key] = dict(worst_err_over_bound=w, at=at, bound_max=float(bnd.max()), stray=stray)
            ok = ok and w <= 1.0 and stray == 0
    return ok, rec, devs


@pytest.mark.parametrize('name', sorted(R.WGRAD_CASES))
def test_wgrad_equals_float64_on_exact_inputs_and_stays_in_bound_on_real_inputs(name):
    """Through wgrad32(): the reservation of the backward buffers, the capacity check of the partial sums, the launch per slab and the ordered
    slab reduction.  With B = 3 the reference zeroes an A row that `shift` takes before ITS utterance's start: a read from the previous
    utterance shows on exact inputs.  Real inputs where B * T <= 160 (the bound's condition)."""
    case = R.WGRAD_CASES[name]
    ok_e, rec_e, _ = check_wgrad(name, case, 'exact')
    RECORDS['wgrad'][name] = dict(exact=rec_e)
    assert ok_e, rec_e
    if R.wgrad_runs_real(case):
        ok_r, rec_r, _ = check_wgrad(name, case, 'real')
        RECORDS['wgrad'][name]['real'] = rec_r
        assert ok_r, rec_r


@pytest.mark.parametrize('name', ['taps_tap1', 'cin_k128_two', 'taps_tap_d130_b1', 'fin2_o2'])
def test_wgrad_bits_do_not_depend_on_operand_alignment(name):
    case = R.WGRAD_CASES[name]
    _, _, base = check_wgrad(name, case, 'real')
    for a_off, b_off in ((1, 0), (0, 1)):
        ok, rec, devs = check_wgrad(name, case, 'real', a_off, b_off)
        assert ok, rec
        for k in base:
            assert torch.equal(devs[k].view(torch.int32), base[k].view(torch.int32)), (name, k, a_off, b_off)
        ok, rec, _ = check_wgrad(name, case, 'exact', a_off, b_off)
        assert ok, rec


def test_hooks_refuse_what_the_context_cannot_hold():
    from wavenet_vocoder import _ext
    eng = hook_engine()
    z = torch.zeros(1 << 16, device='cuda')
    for B, T in ((MAXB + 1, 5), (1, MAXT + 1), (0, 5)):
        with pytest.raises(_ext.WnError) as e:
            eng.f32_sgemm(B, T, z, 16, z, 16, 1, 16, 16, z, 16)
        assert e.value.code == -1
        with pytest.raises(_ext.WnError) as e:
            eng.f32_wgrad(B, T, z, 16, 16, z, 16, 16, z, 16)
        assert e.value.code == -1
    big = torch.zeros(3 * 2072 * 300, device='cuda')
    with pytest.raises(_ext.WnError) as e:      # 6 slabs x 300 x 136 floats > the partial-sum buffer (6 x 129 x 256)
        eng.f32_wgrad(3, 2072, big, 300, 300, big, 136, 136, big, 136)
    assert e.value.code == -5
    bf = _ext.Engine(make_hp(**dict(SMALL, layers=2, stacks=1)), 1, 64)
    with pytest.raises(_ext.WnError) as e:
        bf.f32_sgemm(1, 5, z, 16, z, 16, 1, 16, 16, z, 16)
    assert e.value.code == -5
    with pytest.raises(_ext.WnError) as e:
        bf.f32_gate(z[:64].view(2, 32), z[:32].view(2, 16))
    assert e.value.code == -5
    torch.cuda.synchronize()


def test_hooks_leave_a_pending_backward_as_it_was():
    """The hooks set the context's forward shape and dropout seed for one call and put them back: a train_bwd after hook calls at another
    (B, T, seed) returns the gradients of a train_bwd without them.  Left at the hook's B = 1, T = 5 or at its seed (other dropout masks) the
    gradients would differ in the first digit; 1e-6 relative only leaves room for a summation that is not ordered."""
    from wavenet_vocoder import _ext
    from hip_util import rel_err
    hp = make_hp(**dict(SMALL, wavenet_dropout=0.5, mi355_compute_dtype='fp32'))
    cfg = oracle_cfg(hp)
    B, T = 2, 64
    eng = _ext.Engine(hp, B, T)
    eng.pack_weights(upload_params(eng, O.init_params(cfg, seed=5339, bias_scale=0.05)))
    wav, c = synth_batch(cfg, B, T, seed=3)
    x, y = wav.view(B, 1, T).contiguous().cuda(), wav.view(B, T, 1).contiguous().cuda()
    ln = torch.full((B,), T, dtype=torch.int32, device='cuda')
    loss = torch.zeros(1, device='cuda')
    grads = []
    for with_hooks in (False, True):
        eng.train_fwd(x, c.cuda(), y, ln, 99, loss)
        if with_hooks:
            a = torch.ones(5 * 16, device='cuda'); o = torch.zeros(16 * 16, device='cuda'); bo = torch.zeros(16, device='cuda')
            eng.f32_sgemm(1, 5, a, 16, o.clone(), 16, 1, 16, 16, o, 16)
            eng.f32_wgrad(1, 5, a, 16, 16, a, 16, 16, o, 16, drop_layer=1, seed=12345, bias_out=bo)
        g = torch.full((eng.n_params,), float('nan'), device='cuda')
        eng.train_bwd(g)
        torch.cuda.synchronize()
        grads.append(g.cpu())
    assert torch.isfinite(grads[0]).all() and float(grads[0].abs().sum()) > 0
    assert rel_err(grads[1], grads[0]) <= 1e-6, rel_err(grads[1], grads[0])


# ------------------------------------------------------------------------------------------------------------------ gate
def test_gate_and_its_derivative_against_float64():
    """Z in [-20, 20] with +-0, the integers and saturated values; GU real with exact zeros.  Bound per element: 8 x |float32 CPU evaluation of
    the same formula - float64|, floored at 2^-22 max(|ref|, |gu|) (f32_ref.gate_bounds, measured on the reference here).  The ratio of the
    device's worst error to the yardstick's goes into the report."""
    gen = torch.Generator().manual_seed(77)
    rows, GH = 333, 72
    Z = (torch.rand(rows, 2 * GH, generator=gen) * 40.0 - 20.0).float()
    special = torch.tensor([0.0, -0.0, 20.0, -20.0, 17.5, -17.5, 9.0, -9.0, 1.0, -1.0, 2.0 ** -20, -2.0 ** -20, 88.0, -88.0][:12])
    Z[0, :12] = special; Z[0, GH:GH + 12] = special.flip(0); Z[1, :12] = special.flip(0); Z[1, GH:GH + 12] = special
    Z[2] = torch.arange(2 * GH).float() % 41 - 20.0
    GU = R.real_unit(gen, rows, GH).float()
    GU[3] = 0.0
    U64, DZ64, ub, dzb = R.gate_bounds(Z, GU)
    U32, DZ32 = R.ref_gate(Z, GU, torch.float32)
    U, DZ = hook_engine().f32_gate(Z.cuda(), GU.cuda())
    torch.cuda.synchronize()
    U, DZ = U.cpu(), DZ.cpu()
    rec = {}
    for key, dev, ref, bnd, y32 in (('U', U, U64, ub, U32), ('DZ', DZ, DZ64, dzb, DZ32)):
        w, at = worst(dev, ref, bnd)
        e_dev, e_32 = float((dev.double() - ref).abs().max()), float((y32.double() - ref).abs().max())
        rec[key] = dict(worst_err_over_bound=w, at=at, z=[float(Z[at[0], at[1] % GH]), float(Z[at[0], GH + at[1] % GH])], max_err_device=e_dev, max_err_float32_cpu=e_32,
                        device_over_yardstick=e_dev / e_32)
        print('\n  gate %-2s: worst |dev - ref| / bound = %.3g at %s; max error device %.3e, float32 CPU %.3e (ratio %.2f)' % (key, w, at, e_dev, e_32, e_dev / e_32))
    RECORDS['gate'] = rec
    assert torch.isfinite(U).all() and torch.isfinite(DZ).all()
    assert rec['U']['worst_err_over_bound'] <= 1.0 and rec['DZ']['worst_err_over_bound'] <= 1.0, rec


# ------------------------------------------------------------------------------------------------------------------ the live forward
def test_live_forward_wiring_from_the_devices_own_buffers():
    """One train_fwd of an fp32 engine (B = 3, T = 144, ragged lengths; SMALL with 6 layers, 2 stacks, dropout 0.1, global conditioning,
    legacy scaling): every buffer the forward keeps from the buffers it was computed from -- Z_l from X_l (three taps on the dropped input
    + conditioning + the per-utterance bias), U_l from Z_l, X_{l+1} from U_l and X_l, SK from all U_l, H1 from SK, y_hat from H1 -- every
    element, under the sgemm bound summed over the launches that accumulate into the buffer (f32_ref) and the gate bound.  The first 2d
    rows of the utterances b >= 1 are their own group: the error there stays below half of what a read across the utterance start adds."""
    from wavenet_vocoder import _ext
    from hip_util import dropout_mask
    over = dict(SMALL, layers=6, stacks=2, wavenet_dropout=0.1, legacy=True, gin_channels=16, use_speaker_embedding=False, mi355_compute_dtype='fp32')
    hp = make_hp(**over)
    cfg = oracle_cfg(hp)
    B, T, seed = 3, 144, 4242
    L, Rc, G, GH, S, C, Oc = cfg.layers, cfg.residual_channels, cfg.gate_channels, cfg.gate_channels // 2, cfg.skip_out_channels, cfg.cin_channels, cfg.out_channels
    eng = _ext.Engine(hp, B, T)
    params = O.init_params(cfg, seed=5339, bias_scale=0.05)
    eng.pack_weights(upload_params(eng, params))
    wav, c = synth_batch(cfg, B, T, seed=3)
    gvec = torch.randn(B, cfg.gin_channels, generator=torch.Generator().manual_seed(9)).float()
    eng.set_global_condition(gvec.cuda())
    ln = torch.tensor([T, T - 37, T - 74], dtype=torch.int32).cuda()
    loss = torch.zeros(1, device='cuda'); yhat = torch.empty(B, Oc, T, device='cuda')
    eng.train_fwd(wav.view(B, 1, T).contiguous().cuda(), c.cuda(), wav.view(B, T, 1).contiguous().cuda(), ln, seed, loss, yhat)
    torch.cuda.synchronize()
    N = B * T
    dl = lambda name, l, ch: eng.debug_copy(name, l, N, ch).cpu().double()      # noqa: E731
    W = LR.Weights(params, cfg, rounded=False)
    skip_scale = [float(np.float32(LR.SQRT_HALF_F32 ** (L - 1 if l == 0 else L - l))) for l in range(L)]      # the device's float32 factors
    bias, ebias = LR.ref_gate_bias(W, params, cfg, gvec)                          # [L, B, G] and the error of the device's fp32 vector
    cup = eng.debug_copy('CUP', eng.cfg.n_upsample - 1, B * C, T).cpu().double().view(B, C, T)
    C32 = cup.permute(0, 2, 1).reshape(N, C)
    skipb = eng.debug_copy('SKIPB', 0, 1, S).cpu().double().reshape(-1)
    keep_scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.1)))
    rec, fails = {}, []

    def note(key, dev, ref, bound, rows=None):
        if rows is not None:
            dev, ref, bound = dev[rows], ref[rows], bound[rows]
        w, at = worst(dev, ref, bound)
        rec[key] = dict(worst_err_over_bound=w, at=at)
        if not w <= 1.0:
            fails.append('%s: worst |dev - ref| / bound = %.3g at %s' % (key, w, at))

    X = [dl('X', l, Rc) for l in range(L)]
    U = [dl('U', l, GH) for l in range(L)]
    sk, sk_b = None, None
    for l in range(L):
        d = W.dil[l]
        Z = dl('Z', l, G)
        keep = torch.from_numpy(dropout_mask(seed, l, N, Rc, 0.1)).double()
        z, zb = None, torch.zeros(N, G, dtype=torch.float64)
        for tap in range(3):
            z, b_ = R.ref_sgemm(X[l], W.w_dil[l][tap], B, T, shift=-(2 - tap) * d, prev=z, bias=bias[l] if tap == 0 else None, keep_a=keep, keep_scale=keep_scale)
            zb = zb + b_
        z, b_ = R.ref_sgemm(C32, W.w_cin[l], B, T, prev=z)
        zb = zb + b_ + ebias[l].repeat_interleave(T, dim=0)
        note('Z %d' % l, Z, z, zb)
        start = torch.zeros(B, T, dtype=torch.bool); start[1:, :min(2 * d, T)] = True
        note('Z %d start' % l, Z, z, zb, rows=start.reshape(-1))
        leak = LR.gate_start_leak(W, l, (X[l] * keep * keep_scale).view(B, T, Rc)).reshape(N, G)
        e_start, e_leak = float((Z - z)[start.reshape(-1)].norm()), float(leak.norm())
        rec['Z %d start' % l]['error_over_leak'] = e_start / e_leak
        if not e_start < 0.5 * e_leak:
            fails.append('Z %d: |dev - ref| = %.3e on the first 2d rows of the utterances b >= 1 is not below half of what reading the previous utterance adds (%.3e)' % (l, e_start, e_leak))
        u64, _, ub, _ = R.gate_bounds(Z.float(), torch.ones(N, GH))
        note('U %d' % l, U[l], u64, ub)
        if l + 1 < L:
            x, xb = R.ref_sgemm(U[l], W.w_out[l], B, T, bias=W.b_out[l], add=X[l], scale=W.res_scale)
            note('X %d' % (l + 1), X[l + 1], x, xb)
        sk, b_ = R.ref_sgemm(U[l], W.w_skip[l] / W.skip_scale[l], B, T, alpha=skip_scale[l], prev=sk)
        sk_b = b_ if sk_b is None else sk_b + b_
    SK, H1 = dl('SK', 0, S), dl('H1', 0, S)
    pre = sk + skipb
    note('SK', SK, pre.clamp_min(0.0), sk_b + 2.0 ** -24 * (sk.abs() + skipb.abs()))      # wn_f32_bias_relu: one more addition
    h1, hb = R.ref_sgemm(SK, W.fin1, B, T, bias=W.b_fin1, relu=True)
    note('H1', H1, h1, hb)
    y, yb = R.ref_sgemm(H1, W.fin2, B, T, bias=W.b_fin2)
    note('YHAT', yhat.cpu().double().permute(0, 2, 1).reshape(N, Oc), y, yb)
    assert torch.equal(yhat.cpu().double(), R.to_bot(yhat.cpu().double().permute(0, 2, 1).reshape(N, Oc), B, T))
    RECORDS['live_forward'] = rec
    print('\n  live forward: ' + '  '.join('%s %.2g' % (k, v['worst_err_over_bound']) for k, v in rec.items()))
    assert not fails, '\n'.join(fails)


def test_write_parity_report():
    d = os.environ.get('WN_PARITY_REPORT_DIR')
    if d:
        with open(os.path.join(d, 'f32_kernels_parity.json'), 'w') as f:
            f.write('{\n "note": %s,\n' % json.dumps('per case: exact = elements that differ from float64 (must be 0) and floats written outside the output; real = worst |dev - ref| / bound '
                                                     'and where; gate: device error over the float32 CPU yardstick; records of one run, the tests assert'))
            f.write(',\n'.join(' %s: {\n%s\n }' % (json.dumps(k), ',\n'.join('  %s: %s' % (json.dumps(n), json.dumps(v)) for n, v in sorted(g.items()))) for k, g in RECORDS.items()) + '\n}\n')
