"""Training steps on a REUSED, larger context (pytest -m gpu): what production training does and no other parity test does.

Every other GPU parity test builds its engine at exactly the geometry it then runs once.  wavenet_vocoder/train.py builds ONE context at
(wavenet_batch_size, max(max_time_steps, eval_max_time)) and feeds it batches padded to the longest utterance of each batch, with validation
forwards at yet another geometry in between.  Inside the context the layer stride of every activation buffer is max_batch * max_time while
the rows of a step are packed as b * T + t, so on a reused context everything past row B * T of every layer slab, and everything in the
partial-sum buffers, holds the PREVIOUS step's live values; nothing clears them.  A launch that reads a row, a tile tail or a partial block
it did not write this step -- the stale-operand class -- computes from those.  On a fresh context the same bytes are zeros and nothing shows.

Here one context of (7, 656) -- 4592 rows per layer, no multiple of 128 -- runs S1 = 7 x 656 (all full, other data: every row of every slab
and every partial is live), then the shrinking / growing / sub-tile / fewer-utterances steps S2 .. S5 below, whole steps each.  Two modes:
  live   nothing between the steps: stale bytes are the previous step's finite values;
  nan    Engine.poison_workspace() (wn_test_poison_workspace: 0xFF bytes, NaN in bf16 and fp32, over the whole allocation of every buffer
         only training steps write) before each of S2 .. S5.
After each of S2 .. S5:
  (a) check_step of test_hip_launch_local.py, unchanged: every launch against its float64 reference, every element, the bounds that helper
      derives (no tolerance is introduced here), with the report that counts a non-finite device value as a failure; loss, all of y_hat and
      all gradient floats (the buffer pre-filled with NaN) are finite;
  (b) live mode: a twin context of the same size with the same packed weights, which runs only that step.  Same size, same dispatch: the
      element-wise buffers must be byte-identical.  Gradients: the twin runs the step twice; every tensor the library reduces in a fixed order
      must have the same bits in both of its runs and in the reused context.  The tensors it accumulates with float atomics (atomic_tensors:
      the id scatter of softmax_c1, the Resize and 1D parameter gradients, the speaker-embedding gradient, the per-layer weight-gradient kernel
      of the 64-channel models at B > 2) are judged by (a) alone, and the test prints how many.  (Asking the twin to reproduce ITSELF first and
      only then comparing decides those tensors by luck: two runs of an atomic sum often agree and a third differs in the last bit --
      measured: softmax_c1 at 2 x 656, input_convolution/kernel, rel-L2 3.0e-10.)
The fp32 compute mode has no launch-local reference: the twin is the judge there, in both modes."""
import numpy as np
import pytest
import torch

from hip_util import SMALL, download_grads, make_hp, oracle_cfg, rel_err, upload_params
from oracle import wavenet_oracle as O
from test_hip_launch_local import check_forward, check_step
from test_hip_parity import CONFIGS, _inputs
from test_hip_round6 import GEOMETRIES

pytestmark = pytest.mark.gpu

MAXB, MAXT = 7, 656
S1 = (7, 656, [656] * 7)
S2, S3, S4, S5 = (3, 144, [144, 129, 2]), (5, 272, [272, 256, 255, 130, 16]), (1, 112, [112]), (2, 656, [656, 513])
STEPS = [('S2', S2), ('S3', S3), ('S4', S4), ('S5', S5)]
assert all(s in GEOMETRIES for _, s in STEPS) and (MAXB * MAXT) % 128 != 0
S1_DATA_SEED, DATA_SEED, DROP_SEED = 21, 0, 1234


class Model:
    """One configuration: hparams, oracle configuration and the parameters of test_hip_parity._run_fwd (moved upsample kernels and gains)."""

    def __init__(self, name, **over):
        self.name = name
        self.hp = make_hp(**dict(dict(SMALL, **CONFIGS[name]), **over))
        self.cfg = cfg = oracle_cfg(self.hp)
        assert cfg.hop == 16 and MAXT % cfg.hop == 0
        self.params = params = O.init_params(cfg, seed=5339, bias_scale=0.05)
        g = torch.Generator().manual_seed(7)
        for k in params:
            if k.startswith('local_conditioning') and k.endswith('kernel'):
                params[k] = params[k] + 0.05 * torch.randn(params[k].shape, generator=g)
        for k in params:
            if k.endswith('/g'):
                params[k] = params[k] * (torch.rand(params[k].shape, generator=g) * 0.8 + 0.6)
        self.flat = None

    def engine(self, grad_buckets=None):
        from wavenet_vocoder import _ext
        eng = _ext.Engine(self.hp, MAXB, MAXT, grad_buckets=grad_buckets)
        if self.flat is None:
            self.flat = upload_params(eng, self.params)      # (packed once per engine from the one flat buffer)
        eng.pack_weights(self.flat)
        return eng

    def data(self, B, T, seed):
        cfg = self.cfg
        x_dev, y_dev, x_or, y_or, c = _inputs(cfg, self.hp, B, T, seed)
        g = None
        if cfg.gin_channels > 0:
            gg = torch.Generator().manual_seed(11 + B)
            g = torch.randint(0, cfg.n_speakers, (B,), generator=gg).int() if cfg.use_speaker_embedding else torch.randn(B, cfg.gin_channels, generator=gg)
        quant = cfg.input_type == 'mulaw-quantize'
        return dict(B=B, T=T, x_dev=x_dev, y_dev=y_dev, x_or=x_or, y_or=y_or, c=c, g=g, x_in=y_or if quant else x_or.view(B, T))


def run_step(m, eng, d, lengths, seed, set_g=True):
    """One whole step.  y_hat and the gradient buffer are pre-filled with NaN: whatever the step does not write shows."""
    B, T, cfg = d['B'], d['T'], m.cfg
    if d['g'] is not None and set_g:
        eng.set_global_condition(d['g'].cuda())
    loss = torch.full((1,), float('nan'), device='cuda')
    yhat = torch.full((B, cfg.out_channels, T), float('nan'), device='cuda')
    grads = torch.full((eng.n_params,), float('nan'), device='cuda')
    eng.train_fwd(d['x_dev'], d['c'].cuda(), d['y_dev'], torch.tensor(lengths, dtype=torch.int32).cuda(), seed, loss, yhat)
    eng.train_bwd(grads)
    torch.cuda.synchronize()
    return loss, yhat, grads


def assert_finite(tag, loss, yhat, grads):
    assert np.isfinite(float(loss.item())), '%s: loss %r' % (tag, float(loss.item()))
    assert bool(torch.isfinite(yhat).all()), '%s: %d of %d y_hat values are not finite' % (tag, int((~torch.isfinite(yhat)).sum()), yhat.numel())
    bad = ~torch.isfinite(grads)
    assert not bool(bad.any()), '%s: %d of %d gradient floats are not finite, first at flat index %d' % (tag, int(bad.sum()), grads.numel(), int(bad.int().argmax()))


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def snapshot(eng, cfg, B, T):
    """Every element-wise buffer of the last step, B * T rows per layer, as bits."""
    L, R, G, S, C, Oc = cfg.layers, cfg.residual_channels, cfg.gate_channels, cfg.skip_out_channels, cfg.cin_channels, cfg.out_channels
    n, GH, ldDY = B * T, G // 2, (Oc + 15) // 16 * 16
    out = {}
    for l in range(L):
        for nm, ch in (('X', R), ('XD', R), ('TS', GH), ('U', GH), ('DZ', G)):
            out['%s[%d]' % (nm, l)] = _bits(eng.debug_copy(nm, l, n, ch))
    for l in range(L + 1):
        out['GX[%d]' % l] = _bits(eng.debug_copy('GX', l, n, R))
    for nm, ch in (('R1', S), ('H2', S), ('DY', ldDY), ('cbt', C)):
        out[nm] = _bits(eng.debug_copy(nm, 0, n, ch))
    out['YHAT'] = _bits(eng.debug_copy('YHAT', 0, B * Oc, T))
    nearest = cfg.upsample_type == 'NearestNeighbor'
    if not nearest:      # (NearestNeighbor has no upsample parameters: nothing computes d c)
        out['DC'] = _bits(eng.debug_copy('DC', 0, B * C, T))
    Tl = T // cfg.hop
    for i in range(1 if nearest else len(cfg.upsample_scales)):
        Tl *= cfg.hop if nearest else cfg.upsample_scales[i]
        out['CUP[%d]' % i] = _bits(eng.debug_copy('CUP', i, B * C, Tl))
    assert Tl == T
    return out


def snapshot_f32(eng, cfg, B, T):
    L, R, G, S = cfg.layers, cfg.residual_channels, cfg.gate_channels, cfg.skip_out_channels
    out = {}
    for l in range(L):
        for nm, ch in (('X', R), ('U', G // 2), ('Z', G)):
            out['%s[%d]' % (nm, l)] = _bits(eng.debug_copy(nm, l, B * T, ch))
    for nm in ('SK', 'H1'):
        out[nm] = _bits(eng.debug_copy(nm, 0, B * T, S))
    return out


def assert_same_bits(tag, mine, twin):
    assert mine.keys() == twin.keys() and len(mine) > 0
    for k in mine:
        diff = mine[k] != twin[k]
        if bool(diff.any()):
            idx = int(diff.flatten().int().argmax())
            row, ch = divmod(idx, mine[k].shape[-1])
            raise AssertionError('%s: %s of the reused context differs from the twin context in %d of %d elements, first at row %d column %d: %s vs %s (as float32)' % (
                tag, k, int(diff.sum()), diff.numel(), row, ch, float(mine[k].view(torch.float32).flatten()[idx]), float(twin[k].view(torch.float32).flatten()[idx])))
    return len(mine)


def atomic_tensors(cfg, B, fp32=False):
    """Prefixes of the gradient tensors that the library accumulates with FLOAT ATOMICS from more than two workgroups, read off its launches:
    their bits depend on the order in which workgroups retire, so two runs of one context may or may not agree (when they do it is luck: a
    rule that asks the twin to reproduce itself first is decided by chance for them).  Every other tensor is reduced in a fixed order."""
    out = []
    if cfg.input_type == 'mulaw-quantize':
        out.append('input_convolution/kernel')                         # the row scatter by class id (wn_first_conv_bwd_ids)
    if cfg.upsample_type in ('Resize', '1D'):
        out.append('local_conditioning_upsampling')                    # wn_up_bwd_params_generic
    if cfg.gin_channels > 0 and cfg.use_speaker_embedding:
        out.append('gc_embedding')                                     # the scatter into the speaker's row (wn_gin_dg_kernel)
    if not fp32 and B > 2:      # the per-layer kernel wn_wgrad_kernel adds one tile per utterance (T <= its slab of 4096): 0 + a + b is ordered, three addends are not
        if cfg.residual_channels % 128 != 0:
            out.append('ResidualConv1DGLU_')                           # narrow models: no grouped kernel (wn_wgrad_v2_ok)
        if cfg.out_channels > 128 or cfg.skip_out_channels % 8 != 0 or cfg.residual_channels % 128 != 0:
            out.append('final_convolution')                            # the head on the same kernel (wgrad_heads_ok: O > 128; the 64-channel models are left to (a) with their stack)
    return tuple(out)


def twin_check(tag, m, d, lengths, seed, mine_snap, mine_grads, mine_yhat, snap_fn, grad_buckets=None, fp32=False):
    """A fresh context of the same size runs only this step: element-wise buffers byte-identical.  Gradients: the twin runs the step twice.
    Every tensor that is reduced in a fixed order must come out with the same bits from both of its runs AND from the reused context; the
    tensors of atomic_tensors() are left to the launch-local check, and the test says which.  Returns (buffers compared, tensors compared)."""
    twin = m.engine(grad_buckets=grad_buckets)
    try:
        _, y1, g1 = run_step(m, twin, d, lengths, seed)
        n = assert_same_bits(tag, mine_snap, snap_fn(twin, m.cfg, d['B'], d['T']))
        assert torch.equal(_bits(mine_yhat), _bits(y1)), '%s: y_hat of the reused context differs from the twin context' % tag
        _, _, g2 = run_step(m, twin, d, lengths, seed)
        a, b1, b2 = download_grads(twin, mine_grads), download_grads(twin, g1), download_grads(twin, g2)
        atomic = atomic_tensors(m.cfg, d['B'], fp32)
        if atomic and m.cfg.wavenet_weight_normalization:      # (d v, d g mix the effective gradients of a whole tensor, and the clip-free mapping is shared: all to (a))
            atomic = ('',)
        left, compared, far, spread = [], 0, 0.0, 0.0
        for k in a:
            if atomic and k.startswith(atomic):
                if not torch.equal(_bits(b1[k]), _bits(b2[k])) or not torch.equal(_bits(a[k]), _bits(b1[k])):
                    left.append(k)
                    far, spread = max(far, rel_err(a[k], b1[k])), max(spread, rel_err(b2[k], b1[k]))
                continue
            assert torch.equal(_bits(b1[k]), _bits(b2[k])), '%s: %s is reduced in a fixed order, yet two runs of the twin context differ (rel-L2 %.3e)' % (tag, k, rel_err(b2[k], b1[k]))
            assert torch.equal(_bits(a[k]), _bits(b1[k])), '%s: %s of the reused context differs from the twin context, which reproduces its own bits (rel-L2 %.3e)' % (
                tag, k, rel_err(a[k], b1[k]))
            compared += 1
        if not atomic:
            assert compared == len(a) > 0, (tag, compared, len(a))      # (nothing accumulated with atomics: every tensor was held to the twin's bits)
        # a record, not a threshold: two draws of an atomic sum can agree by luck, so the twin's own spread bounds nothing (the launch-local check holds these to float64)
        print('[%s] gradients: %d of %d tensors bit-identical with the twin context (and the twin with itself)%s' % (tag, compared, len(a), '' if not atomic else
              '; %d accumulated with float atomics are left to the launch-local check, %d of them differ between the three runs: worst rel-L2 reused vs twin %.1e, twin vs twin %.1e' % (
                  len(a) - compared, len(left), far, spread)))
        return n, compared
    finally:
        twin.close()


def checked_step(m, eng, label, geom, stale, seed, grad_buckets=None):
    """Poison (nan mode), run the step, (a) and, in live mode, (b)."""
    B, T, lengths = geom
    tag = '%s %s %s B=%d T=%d' % (m.name, stale, label, B, T)
    d = m.data(B, T, DATA_SEED)
    if stale == 'nan':
        eng.poison_workspace()
    loss, yhat, grads = run_step(m, eng, d, lengths, seed)
    snap = snapshot(eng, m.cfg, B, T) if stale == 'live' else None
    check_step(tag, eng, m.cfg, m.params, B, T, lengths, seed, d['x_in'], d['y_or'], d['c'], grads, g=d['g'])      # (first: its report names the launch)
    assert_finite(tag, loss, yhat, grads)
    if stale == 'live':
        n, _ = twin_check(tag, m, d, lengths, seed, snap, grads, yhat, snapshot, grad_buckets=grad_buckets)      # (tensors compared: printed there)
        assert n >= 5 * m.cfg.layers + 8      # (the element-wise half of (b) ran, on every buffer)
    return d, grads


REUSE_CONFIGS = ['paper_width_drop', 'wide', 'gauss_subpixel', 'mol_gin_embed', 'softmax_c1', 'mol_weightnorm', 'mol_resize', 'gauss_1d', 'gauss_cdf_nn']


@pytest.mark.parametrize('stale', ['live', 'nan'])
@pytest.mark.parametrize('name', REUSE_CONFIGS)
def test_steps_on_a_reused_larger_context(name, stale):
    """S1 = 7 x 656 on a context of (7, 656), then S2 .. S5 with the checks of the module docstring after each."""
    from wavenet_vocoder import _ext
    m = Model(name)
    eng = m.engine()
    try:
        if stale == 'nan' and name == 'paper_width_drop':
            eng.poison_workspace()      # (once on the fresh context too: the hook before anything has run)
        B, T, lengths = S1
        d1 = m.data(B, T, S1_DATA_SEED)
        loss, yhat, grads = run_step(m, eng, d1, lengths, DROP_SEED)
        assert_finite('%s %s S1' % (name, stale), loss, yhat, grads)
        if m.cfg.gin_channels > 0:      # a step whose B is not the B of the last wn_set_global_condition is refused, not run on S1's table
            B2, T2, len2 = S2
            d2 = m.data(B2, T2, DATA_SEED)
            with pytest.raises(_ext.WnError) as ei:
                run_step(m, eng, d2, len2, DROP_SEED + 1, set_g=False)
            assert ei.value.code == -5 and 'wn_set_global_condition' in str(ei.value)
        for i, (label, geom) in enumerate(STEPS):
            checked_step(m, eng, label, geom, stale, DROP_SEED + 1 + i)
    finally:
        eng.close()


@pytest.mark.parametrize('stale', ['live', 'nan'])
def test_validation_forward_between_training_steps(stale):
    """S1 train, wn_eval_fwd at the S2 geometry (forward checks with the gate reading X), then S3 train with the full checks: the XD and DY
    of S1 need not survive the evaluation, and S3 must not see them."""
    m = Model('paper_width_drop')
    eng = m.engine()
    try:
        B, T, lengths = S1
        loss, yhat, grads = run_step(m, eng, m.data(B, T, S1_DATA_SEED), lengths, DROP_SEED)
        assert_finite('validation %s S1' % stale, loss, yhat, grads)
        B, T, lengths = S2
        d = m.data(B, T, DATA_SEED)
        if stale == 'nan':
            eng.poison_workspace()
        stats = torch.full((B, 3), float('nan'), device='cuda')
        nll = torch.full((B, T), float('nan'), device='cuda')
        yh = torch.full((B, m.cfg.out_channels, T), float('nan'), device='cuda')
        eng.eval_fwd(d['x_dev'], d['c'].cuda(), d['y_dev'], torch.tensor(lengths, dtype=torch.int32).cuda(), stats, nll, yh)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(nll).all()) and bool(torch.isfinite(yh).all())
        check_forward('validation %s eval B=%d T=%d' % (stale, B, T), eng, m.cfg, m.params, B, T, 0, d['x_in'], d['c'], eval_mode=True, x_checks=True)
        checked_step(m, eng, 'S3', S3, stale, DROP_SEED + 2)
    finally:
        eng.close()


@pytest.mark.parametrize('stale', ['live', 'nan'])
def test_gradient_buckets_on_a_reused_context(stale):
    """grad_buckets = 3 (two early layer groups under the chain): at S2 and S3 on the reused context a side stream that waits for bucket i
    only sees finite values that are the final bits, and the steps pass the full checks."""
    m = Model('paper_width_drop')
    eng = m.engine(grad_buckets=3)
    try:
        buckets = eng.grad_buckets()
        assert len(buckets) == 4 and sum(n for _, n in buckets) == eng.n_params
        B, T, lengths = S1
        loss, yhat, grads = run_step(m, eng, m.data(B, T, S1_DATA_SEED), lengths, DROP_SEED)
        assert_finite('buckets %s S1' % stale, loss, yhat, grads)
        side = torch.cuda.Stream()
        for i, (label, geom) in enumerate([('S2', S2), ('S3', S3)]):
            B, T, lengths = geom
            d = m.data(B, T, DATA_SEED)
            if stale == 'nan':
                eng.poison_workspace()
            loss = torch.zeros(1, device='cuda')
            grads = torch.full((eng.n_params,), float('nan'), device='cuda')
            eng.train_fwd(d['x_dev'], d['c'].cuda(), d['y_dev'], torch.tensor(lengths, dtype=torch.int32).cuda(), DROP_SEED + 1 + i, loss)
            eng.train_bwd(grads)
            snaps = []
            for k, (off, n) in enumerate(buckets):
                eng.wait_bucket(k, side)
                with torch.cuda.stream(side):
                    snaps.append(grads[off:off + n].clone())
            torch.cuda.synchronize()
            for k, ((off, n), s) in enumerate(zip(buckets, snaps)):
                assert bool(torch.isfinite(s).all()), 'bucket %d of %s is not finite after wn_bwd_wait_bucket' % (k, label)
                assert torch.equal(_bits(s), _bits(grads[off:off + n])), 'bucket %d of %s was not final after wn_bwd_wait_bucket' % (k, label)
            checked_step(m, eng, label, geom, stale, DROP_SEED + 1 + i, grad_buckets=3)      # (the same step again, with the full checks)
    finally:
        eng.close()


@pytest.mark.parametrize('stale', ['live', 'nan'])
def test_fp32_mode_steps_on_a_reused_larger_context(stale):
    """The fp32 compute mode (mol_2d) through S1, S2, S5.  It has no launch-local reference: a twin context that runs only the step judges
    y_hat, the fp32 debug copies X / U / Z / SK / H1 and every gradient tensor, bit for bit (this configuration accumulates nothing with
    float atomics: the twin must reproduce its own bits and the reused context must give the same).  Everything is finite, in both modes."""
    m = Model('mol_2d', mi355_compute_dtype='fp32')
    eng = m.engine()
    try:
        B, T, lengths = S1
        loss, yhat, grads = run_step(m, eng, m.data(B, T, S1_DATA_SEED), lengths, DROP_SEED)
        assert_finite('fp32 %s S1' % stale, loss, yhat, grads)
        for i, (label, geom) in enumerate([('S2', S2), ('S5', S5)]):
            B, T, lengths = geom
            tag = 'fp32 %s %s B=%d T=%d' % (stale, label, B, T)
            d = m.data(B, T, DATA_SEED)
            if stale == 'nan':
                eng.poison_workspace()
            loss, yhat, grads = run_step(m, eng, d, lengths, DROP_SEED + 1 + i)
            assert_finite(tag, loss, yhat, grads)
            snap = snapshot_f32(eng, m.cfg, B, T)
            for k, v in snap.items():
                assert bool(torch.isfinite(v.view(torch.float32)).all()), '%s: %s has non-finite elements' % (tag, k)
            n, compared = twin_check(tag, m, d, lengths, DROP_SEED + 1 + i, snap, grads, yhat, snapshot_f32, fp32=True)
            assert n == 3 * m.cfg.layers + 2 and compared == len(eng.layout)      # (nothing of this configuration is accumulated with atomics: every tensor, bit for bit)
    finally:
        eng.close()


def test_poison_hook_forgets_the_last_forward_and_refuses_inference_contexts():
    from wavenet_vocoder import _ext
    m = Model('mol_2d')
    eng = m.engine()
    try:
        B, T, lengths = S4
        d = m.data(B, T, DATA_SEED)
        loss = torch.zeros(1, device='cuda')
        eng.train_fwd(d['x_dev'], d['c'].cuda(), d['y_dev'], torch.tensor(lengths, dtype=torch.int32).cuda(), DROP_SEED, loss)
        eng.poison_workspace()
        with pytest.raises(_ext.WnError) as ei:      # a backward on poisoned buffers is refused
            eng.train_bwd(torch.empty(eng.n_params, device='cuda'))
        assert ei.value.code == -5
        torch.cuda.synchronize()
        assert not bool(torch.isfinite(eng.debug_copy('U', 0, MAXB * MAXT, m.cfg.gate_channels // 2)).any())      # the whole slab, not B * T rows
        assert bool(torch.isfinite(eng.debug_copy('PARAMS', 0, 1, eng.n_params)).all()) and bool(torch.isfinite(eng.debug_copy('B1SUM', 0, m.cfg.layers, m.cfg.gate_channels)).all())
        assert bool(torch.isfinite(eng.debug_copy('SKIPB', 0, 1, m.cfg.skip_out_channels)).all())      # (zero page, scalars and score partials: the nan-mode steps and the validation case rest on them)
    finally:
        eng.close()
    inf = _ext.Engine(m.hp, 1, 64, inference_only=True)
    try:
        with pytest.raises(_ext.WnError) as ei:
            inf.poison_workspace()
        assert ei.value.code == -5 and 'inference-only' in str(ei.value)
    finally:
        inf.close()
