"""Launch-local parity of the forward and the backward chain against the float64 references of tests/launch_ref.py (pytest -m gpu).

Every other GPU test of the backward compares final weight-gradient tensors (sums over all B x T rows) with autograd as a rel-L2 per
tensor (1.4e-2 and wider): a fault confined to a few rows of d z or d h -- a tap that reads the next utterance at an utterance end, a
skipped tail tile, a keep-mask off by one element, a wrong b0 offset of the second stream -- is averaged away before anything is
compared.  Here one ordinary training step runs through the engine, and then EVERY buffer a launch wrote is compared with the
reference of that launch applied to the device's OWN inputs of that launch, element by element, every element, no exclusions:

    |dev - ref| <= 2^-8 |ref| + K 2^-23 A + E          (terms derived in launch_ref.py, launch by launch; nothing is fitted)

and exactly 0 where reference and operands are 0 (rows past a ragged length, GX[L], the masked half of EPI_MASK_STORE).  XD[l] is
bit-exact.  DY: 2^-8 |ref| + 8 x the max-abs distance between the float32 and the float64 evaluation of the same oracle gradient on the
same YHAT (measured on the CPU inside the test).

Weight-gradient tensors are sums over all rows, where a worst-case bound is useless.  Their tolerance is a yardstick measured on the
reference, in the test, per tensor: the same contraction of the same downloaded buffers in float32 with one running accumulator over
128-row blocks in row order, against float64 (floored at 2^-24, the final rounding of any float32 result: WGRAD_YARD_FLOOR in launch_report.py).  The
device gets 8 x that rel-L2 (different summation tree, float atomics between splits) and never more than 1e-5 (a condition, not a measurement: one wrong row in 22 000, all rows agreeing in sign, is 4.5e-5).  A
tensor whose reference is all zeros (the top layer's W_out) must be exact zeros.  With weight normalisation the tensors compared are the
effective-kernel gradients the launches wrote (wn_debug_copy 'DEFF'), not the d v / d g of the flat buffer (those: test_hip_weightnorm.py).  The upsample-net gradients: float64 backward of
O.upsample from the device's DC, yardstick = the float32 backward.

Per launch kind and layer the test prints the largest err / bound, the rel-L2 and where the worst element is (the small sweep engines:
per launch kind, with the worst layer; WN_LAUNCH_LOCAL_DETAIL=1 prints every layer there too); on failure it names
launch, layer, utterance, t, channel, tile index (row // 128) and whether the row is within 2 d of an utterance end.  For GX[l] the
last 2 d rows of every utterance and the first 2 d rows of the next one are their own group ('GX edge'), and the tap gradients must be
closer to the reference than HALF of what a read across the utterance start would add ('taps leak'), so a leak across b shows by name.
The printed ratios are records, not thresholds.

The forward chain (check_forward; check_step runs it first, and the backward checks then rest on checked TS / U / R1 / H2 / cbt): CUP0..n
(every upsample level from the device's own input of that level), cbt (bit-exact from the device's last level), per layer TS and U (from
the device's XD[l] -- X[l] with dropout 0 and under wn_eval_fwd -- and cbt, with the fp32 gate bias restated from the parameters), R1 (the
device's U of all layers), H2 (the device's R1), YHAT (the device's H2; fp32, exactly O channels), same form of bound, no exclusions.
'U start' is the forward twin of 'GX edge': the first 2d rows of every utterance b >= 1 and the rows of a partial last tile; 'start leak'
holds |U dev - ref| on those first rows below HALF of what reading the previous utterance's last rows would add to U."""
import numpy as np
import pytest
import torch

import launch_ref as LR
import wnorm_ref as WR
from launch_report import WGRAD_CAP, WGRAD_FACTOR, WGRAD_YARD_FLOOR, Report      # noqa: F401  (the report and its constants: a plain module, CPU-tested)
from hip_util import SMALL, download_grads, dropout_mask_rows, make_hp, oracle_cfg, synth_batch, upload_params
from oracle import wavenet_oracle as O
from test_hip_bench_geometry import C5, PAPER
from test_hip_parity import _run_fwd
from test_hip_round6 import GEOMETRIES

pytestmark = pytest.mark.gpu


def _edge_group(B, T, d):
    """1 on the last 2d rows of every utterance and the first 2d rows of the next one."""
    g = torch.zeros(B, T, 1, dtype=torch.float64)
    n = min(2 * d, T)
    g[:, T - n:] = 1.0
    g[1:, :n] = 1.0
    return g


def _start_group(B, T, d):
    """1 on the first 2d rows of every utterance b >= 1 and on the rows of a partial last time tile (128- and 64-row tiles)."""
    g = torch.zeros(B, T, 1, dtype=torch.float64)
    g[1:, :min(2 * d, T)] = 1.0
    for tile in (128, 64):
        if T % tile:
            g[:, T - T % tile:] = 1.0
    return g


def check_forward(tag, eng, cfg, params, B, T, seed, x_in, c_in, g=None, chain_layers=None, detail=False, eval_mode=False, x_checks=True, rep=None):
    """The buffers the forward launches wrote (after train_fwd, or after eval_fwd with eval_mode=True: the gate then staged X and nothing wrote
    XD) against launch_ref, every element, each launch from the device's OWN inputs of that launch, one layer resident at a time:
    CUP0..n, cbt (exact), per layer in chain_layers TS / U (+ 'U start': the first 2d rows of the utterances b >= 1 and the rows of a partial
    last tile; there the device must also be closer to the reference than HALF of what reading the previous utterance's rows would add to U),
    R1 (always all layers), H2, YHAT (exactly O channels).  x_checks: X0 and X_next too (check_step has them in its own loop).
    rep: a Report to add to (the caller finishes it); otherwise a new one, finished here."""
    L, R, G, S, C = cfg.layers, cfg.residual_channels, cfg.gate_channels, cfg.skip_out_channels, cfg.cin_channels
    GH, Oc = G // 2, cfg.out_channels
    n = B * T
    chain_layers = set(range(L)) if chain_layers is None else set(chain_layers)
    W = LR.Weights(params, cfg, rounded=True)
    own = rep is None
    rep = Report(tag, B, T, detail) if own else rep
    p = float(cfg.wavenet_dropout)
    dropped = p > 0 and not eval_mode
    w_ulps = 8 if cfg.wavenet_weight_normalization else 0      # (both sides compute v g / ||v|| in fp32: launch_ref.ref_x0)

    def dl(name, l, ch):
        return eng.debug_copy(name, l, n, ch).cpu().double().view(B, T, ch)

    # ---- upsample net: every level from the device's own input of that level; cbt from the device's own last level
    nearest = cfg.upsample_type == 'NearestNeighbor'
    inp = c_in.double()
    for i in range(1 if nearest else len(cfg.upsample_scales)):
        Tout = inp.shape[-1] * (cfg.hop if nearest else cfg.upsample_scales[i])
        dev = eng.debug_copy('CUP', i, B * C, Tout).cpu().double().view(B, C, Tout)
        ref, bound = LR.ref_cup_level(params, cfg, i, inp, True, w_ulps=w_ulps)
        rep.elementwise('CUP%d' % i, 0, dev.permute(0, 2, 1), ref.permute(0, 2, 1), bound.permute(0, 2, 1))      # (reported as utterance : t at that level : frequency)
        inp = dev
    assert inp.shape[-1] == T
    cbt = dl('cbt', 0, C)
    rep.exact('cbt', 0, cbt, LR.ref_cbt(inp))
    rep.flush('upsample')
    del inp
    # ---- the gate bias (b1sum / gbias are not downloadable: float64 from the parameters, with the error of the device's fp32 sums)
    gvec = None
    if g is not None:
        gvec = params['gc_embedding'][g.long()] if cfg.use_speaker_embedding else g
    bias, ebias = LR.ref_gate_bias(W, params, cfg, gvec, w_ulps=w_ulps)
    # ---- layers
    for l in range(L):
        if l not in chain_layers:
            continue
        d = W.dil[l]
        XD = dl('XD' if dropped else 'X', l, R)
        TS, U = dl('TS', l, GH), dl('U', l, GH)
        zs = []
        (rTS, rU), (bTS, bU) = LR.ref_gate(W, l, XD, cbt, (bias[l], ebias[l]), True, z_out=zs)
        rep.elementwise('TS', l, TS, rTS, bTS, d)
        rep.elementwise('U', l, U, rU, bU, d)
        grp = _start_group(B, T, d)
        rep.elementwise('U start', l, U, rU, bU, d, group=grp)
        if B > 1:      # a tap that read across the utterance start would move U by `leak` on the first 2d rows: the device must be far closer than that
            z = zs[0] + LR.gate_start_leak(W, l, XD)
            nrow = min(2 * d, T)
            leak = float((torch.tanh(z[1:, :nrow, :GH]) * torch.sigmoid(z[1:, :nrow, GH:]) - rU[1:, :nrow]).norm())
            err = float((U[1:, :nrow] - rU[1:, :nrow]).norm())
            rep._note('start leak', l, err / leak if leak > 0 else 0.0, 'start leak %.1e/%.1e' % (err, leak))
            if leak > 0 and not err < 0.5 * leak:
                rep.fail.append('[%s] start leak layer %d (d = %d): |U dev - ref| = %.3e on the first 2d rows of the utterances b >= 1 is not below half of what reading the '
                                'previous utterance adds (%.3e)' % (tag, l, d, err, leak))
            del z
        del zs, rTS, rU, bTS, bU, TS
        if x_checks:
            X = dl('X', l, R)
            if l == 0:
                rep.elementwise('X0', 0, X, *LR.ref_x0(W, x_in, True, w_ulps=w_ulps))
            if l < L - 1:
                rep.elementwise('X_next', l, dl('X', l + 1, R), *LR.ref_x_next(W, l, U, X, True))
            if dropped:
                m = torch.from_numpy(dropout_mask_rows(seed, l, 0, n, R, p)).double().view(B, T, R)
                rep.exact('XD', l, XD, LR.ref_xd(W, X, m))
            del X
        del XD, U
        rep.flush('L%02d fwd' % l)
    # ---- skip sum (all layers, one resident at a time) and head, each from the device's own input
    R1 = dl('R1', 0, S)
    rep.elementwise('R1', 0, R1, *LR.ref_r1(W, (dl('U', l, GH) for l in range(L)), True))
    H2 = dl('H2', 0, S)
    rep.elementwise('H2', 0, H2, *LR.ref_h2(W, R1, True))
    yhat = eng.debug_copy('YHAT', 0, B * Oc, T).cpu().double().view(B, Oc, T)
    ref, bound = LR.ref_yhat(W, H2, True)
    assert tuple(ref.shape) == (B, Oc, T)
    rep.elementwise('YHAT', 0, yhat.permute(0, 2, 1), ref.permute(0, 2, 1), bound.permute(0, 2, 1))
    rep.flush('fwd tail')
    if own:
        rep.finish()
    return rep


def check_step(tag, eng, cfg, params, B, T, lengths, seed, x_in, y_or, c_in, grads_flat, g=None, chain_layers=None, wgrad_layers=None, wgrads=True, detail=False):
    """The device's buffers after one train_fwd + train_bwd against launch_ref, one layer resident at a time: the forward launches
    (check_forward), then the backward chain."""
    L, R, G, S, C = cfg.layers, cfg.residual_channels, cfg.gate_channels, cfg.skip_out_channels, cfg.cin_channels
    GH, Oc = G // 2, cfg.out_channels
    ldDY = (Oc + 15) // 16 * 16
    n = B * T
    chain_layers = set(range(L)) if chain_layers is None else set(chain_layers)
    wgrad_layers = (set(range(L)) if wgrad_layers is None else set(wgrad_layers)) if wgrads else set()
    W = LR.Weights(params, cfg, rounded=True)
    rep = Report(tag, B, T, detail)
    p = float(cfg.wavenet_dropout)
    g_dev, eff_params = {}, params
    if wgrads and not cfg.wavenet_weight_normalization:
        g_dev = download_grads(eng, grads_flat)
    elif wgrads:
        # weight normalisation: the flat buffer holds d v, d g (tests/test_hip_weightnorm.py maps them back).  What the GEMMs wrote are the gradients
        # of the EFFECTIVE tensors, the context's 'DEFF' (effective layout); the device's own effective parameters feed the gin / upsample references
        lay, n_eff = WR.effective_layout(eng.layout)
        deff, peff = (eng.debug_copy(nm, 0, 1, n_eff).cpu().view(-1) for nm in ('DEFF', 'PARAMS'))
        g_dev = {k: deff[off:off + int(np.prod(shape))].view(*shape).clone() for k, (shape, off) in lay.items()}
        eff_params = {k: peff[off:off + int(np.prod(shape))].view(*shape).clone() for k, (shape, off) in lay.items()}
    check_forward(tag, eng, cfg, params, B, T, seed, x_in, c_in, g=g, chain_layers=chain_layers, x_checks=False, rep=rep)      # (X0 / X_next / XD: in the loop below)

    def dl(name, l, ch):
        return eng.debug_copy(name, l, n, ch).cpu().double().view(B, T, ch)

    def mask(l):
        return torch.from_numpy(dropout_mask_rows(seed, l, 0, n, R, p)).double().view(B, T, R) if p > 0 else None

    def tensors(label, l, refs, flush=True):
        for k, (r, y) in refs.items():
            if k in g_dev:
                rep.tensor(k, l, g_dev[k], r, y)
        if flush:
            rep.flush(label)

    # ---- loss: DY from the device's own YHAT
    yhat = eng.debug_copy('YHAT', 0, B * Oc, T).cpu().view(B, Oc, T)
    DY = dl('DY', 0, ldDY)
    if ldDY > Oc:
        assert float(DY[..., Oc:].abs().max()) == 0.0, 'DY padding columns must be 0'
    dy64 = LR.ref_dy(cfg, yhat, y_or, lengths, torch.float64)
    dy32 = LR.ref_dy(cfg, yhat, y_or, lengths, torch.float32).double()
    e32 = float((dy32 - dy64).abs().max())
    scored = (torch.arange(T)[None, :] < (torch.as_tensor(lengths)[:, None] - 1)).double()[..., None]      # prediction t is scored against sample t + 1 < length
    assert float((dy64 * (1 - scored)).abs().max()) == 0.0
    rep.elementwise('DY', 0, DY[..., :Oc], dy64, LR.BF * dy64.abs() + 8.0 * e32 * scored)      # (rows that are not scored: exactly 0)
    del dy64, dy32, yhat
    # ---- head
    H2, R1, DPRE1, DSKIP = dl('H2', 0, S), dl('R1', 0, S), dl('DPRE1', 0, S), dl('DSKIP', 0, S)
    rep.elementwise('DPRE1', 0, DPRE1, *LR.ref_dpre1(W, DY, H2, True))
    rep.elementwise('DSKIP', 0, DSKIP, *LR.ref_dskip(W, DPRE1, R1, True))
    rep.flush('head')
    if wgrads:
        tensors('head wg', 0, LR.ref_wgrads_head(W, R1, H2, DPRE1, DY, True))
    del H2, R1, DPRE1, DY
    cbt = dl('cbt', 0, C) if wgrad_layers else None
    # ---- the chain, top to bottom; one layer's buffers resident at a time
    GX_up = dl('GX', L, R)
    assert float(GX_up.abs().max()) == 0.0, 'GX[L] (the dead residual branch of the top layer) must be zero-filled'
    dc = None
    want_dc = cfg.upsample_type != 'NearestNeighbor'
    colsums, colsums32 = [], []
    for l in range(L - 1, -1, -1):
        d = W.dil[l]
        DZ = dl('DZ', l, G)
        if want_dc:
            dc = LR.ref_dc_accumulate(W, l, DZ, dc, True)
        if g is not None:
            colsums.insert(0, DZ.sum(1))
            a32, z32 = torch.zeros(B, G), DZ.float()
            for r0 in range(0, T, 128):
                a32 += z32[:, r0:r0 + 128].sum(1)
            colsums32.insert(0, a32)
            del z32
        GX = dl('GX', l, R)
        if l in chain_layers or l in wgrad_layers:
            TS, U = dl('TS', l, GH), dl('U', l, GH)
        if l in chain_layers:
            rep.elementwise('DZ', l, DZ, *LR.ref_dz(W, l, GX_up, DSKIP, TS, U, True))
            m = mask(l)
            ref, bound = LR.ref_gx(W, l, DZ, m, GX_up if l < L - 1 else None, True)
            rep.elementwise('GX', l, GX, ref, bound, d)
            rep.elementwise('GX edge', l, GX, ref, bound, d, group=_edge_group(B, T, d))
            del ref, bound
            X = dl('X', l, R)
            rep.exact('XD', l, dl('XD', l, R), LR.ref_xd(W, X, m))
            if l == 0:
                rep.elementwise('X0', 0, X, *LR.ref_x0(W, x_in, True, w_ulps=8 if cfg.wavenet_weight_normalization else 0))
            if l < L - 1:
                rep.elementwise('X_next', l, dl('X', l + 1, R), *LR.ref_x_next(W, l, U, X, True))
            del X, m
            rep.flush('L%02d d=%d' % (l, d))
        if l in wgrad_layers:
            XD = dl('XD', l, R)
            refs = LR.ref_wgrads_layer(W, l, XD, cbt, DZ, U, DSKIP, GX_up, True)
            tensors('L%02d wg' % l, l, refs, flush=False)
            if B > 1:      # a tap that read across the utterance start would add `leak`: the device must be far closer to the reference than that
                k = 'ResidualConv1DGLU_%d/residual_block_causal_conv/kernel' % l
                leak = float(LR.taps_leak(W, l, XD, DZ).norm())
                err = float((g_dev[k].double() - refs[k][0]).norm())
                rep._note('taps leak', l, err / leak if leak > 0 else 0.0, 'taps leak %.1e/%.1e' % (err, leak))      # |dev - ref| / |what a read across the utterance start adds|
                if leak > 0 and not err < 0.5 * leak:
                    rep.fail.append('[%s] taps leak layer %d (d = %d): |dev - ref| = %.3e is not below half of what reading across the utterance start adds (%.3e)' % (tag, l, d, err, leak))
            rep.flush('L%02d wg' % l)
            del XD, refs
        GX_up = GX
    if want_dc:
        DC = eng.debug_copy('DC', 0, B * C, T).cpu().double().view(B, C, T).permute(0, 2, 1)
        rep.elementwise('DC', 0, DC, dc[0], LR.dc_bound(W, dc, G))
        rep.flush('d c')
    if wgrads:
        tensors('input wg', 0, LR.ref_wgrads_input(W, x_in, GX_up, True))
        if g is not None:
            ids = g.long() if cfg.use_speaker_embedding else None
            gvec = eff_params['gc_embedding'][ids] if ids is not None else g
            r64 = LR.ref_wgrads_gin(eff_params, cfg, gvec, ids, colsums, torch.float64)
            r32 = LR.ref_wgrads_gin(eff_params, cfg, gvec, ids, colsums32, torch.float32)      # yardstick: float32 column sums (128-row blocks in row order) through the float32 contraction
            tensors('gin wg', 0, {k: (r64[k], float((r32[k].double() - r64[k]).norm()) / max(float(r64[k].norm()), 1e-300)) for k in r64})
        if want_dc:      # upsample net: float64 backward of O.upsample from the device's DC; yardstick = the float32 backward
            up = {}
            for dt in (torch.float64, torch.float32):
                leaf = {k: v.to(dt).clone().requires_grad_(True) for k, v in eff_params.items() if k.startswith('local_conditioning')}
                out = O.upsample(leaf, cfg, c_in.to(dt))
                out.backward(DC.permute(0, 2, 1).to(dt))
                up[dt] = {k: v.grad.double() for k, v in leaf.items()}
            tensors('up wg', 0, {k: (r, float((up[torch.float32][k] - r).norm()) / max(float(r.norm()), 1e-300)) for k, r in up[torch.float64].items()})
    rep.finish()
    return rep


# ------------------------------------------------------------------------------------------------------------------ small configurations
SMALL_CONFIGS = ['paper_width_drop', 'wide', 'mol_2d', 'gauss_subpixel', 'mol_2d_legacy_drop', 'mol_gin_embed', 'mol_nobias', 'softmax_c1', 'mol_weightnorm', 'gauss_weightnorm_gin_nobias']


@pytest.mark.parametrize('name', SMALL_CONFIGS)
def test_launch_local_geometry_sweep(name):
    """The six batch / time geometries of the tile-boundary sweep x one configuration, all layers, every launch."""
    for B, T, lengths in GEOMETRIES:
        r = _run_fwd(name, B=B, T=T, lengths=lengths)
        cfg, eng = r['cfg'], r['eng']
        assert r['T'] == T
        grads = torch.empty(eng.n_params, device='cuda')
        eng.train_bwd(grads)
        torch.cuda.synchronize()
        quant = cfg.input_type == 'mulaw-quantize'
        x_in = r['y_or'] if quant else r['x_or'].view(B, T)
        try:
            check_step('%s B=%d T=%d' % (name, B, T), eng, cfg, r['params'], B, T, lengths, r['seed'], x_in, r['y_or'], r['c'], grads, g=r['g'])
        finally:
            eng.close()


def _x_in(r):
    return r['y_or'] if r['cfg'].input_type == 'mulaw-quantize' else r['x_or'].view(r['B'], r['T'])


@pytest.mark.parametrize('name', ['mol_resize_odd', 'gauss_1d', 'gauss_cdf_nn'])
def test_launch_local_forward_upsample_types(name):
    """The three upsamplers SMALL_CONFIGS lacks (Resize with odd scales, 1D, NearestNeighbor) at B = 3, T = the smallest multiple of the hop
    above 128 that is no multiple of 128 (144 at hop 16, 150 at hop 15), lengths [T, 129, 2]: the forward checks inside the full check_step."""
    from test_hip_parity import CONFIGS
    hop = int(np.prod(dict(SMALL, **CONFIGS[name])['upsample_scales']))
    T = {16: 144, 15: 150}[hop]
    assert T % hop == 0 and T > 128 and T % 128 != 0
    B, lengths = 3, [T, 129, 2]
    r = _run_fwd(name, B=B, T=T, lengths=lengths)
    cfg, eng = r['cfg'], r['eng']
    assert r['T'] == T
    try:
        grads = torch.empty(eng.n_params, device='cuda')
        eng.train_bwd(grads)
        torch.cuda.synchronize()
        check_step('%s B=%d T=%d' % (name, B, T), eng, cfg, r['params'], B, T, lengths, r['seed'], _x_in(r), r['y_or'], r['c'], grads, g=r['g'], detail=True)
    finally:
        eng.close()


@pytest.mark.parametrize('B,T,lengths', [(3, 144, [144, 129, 2]), (5, 272, [272, 256, 255, 130, 16])])
@pytest.mark.parametrize('name', ['paper_width_drop', 'mol_2d_legacy_drop'])
def test_launch_local_eval_forward(name, B, T, lengths):
    """wn_eval_fwd reuses the forward launches with other host arguments (the gate stages X, nothing writes XD).  After a train_fwd (whose XD
    and DY are snapshotted) an eval_fwd on the same inputs: the forward checks hold with the gate reading X, X0 / X_next hold, XD (and DY) are
    byte-identical to the snapshot, and the per-sample NLL it returns is wn_score's on the device's own YHAT, bit for bit."""
    r = _run_fwd(name, B=B, T=T, lengths=lengths)
    cfg, eng = r['cfg'], r['eng']
    assert r['T'] == T and cfg.wavenet_dropout > 0 and cfg.input_type == 'raw'
    L, R, Oc = cfg.layers, cfg.residual_channels, cfg.out_channels
    ldDY = (Oc + 15) // 16 * 16
    try:
        snap = [eng.debug_copy('XD', l, B * T, R).cpu() for l in range(L)]
        dy = eng.debug_copy('DY', 0, B * T, ldDY).cpu()
        assert any(not torch.equal(snap[l], eng.debug_copy('X', l, B * T, R).cpu()) for l in range(L))      # (the training forward did drop)
        ln = torch.tensor(lengths, dtype=torch.int32, device='cuda')
        stats = torch.full((B, 3), float('nan'), device='cuda')
        nll = torch.full((B, T), float('nan'), device='cuda')
        yh = torch.full((B, Oc, T), float('nan'), device='cuda')
        eng.eval_fwd(r['x_or'].cuda(), r['c'].cuda(), r['y_or'].cuda(), ln, stats, nll, yh)
        torch.cuda.synchronize()
        check_forward('%s eval B=%d T=%d' % (name, B, T), eng, cfg, r['params'], B, T, r['seed'], _x_in(r), r['c'], g=r['g'], eval_mode=True, x_checks=True)
        for l in range(L):
            assert torch.equal(snap[l].view(torch.int32), eng.debug_copy('XD', l, B * T, R).cpu().view(torch.int32)), 'eval_fwd wrote XD[%d]' % l
        assert torch.equal(dy.view(torch.int32), eng.debug_copy('DY', 0, B * T, ldDY).cpu().view(torch.int32)), 'eval_fwd wrote DY'
        yhat = eng.debug_copy('YHAT', 0, B * Oc, T).view(B, Oc, T).contiguous()
        assert torch.equal(yhat.view(torch.int32), yh.view(torch.int32))
        st2 = torch.full((B, 3), float('nan'), device='cuda')
        nl2 = torch.full((B, T), float('nan'), device='cuda')
        eng.score(yhat, r['y_or'].cuda(), ln, 1, st2, nl2)
        torch.cuda.synchronize()
        assert torch.equal(nll.cpu().view(torch.int32), nl2.cpu().view(torch.int32)), 'per-sample NLL of eval_fwd != wn_score on the device\'s YHAT'
        assert torch.equal(stats.cpu().view(torch.int32), st2.cpu().view(torch.int32))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ benched geometries
def _big(tag, hp, B, T, lengths, chain_layers=None, wgrad_layers=None, grad_buckets=None, batch_parts=0, seed=1234, expect_8p=None, detail=True):
    from wavenet_vocoder import _ext
    cfg = oracle_cfg(hp)
    assert T % cfg.hop == 0
    eng = _ext.Engine(hp, B, T, grad_buckets=grad_buckets)
    try:
        if expect_8p is not None:
            assert eng.lib.wn_test_gemm8p_mask(eng.h) == expect_8p
        params = O.init_params(cfg, seed=5339, bias_scale=0.05)
        gen = torch.Generator().manual_seed(7)
        for k in params:
            if k.startswith('local_conditioning') and k.endswith('kernel'):
                params[k] = params[k] + 0.02 * torch.randn(params[k].shape, generator=gen)
        eng.pack_weights(upload_params(eng, params))
        if batch_parts:
            eng.set_batch_parts(batch_parts)
        wav, c = synth_batch(cfg, B, T, seed=3)
        loss = torch.zeros(1, device='cuda')
        eng.train_fwd(wav.view(B, 1, T).contiguous().cuda(), c.cuda(), wav.view(B, T, 1).contiguous().cuda(), torch.tensor(lengths, dtype=torch.int32).cuda(), seed, loss)
        grads = torch.empty(eng.n_params, device='cuda')
        eng.train_bwd(grads)
        torch.cuda.synchronize()
        assert np.isfinite(float(loss.item()))
        return check_step(tag, eng, cfg, params, B, T, lengths, seed, wav, wav.view(B, T, 1), c, grads, chain_layers=chain_layers, wgrad_layers=wgrad_layers, detail=detail)
    finally:
        eng.close()


def test_launch_local_c2_b2_two_streams():
    """C2 at B = 2 x 11 000, lengths [11000, 9377], grad_buckets = 3: dilations to 2048, the 11000 % 128 tail tile, one utterance per stream."""
    _big('c2_b2', make_hp(**PAPER), 2, 11000, [11000, 9377], grad_buckets=3)


def test_launch_local_c2_b2_single_stream():
    _big('c2_b2_parts1', make_hp(**PAPER), 2, 11000, [11000, 9377], grad_buckets=3, batch_parts=1, detail=False)      # (same launches as above, other stream order)


def test_launch_local_c2_b2_on_the_8phase_kernel(monkeypatch):
    monkeypatch.setenv('WN_GEMM8P', '3')
    _big('c2_b2_gemm8p', make_hp(**PAPER), 2, 11000, [11000, 9377], grad_buckets=3, expect_8p=3, detail=False)


def test_launch_local_c2_b8_bench_batch():
    """The bench batch: chain at layers {0, 10, 11, 12, 23}, weight gradients of all layers."""
    _big('c2_b8', make_hp(**PAPER), 8, 11000, [11000] * 8, chain_layers=[0, 10, 11, 12, 23])


def test_launch_local_default_hparams_model_b8():
    """hparams.py's own model (20 layers / 2 stacks, R = S = 128, G = 256, Gaussian, SubPixel [11, 25], flags as the file has them)."""
    import hparams as H
    hp = H._build()
    cfg = oracle_cfg(hp)
    assert (cfg.layers, cfg.stacks, cfg.residual_channels, cfg.gate_channels, cfg.out_channels, cfg.upsample_type) == (20, 2, 128, 256, 2, 'SubPixel')
    _big('hparams_b8', hp, 8, 11000, [11000] * 8)


def test_launch_local_c5_width_full_depth():
    _big('c5_b2', make_hp(**C5), 2, 12000, [12000, 12000], chain_layers=[0, 9, 10, 29], wgrad_layers=[0, 9, 10, 29])
