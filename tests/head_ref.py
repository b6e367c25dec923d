"""Float64 references of the two ends of the training step (plain torch, CPU): the loss heads with their gradient (csrc/wn_loss.hip) and the
optimiser (csrc/wn_optim.hip), the recipes that drive every branch of both, and the element-wise checks that tests/test_head_ref_cpu.py applies
to a float32 evaluation of the references and tests/test_hip_heads.py to the device.

Loss heads.  ref_heads restates the oracle's expressions (oracle/wavenet_oracle.py: discretized_mix_logistic_loss, gaussian_mle_loss,
training_loss) and differentiates them with autograd.  Every discrete choice is made the way float32 TensorFlow makes it and enters the float64
arithmetic as a mask:
  * y < -0.999 and y > 0.999 compare the float32 target with the float32 constants (the oracle in float64 widens the target and compares it with
    a double: a target equal to float32(+-0.999) then takes another branch than TensorFlow and the device);
  * the softmax denominator counts the positions whose FLOAT32 loss is non-zero (a target logit 30 above the rest gives exactly 0 in float32 and
    1e-13 in float64);
  * the clamp constants log_scale_min / log_scale_min_gauss are the float32 values the device and TensorFlow hold;
  * cdf_delta > 1e-5, diff >= 1e-12 and lsr >= log_scale_min are decided in the arithmetic's own type (the recipes keep float32 and float64 on
    the same side; a position where they are not is excluded and counted).

Optimiser.  ref_optim works per tensor of the engine's layout (for weight-normalised models the raw v / g variables): clip by norm, clip by
value, TF-Adam on the float32 hyper-parameter values, EMA; and it returns the per-element bound derived in its docstring."""
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24                                 # unit roundoff of float32
BF = 2.0 ** -8                                   # one bf16 store (DY is a bf16 buffer)
FACTOR = 8.0                                     # the project's margin over the float32 yardstick
MAX_EXCLUDED = 0.05
TINY = 2.0 ** -120                               # float32 underflow, see heads_check
# the heads of the validation suite (test_hip_validation.SCORE_HEADS) plus one and WN_MAX_MIX = 16 mixture components
HEADS = {
    'mol_65536': dict(out_channels=30, quantize_channels=65536, log_scale_min=-7.0),
    'mol_256': dict(out_channels=30, quantize_channels=256, log_scale_min=-7.0),
    'gauss_pdf': dict(out_channels=2, log_scale_min_gauss=float(np.log(1e-7))),
    'gauss_cdf': dict(out_channels=2, cdf_loss=True, log_scale_min_gauss=float(np.log(9.1188196e-4))),
    'softmax': dict(input_type='mulaw-quantize', out_channels=256, quantize_channels=256),
    'mol_m1': dict(out_channels=3, quantize_channels=65536, log_scale_min=-7.0),
    'mol_m16': dict(out_channels=48, quantize_channels=65536, log_scale_min=-7.0),
}
HEAD_B, HEAD_T = 3, 300                          # 900 rows: three full 256-thread blocks and a partial one whose last wave is partial
HEAD_LENGTHS = ((300, 171, 64), (400, 1, 0))     # the second: longer than T (clamped), 1 (nothing counted at shift 1), 0
BR_LEFT, BR_RIGHT, BR_QUOT, BR_DENS = 0, 1, 2, 3           # MoL, per position and component
BR_NEAR, BR_NEG, BR_FAR, BR_POS = 0, 1, 2, 3               # Gaussian cdf head, per position
HEAD_FAULTS = ('right_edge_gs_sign', 'no_clamp_gate')
OPTIM_FAULTS = ('ema_decay_0.999', 'value_clip_first', 'bias_correction_t_is_step')


def _f32(x):
    return float(np.float32(x))


def head_kind(cfg):
    return 'softmax' if cfg.input_type == 'mulaw-quantize' else ('gauss' if cfg.out_channels == 2 else 'mol')


def counted_mask(lengths, T, shift):
    """[B, T] bool: the prediction at t is scored against sample t + shift of an utterance of min(length, T) samples"""
    ln = torch.clamp(torch.as_tensor(lengths, dtype=torch.int64), min=0, max=T)
    return (torch.arange(T)[None, :] + shift) < ln[:, None]


def shifted_target(y, shift):
    """yt[b, t] = y[b, t + shift]; 0 where that sample does not exist (never counted)"""
    y = y.reshape(y.shape[0], -1)
    out = torch.zeros_like(y)
    out[:, :y.shape[1] - shift] = y[:, shift:]
    return out


def _ndtr(x):
    """TF special_math._ndtr: piecewise erf / erfc"""
    hs2 = 0.5 * float(np.sqrt(2.0))
    w = x * hs2
    z = torch.abs(w)
    return 0.5 * torch.where(z < hs2, 1.0 + torch.erf(w), torch.where(w > 0, 2.0 - torch.erfc(z), torch.erfc(z)))


def _mol(cfg, t, yt, fault, oracle_softplus=False):
    M = t.shape[-1] // 3
    Q, lsmin = cfg.quantize_channels, _f32(cfg.log_scale_min)
    logit, means, lsr = t[..., :M], t[..., M:2 * M], t[..., 2 * M:]
    ls = torch.clamp(lsr, min=lsmin)
    if fault == 'no_clamp_gate':
        ls = lsr + (ls - lsr).detach()                         # the clamped value, the gradient of the identity
    y32 = yt.float().unsqueeze(-1)
    left, right = y32 < torch.tensor(-0.999, dtype=torch.float32), y32 > torch.tensor(0.999, dtype=torch.float32)
    y = yt.to(t.dtype).unsqueeze(-1)
    cy = y - means
    inv = torch.exp(-ls)
    plus_in = inv * (cy + 1. / (Q - 1))
    min_in = inv * (cy - 1. / (Q - 1))
    cdf_delta = torch.sigmoid(plus_in) - torch.sigmoid(min_in)
    mid_in = inv * cy
    if oracle_softplus:      # the oracle's library call: F.softplus returns x above 20 (2e-9 off, and p - softplus(p) then has the derivative 0)
        log_cdf_plus, log_one_minus_cdf_min, log_pdf_mid = plus_in - F.softplus(plus_in), -F.softplus(min_in), mid_in - ls - 2. * F.softplus(mid_in)
    else:                    # the same three expressions through log sigmoid(x) = -softplus(-x), exact over the whole range
        log_cdf_plus, log_one_minus_cdf_min, log_pdf_mid = F.logsigmoid(plus_in), F.logsigmoid(-min_in), mid_in - ls + 2. * F.logsigmoid(-mid_in)
    quot = cdf_delta.detach() > 1e-5
    log_probs = torch.where(left, log_cdf_plus,
                            torch.where(right, log_one_minus_cdf_min,
                                        torch.where(quot, torch.log(torch.clamp(cdf_delta, min=1e-12)), log_pdf_mid - float(np.log((Q - 1) / 2)))))
    mx = logit.max(dim=-1, keepdim=True).values
    log_probs = log_probs + (logit - mx - torch.log(torch.sum(torch.exp(logit - mx), dim=-1, keepdim=True)))
    m1 = log_probs.max(dim=-1).values
    nll = -(m1 + torch.log(torch.sum(torch.exp(log_probs - m1.unsqueeze(-1)), dim=-1)))
    one = torch.ones_like(quot)
    branch = torch.where(left & one, BR_LEFT, torch.where(right & one, BR_RIGHT, torch.where(quot, BR_QUOT, BR_DENS)))
    return nll, dict(branch=branch, clamped=(lsr < lsmin).detach(), at_min=(lsr == lsmin).detach(), cdf_delta=cdf_delta.detach())


def _gauss(cfg, t, yt, fault):
    Q, lsmin = cfg.quantize_channels, _f32(cfg.log_scale_min_gauss)
    mean, lsr = t[..., 0], t[..., 1]
    ls = torch.clamp(lsr, min=lsmin)
    if fault == 'no_clamp_gate':
        ls = lsr + (ls - lsr).detach()
    yv = yt.to(t.dtype)
    info = dict(clamped=(lsr < lsmin).detach(), at_min=(lsr == lsmin).detach())
    if cfg.cdf_loss:
        scale = torch.exp(ls)
        diff = _ndtr((yv + 1. / (Q - 1) - mean) / scale) - _ndtr((yv - 1. / (Q - 1) - mean) / scale)
        nll = -torch.log(torch.clamp(diff, min=1e-12))
        z = ((yv - mean) / scale).detach()
        far = diff.detach() < 1e-12
        info.update(diff=diff.detach(), z=z,
                    branch=torch.where(far, BR_FAR, torch.where(z.abs() < 3.5, BR_NEAR, torch.where(z < 0, BR_NEG, BR_POS))))
    else:
        nll = 0.5 * (float(np.log(2. * np.pi)) + 2. * ls + (yv - mean) ** 2 * torch.exp(-2. * ls))
        info.update(branch=torch.zeros(yv.shape, dtype=torch.int64))
    return nll, info


def ce_loss_float32(y_hat, tgt):
    """the per-position softmax loss as float32 arithmetic gives it (max, sum of exponentials, log: sparse_softmax_cross_entropy's and the
    kernel's order): exactly 0 where the other classes vanish beside the target's"""
    x = y_hat.float().transpose(1, 2)
    mx = x.max(dim=-1, keepdim=True).values
    return (mx.squeeze(-1) + torch.log(torch.sum(torch.exp(x - mx), dim=-1))) - x.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)


def _ce(cfg, t, yt, y_hat32, counted):
    tgt = yt.long()
    nll = torch.logsumexp(t, dim=-1) - t.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
    l32 = ce_loss_float32(y_hat32, tgt)
    nonzero = (l32 != 0) & counted
    p_tgt = torch.exp(-nll.detach())
    branch = torch.where(l32 == 0, 2, torch.where(p_tgt > 0.99, 1, 0))      # 0 ordinary, 1 confident (1 - p cancels), 2 float32 loss exactly 0
    return nll, dict(branch=branch, nonzero32=nonzero, count32=int(nonzero.sum()), loss32=l32, target_class=tgt)


def ref_heads(cfg, y_hat, y, lengths, shift, dtype=torch.float64, fault=None, oracle_softplus=False):
    """y_hat [B, O, T] float32, y [B, T] (float32 samples, or int class ids for the softmax head) -> namespace with
    nll [B, T] (0 where nothing is scored), loss (the masked mean), dy [B, T, O] = d loss / d y_hat, counted [B, T], denominator, and per
    position (MoL: and component) the branch taken plus what the exclusion rule needs (cdf_delta / diff).  oracle_softplus: the MoL head with the
    oracle's F.softplus calls, to pin this restatement to the oracle; the default is exact where F.softplus is not (arguments above 20)."""
    B, O, T = y_hat.shape
    kind = head_kind(cfg)
    counted = counted_mask(lengths, T, shift)
    yh = y_hat.detach().to(dtype).clone().requires_grad_(True)
    t = yh.transpose(1, 2)
    yt = shifted_target(y, shift)
    if kind == 'softmax':
        nll, info = _ce(cfg, t, yt, y_hat, counted)
        den = info['count32']
    else:
        nll, info = _mol(cfg, t, yt, fault, oracle_softplus) if kind == 'mol' else _gauss(cfg, t, yt, fault)
        den = int(counted.sum())
    masked = nll * counted.to(dtype)
    loss = masked.sum() / den
    (g,) = torch.autograd.grad(loss, [yh])
    dy = g.permute(0, 2, 1).contiguous()
    if fault == 'right_edge_gs_sign' and kind == 'mol':
        M = O // 3
        dy[..., 2 * M:] = torch.where((info['branch'] == BR_RIGHT), -dy[..., 2 * M:], dy[..., 2 * M:])
    out = types.SimpleNamespace(kind=kind, nll=masked.detach(), loss=loss.detach(), dy=dy, counted=counted, denominator=den, target=yt, **info)
    if dtype == torch.float32:      # the same mean with ONE running float32 accumulator in row order (the plainest float32 evaluation of the sum)
        run = np.cumsum(out.nll.numpy().reshape(-1), dtype=np.float32)[-1]
        out.loss_running = float(np.float32(run) / np.float32(den))
    return out


def loss_yardstick(r64, r32):
    """the float32 evaluation's own error of the scalar loss: the worse of torch's float32 sum and the running float32 accumulator"""
    return max(abs(float(r32.loss) - float(r64.loss)), abs(r32.loss_running - float(r64.loss)))


def heads_excluded(r64, r32):
    """[B, T] bool: a MoL component's float64 cdf_delta inside (0.5e-5, 1e-3) (the quotient form loses its digits in float32 in the reference
    itself), a cdf-head diff inside [1e-13, 1e-10], or float32 and float64 on different branches"""
    ex = torch.zeros_like(r64.counted)
    if r64.kind == 'mol':
        ex |= ((r64.cdf_delta > 0.5e-5) & (r64.cdf_delta < 1e-3)).any(-1)
        ex |= (r64.branch != r32.branch).any(-1) | (r64.clamped != r32.clamped).any(-1)
    elif r64.kind == 'gauss':
        if hasattr(r64, 'diff'):
            ex |= (r64.diff >= 1e-13) & (r64.diff <= 1e-10)
            ex |= (r64.branch == BR_FAR) != (r32.branch == BR_FAR)
        ex |= r64.clamped != r32.clamped
    else:
        ex |= (r64.branch == 2) != (r32.branch == 2)
    return ex


def head_groups(r64):
    """{group: [B, T, O] bool}: the branch groups of the loss-gradient check (every element of a counted row is in exactly one)"""
    B, T, O = r64.dy.shape
    full = torch.ones(B, T, O, dtype=torch.bool)
    if r64.kind == 'mol':
        M = O // 3
        left, right = (r64.branch[..., :1] == BR_LEFT) & full, (r64.branch[..., :1] == BR_RIGHT) & full
        mid = ~left & ~right
        col = torch.arange(O)[None, None, :]
        return {'left_edge': left, 'right_edge': right, 'middle_logit': mid & (col < M), 'middle_mean': mid & (col >= M) & (col < 2 * M),
                'middle_log_scale': mid & (col >= 2 * M)}
    if r64.kind == 'gauss':
        if not hasattr(r64, 'diff'):
            return {'pdf': full}
        return {n: (r64.branch == k).unsqueeze(-1) & full for n, k in (('cdf_near', BR_NEAR), ('cdf_negative', BR_NEG), ('cdf_far', BR_FAR), ('cdf_positive', BR_POS))}
    # softmax: the target's column of a confident row is 1 - p with p near 1 (cancels in float32, and is exactly 0 where the float32 loss is): its own groups
    tcol = torch.zeros(B, T, O, dtype=torch.bool).scatter(-1, r64.target_class.unsqueeze(-1), True)
    br = r64.branch.unsqueeze(-1)
    return {'softmax': (br == 0) & full, 'softmax_confident': (br == 1) & ~tcol, 'softmax_confident_target': (br == 1) & tcol,
            'softmax_zero_loss': (br == 2) & ~tcol, 'softmax_zero_loss_target': (br == 2) & tcol}


def heads_check(dev, r64, r32, what='', factor=FACTOR):
    """dev [B, T, ld >= O]: the gradient under test.  Rows that are not counted and the columns O .. ld must be exactly 0; on counted, not excluded rows
    |dev - ref64| <= 2^-8 |ref64| + factor * r32(group) * rowmax |ref64| + TINY, r32(group) the worst |ref32 - ref64| / max(rowmax |ref64|, TINY)
    of the group.  TINY = 2^-120 is float32's underflow: a factor exp(-p) below 2^-126 is flushed to zero, and the factors it meets (exp(-log_scale_min) /
    denominator) stay below 2^6, so a gradient under 2^-120 may come out as 0 in any float32 evaluation (with one mixture component whole rows are that small).
    -> {group: dict(n, r32, worst = worst err / bound)}, excluded share in ['excluded']; raises AssertionError naming the groups that fail."""
    B, T, O = r64.dy.shape
    dev = dev.double()
    ref, ref32 = r64.dy, r32.dy.double()
    counted = r64.counted
    bad = []
    if dev.shape[-1] > O and float(dev[..., O:].abs().max()) != 0.0:
        bad.append('padding columns: not zero')
    if (~counted).any() and float(dev[~counted].abs().max()) != 0.0:
        bad.append('uncounted rows: not zero (max %.3e)' % float(dev[~counted].abs().max()))
    excl = heads_excluded(r64, r32) & counted
    keep = (counted & ~excl).unsqueeze(-1)
    rowmax = ref.abs().amax(dim=-1, keepdim=True).expand(B, T, O)
    e32 = (ref32 - ref).abs() / torch.clamp(rowmax, min=TINY)
    err = (dev[..., :O] - ref).abs()
    out = {'excluded': float(excl.sum()) / max(1, int(counted.sum()))}
    for name, g in head_groups(r64).items():
        g = g & keep
        if not g.any():
            continue
        y32 = float(e32[g].max())
        bound = BF * ref.abs() + factor * y32 * rowmax + TINY
        ratio = torch.where(g, err / bound, torch.zeros_like(err))
        w = float(ratio.max())
        out[name] = dict(n=int(g.sum()), r32=y32, worst=w)
        if not w <= 1.0:
            b, tt, o = np.unravel_index(int(ratio.argmax()), ratio.shape)
            bad.append('%s: err / bound = %.3g at (b %d, t %d, column %d): got %.6e, reference %.6e, row max %.3e, r32 %.2e; %d elements over'
                       % (name, w, b, tt, o, float(dev[b, tt, o]), float(ref[b, tt, o]), float(rowmax[b, tt, o]), y32, int((ratio > 1).sum())))
    if out['excluded'] > MAX_EXCLUDED:
        bad.append('excluded share %.2f %% above the cap' % (100 * out['excluded']))
    assert not bad, '%s loss gradient outside its bound:\n  ' % what + '\n  '.join(bad)
    return out


# ------------------------------------------------------------------------------------------------------------------ recipes
def _spread(gen, shape, parts):
    """int tensor: value k with probability parts[k] (the remainder: len(parts))"""
    u = torch.rand(shape, generator=gen, dtype=torch.float64)
    edges = torch.cumsum(torch.tensor(parts, dtype=torch.float64), 0)
    return torch.bucketize(u, edges, right=True)


def mol_targets(B, T, gen):
    """U(-0.99, 0.99); 40 % replaced, 5 % each, by -1, +1, float32(-0.999) and its two float32 neighbours, float32(0.999) and its two"""
    y = (torch.rand(B, T, generator=gen, dtype=torch.float64) * 1.98 - 0.99).float()
    lo, hi = np.float32(-0.999), np.float32(0.999)
    special = [-1.0, 1.0, lo, np.nextafter(lo, np.float32(-2)), np.nextafter(lo, np.float32(2)), hi, np.nextafter(hi, np.float32(-2)), np.nextafter(hi, np.float32(2))]
    k = _spread(gen, (B, T), [0.05] * 8)
    for i, s in enumerate(special):
        y = torch.where(k == i, torch.tensor(float(s), dtype=torch.float32), y)
    return y


def mol_inputs(cfg, B, T, shift, seed=2025, rounds=30):
    """-> y_hat [B, 3M, T] float32, y [B, T] float32, rounds of redrawing used"""
    gen = torch.Generator().manual_seed(seed)
    M, Q, lsmin = cfg.out_channels // 3, cfg.quantize_channels, _f32(cfg.log_scale_min)
    y = mol_targets(B, T, gen)
    yt = shifted_target(y, shift).double().unsqueeze(-1)

    def draw():
        ls = torch.rand(B, T, M, generator=gen, dtype=torch.float64) * 8.5 - 9.0
        ls = torch.where(torch.rand(B, T, M, generator=gen) < 0.05, torch.full_like(ls, lsmin), ls)
        kind = _spread(gen, (B, T, M), [0.49, 0.49])                                             # 0 ordinary, 1 far, 2 (2 %) overflow tail
        sign = torch.where(torch.rand(B, T, M, generator=gen) < 0.5, -1.0, 1.0).double()
        k = torch.where(kind == 0, 1.5 * torch.randn(B, T, M, generator=gen, dtype=torch.float64),
                        sign * torch.where(kind == 1, 15 + 25 * torch.rand(B, T, M, generator=gen, dtype=torch.float64),
                                           100 + 200 * torch.rand(B, T, M, generator=gen, dtype=torch.float64)))
        return (yt - k * torch.exp(torch.clamp(ls, min=lsmin))).float(), ls.float()
    means, ls = draw()
    logits = 2 * torch.randn(B, T, M, generator=gen)
    used = 0
    for used in range(rounds + 1):
        inv = torch.exp(-torch.clamp(ls.double(), min=lsmin)); cy = yt - means.double()
        cd = torch.sigmoid(inv * (cy + 1. / (Q - 1))) - torch.sigmoid(inv * (cy - 1. / (Q - 1)))
        band = (cd > 0.5e-5) & (cd < 1e-3)
        if not band.any() or used == rounds:
            break
        m2, l2 = draw()
        means, ls = torch.where(band, m2, means), torch.where(band, l2, ls)
    y_hat = torch.cat([logits, means, ls], -1).permute(0, 2, 1).contiguous()
    return y_hat, y, used


def gauss_targets(B, T, gen):
    """U(-1, 1) with 5 % at each of -1 and +1 (the validation suite's targets)"""
    y = torch.rand(B, T, generator=gen, dtype=torch.float64) * 2 - 1
    edge = torch.rand(B, T, generator=gen, dtype=torch.float64)
    return torch.where(edge < 0.05, -torch.ones_like(y), torch.where(edge > 0.95, torch.ones_like(y), y)).float()


def gauss_inputs(cfg, B, T, shift, seed=2025):
    gen = torch.Generator().manual_seed(seed)
    lsmin = _f32(cfg.log_scale_min_gauss)
    y = gauss_targets(B, T, gen)
    yt = shifted_target(y, shift).double()
    top = -3.0 if cfg.cdf_loss else -1.0
    ls = torch.rand(B, T, generator=gen, dtype=torch.float64) * (top + 9.0) - 9.0
    ls = torch.where(torch.rand(B, T, generator=gen) < 0.05, torch.full_like(ls, lsmin), ls)
    kind = _spread(gen, (B, T), [0.70, 0.15])
    sign = torch.where(torch.rand(B, T, generator=gen) < 0.5, -1.0, 1.0).double()
    z = torch.where(kind == 0, torch.clamp(torch.randn(B, T, generator=gen, dtype=torch.float64), -2.5, 2.5),
                    torch.where(kind == 1, -(4 + torch.rand(B, T, generator=gen, dtype=torch.float64)), sign * (9 + 3 * torch.rand(B, T, generator=gen, dtype=torch.float64))))
    mu = yt - z * torch.exp(torch.clamp(ls, min=lsmin))
    return torch.stack([mu.float(), ls.float()], 1).contiguous(), y


def softmax_inputs(cfg, B, T, shift, seed=2025):
    gen = torch.Generator().manual_seed(seed)
    Q = cfg.out_channels
    x = 3 * torch.randn(B, T, Q, generator=gen)
    y = torch.randint(0, Q, (B, T), generator=gen).int()
    tgt = shifted_target(y, shift).long().unsqueeze(-1)
    kind = _spread(gen, (B, T), [0.10, 0.10]).unsqueeze(-1)
    others = x.scatter(-1, tgt, float('-inf')).max(dim=-1, keepdim=True).values
    cur = x.gather(-1, tgt)
    x = x.scatter(-1, tgt, torch.where(kind == 0, others + 30.0, torch.where(kind == 1, others + 12.0, cur)))
    return x.permute(0, 2, 1).contiguous(), y


def head_inputs(cfg, B, T, shift, seed=2025):
    kind = head_kind(cfg)
    if kind == 'mol':
        return mol_inputs(cfg, B, T, shift, seed)[:2]
    return (gauss_inputs if kind == 'gauss' else softmax_inputs)(cfg, B, T, shift, seed)


# ------------------------------------------------------------------------------------------------------------------ optimiser
NORM_SPAN = 4096                                 # csrc/wn_optim.hip: floats per wave of the first norm stage
SECOND_ORDER = 1.001                             # the bound is first order in 2^-24; this covers the products of two such terms many times over


def optim_hparams(hp):
    """the hyper-parameters as the float32 values the device and TensorFlow's kernels hold"""
    return dict(clip=bool(hp.wavenet_clip_gradients), max_norm=_f32(hp.wavenet_gradient_max_norm), max_value=_f32(hp.wavenet_gradient_max_value),
                beta1=_f32(hp.wavenet_adam_beta1), beta2=_f32(hp.wavenet_adam_beta2), eps=_f32(hp.wavenet_adam_epsilon), ema_decay=_f32(hp.wavenet_ema_decay))


def adam_lr_t(lr, step, h):
    """lr_t of the update number step + 1: double arithmetic on the float32 values, rounded to float32 once"""
    t = float(step + 1)
    return _f32(_f32(lr) * math.sqrt(1.0 - h['beta2'] ** t) / (1.0 - h['beta1'] ** t))


def tensor_slices(layout, n):
    """[(name, first, numel, end of the tensor's padded range)] in buffer order; the padding floats after a tensor belong to it (the kernel's
    find_tensor), the last tensor's run to n"""
    items = sorted(((off, name, int(np.prod(shape))) for name, (shape, off) in layout.items()))
    return [(name, off, numel, items[i + 1][0] if i + 1 < len(items) else n) for i, (off, name, numel) in enumerate(items)]


def ref_optim(layout, p, g, m, v, ema, lr, step, hp, dtype=torch.float64, fault=None):
    """One optimiser step on the flat buffers (float32 CPU tensors), per tensor of `layout`:
        gc  = clip(g * max_norm / max(||g||, max_norm), +-max_value)         (wavenet_clip_gradients)
        m'  = b1 m + (1 - b1) gc          v' = b2 v + (1 - b2) gc gc          (1 - b: float32 subtractions, exact)
        p'  = p - lr_t m' / (sqrt(v') + eps)                                   lr_t: adam_lr_t
        e'  = e - (1 - decay) (e - p')
    evaluated in `dtype`.  Returns the new p, m, v, ema (flat, `dtype`; the padding keeps its input values) and, for every element, the bound
    on |float32 kernel - this reference| below, with the magnitude sums it is made of.

    The bound, u = 2^-24, first order in u.  Every float32 operation rounds once, relative error <= u (hipcc's default division and sqrt are
    correctly rounded; a contracted multiply-add rounds less often, never more):
      norm  sum g^2 over a tensor of S spans of 4096 floats: a square (1), the lane's chain of 16 x 4 = 64 additions, 6 butterfly steps, then
            ceil(S / 64) additions per lane and 6 butterfly steps in the second stage.  All terms are >= 0, so the sum's relative error is at most
            the number of roundings a term passes through: N = 1 + 64 + 6 + ceil(S / 64) + 6 (= 79 for the 96-span tensor).  sqrt halves it and
            rounds once; max(., max_norm) is 1-Lipschitz: the denominator's relative error is dc = (N / 2 + 1) u.
      gc    (g * max_norm) / cs: two roundings and dc -> Kg = N / 2 + 3, eg = Kg u |g max_norm / cs|; the value clip is 1-Lipschitz, and an
            element whose unclipped value lies beyond max_value by more than eg is max_value on both sides: eg = 0.  No clipping: eg = 0.
      m'    two products (1 each), one sum: u |m'| + 1 u (|b1 m| + |(1 - b1) gc|) + (1 - b1) eg
      v'    ((1 - b2) gc) gc has two roundings, b2 v one: u |v'| + 2 u (|b2 v| + |(1 - b2) gc^2|) + (1 - b2) 2 |gc| eg
      p'    q = lr_t m' / (sqrt(v') + eps) on the kernel's own m', v': product, sqrt, sum, quotient -> 4 u |q|; m' and v' carry their whole
            bounds em, ev:  u |p'| + 4 u |q| + lr_t em / (sqrt(v') + eps) + |q| ev / (2 sqrt(v') (sqrt(v') + eps))
      e'    d = e - p' (1), (1 - decay) d (1), the final difference: u |e'| + 2 u (1 - decay) |d| + (1 - decay) ep
    The leading u |new value| is the final store, K = 1, 2, 4, 2 the operation counts of m', v', p', e', the rest what the clip scale and the
    earlier quantities propagate.  The whole is multiplied by 1.001 for the terms of order u^2 (below 1e-6 of the bound)."""
    h = optim_hparams(hp)
    n = p.numel()
    dt = dtype
    b1, b2, dec = h['beta1'], h['beta2'], h['ema_decay']
    omb1, omb2, omdec = _f32(np.float32(1) - np.float32(b1)), _f32(np.float32(1) - np.float32(b2)), _f32(np.float32(1) - np.float32(dec))
    if fault == 'ema_decay_0.999':
        omdec = _f32(np.float32(1) - np.float32(0.999))
    lr_t = adam_lr_t(lr, step - 1 if fault == 'bias_correction_t_is_step' else step, h)
    out = {k: x.detach().to(dt).clone() for k, x in (('p', p), ('m', m), ('v', v), ('ema', ema))}
    bound = {k: torch.zeros(n, dtype=torch.float64) for k in out}
    mags = {k: torch.zeros(n, dtype=torch.float64) for k in out}
    norms = {}
    for name, off, numel, end in tensor_slices(layout, n):
        sl = slice(off, off + numel)
        gs, p0, m0, v0, e0 = (x[sl].to(dt) for x in (g, p, m, v, ema))
        eg = torch.zeros(numel, dtype=torch.float64)
        gc = gs
        if h['clip']:
            if fault == 'value_clip_first':
                gs = torch.clamp(gs, -h['max_value'], h['max_value'])
            nrm = torch.sqrt((gs * gs).sum())
            cs = torch.clamp(nrm, min=h['max_norm'])
            pre = gs * h['max_norm'] / cs
            gc = torch.clamp(pre, -h['max_value'], h['max_value'])
            norms[name] = float(nrm)
            S = -(-(end - off) // NORM_SPAN)                                    # spans of the tensor (its padding included)
            N = 1 + 64 + 6 + -(-S // 64) + 6
            eg = (N / 2 + 3) * U24 * pre.double().abs()
            eg = torch.where(pre.double().abs() - eg > h['max_value'], torch.zeros_like(eg), eg)
        m1 = b1 * m0 + omb1 * gc
        v1 = b2 * v0 + omb2 * gc * gc
        den = torch.sqrt(v1) + h['eps']
        q = lr_t * m1 / den
        p1 = p0 - q
        d = e0 - p1
        e1 = e0 - omdec * d
        out['m'][sl], out['v'][sl], out['p'][sl], out['ema'][sl] = m1, v1, p1, e1
        if dt == torch.float64:
            Sm = (b1 * m0).abs() + (omb1 * gc).abs()
            Sv = (b2 * v0).abs() + (omb2 * gc * gc).abs()
            em = U24 * m1.abs() + U24 * Sm + omb1 * eg
            ev = U24 * v1.abs() + 2 * U24 * Sv + omb2 * 2 * gc.abs() * eg
            rt = torch.sqrt(v1)
            prop_v = torch.where(ev > 0, q.abs() * ev / torch.where(ev > 0, 2 * rt * den, torch.ones_like(den)), torch.zeros_like(ev))
            ep = U24 * p1.abs() + 4 * U24 * q.abs() + lr_t * em / den + prop_v
            ee = U24 * e1.abs() + 2 * U24 * omdec * d.abs() + omdec * ep
            bound['m'][sl], bound['v'][sl], bound['p'][sl], bound['ema'][sl] = (SECOND_ORDER * x for x in (em, ev, ep, ee))
            mags['m'][sl], mags['v'][sl], mags['p'][sl], mags['ema'][sl] = Sm, Sv, q.abs(), (omdec * d).abs()
    return types.SimpleNamespace(bound=bound, mags=mags, norms=norms, lr_t=lr_t, hp=h, **out)


def optim_check(dev, start, ref, layout, what=''):
    """dev / start: {'p', 'm', 'v', 'ema'} flat float32 tensors after / before the step; the increments dev - start, formed in float64, against the
    reference's, element by element under ref.bound.  The padding between tensors must keep its bits.  -> {quantity: worst err / bound}; raises
    AssertionError naming quantity and tensor."""
    n = ref.p.numel()
    worst, bad = {}, []
    inside = torch.zeros(n, dtype=torch.bool)
    sls = tensor_slices(layout, n)
    for name, off, numel, end in sls:
        inside[off:off + numel] = True
    for k in ('m', 'v', 'p', 'ema'):
        d0 = start[k].double()
        err = ((dev[k].double() - d0) - (getattr(ref, k).double() - d0)).abs()
        b = ref.bound[k]
        ratio = torch.where(b > 0, err / torch.where(b > 0, b, torch.ones_like(b)), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
        worst[k] = float(ratio[inside].max())
        if (~inside).any() and not torch.equal(dev[k][~inside].view(torch.int32), start[k][~inside].view(torch.int32)):
            bad.append('%s: the padding between tensors changed' % k)
        if not worst[k] <= 1.0:
            i = int(torch.where(inside, ratio, torch.zeros_like(ratio)).argmax())
            name = [s[0] for s in sls if s[1] <= i < s[1] + s[2]][0]
            bad.append('%s: increment err / bound = %.3g in %s (flat %d): got %.9e, reference %.9e, start %.9e; %d elements over'
                       % (k, worst[k], name, i, float(dev[k][i]), float(getattr(ref, k)[i]), float(start[k][i]), int((ratio[inside] > 1).sum())))
    assert not bad, '%s optimiser step outside its bound:\n  ' % what + '\n  '.join(bad)
    return worst


def optim_gradients(layout, n, hp, seed=3):
    """flat gradient [n] float32, zero in the padding; tensor i takes pattern i % 6: 0 norm well below max_norm, 1 that x 400, 2 ordinary with a few
    elements at +-1e4 (the value clip after the norm clip), 3 all zeros, 4 / 5 norm = max_norm (1 +- 1e-3).  -> g, {name: pattern}"""
    gen = torch.Generator().manual_seed(seed)
    max_norm = float(hp.wavenet_gradient_max_norm)
    g = torch.zeros(n, dtype=torch.float32)
    pattern = {}
    for i, (name, off, numel, end) in enumerate(tensor_slices(layout, n)):
        x = torch.randn(numel, generator=gen, dtype=torch.float64)
        x = x / x.norm() * (0.1 * max_norm)
        k = i % 6
        if k == 1:
            x = x * 400.0
        elif k == 2:
            idx = torch.randperm(numel, generator=gen)[:min(4, numel)]
            x[idx] = torch.where(torch.arange(idx.numel()) % 2 == 0, 1e4, -1e4).double()
        elif k == 3:
            x = torch.zeros_like(x)
        elif k >= 4:
            x = x * (10.0 * (1 + 1e-3 if k == 4 else 1 - 1e-3))
        g[off:off + numel] = x.float()
        pattern[name] = k
    return g, pattern


def optim_state(layout, n, seed=4, zero_moments=False):
    """p0 ~ 0.3 N(0, 1), m0, v0 ~ 0.01 U, ema0 = p0 + 0.1 N(0, 1) inside the tensors, 0 in the padding"""
    gen = torch.Generator().manual_seed(seed)
    inside = torch.zeros(n, dtype=torch.bool)
    for name, off, numel, end in tensor_slices(layout, n):
        inside[off:off + numel] = True
    p = 0.3 * torch.randn(n, generator=gen)
    m = 0.01 * torch.rand(n, generator=gen)
    v = 0.01 * torch.rand(n, generator=gen)
    e = p + 0.1 * torch.randn(n, generator=gen)
    if zero_moments:
        m, v = torch.zeros(n), torch.zeros(n)
    z = torch.zeros(n)
    return {k: torch.where(inside, x, z).contiguous() for k, x in (('p', p), ('m', m), ('v', v), ('ema', e))}
