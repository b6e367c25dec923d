"""Teacher-forced synthesis (WaveNet.incremental, wavenet.py:724-911) restated in float64 for [B] streams, and the per-step check of
a device run against it: every element of raw [B, O, T] under ONE bound per output channel.

The batch formulation: incremental generation under teacher forcing == the batch forward on the input shifted by one sample
behind the silence start frame (wavenet.py:433-445); a tap before the utterance reads the zero queue (wavenet.py:815-816).  Layout
[B, T, channels]; kernels keep the TensorFlow layouts of the parameter table.  Free-running runs use the same function, fed the DEVICE's
own samples as the teacher-forcing input.

`store=` (None | 'fp32' | 'bf16' | 'fp16') rounds where a device path STORES a value in that type; the arithmetic between two roundings
stays float64 (or `arith`, see the stand-in below).  One set of rounding points per path, restated from the kernels:

  'pipeline' (csrc/wn_synth_pipe.hip, the persistent dataflow kernel; store = 'fp16' by default, 'bf16' after pipeline_dtype(False))
     weights              wn_pipe_slice_kernel :199-200 (scale * param in fp32, then the 16-bit store; scale = the legacy skip factor
                          for W_skip :1135, 1 otherwise), W_h2 in wn_pipe_fixup_kernel :1189-1190; the input convolution stays fp32 :1145
     x_0                  publish_input :817-819 (fp32 input convolution, 16-bit store)
     conditioning rows    cbt is bf16 (csrc/wn_frontend.hip:197 / :231), converted to the storage type: cvt8_bf16 :161-168, used :334 / :389 / :449
     z_past               fp32 in LDS: :343 / :398 / :507-508 (taps t - 2d, t - d, conditioning, bias)
     u                    :619 (fast path) / :657
     partials of x_{l+1}  CU j of P rounds rho (W_out[:, its 32 gate outputs] u_j [+ x_l + b on CU 0]) BEFORE the sum: :631 / :665;
                          the consumer adds the P partials in fp32 and stores x_{l+1} in 16 bits: :586-602 / :643 -- that value is the
                          queue row (:751)
     skip sum             P independent fp32 running sums, one per CU column: :715-718 / :736-740, reduced by the head :891-892
     head                 relu(skip) :893, hidden layer :904 / :906 in 16 bits; raw outputs fp32 :915 / :917
  'launch' (csrc/wn_synth.hip, launch per layer; store = 'bf16')
     weights              csrc/wn_pack.hip:44 (scale * param, bf16 store; the legacy factor folded into W_skip :100)
     x_0                  wn_synth_sample :261-262;   conditioning rows: cbt bf16, read at wn_synth_gate :82
     u                    wn_synth_gate :108;         queue rows x_{l+1}: wn_synth_out :163
     skip sum             fp32 in memory, layer after layer: wn_synth_out :157
     head                 relu(skip) wn_synth_head1 :183, hidden layer :196 in bf16; raw outputs fp32 wn_synth_head2 :222
  'f32' (csrc/wn_synth_f32.hip, the fp32 mode; store = 'fp32'): every point above is an fp32 store -- conditioning CUP fp32 (read :93),
     u :101, queue rows :130 / :184, skip sum :127 (the legacy factor applied to the product, not folded into the weight), head :152.
The per-stream gate bias b_dil + b_cin (+ W_g^T g + b_g) is an fp32 vector on every path (csrc/wn_pack.hip:203, csrc/wn_frontend.hip:636).

What cannot be mirrored (the order of the fp32 additions inside a contraction, __expf / rcp in the gate, the fp32 upsampling network)
is covered by the factor F of the check and by nothing else; nothing is fitted per case."""
import numpy as np
import torch

from oracle import wavenet_oracle as O

FLOOR = 2.0 ** -24                 # Y[o] >= FLOOR * max |ref[:, o, :]|: half an ulp of the fp32 raw output
F_16BIT = 4.0                      # see check_steps
F_FP32 = 8.0
SQRT_HALF_F32 = float(np.float32(0.70710678118654752440))      # csrc/wn_common.h: WN_SQRT_HALF
PATHS = ('pipeline', 'launch', 'f32')
FACTOR = {'bf16': F_16BIT, 'fp16': F_16BIT, 'fp32': F_FP32}


def _rounder(store, dt):
    """value -> the nearest value of the storage type (round to nearest even, as the device's conversions), kept in dtype dt."""
    if store is None:
        return lambda t: t
    st = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}[store]
    return lambda t: t.to(torch.float32).to(st).to(dt)


def ring_slots(path, d):
    """slots of a layer's ring queue: 4d on the launch-per-layer and fp32 paths (wn_synth.hip:321, wn_synth_f32.hip:203), the power of two
    >= 2d + 1 on the pipeline (wn_synth_pipe.hip:1273); at least 4."""
    need = 2 * d + 1 if path == 'pipeline' else 4 * d
    s = 4
    while s < need:
        s <<= 1
    return s


def _shift(x, s):
    """y[:, t] = x[:, t - s], zero for t < s (the zero queue)."""
    if s == 0:
        return x
    y = torch.zeros_like(x)
    if s < x.shape[1]:
        y[:, s:] = x[:, :x.shape[1] - s]
    return y


def start_class(cfg):
    return int(O.initial_input(cfg, 1)[0].argmax())


def shifted_input(cfg, inputs, dt=torch.float64):
    """Teacher-forcing inputs (scalar [B, T] floats, or [B, T] class ids) -> the network input of every step [B, T, Cin]: the silence start
    frame at t = 0, then the given sample t - 1 (wavenet.py:433-445, :877-878)."""
    B, T = inputs.shape
    if cfg.scalar_input:
        x = torch.zeros(B, T, 1, dtype=dt)
        x[:, 1:, 0] = inputs[:, :-1].to(dt)
        return x
    ids = torch.cat([torch.full((B, 1), start_class(cfg), dtype=torch.long), inputs[:, :-1].long()], 1)
    return torch.nn.functional.one_hot(ids, cfg.quantize_channels).to(dt)


def synth_ref(params, cfg, inputs, c, g=None, store=None, path='pipeline', arith=torch.float64, fault=None, ksplit=1):
    """raw [B, O, T] of teacher-forced synthesis.  params: the oracle's table (any float dtype), inputs [B, T] (see shifted_input),
    c [B, C, Tc], g: speaker ids [B] / features [B, gin] / None.

    arith: the dtype of the arithmetic between roundings (float64: the reference / the yardstick; float32: the CPU stand-in of a correct
    device).  ksplit: every contraction as that many chains over K added in order (another order of the same sums; the stand-in of the
    fp32 mode).  fault: None, or a dict that seeds ONE fault of the kind a kernel edge produces (tests only).

    store = 'fp32' is evaluated in float32 ARITHMETIC whatever `arith` says: in the fp32 mode the accumulator of every contraction is an
    fp32 register, each fma of the chain rounds to it (wn_synth_f32.hip:50, the partial sums :58 / :68) -- K = 3 R + C roundings per gate
    pre-activation against ONE for the stored result.  That is the project's float32 yardstick (tests/mel_util.py, tests/temper_util.py):
    the same formulas with every operation rounding to float32, whose error differs from the device's by the order of the sums."""
    assert path in PATHS and store in (None, 'fp32', 'bf16', 'fp16')
    dt = torch.float32 if store == 'fp32' else arith
    q = _rounder(store, dt)                                          # the path's storage type
    q32 = _rounder(None if store is None else 'fp32', dt)            # what every path keeps in fp32
    rounded = store is not None
    fault = fault or {}
    fk = fault.get('kind')
    eff = O.effective_params(params, cfg)
    P64 = {k: v.to(torch.float64) for k, v in eff.items()}
    L, R, GH = cfg.layers, cfg.residual_channels, cfg.gate_channels // 2
    dil = cfg.dilations()
    half = SQRT_HALF_F32 if rounded else O.SQRT_HALF
    rho = half if cfg.residual_legacy else 1.0
    expo = [((L - 1 if l == 0 else L - l) if cfg.legacy else 0) for l in range(L)]      # wavenet.py:706-715 unrolled (csrc/wn_api.hip:262)
    scale = [float(np.float32(half ** e)) if rounded else half ** e for e in expo]
    fold = path != 'f32'                                             # the legacy factor folded into W_skip before its rounding

    def W(name, s=1.0):
        w = P64[name]
        if rounded:
            w = (w.to(torch.float32) * torch.tensor(s, dtype=torch.float32)) if s != 1.0 else w
        else:
            w = w * s
        return q(w.to(dt))

    def bias(name):
        b = P64.get(name)
        return None if b is None else b.to(dt)

    def mm(a, w):
        if ksplit <= 1:
            return a @ w
        K = w.shape[0]; per = (K + ksplit - 1) // ksplit
        out = None
        for k0 in range(0, K, per):
            v = a[..., k0:k0 + per] @ w[k0:k0 + per]
            out = v if out is None else out + v
        return out

    B, T = inputs.shape
    # ---- conditioning rows [B, T, C]: the fp32 upsampling network, then bf16 rows on the 16-bit paths
    cu = None
    if c is not None:
        cu = O.upsample(P64, cfg, c.to(torch.float64)).to(dt)         # wavenet.py:781-803
        assert cu.shape[-1] == T, (cu.shape, T)
        cu = q32(cu.transpose(1, 2).contiguous())
        if rounded and path != 'f32':
            cu = q(_rounder('bf16', dt)(cu))
        if fk == 'prev_cond':                                        # one hop boundary reads the previous conditioning row
            cu = cu.clone(); cu[fault['stream'], fault['step']] = cu[fault['stream'], fault['step'] - 1]
    gvec = O.global_features(P64, cfg, g)                            # wavenet.py:766-777
    if gvec is not None:
        gvec = gvec.to(dt)
        if fk == 'gbias_swap':                                       # one stream given another stream's global-conditioning bias
            gvec = gvec.clone(); gvec[fault['stream']] = gvec[fault['other']]
    # ---- x_0: the input convolution stays fp32, its result is a queue row
    x = shifted_input(cfg, inputs, dt)
    h = q(x @ P64['input_convolution/kernel'][0].to(dt) + P64['input_convolution/bias'].to(dt))        # wavenet.py:826
    Pn = cfg.gate_channels // 64 if path == 'pipeline' else 1        # CUs per layer on the pipeline: 32 gate pairs each
    skip = [None] * Pn
    for l, d in enumerate(dil):
        p = 'ResidualConv1DGLU_%d/' % l
        Wd = W(p + 'residual_block_causal_conv/kernel')              # [3, R, G]
        tap0 = _shift(h, 2 * d)
        if fk == 'zero_tap2' and fault['layer'] == l:                # one stream, one step reads a zero where x(t - 2d) belongs
            tap0 = tap0.clone(); tap0[fault['stream'], fault['step']] = 0
        zb = None
        for k in ('residual_block_causal_conv/bias', 'residual_block_cin_conv/bias'):
            if bias(p + k) is not None:
                zb = bias(p + k) if zb is None else zb + bias(p + k)
        zp = mm(tap0, Wd[0]) + mm(_shift(h, d), Wd[1])                     # modules.py:291-297
        if cu is not None:
            zp = zp + mm(cu, W(p + 'residual_block_cin_conv/kernel')[0])
        bvec = torch.zeros(1, P64[p + 'residual_block_causal_conv/kernel'].shape[-1], dtype=dt) if zb is None else zb[None, :]
        if gvec is not None:                                         # modules.py:503-508: fp32 matvec, per-stream bias
            bg = bias(p + 'residual_block_gin_conv/bias')
            zg = gvec @ P64[p + 'residual_block_gin_conv/kernel'][0].to(dt)
            bvec = bvec + (zg if bg is None else zg + bg)
        zp = zp + q32(bvec)[:, None, :]
        if path == 'pipeline':
            zp = q32(zp)                                             # z_past
        z = zp + mm(h, Wd[2])
        u = q(torch.tanh(z[..., :GH]) * torch.sigmoid(z[..., GH:]))  # modules.py:494, :510
        Ws = W(p + 'residual_block_skip_conv/kernel', scale[l] if fold else 1.0)[0]      # [GH, S]
        for j in range(Pn):
            cols = slice(32 * j, 32 * j + 32) if Pn > 1 else slice(None)
            v = mm(u[..., cols], Ws[cols])
            if not fold:
                v = v * scale[l]
            skip[j] = q32(v) if skip[j] is None else q32(skip[j] + v)
        if l + 1 < L:
            Wo = W(p + 'residual_block_out_conv/kernel')[0]          # [GH, R]
            bo = bias(p + 'residual_block_out_conv/bias')
            if Pn > 1:
                acc = None
                for j in range(Pn):
                    cols = slice(32 * j, 32 * j + 32)
                    o = mm(u[..., cols], Wo[cols])
                    if j == 0:
                        o = o + h if bo is None else o + h + bo
                    o = q(o * rho)
                    acc = o if acc is None else acc + o
                h = q(acc)
            else:
                o = mm(u, Wo)
                h = q(((o if bo is None else o + bo) + h) * rho)     # modules.py:512-521
    sb = None
    for l in range(L):
        b = bias('ResidualConv1DGLU_%d/residual_block_skip_conv/bias' % l)
        if b is not None:
            sb = b * scale[l] if sb is None else sb + b * scale[l]
    tot = skip[0]
    for j in range(1, Pn):
        tot = tot + skip[j]
    if sb is not None:
        tot = tot + q32(sb)
    r1 = q(torch.relu(tot))                                          # wavenet.py:840
    h2 = q(torch.relu(mm(r1, W('final_convolution_1/kernel')[0]) + bias('final_convolution_1/bias')))
    y = q32(mm(h2, W('final_convolution_2/kernel')[0]) + bias('final_convolution_2/bias'))
    y = y.transpose(1, 2).contiguous()
    if fk == 'neighbour':                                            # one step delivers its neighbour's output
        y[fault['stream'], :, fault['step']] = y[fault['stream'], :, fault['step'] - 1]
    return y.to(torch.float64)


def f64_params(params):
    return {k: v.to(torch.float64) for k, v in params.items()}


# ------------------------------------------------------------------------------------------------------------------ the check
def yardstick(ref, emul):
    """Y[o] = max over (b, t) of |emul - ref|, floored at 2^-24 max |ref[:, o, :]|."""
    y = (emul - ref).abs().amax(dim=(0, 2))
    return torch.maximum(y, FLOOR * ref.abs().amax(dim=(0, 2)))


def describe_step(cfg, path, b, t, T, head_cus=1, instance_of=None):
    """Which kernel edges step t of stream b sits on."""
    notes, again = [], []
    for l, d in enumerate(cfg.dilations()):
        s = ring_slots(path, d)
        names = {d - 1: 'd-1', d: 'd', 2 * d - 1: '2d-1', 2 * d: '2d', s - 1: 'slots-1', s: 'slots', s + d: 'slots+d', s + 2 * d: 'slots+2d'}
        if t in names:
            notes.append('layer %d (d=%d, %d slots): t=%s' % (l, d, s, names[t]))
        elif t > s and t % s == 0:
            again.append(l)
    if again:
        notes.append('slot 0 of the rings of layers %s written again' % ', '.join(map(str, again)))
    if t > 0 and t % cfg.hop == 0:
        notes.append('hop boundary (frame %d)' % (t // cfg.hop))
    if t == 0:
        notes.append('first step')
    if t == T - 1:
        notes.append('last step')
    inst = 0 if instance_of is None else int(instance_of[b])
    first = 0 if instance_of is None else list(instance_of).index(inst)
    notes.append('head CU %d of %d, instance %d' % ((b - first) % max(head_cus, 1), max(head_cus, 1), inst))
    return notes


def instance_map(B, ni):
    """stream -> pipeline instance (wn_synth_pipe.hip:1317: iB[i] = B / ni + (i < B % ni))."""
    out = []
    for i in range(ni):
        out += [i] * (B // ni + (1 if i < B % ni else 0))
    return out


def check_steps(dev, ref, emul, factor, cfg, path, head_cus=1, instances=1, what=''):
    """Every element, no exclusions:  |dev - ref|[b, o, t] <= factor * Y[o].

    factor = 4 on the 16-bit paths: Y is already the maximum over B * T draws of the error population a correct implementation belongs
    to (the per-step maximum is 1.9 - 3.7 x its median; the same emulation in float32 arithmetic lands at 0.99 - 1.58 x Y), and the mildest
    seeded fault lands at 6.4 x Y.  factor = 8 for the fp32 mode: the project's convention for a float32 yardstick.
    Raises AssertionError naming where; returns the record of the worst element (a record, not a threshold)."""
    dev = dev.to(torch.float64); B, Oc, T = ref.shape
    assert dev.shape == ref.shape and torch.isfinite(dev).all()
    Y = yardstick(ref, emul)
    ratio = (dev - ref).abs() / Y[None, :, None]
    inst = instance_map(B, instances)
    worst = int(ratio.argmax())
    b, o, t = worst // (Oc * T), (worst // T) % Oc, worst % T
    rec = {'worst_ratio': float(ratio[b, o, t]), 'stream': b, 'channel': o, 'step': t, 'factor': factor, 'floor': FLOOR,
           'Y_min': float(Y.min()), 'Y_max': float(Y.max()), 'where': describe_step(cfg, path, b, t, T, head_cus, inst),
           'rel_l2': float((dev - ref).norm() / ref.norm())}
    bad = ratio > factor
    if bad.any():
        per_step = ratio.amax(dim=1)                                # [B, T]
        lines = []
        order = torch.argsort(per_step.flatten(), descending=True)[:8]
        for i in order.tolist():
            bb, tt = i // T, i % T
            if per_step[bb, tt] <= factor:
                break
            oo = int(ratio[bb, :, tt].argmax())
            lines.append('  stream %d step %d channel %d: err %.3e / bound %.3e = %.2f x F | %s' % (
                bb, tt, oo, float((dev - ref).abs()[bb, oo, tt]), factor * float(Y[oo]), float(ratio[bb, oo, tt]) / factor,
                '; '.join(describe_step(cfg, path, bb, tt, T, head_cus, inst))))
        raise AssertionError('%s [%s]: %d of %d elements (%d steps) beyond %g x Y\n%s' % (
            what, path, int(bad.sum()), bad.numel(), int((per_step > factor).sum()), factor, '\n'.join(lines)))
    return rec


# ------------------------------------------------------------------------------------------------------------------ the models
PAPER_WIDTH = dict(residual_channels=256, gate_channels=512, skip_out_channels=256, cin_channels=80, num_mels=80)
S6 = dict(layers=6, stacks=1)
MODELS = {       # overrides of hip_util.SMALL
    's6': dict(S6),                                                 # d = 1 ... 32: the d = 32 ring has 128 slots on every path, t = 128 ... 192 read wrapped slots
    's8x2': dict(layers=8, stacks=2),                               # the dilation cycle restarts (d = 8 followed by d = 1)
    's6_gauss': dict(S6, out_channels=2, legacy=True, residual_legacy=True, upsample_type='SubPixel'),
    's6_softmax': dict(S6, input_type='mulaw-quantize', out_channels=256, quantize_channels=256),
    's6_gin': dict(S6, gin_channels=16, use_speaker_embedding=True, n_speakers=4),
    's6_gin_raw_1d': dict(S6, gin_channels=8, use_speaker_embedding=False, use_bias=False, upsample_type='1D'),
    'w128': dict(residual_channels=128, skip_out_channels=128, gate_channels=256, layers=8, stacks=2),       # width specialisation 2 (P = 4)
    'w256': dict(PAPER_WIDTH, layers=6, stacks=2),                  # width specialisation 1 (P = 8), batched pre-multiplication
}


def make_case(name, B, T, extra=None):
    """(hp, cfg, params, inputs [B, T] (floats / class ids), wav, c [B, C, Tc], g) of a model of the table: the seeds of test_hip_synth._setup."""
    from hip_util import SMALL, make_hp, oracle_cfg, synth_batch
    from oracle import mulaw as M
    hp = make_hp(**dict(SMALL, **MODELS[name], **(extra or {})))
    cfg = oracle_cfg(hp)
    assert T % cfg.hop == 0
    params = O.init_params(cfg, seed=11, bias_scale=0.05)
    wav, c = synth_batch(cfg, B, T, seed=3)
    inputs = wav if cfg.scalar_input else torch.from_numpy(M.mulaw_quantize(wav.numpy())).int()
    g = None
    if cfg.gin_channels > 0:
        gg = torch.Generator().manual_seed(5)
        g = (torch.randint(0, cfg.n_speakers, (B,), generator=gg).int() if cfg.use_speaker_embedding
             else torch.randn(B, cfg.gin_channels, generator=gg))
    return hp, cfg, params, inputs, wav, c, g
