"""Float64 references of the weight path (csrc/wn_pack.hip): weight normalisation forward and backward, the fragment-ordered bf16 operand
packs, and the two bias sums.  Plain numpy (torch only for the bf16 rounding), no autograd.  tests/test_wnorm_ref_cpu.py pins them to the oracle
and to float64 autograd; tests/test_hip_weightnorm.py holds the device to them element by element.

Every bound below is derived from the arithmetic the kernels document; none is fitted to a device.  u = 2^-24 is the relative error of one fp32
rounding.

rho.  The HIP math documentation (the "HIP math API" page with the ULP table of the device functions) does not come with the ROCm install:
its share/doc/hip holds only the doxygen index of the runtime API, and no .md / .rst / .txt / .html file of the install names rsqrtf.  For that
case rho = 2 ulps is the agreed value for rsqrtf; one ulp is at most 2^-23 relative, i.e. 2 u.

Forward (wn_weightnorm_apply_kernel), per kernel column (one output channel, K = numel / cout elements):
    ss  = sum_k v_k^2          sequential fp32: term k passes through at most K roundings (its product, then the additions behind it), every term
                               is >= 0, so |ss~ - ss| <= K u ss (first order).  max(., 1e-12) does not increase a relative error (the constant
                               1e-12f is itself 1e-12 (1 + <= u)).
    inv = rsqrtf(max(ss, c))   the root halves the relative error of its argument: K/2 u, plus rho ulps of rsqrtf = 2 rho u.
    sc  = g * inv, W = v * sc  two multiplies: 2 u.
    =>  |dev - ref| <= (K/2 + 2 + 2 rho) u |ref|.   A column with ss = 0 has v = 0: every product is exactly 0.
Everything that is not a normalised kernel is a copy: bit-exact.

Backward (wn_weightnorm_grad_kernel), per column, with e_inv = (K/2 + 2 rho) u the relative error of inv from above and
A = sum_k |dW_k v_k|:
    dot = sum_k dW_k v_k       a SIGNED sequential sum: |dot~ - dot| <= K u A (not K u |dot|).
    d g = dot * inv            |err| <= inv ((e_inv + u) |dot| + K u A).
    a   = g * inv              relative error e_inv + u.
    b   = dot * inv * inv      |b~ - b| <= (2 e_inv + 2 u) |b| + K u A inv^2 =: db.
    t   = v_k * b              |err| <= |v_k| db + u |v_k b|.
    d   = dW_k - t             one more rounding of a difference of two numbers of magnitudes |dW_k| and |v_k b|: u (|dW_k| + |v_k| |b|).  The
                               cancellation is bounded through the OPERANDS, never through |d|:
                               |d~ - d| <= |v_k| db + 2 u (|dW_k| + |v_k| |b|) =: E_d.
    d v = a * d                |err| <= |a| (E_d + (e_inv + 2 u) |d|).
Products of two of these relative errors are dropped; each is below K u <= 2^-10 of a first-order term at K <= 2^14, so the first-order sum is
multiplied by SECOND_ORDER = 1 + 2^-10 (the convention of launch_ref.py).  Where the reference is 0 (the K = 1 column of
input_convolution/kernel: v b = dW exactly, d = 0) the bound stays at |a| (|v| db + 4 u |dW|) ~ (2 K + 4 rho + 8) u |g / v| |dW|: about a
dozen fp32 roundings of the two numbers that cancel.
The entries of the 8-float alignment gaps of the raw layout are exactly 0.

B1SUM[l, g] = b_dil + b_cin: ONE fp32 addition, correctly rounded: |err| <= u |ref| (and bit-equal to the numpy float32 sum).
SKIPB[s] = sum_l c_l b_skip_l[s], sequential from 0: term l passes through at most L roundings: |err| <= L u sum_l |c_l b_l|; with every c_l = 1 the
products are exact and the fp32 sum in layer order is reproduced bit for bit (L = 1 included).

Packs: every element is bf16(scale * param) with the product in fp32, a deterministic function of the effective fp32 parameters: bit equality.
The logical matrices are restated from the comments of wn_build_packs, the storage order from the fragment formula at the top of wn_pack.hip:
    out[((mtile * KS + ks) * 64 + lane) * 8 + j]  <->  W[m = mtile * 32 + (lane & 31)][k = ks * 16 + 8 * (lane >> 5) + j],   KS = K / 16."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import wavenet_oracle as O

U24 = 2.0 ** -24
RHO = 2.0                       # ulps of rsqrtf (see the module docstring: the documentation is not on the machine)
CLAMP = 1e-12                   # tf.nn.l2_normalize epsilon (modules.py:98-103)
SECOND_ORDER = 1.0 + 2.0 ** -10
SQRT_HALF_F32 = float(np.float32(0.70710678118654752440))

LAYER_PACKS = ('w1', 'wo', 'ws', 'w2T', 'w1T')
GLOBAL_PACKS = ('wskip', 'wh1', 'wh2', 'wh2T', 'wh1T', 'wcT')
PACK_KINDS = LAYER_PACKS + GLOBAL_PACKS


def np64(t):
    return t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def np32(t):
    return t.detach().cpu().float().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float32)


def is_normalised(raw, k):
    return k.endswith('/kernel') and (k[:-6] + 'g') in raw


# ------------------------------------------------------------------------------------------------------------------ shared cases (CPU and GPU file)
WN = dict(wavenet_weight_normalization=True)
CONFIGS = {
    'mol_weightnorm': dict(WN, wavenet_dropout=0.05),
    'gauss_weightnorm_gin_nobias': dict(WN, out_channels=2, use_bias=False, gin_channels=8, use_speaker_embedding=True, n_speakers=3,
                                        upsample_type='SubPixel', log_scale_min_gauss=float(np.log(1e-7))),
    'wnorm_nobias_1d': dict(WN, out_channels=2, use_bias=False, upsample_type='1D', log_scale_min_gauss=float(np.log(1e-7))),
    'wnorm_resize': dict(WN, upsample_type='Resize', upsample_scales=[2, 8], upsample_activation='LeakyRelu'),
    'wnorm_softmax': dict(WN, input_type='mulaw-quantize', out_channels=256, quantize_channels=256, upsample_activation='LeakyRelu'),
    # both kernels walk channels, and the elements of a copied tensor, with a stride of 4 x 256 threads: cout = 2048 (dilated and conditioning kernels
    # [3, 64, 2048], [1, 16, 2048], gin [1, 16, 2048]) and copies above 1024 floats (the 2048-float biases, an 80 x 16 embedding) take the loops twice
    'gate2048_embed1280': dict(WN, gate_channels=2048, layers=2, stacks=1, gin_channels=16, use_speaker_embedding=True, n_speakers=80),
}
CRAFT_TENSOR = 'ResidualConv1DGLU_1/residual_block_out_conv/kernel'       # [1, GH, R]: K = 64


def wn_params(cfg, seed=5339):
    """Raw (v, g, bias, ...) parameters with the gains moved off ||v|| (as test_hip_parity._run_fwd does)."""
    params = O.init_params(cfg, seed=seed, bias_scale=0.05)
    g = torch.Generator().manual_seed(7)
    for k in params:
        if k.startswith('local_conditioning') and k.endswith('kernel'):
            params[k] = params[k] + 0.05 * torch.randn(params[k].shape, generator=g)
    for k in params:
        if k.endswith('/g'):
            params[k] = params[k] * (torch.rand(params[k].shape, generator=g) * 0.8 + 0.6)
    return params


def craft_columns(params, name=CRAFT_TENSOR):
    """Columns 0 .. 4 of one kernel: zeros; ss = 0.99e-12 (below the clamp); ss = 1.01e-12 (above it); magnitude 1e3; a negative gain."""
    v = params[name].clone()
    K = v.numel() // v.shape[-1]
    v2 = v.view(K, -1)
    v2[:, 0] = 0.0
    for col, ss in ((1, 0.99e-12), (2, 1.01e-12)):
        v2[:, col] = v2[:, col] * float(np.sqrt(ss) / float(v2[:, col].double().norm()))
    v2[:, 3] = v2[:, 3] * float(1e3 / float(v2[:, 3].abs().max()))
    params[name] = v
    g = params[name[:-6] + 'g'].clone()
    g[4] = -g[4].abs() - 0.25
    params[name[:-6] + 'g'] = g
    ss = (v2.double() ** 2).sum(0)
    assert float(ss[0]) == 0.0 and float(ss[1]) < 1e-12 < float(ss[2]) and float(v2[:, 3].abs().max()) > 999.0
    return params


def random_deff(params, seed=3):
    g = torch.Generator().manual_seed(seed)
    return OrderedDict((k, torch.randn(v.shape, generator=g) * 0.1) for k, v in params.items() if not k.endswith('/g'))


# ------------------------------------------------------------------------------------------------------------------ layouts
def effective_layout(raw_layout):
    """The effective layout of csrc/wn_api.hip build_layout from the raw one (name -> (shape, offset) in wn_tensor_info order): the same tensors
    without the gains, each at the next multiple of 8 floats.  Returns (layout, n_params)."""
    out, n = OrderedDict(), 0
    for name, (shape, _) in raw_layout.items():
        if name.endswith('/g'):
            continue
        out[name] = (tuple(shape), n)
        n = (n + int(np.prod(shape)) + 7) // 8 * 8
    return out, n


def split_flat(flat, layout):
    flat = np.asarray(flat)
    return OrderedDict((k, flat[off:off + int(np.prod(shape))].reshape(shape).copy()) for k, (shape, off) in layout.items())


def gap_mask(layout, n):
    """True where no tensor of the layout lives (the alignment gaps)."""
    m = np.ones(n, dtype=bool)
    for shape, off in layout.values():
        m[off:off + int(np.prod(shape))] = False
    return m


# ------------------------------------------------------------------------------------------------------------------ weight normalisation
def ref_effective(raw, cfg):
    """kernel = v * g * rsqrt(max(sum_k v^2, 1e-12)) over all axes but the last, float64; everything else a copy (dtype kept: bit-exact)."""
    out = OrderedDict()
    for k, t in raw.items():
        if k.endswith('/g'):
            continue
        if cfg.wavenet_weight_normalization and is_normalised(raw, k):
            v, g = np64(t), np64(raw[k[:-6] + 'g'])
            v2 = v.reshape(-1, v.shape[-1])
            ss = (v2 * v2).sum(0)
            out[k] = (v2 * g * (1.0 / np.sqrt(np.maximum(ss, CLAMP)))).reshape(v.shape)
        else:
            out[k] = np.array(t.detach().cpu().numpy() if torch.is_tensor(t) else t)
    return out


def bound_effective(raw, cfg, ref):
    """(K/2 + 2 + 2 rho) u |ref| for the normalised kernels, 0 (bit-exact) for the copies."""
    out = OrderedDict()
    for k, r in ref.items():
        if cfg.wavenet_weight_normalization and is_normalised(raw, k):
            K = r.size // r.shape[-1]
            out[k] = (K / 2.0 + 2.0 + 2.0 * RHO) * U24 * np.abs(r)
        else:
            out[k] = np.zeros(r.shape)
    return out


def ref_raw_grads(raw, deff, want_bound=False):
    """d g = dot / n,  d v = (g / n) (dW - v dot / n^2),  n = sqrt(max(ss, 1e-12)),  dot = sum_k dW v  -- the expressions of
    wn_weightnorm_grad_kernel, float64.  deff: name -> d L / d (effective tensor).  Tensors without a gain: copies.  want_bound: also the bound
    of the module docstring per element (0 for the copies)."""
    out, bnd = OrderedDict(), OrderedDict()
    for k, t in raw.items():
        if k.endswith('/g'):
            continue
        if not is_normalised(raw, k):
            out[k] = np.array(np.asarray(deff[k]))
            bnd[k] = np.zeros(out[k].shape)
            continue
        v, g, dW = np64(t), np64(raw[k[:-6] + 'g']), np64(deff[k])
        cout = v.shape[-1]
        v2, d2 = v.reshape(-1, cout), dW.reshape(-1, cout)
        K = v2.shape[0]
        ss = (v2 * v2).sum(0)
        dot = (d2 * v2).sum(0)
        inv = 1.0 / np.sqrt(np.maximum(ss, CLAMP))
        a, b = g * inv, dot * inv * inv
        diff = d2 - v2 * b
        out[k] = (a * diff).reshape(v.shape)
        out[k[:-6] + 'g'] = dot * inv
        if want_bound:
            A = np.abs(d2 * v2).sum(0)
            e_inv = (K / 2.0 + 2.0 * RHO) * U24
            bnd[k[:-6] + 'g'] = SECOND_ORDER * inv * ((e_inv + U24) * np.abs(dot) + K * U24 * A)
            db = (2.0 * e_inv + 2.0 * U24) * np.abs(b) + K * U24 * A * inv * inv
            E_d = np.abs(v2) * db + 2.0 * U24 * (np.abs(d2) + np.abs(v2) * np.abs(b))
            bnd[k] = (SECOND_ORDER * np.abs(a) * (E_d + (e_inv + 2.0 * U24) * np.abs(diff))).reshape(v.shape)
    if want_bound:
        return OrderedDict((k, out[k]) for k in raw), OrderedDict((k, bnd[k]) for k in raw)
    return OrderedDict((k, out[k]) for k in raw)


# ---- the same expressions in numpy float32 with one sequential accumulator over k: the yardstick of the bounds (and, with a fault, the stand-in
# of a wrong kernel in tests/test_wnorm_ref_cpu.py)
F32_FAULTS = ('gain_omitted', 'clamp_on_sqrt', 'no_projection')


def _f32_column_sums(v2, d2=None):
    ss = np.zeros(v2.shape[1], dtype=np.float32)
    dot = np.zeros(v2.shape[1], dtype=np.float32)
    for k in range(v2.shape[0]):
        ss = ss + v2[k] * v2[k]
        if d2 is not None:
            dot = dot + d2[k] * v2[k]
    return ss, dot


def _f32_inv(ss, fault):
    one, c = np.float32(1.0), np.float32(CLAMP)
    if fault == 'clamp_on_sqrt':
        return one / np.maximum(np.sqrt(ss), c)
    return one / np.sqrt(np.maximum(ss, c))


def f32_effective(raw, cfg, fault=None):
    out = OrderedDict()
    for k, t in raw.items():
        if k.endswith('/g'):
            continue
        if cfg.wavenet_weight_normalization and is_normalised(raw, k):
            v, g = np32(t), np32(raw[k[:-6] + 'g'])
            v2 = v.reshape(-1, v.shape[-1])
            ss, _ = _f32_column_sums(v2)
            sc = _f32_inv(ss, fault) * (np.float32(1.0) if fault == 'gain_omitted' else g)
            out[k] = (v2 * sc).reshape(v.shape)
        else:
            out[k] = np.array(t.detach().cpu().numpy() if torch.is_tensor(t) else t)
    return out


def f32_raw_grads(raw, deff, fault=None):
    out = OrderedDict()
    for k, t in raw.items():
        if k.endswith('/g'):
            continue
        if not is_normalised(raw, k):
            out[k] = np.array(np.asarray(deff[k]))
            continue
        v, g, dW = np32(t), np32(raw[k[:-6] + 'g']), np32(deff[k])
        v2, d2 = v.reshape(-1, v.shape[-1]), dW.reshape(-1, v.shape[-1])
        ss, dot = _f32_column_sums(v2, d2)
        inv = _f32_inv(ss, fault)
        a = (np.float32(1.0) if fault == 'gain_omitted' else g) * inv
        b = dot * inv * inv
        out[k] = (a * (d2 if fault == 'no_projection' else d2 - v2 * b)).reshape(v.shape)
        out[k[:-6] + 'g'] = dot * inv
    return OrderedDict((k, out[k]) for k in raw)


# ------------------------------------------------------------------------------------------------------------------ bias sums
def layer_bias(eff, l, which, n):
    b = eff.get('ResidualConv1DGLU_%d/residual_block_%s_conv/bias' % (l, which))
    return np.zeros(n, dtype=np.float32) if b is None else np32(b)      # (use_bias = False: the device reads its zero tail)


def skip_scales(cfg):
    """csrc/wn_api.hip: (float)pow((double)WN_SQRT_HALF, e), e = L - 1 for layer 0, else L - l, when legacy; 1 otherwise."""
    L = cfg.layers
    return [np.float32(SQRT_HALF_F32 ** ((L - 1 if l == 0 else L - l) if cfg.legacy else 0)) for l in range(L)]


def ref_b1sum(eff, cfg):
    """[L, G] float64, its bound u |ref|, and the fp32 sum (one correctly rounded addition: the device must equal it bit for bit)."""
    G = cfg.gate_channels
    a = np.stack([layer_bias(eff, l, 'causal', G) for l in range(cfg.layers)])
    b = np.stack([layer_bias(eff, l, 'cin', G) for l in range(cfg.layers)])
    ref = a.astype(np.float64) + b.astype(np.float64)
    return ref, U24 * np.abs(ref), a + b


def ref_skipb(eff, cfg):
    """[S] float64, its bound L u sum_l |c_l b_l|, the fp32 sum in layer order (a += c_l * b_l, product and sum rounded separately), and whether
    that sum must be met bit for bit: when every c_l is 1 the products are exact; otherwise the device may fuse product and sum."""
    S, L = cfg.skip_out_channels, cfg.layers
    sc = skip_scales(cfg)
    bs = [layer_bias(eff, l, 'skip', S) for l in range(L)]
    ref = sum(float(sc[l]) * bs[l].astype(np.float64) for l in range(L))
    bound = L * U24 * sum(abs(float(sc[l])) * np.abs(bs[l].astype(np.float64)) for l in range(L))
    f32 = np.zeros(S, dtype=np.float32)
    for l in range(L):
        f32 = f32 + sc[l] * bs[l]
    return ref, bound, f32, all(float(s) == 1.0 for s in sc)


# ------------------------------------------------------------------------------------------------------------------ packs
def bf16_round(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def pack_geometry(cfg, kind, gemm8p=0, NT=0):
    """(M, K, kil, gate_interleave) of a pack from the configuration alone (wn_build_packs: M to 32 rows -- wcT to 96 or 128 --, K to 16
    columns; kil = 32 where the LDS-DMA tile engine takes the matrix, 64 where the 8-phase kernel was asked for (gemm8p bit 0: w1, bit 1: w1T)
    and fits; NT = max_batch * max_time enters its 32-bit offset condition)."""
    L, R, G, S, O, C = cfg.layers, cfg.residual_channels, cfg.gate_channels, cfg.skip_out_channels, cfg.out_channels, cfg.cin_channels
    GH = G // 2
    up = lambda x, a: (x + a - 1) // a * a      # noqa: E731
    dims = {'w1': (G, 3 * R + C), 'wo': (R, GH), 'ws': (S, GH), 'w2T': (GH, R + S), 'w1T': (R, 3 * G), 'wskip': (S, L * GH), 'wh1': (S, S),
            'wh2': (O, S), 'wh2T': (S, O), 'wh1T': (S, S), 'wcT': (C, L * G)}
    m, k = dims[kind]
    M = up(m, (96 if C <= 96 else 128) if kind == 'wcT' else 32)
    kil = 0
    if kind == 'w1':
        kil = 32 if (G % 128 == 0 and R % 32 == 0) else 0
        if (gemm8p & 1) and G % 256 == 0 and R % 64 == 0 and C % 16 == 0 and NT * max(R, C) * 2 < 2 ** 31:
            kil = 64
    if kind == 'w1T':
        kil = 32 if (R % 128 == 0 and G % 32 == 0) else 0
        if (gemm8p & 2) and R % 256 == 0 and G % 64 == 0 and NT * G * 2 < 2 ** 31:
            kil = 64
    return M, up(k, 16), kil, 1 if kind == 'w1' else 0


def _taps_along_k(a, kil):
    """a [rows, 3, n] (tap, channel) -> [rows, 3 n]: tap-major, or with kil > 0 in blocks of kil channels [tap0 blk0 | tap1 blk0 | tap2 blk0 | tap0 blk1 ...]."""
    rows, _, n = a.shape
    if kil:
        assert n % kil == 0
        a = a.reshape(rows, 3, n // kil, kil).transpose(0, 2, 1, 3)
    return a.reshape(rows, 3 * n)


def logical_matrix(eff, cfg, kind, layer, kil):
    """The padded [M, K] matrix a pack holds, row m / column k as the MFMA A operand sees them, bf16-rounded values in float32.
    eff: the EFFECTIVE fp32 parameters.  Sources (comments of wn_build_packs):
        w1    rows = gate channels in 64-row groups [32 tanh rows | their 32 sigmoid partners], K = [tap0 R | tap1 R | tap2 R | cin C]: dil[j][r][g], cin[c][g]
        wo    [r][g'] = out_k[g'][r]          ws [s][g'] = c_l skip_k[g'][s]          w2T [g'][r | R + s] = out_k[g'][r] | c_l skip_k[g'][s]
        w1T   [r][j G + g] = dil[j][r][g]     wskip [s][l GH + g'] = c_l skip_k_l[g'][s]
        wh1   [o][i] = fin1[i][o]             wh2 [o][i] = fin2[i][o]                 wh2T [i][o] = fin2[i][o]        wh1T [i][o] = fin1[i][o]
        wcT   [c][l G + g] = cin_l[c][g]
    c_l (the legacy skip factor) multiplies in fp32 BEFORE the bf16 rounding; padding rows and columns are exact zeros."""
    L, G = cfg.layers, cfg.gate_channels
    GH = G // 2
    q = 'ResidualConv1DGLU_%d/residual_block_' % layer
    e = lambda name: np32(eff[name])      # noqa: E731
    sc = skip_scales(cfg)
    if kind == 'w1':
        dil, cin = e(q + 'causal_conv/kernel'), e(q + 'cin_conv/kernel')[0]           # [3, R, G], [C, G]
        W = np.concatenate([_taps_along_k(dil.transpose(2, 0, 1), kil), cin.T], axis=1)
        # packed row (group, half, i) <- gate channel half * GH + group * 32 + i
        src = np.arange(G // 64)[:, None, None] * 32 + np.arange(2)[None, :, None] * GH + np.arange(32)[None, None, :]
        W = W[src.reshape(-1)]
    elif kind == 'wo':
        W = e(q + 'out_conv/kernel')[0].T
    elif kind == 'ws':
        W = (sc[layer] * e(q + 'skip_conv/kernel')[0]).T
    elif kind == 'w2T':
        W = np.concatenate([e(q + 'out_conv/kernel')[0], sc[layer] * e(q + 'skip_conv/kernel')[0]], axis=1)
    elif kind == 'w1T':
        W = _taps_along_k(e(q + 'causal_conv/kernel').transpose(1, 0, 2), kil)        # [R, 3, G]
    elif kind == 'wskip':
        W = np.concatenate([(sc[l] * e('ResidualConv1DGLU_%d/residual_block_skip_conv/kernel' % l)[0]).T for l in range(L)], axis=1)
    elif kind == 'wh1':
        W = e('final_convolution_1/kernel')[0].T
    elif kind == 'wh2':
        W = e('final_convolution_2/kernel')[0].T
    elif kind == 'wh2T':
        W = e('final_convolution_2/kernel')[0]
    elif kind == 'wh1T':
        W = e('final_convolution_1/kernel')[0]
    elif kind == 'wcT':
        W = np.concatenate([e('ResidualConv1DGLU_%d/residual_block_cin_conv/kernel' % l)[0] for l in range(L)], axis=1)
    else:
        raise KeyError(kind)
    assert W.dtype == np.float32
    M, K, _, _ = pack_geometry(cfg, kind)
    out = np.zeros((M, K), dtype=np.float32)
    out[:W.shape[0], :W.shape[1]] = bf16_round(W)
    return out


def fragment_order(W):
    """[M, K] -> storage order: element (mtile, ks, lane, j) = W[mtile * 32 + (lane & 31)][ks * 16 + 8 * (lane >> 5) + j]."""
    M, K = W.shape
    assert M % 32 == 0 and K % 16 == 0
    a = W.reshape(M // 32, 32, K // 16, 2, 8)          # (mtile, lane & 31, ks, lane >> 5, j)
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1, 4)).reshape(-1)


def unfragment(flat, M, K):
    """The inverse of fragment_order, written per element from the formula (not as the inverse transpose)."""
    flat = np.asarray(flat)
    assert flat.size == M * K
    i = np.arange(M * K)
    j, lane, rest = i % 8, (i // 8) % 64, i // 512
    KS = K // 16
    ks, mtile = rest % KS, rest // KS
    W = np.empty((M, K), dtype=flat.dtype)
    W[mtile * 32 + (lane & 31), ks * 16 + 8 * (lane >> 5) + j] = flat
    return W


def ref_pack(eff, cfg, kind, layer, kil):
    return fragment_order(logical_matrix(eff, cfg, kind, layer, kil))


# ------------------------------------------------------------------------------------------------------------------ comparison
def compare(kind, tensor, dev, ref, bound):
    """Every element: |dev - ref| <= bound, and exactly equal where the bound is 0.  Returns (worst err / bound, index of the worst element,
    message or None); the message names kind and tensor."""
    dev64, ref64, bound = np64(dev).reshape(-1), np64(ref).reshape(-1), np64(bound).reshape(-1)
    assert dev64.shape == ref64.shape == bound.shape, (kind, tensor, dev64.shape, ref64.shape, bound.shape)
    if dev64.size == 0:
        return 0.0, 0, None
    err = np.abs(dev64 - ref64)
    err = np.where(np.isfinite(dev64), err, np.inf)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(ratio))
    worst = float(ratio[i])
    msg = None
    if worst > 1.0:
        msg = '%s %s: %d of %d elements over the bound, worst err/bound %.3g at flat index %d: dev %.9g ref %.9g bound %.3g' % (
            kind, tensor, int((ratio > 1.0).sum()), ratio.size, worst, i, dev64[i], ref64[i], bound[i])
    return worst, i, msg


def compare_bits(kind, tensor, dev, ref):
    """Bit equality of two float32 arrays.  Returns (number of differing elements, first index, message or None)."""
    d = np.ascontiguousarray(np32(dev)).reshape(-1).view(np.uint32)
    r = np.ascontiguousarray(np32(ref)).reshape(-1).view(np.uint32)
    assert d.shape == r.shape, (kind, tensor, d.shape, r.shape)
    bad = np.nonzero(d != r)[0]
    if bad.size == 0:
        return 0, 0, None
    i = int(bad[0])
    return int(bad.size), i, '%s %s: %d of %d elements differ in their bits, first at storage index %d: dev %.9g ref %.9g' % (
        kind, tensor, bad.size, d.size, i, float(d[i:i + 1].view(np.float32)[0]), float(r[i:i + 1].view(np.float32)[0]))
