"""Every launch of the training forward and backward chains restated as ONE operation on stored buffers,
in float64: plain torch, no autograd (except ref_dy, see there).  Inputs are exactly the buffers the kernel reads, outputs the buffers
it writes, so a comparison against the device sees one launch at a time: which launch, which layer, which row.

Layouts: activations / gradients are [B, T, channels] (the device's row = b * T + t, channels contiguous); kernels keep the TensorFlow
layouts of the parameter table.  Taps never cross an utterance: a row outside [0, T) of ITS utterance is zero.

Two modes of the operands (`Weights(..., rounded=)`):
  * rounded=True  -- what the device's contractions see: kernels rounded to bf16 the way csrc/wn_pack.hip rounds them (the legacy skip
    factor folded in fp32 BEFORE the rounding: bf16(W_skip * float32(c_l))), float32 epilogue constants (sqrt(.5), 1 / (1 - p));
  * rounded=False -- the same expressions on unrounded float64 operands: tests/test_launch_ref_cpu.py pins them to float64 autograd of the
    oracle to 1e-10, so that a misreading shared between these formulas and the kernels cannot hide.

Every chain function returns (ref, bound); bound is None unless want_bound.  The bound is the element-wise
    |dev - ref| <= 2^-8 |ref| + K 2^-23 A' + E
  * 2^-8 |ref|: the final bf16 store (half an ulp is at most 2^-8 relative at the bottom of a binade); absent for fp32 outputs;
  * K 2^-23 A': worst-case fp32 accumulation of K products, A = sum_k |a_k| |b_k| in float64, pushed through the epilogue's factors
    (2^-23 rather than 2^-24 so that a truncating MFMA adder is covered);
  * E: the epilogue's own fp32 arithmetic, derived per launch in the function's docstring.
All three are derived from the arithmetic; nothing is fitted to what a device returns.  Where ref == 0 and A == 0 the bound is 0: the
device must be exactly 0 there (rows past a ragged length, GX[L], the masked half of EPI_MASK_STORE)."""
import numpy as np
import torch

from oracle import wavenet_oracle as O

U23 = 2.0 ** -23
U24 = 2.0 ** -24
BF = 2.0 ** -8
SQRT_HALF_F32 = float(np.float32(0.70710678118654752440))      # csrc/wn_common.h: WN_SQRT_HALF


def bf16(t):
    """float -> float32 -> bf16 (round to nearest even, as v_cvt_pk_bf16_f32 / torch) -> float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def rows(x):
    """[B, T, ch] -> [B * T, ch]"""
    return x.reshape(-1, x.shape[-1])


def shift_time(x, s):
    """y[b, t] = x[b, t + s] inside the utterance, 0 outside (x [B, T, ch])."""
    if s == 0:
        return x
    T = x.shape[1]
    y = torch.zeros_like(x)
    if abs(s) >= T:
        return y
    if s > 0:
        y[:, :T - s] = x[:, s:]
    else:
        y[:, -s:] = x[:, :T + s]
    return y


class Weights:
    """The kernels of every contraction as the launch sees them, float64, + the epilogue constants."""

    def __init__(self, params, cfg, rounded=True):
        eff = O.effective_params(params, cfg)
        self.cfg, self.rounded = cfg, rounded
        L = cfg.layers
        self.L = L
        rd = bf16 if rounded else (lambda t: t.to(torch.float64))
        p = float(cfg.wavenet_dropout)
        if rounded:
            half = SQRT_HALF_F32
            self.res_scale = half if cfg.residual_legacy else 1.0
            # csrc/wn_api.hip: (float)pow((double)WN_SQRT_HALF, e), e = L-1 for layer 0, else L-l, when legacy
            self.skip_scale = [float(np.float32(half ** ((L - 1 if l == 0 else L - l) if cfg.legacy else 0))) for l in range(L)]
            self.keep_scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
        else:
            half = O.SQRT_HALF
            self.res_scale = half if cfg.residual_legacy else 1.0
            self.skip_scale = [half ** ((L - 1 if l == 0 else L - l) if cfg.legacy else 0) for l in range(L)]
            self.keep_scale = 1.0 / (1.0 - p)
        self.dil = cfg.dilations()
        self.w_dil, self.w_cin, self.w_out, self.w_skip, self.b_out = [], [], [], [], []
        for l in range(L):
            q = 'ResidualConv1DGLU_%d/' % l
            self.w_dil.append(rd(eff[q + 'residual_block_causal_conv/kernel']))            # [3, R, G]
            self.w_cin.append(rd(eff[q + 'residual_block_cin_conv/kernel'][0]))             # [C, G]
            self.w_out.append(rd(eff[q + 'residual_block_out_conv/kernel'][0]))             # [GH, R]
            ws = eff[q + 'residual_block_skip_conv/kernel'][0]                              # [GH, S]
            if rounded:      # wn_pack_kernel: sg.scale * params[...] in fp32, then the bf16 store
                self.w_skip.append(bf16(ws.to(torch.float32) * torch.tensor(self.skip_scale[l], dtype=torch.float32)))
            else:
                self.w_skip.append(ws.to(torch.float64) * self.skip_scale[l])
            b = eff.get(q + 'residual_block_out_conv/bias')
            self.b_out.append(None if b is None else b.to(torch.float64))
        self.fin1 = rd(eff['final_convolution_1/kernel'][0])      # [S, S]  (in, out)
        self.fin2 = rd(eff['final_convolution_2/kernel'][0])      # [S, O]
        self.w_in = eff['input_convolution/kernel'][0].to(torch.float64)      # [Cin, R]: fp32 on the device, never rounded
        self.b_in = eff['input_convolution/bias'].to(torch.float64)
        # the forward launches' fp32 biases (None: use_bias = False, the device reads zeros) and the fp32 global-conditioning kernel
        f64 = lambda k: None if eff.get(k) is None else eff[k].to(torch.float64)      # noqa: E731
        self.b_dil = [f64('ResidualConv1DGLU_%d/residual_block_causal_conv/bias' % l) for l in range(L)]
        self.b_cin = [f64('ResidualConv1DGLU_%d/residual_block_cin_conv/bias' % l) for l in range(L)]
        self.b_gin = [f64('ResidualConv1DGLU_%d/residual_block_gin_conv/bias' % l) for l in range(L)]
        self.b_skip = [f64('ResidualConv1DGLU_%d/residual_block_skip_conv/bias' % l) for l in range(L)]
        self.w_gin = [None if cfg.gin_channels <= 0 else eff['ResidualConv1DGLU_%d/residual_block_gin_conv/kernel' % l][0].to(torch.float64) for l in range(L)]      # [gin, G]
        self.b_fin1 = eff['final_convolution_1/bias'].to(torch.float64)
        self.b_fin2 = eff['final_convolution_2/bias'].to(torch.float64)


def _mm(a, b):
    return torch.matmul(a, b)


# ------------------------------------------------------------------------------------------------------------------ head
def ref_dpre1(W, DY, H2, want_bound=False):
    """csrc/wn_train.hip bwd_head, EPI_MASK_STORE: d pre1[row, s] = (H2 > 0) ? sum_o DY[row, o] fin2[s, o] : 0.
    DY [B, T, ldDY] (columns >= O are zero padding and take no part).  K = ldDY.  E = 0: the epilogue multiplies by scale = 1 (exact)."""
    Oc = W.fin2.shape[1]
    v = _mm(DY[..., :Oc], W.fin2.t())
    keep = H2 > 0
    ref = torch.where(keep, v, torch.zeros_like(v))
    if not want_bound:
        return ref, None
    A = torch.where(keep, _mm(DY[..., :Oc].abs(), W.fin2.t().abs()), torch.zeros_like(v))
    return ref, BF * ref.abs() + DY.shape[-1] * U23 * A


def ref_dskip(W, DPRE1, R1, want_bound=False):
    """bwd_head, EPI_MASK_STORE: d skip[row, s] = (R1 > 0) ? sum_k DPRE1[row, k] fin1[s, k] : 0.  K = S, E = 0."""
    v = _mm(DPRE1, W.fin1.t())
    keep = R1 > 0
    ref = torch.where(keep, v, torch.zeros_like(v))
    if not want_bound:
        return ref, None
    A = torch.where(keep, _mm(DPRE1.abs(), W.fin1.t().abs()), torch.zeros_like(v))
    return ref, BF * ref.abs() + W.fin1.shape[0] * U23 * A


# ------------------------------------------------------------------------------------------------------------------ chain
def gate_tanh_from(u, s):
    """csrc/wn_tile.h gate_tanh_from: tanh recovered from the stored u = tanh * sigmoid and s = sigmoid."""
    t = torch.where(s > 0, u / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(u))
    return t.clamp(-1.0, 1.0)


def ref_dz(W, l, GX_up, DSKIP, TS, U, want_bound=False):
    """mk_dgate / EPI_DGATE / gate_backward of layer l:
        g[row, c] = sum_r GX[l+1][row, r] W_out[c, r] + sum_s DSKIP[row, s] (c_l W_skip)[c, s]          (K = R + S)
        t = clamp(u / s, -1, 1) (0 where s == 0);   d a = g s (1 - t^2);   d b = g u (1 - s);   DZ[l] = [d a | d b].
    E: with |g| <= |g_ref| + K 2^-23 A =: gm.  t = u * rcp(s): the 1-ulp v_rcp_f32 and one product, |dt| <= 3 * 2^-24 |t|;
    1 - t^2 is ONE fma (2^-24 absolute, its value is <= 1) + 2 |t| |dt| <= 6 * 2^-24: 7 * 2^-24 ABSOLUTE (the subtraction cancels, so the
    error of d a is absolute in |g| s); the two products add 2 * 2^-24 relative:  E(d a) = 10 * 2^-24 gm s.
    1 - s: exact for s >= 1/2 (Sterbenz), else 2^-25 absolute on a value >= 1/2; two products:  E(d b) = 4 * 2^-24 gm |u| (1 - s)."""
    g = _mm(GX_up, W.w_out[l].t()) + _mm(DSKIP, W.w_skip[l].t())
    t = gate_tanh_from(U, TS)
    fa = TS * (1.0 - t * t)
    fb = U * (1.0 - TS)
    ref = torch.cat([g * fa, g * fb], dim=-1)
    if not want_bound:
        return ref, None
    A = _mm(GX_up.abs(), W.w_out[l].t().abs()) + _mm(DSKIP.abs(), W.w_skip[l].t().abs())
    K = GX_up.shape[-1] + DSKIP.shape[-1]
    acc = K * U23 * A
    gm = g.abs() + acc
    bound = BF * ref.abs() + torch.cat([acc * fa.abs() + 10 * U24 * gm * TS, acc * fb.abs() + 4 * U24 * gm * fb.abs()], dim=-1)
    return ref, bound


def ref_gx(W, l, DZ, mask, GX_up, want_bound=False):
    """mk_dx / EPI_DX of layer l (modules.py:484, 517-520 differentiated):
        v[b, t, r] = sum_j sum_g W_dil[j, r, g] DZ[l][b, t + (2 - j) d, g]      (rows past the utterance end are zero; K = 3 G)
        GX[l] = scale * (mask ? v / (1 - p) : 0  +  GX[l+1]),   scale = res_scale for l > 0, 1 for layer 0; no GX[l+1] term for the top layer.
    mask: {0,1} [B, T, R] or None (dropout 0).  GX_up: GX[l+1] or None (top layer).
    E: three fp32 roundings (v * keep_scale, + GX[l+1], * scale), each half an ulp of an intermediate that is at most
    (|v| keep_scale + |GX[l+1]|):  E = 4 * 2^-24 (gm keep_scale + |GX[l+1]|) scale, gm = |v_ref| + K 2^-23 A."""
    d = W.dil[l]
    G = DZ.shape[-1]
    v = 0
    for j in range(3):
        v = v + _mm(shift_time(DZ, (2 - j) * d), W.w_dil[l][j].t())
    ks = W.keep_scale if mask is not None else 1.0
    scale = W.res_scale if l > 0 else 1.0
    m = mask if mask is not None else 1.0
    ref = v * m * ks
    if GX_up is not None:
        ref = ref + GX_up
    ref = ref * scale
    if not want_bound:
        return ref, None
    A = 0
    Da = DZ.abs()
    for j in range(3):
        A = A + _mm(shift_time(Da, (2 - j) * d), W.w_dil[l][j].t().abs())
    acc = 3 * G * U23 * A * m * ks
    gm = (v.abs() * m + 3 * G * U23 * A * m) * ks
    up = GX_up.abs() if GX_up is not None else 0.0
    bound = BF * ref.abs() + (acc + 4 * U24 * (gm + up)) * scale
    return ref, bound


def ref_x_next(W, l, U, X, want_bound=False):
    """mk_out / EPI_STORE_BF16 of layer l <= L-2 (modules.py:517-520): X[l+1] = (U[l] W_out + b_out + X[l]) * res_scale.
    K = GH + 1 (the bias is one more addend of the accumulator).  E: + X[l] and * res_scale, half an ulp each of at most
    (|acc| + |X[l]|):  E = 3 * 2^-24 (gm + |X[l]|) res_scale, gm = |acc_ref| + K 2^-23 A."""
    v = _mm(U, W.w_out[l])
    b = W.b_out[l]
    if b is not None:
        v = v + b
    ref = (v + X) * W.res_scale
    if not want_bound:
        return ref, None
    A = _mm(U.abs(), W.w_out[l].abs())
    if b is not None:
        A = A + b.abs()
    K = U.shape[-1] + 1
    acc = K * U23 * A
    bound = BF * ref.abs() + (acc + 3 * U24 * (v.abs() + acc + X.abs())) * W.res_scale
    return ref, bound


def ref_xd(W, X_dev, mask):
    """The dropout-applied conv input, BIT-EXACT from the device's own X: bf16(float32(X) * float32(1 / (1 - p))) where kept, else 0
    (csrc/wn_tile.h EPI_STORE_BF16 out1, csrc/wn_frontend.hip wn_first_conv_fwd).  The fp32 product rounds before the bf16 store."""
    if mask is None:
        return X_dev
    prod = X_dev.to(torch.float32) * torch.tensor(W.keep_scale, dtype=torch.float32)
    return torch.where(mask > 0, prod, torch.zeros_like(prod)).to(torch.bfloat16).to(torch.float64)


def ref_x0(W, x_in, want_bound=False, w_ulps=0):
    """csrc/wn_frontend.hip wn_first_conv_fwd (wavenet.py:705): X[0][row, r] = W_in[cin, r] x[cin] + b[r] with the fp32 kernel (never rounded).
    x_in: [B, T] float (scalar input) or [B, T] int64 class ids (one-hot input: a row gather).
    E: one product and one sum in fp32 (or one fma): 2 * 2^-24 (|W x| + |b|).  w_ulps: fp32 ulps by which the device's kernel may differ
    from W.w_in -- 0 for a stored kernel; 8 under weight normalisation, where both sides COMPUTE v g / ||v|| in fp32 (square, rsqrt, two
    products: up to 4 roundings each side)."""
    if x_in.dtype in (torch.int32, torch.int64):
        prod = W.w_in[x_in.long()]
    else:
        prod = x_in.to(torch.float64)[..., None] * W.w_in[0]
    ref = prod + W.b_in
    if not want_bound:
        return ref, None
    return ref, BF * ref.abs() + 2 * U24 * (prod.abs() + W.b_in.abs()) + w_ulps * U24 * prod.abs()


def ref_dc_accumulate(W, l, DZ, acc, want_bound=False):
    """One layer's share of d c_up (csrc/wn_train.hip, the d c GEMM: ONE contraction over all layers, K = L * G):
    DC[b, cc, t] = sum_l sum_g DZ[l][b, t, g] W_cin[l][cc, g].  acc = (ref, A) running sums ([B, T, C]) or None."""
    r = _mm(DZ, W.w_cin[l].t())
    a = _mm(DZ.abs(), W.w_cin[l].t().abs()) if want_bound else None
    if acc is None:
        return r, a
    return acc[0] + r, (acc[1] + a if want_bound else None)


def dc_bound(W, acc, G):
    """fp32 output, EPI_STORE_F32_BOT with scale = 1 and no bias (v * 1 + 0 is exact): K 2^-23 A alone, K = L * G."""
    return W.L * G * U23 * acc[1]


# ------------------------------------------------------------------------------------------------------------------ loss
def ref_dy(cfg, yhat, y, lengths, dtype=torch.float64):
    """d loss / d y_hat as autograd of the oracle's loss gives it on the device's own YHAT ([B, O, T] fp32): the one place where autograd
    IS the plain reference.  Returns [B, T, O]."""
    yh = yhat.to(dtype).clone().requires_grad_(True)
    yy = y if y.dtype in (torch.int32, torch.int64) else y.to(dtype)
    loss = O.training_loss(cfg, yh, yy, lengths)
    (g,) = torch.autograd.grad(loss, [yh])
    return g.permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------------------------------------------------------ weight gradients
def contract(A, B, scale=1.0, yardstick=False):
    """scale * A^T B over all rows (A [rows, m], B [rows, n]) in float64; with yardstick also the rel-L2 distance of the SAME contraction
    evaluated in float32 with one running accumulator over 128-row blocks in row order (a longer dependent chain than the device's
    split-K) from the float64 result."""
    ref = _mm(A.t(), B) * scale
    if not yardstick:
        return ref, None
    A32, B32 = A.to(torch.float32), B.to(torch.float32)
    acc = torch.zeros(A.shape[1], B.shape[1], dtype=torch.float32)
    for r0 in range(0, A.shape[0], 128):
        acc += _mm(A32[r0:r0 + 128].t(), B32[r0:r0 + 128])
    acc = acc * torch.tensor(scale, dtype=torch.float32)
    n = float(ref.norm())
    return ref, (float((acc.to(torch.float64) - ref).norm()) / n if n > 0 else 0.0)


def colsum(B, scale=1.0, yardstick=False):
    ref = B.sum(0) * scale
    if not yardstick:
        return ref, None
    B32 = B.to(torch.float32)
    acc = torch.zeros(B.shape[1], dtype=torch.float32)
    for r0 in range(0, B.shape[0], 128):
        acc += B32[r0:r0 + 128].sum(0)
    acc = acc * torch.tensor(scale, dtype=torch.float32)
    n = float(ref.norm())
    return ref, (float((acc.to(torch.float64) - ref).norm()) / n if n > 0 else 0.0)


def ref_wgrads_layer(W, l, XD, cbt, DZ, U, DSKIP, GX_up, yardstick=False):
    """The weight gradients of layer l (csrc/wn_train.hip wgrad_*_args, stack_wgrads) from the stored buffers, name -> (ref, yardstick):
        d W_dil[j, r, g] = sum_{b,t} XD[l][b, t - (2 - j) d, r] DZ[l][b, t, g]      (rows before the utterance start are zero)
        d W_cin[cc, g]   = sum cbt[b, t, cc] DZ[l][b, t, g];     d b_dil = d b_cin = column sums of DZ[l]
        d W_skip[c, s]   = c_l sum U[l][b, t, c] DSKIP[b, t, s];  d b_skip = c_l column sums of DSKIP
        d W_out[c, r]    = sum U[l][b, t, c] GX[l+1][b, t, r];    d b_out = column sums of GX[l+1]      (exact zeros for the top layer)."""
    d = W.dil[l]
    q = 'ResidualConv1DGLU_%d/' % l
    out = {}
    dz = rows(DZ)
    taps = [contract(rows(shift_time(XD, -(2 - j) * d)), dz, 1.0, yardstick) for j in range(3)]
    out[q + 'residual_block_causal_conv/kernel'] = (torch.stack([t[0] for t in taps]), max(t[1] for t in taps) if yardstick else None)
    r, y = contract(rows(cbt), dz, 1.0, yardstick)
    out[q + 'residual_block_cin_conv/kernel'] = (r[None], y)
    bz = colsum(dz, 1.0, yardstick)
    out[q + 'residual_block_causal_conv/bias'] = bz
    out[q + 'residual_block_cin_conv/bias'] = bz
    r, y = contract(rows(U), rows(DSKIP), W.skip_scale[l], yardstick)
    out[q + 'residual_block_skip_conv/kernel'] = (r[None], y)
    out[q + 'residual_block_skip_conv/bias'] = colsum(rows(DSKIP), W.skip_scale[l], yardstick)
    r, y = contract(rows(U), rows(GX_up), 1.0, yardstick)
    out[q + 'residual_block_out_conv/kernel'] = (r[None], y)
    out[q + 'residual_block_out_conv/bias'] = colsum(rows(GX_up), 1.0, yardstick)
    return out


def taps_leak(W, l, XD, DZ):
    """What d W_dil of layer l would GAIN if the taps read across the utterance start into the previous utterance's last rows (the rows
    b * T + t - (2 - j) d of the flat buffer with t - (2 - j) d < 0, b > 0): [3, R, G].  Zero for a single utterance."""
    d = W.dil[l]
    B, T, R = XD.shape
    flat = rows(XD)
    out = []
    for j in range(3):
        s = (2 - j) * d
        acc = torch.zeros(R, DZ.shape[-1], dtype=torch.float64)
        n = min(s, T)
        for b in range(1, B):
            first = b * T - s                      # flat row that t = 0 of utterance b would read
            skip = max(0, -first)                  # (a tap longer than everything in front of b: nothing there to leak from)
            if n > skip:
                acc += _mm(flat[first + skip: first + n].t(), DZ[b, skip:n])
        out.append(acc)
    return torch.stack(out)


def ref_wgrads_head(W, R1, H2, DPRE1, DY, yardstick=False):
    """d final_convolution_1 [S, S] = R1^T DPRE1 (+ bias = column sums of DPRE1), d final_convolution_2 [S, O] = H2^T DY (+ column sums of DY)."""
    Oc = W.fin2.shape[1]
    out = {}
    r, y = contract(rows(R1), rows(DPRE1), 1.0, yardstick)
    out['final_convolution_1/kernel'] = (r[None], y)
    out['final_convolution_1/bias'] = colsum(rows(DPRE1), 1.0, yardstick)
    r, y = contract(rows(H2), rows(DY)[:, :Oc], 1.0, yardstick)
    out['final_convolution_2/kernel'] = (r[None], y)
    out['final_convolution_2/bias'] = colsum(rows(DY)[:, :Oc], 1.0, yardstick)
    return out


def ref_wgrads_input(W, x_in, GX0, yardstick=False):
    """csrc/wn_frontend.hip wn_first_conv_grad: d W_in[cin, r] = sum_rows x[cin] GX[0][row, r], d b_in = column sums of GX[0]."""
    g = rows(GX0)
    if x_in.dtype in (torch.int32, torch.int64):
        a = torch.nn.functional.one_hot(x_in.reshape(-1).long(), W.w_in.shape[0]).to(torch.float64)
    else:
        a = x_in.reshape(-1, 1).to(torch.float64)
    out = {}
    r, y = contract(a, g, 1.0, yardstick)
    out['input_convolution/kernel'] = (r[None], y)
    out['input_convolution/bias'] = colsum(g, 1.0, yardstick)
    return out


def ref_wgrads_gin(params, cfg, gvec, ids, DZ_colsums, dtype=torch.float64):
    """csrc/wn_frontend.hip wn_gin_bwd from the per-utterance column sums of DZ (list over layers of [B, G] float64):
    d b_g[l] = sum_b colsum;  d W_g[l][k, g] = sum_b g_b[k] colsum[l][b, g];  d embedding[id_b, k] += sum_l sum_g W_g[l][k, g] colsum[l][b, g]."""
    out = {}
    gv = gvec.to(dtype)
    demb = torch.zeros(cfg.n_speakers, cfg.gin_channels, dtype=dtype) if ids is not None else None
    for l, cs in enumerate(DZ_colsums):
        cs = cs.to(dtype)
        q = 'ResidualConv1DGLU_%d/' % l
        out[q + 'residual_block_gin_conv/kernel'] = _mm(gv.t(), cs)[None]
        out[q + 'residual_block_gin_conv/bias'] = cs.sum(0)
        if demb is not None:
            dg = _mm(cs, params[q + 'residual_block_gin_conv/kernel'][0].to(dtype).t())      # [B, gin]
            demb.index_add_(0, ids.long(), dg)
    if demb is not None:
        out['gc_embedding'] = demb
    return out


# ------------------------------------------------------------------------------------------------------------------ forward chain
# Every function below: store=False leaves the bf16 store out of the bound (tests/test_launch_ref_cpu.py holds a plain float32 evaluation,
# which stores nothing to bf16, to the K 2^-23 A + E part alone).  With the store the bound is 2^-8 (|ref| + e) + e, e = K 2^-23 A + E: the
# store rounds the DEVICE's fp32 value, which is at most |ref| + e.
TINY = 2.0 ** -126                    # v_exp_f32 / v_rcp_f32 flush denormal results: an absolute 2^-126 where a function is saturated
TANH_D2 = 4.0 / (3.0 * 3.0 ** 0.5)    # sup |tanh''|    = 4 / (3 sqrt 3), at tanh^2 = 1/3
SIGM_D2 = 1.0 / (6.0 * 3.0 ** 0.5)    # sup |sigmoid''| = 1 / (6 sqrt 3), at sigmoid = 1/2 +- 1 / (2 sqrt 3)
SECOND_ORDER = 1.0 + 2.0 ** -10       # products of two of the relative errors counted in E (each below 2^-10 of a first-order term, see ref_gate)


def _with_store(ref_abs, e, store):
    return BF * (ref_abs + e) + e if store else e


def ref_gate_bias(W, params, cfg, gvec, w_ulps=0):
    """The fp32 bias vector mk_gate passes to EPI_GATE, float64, + the absolute error of the device's fp32 value: (bias, err), each [L, Bb, G],
    Bb = 1 without global conditioning, else B (bias_bstride = G: one vector per utterance).
      * csrc/wn_pack.hip wn_pairsum_kernel: b1sum[l] = fl(b_dil[l] + b_cin[l]) (zeros when use_bias = False): ONE rounding, 2^-24 |b_dil + b_cin|
        <= 2^-24 (|b_dil| + |b_cin|);
      * csrc/wn_frontend.hip wn_gbias_kernel: a = fl(b1sum + b_g), then a = fl(a + g_b[k] W_g[k]) for k < gin, sequentially.  Every addend
        passes through at most gin + 1 further additions and each product through one rounding of its own (none if the compiler contracts
        to an fma): (gin + 3) 2^-24 Ab, Ab = |b_dil| + |b_cin| + |b_g| + sum_k |g_b[k]| |W_g[k]|, pairsum included.
    gvec [B, gin]: the embedding rows (an exact fp32 copy, wn_gvec_kernel) or the raw features; W_g is the fp32 kernel (never rounded).
    w_ulps: fp32 ulps by which the device's W_g may differ from W.w_gin (weight normalisation, as in ref_x0)."""
    L, G = W.L, W.w_dil[0].shape[-1]
    zero = torch.zeros(G, dtype=torch.float64)
    bias, err = [], []
    for l in range(L):
        bd = W.b_dil[l] if W.b_dil[l] is not None else zero
        bc = W.b_cin[l] if W.b_cin[l] is not None else zero
        if cfg.gin_channels <= 0 or gvec is None:
            bias.append((bd + bc)[None])
            err.append(U24 * (bd.abs() + bc.abs())[None])
            continue
        bg = W.b_gin[l] if W.b_gin[l] is not None else zero
        gv = gvec.to(torch.float64)
        mv = _mm(gv, W.w_gin[l])                                   # [B, G]
        Amv = _mm(gv.abs(), W.w_gin[l].abs())
        bias.append(bd + bc + bg + mv)
        err.append((cfg.gin_channels + 3) * U24 * (bd.abs() + bc.abs() + bg.abs() + Amv) + w_ulps * U24 * Amv)
    return torch.stack(bias), torch.stack(err)


def _fast_sigmoid_err(xabs, s, one_minus_s):
    """|fast_sigmoid(x) - sigmoid(x)| of csrc/wn_tile.h for fp32 x (arguments: upper bounds of |x|, sigmoid, 1 - sigmoid):
        p = fl(x * c), c = fl(-log2 e): two roundings, |dp| <= 2 * 2^-24 |p|, so 2^p moves by ln 2 |dp| = 2 * 2^-24 |x| relative;
        e = v_exp_f32(p): 1 ulp = 2 * 2^-24 relative           -> rel(e) <= 2^-24 (2 |x| + 2)
        q = fl(1 + e): e / (1 + e) = 1 - sigmoid of rel(e), + 2^-24
        s = v_rcp_f32(q): 1 ulp = 2 * 2^-24                     -> rel(s) <= 2^-24 ((1 - s) (2 |x| + 2) + 3)."""
    return s * U24 * (one_minus_s * (2.0 * xabs + 2.0) + 3.0) * SECOND_ORDER + TINY


def _fast_tanh_err(xabs, tabs, one_minus_t, half_one_plus_t):
    """|fast_tanh(x) - tanh(x)| (arguments: upper bounds of |x|, |tanh|, 1 - tanh, (1 + tanh) / 2):
        p = fl(x * c), c = fl(2 log2 e): 2^p moves by ln 2 |dp| = 2 * 2^-24 * 2 |x| relative; e = v_exp_f32(p): + 2 * 2^-24  -> rel(e) <= 2^-24 (4 |x| + 2)
        q = fl(e + 1): e / (1 + e) = (1 + tanh) / 2 of rel(e), + 2^-24;   r = v_rcp_f32(q): + 2 * 2^-24
        t = fl(1 - 2 r) (2 r is exact; one rounding, fma or not): 2 r = 1 - tanh, so |dt| <= (1 - tanh) rel(r) + 2^-24 |t|."""
    return (one_minus_t * U24 * (half_one_plus_t * (4.0 * xabs + 2.0) + 3.0) + U24 * tabs) * SECOND_ORDER + 2.0 * TINY


def gate_preactivation(W, l, XD, cbt, bias, want_bound=False):
    """z [B, T, G] of layer l and (want_bound) the bound of the device's fp32 accumulator against it:
        z = sum_j shift_time(XD, -(2 - j) d) W_dil[j] + cbt W_cin + bias       (taps before the utterance start are zero)
    K = 3 R + C + 1: the bias is one more addend (the ring / 8-phase main loops START the accumulators at it, the 64-row tile kernel adds it in
    the epilogue: one rounding either way).  dz = K 2^-23 A + err(bias), A = sum |x| |w| + |bias|."""
    d = W.dil[l]
    b, eb = bias
    z = _mm(cbt, W.w_cin[l]) + b[:, None, :]
    for j in range(3):
        z = z + _mm(shift_time(XD, -(2 - j) * d), W.w_dil[l][j])
    if not want_bound:
        return z, None
    A = _mm(cbt.abs(), W.w_cin[l].abs()) + b.abs()[:, None, :]
    Xa = XD.abs()
    for j in range(3):
        A = A + _mm(shift_time(Xa, -(2 - j) * d), W.w_dil[l][j].abs())
    K = 3 * XD.shape[-1] + cbt.shape[-1] + 1
    return z, K * U23 * A + eb[:, None, :]


def ref_gate(W, l, XD, cbt, bias, want_bound=False, store=True, z_out=None):
    """mk_gate / EPI_GATE of layer l (modules.py:484-510): ref = (TS, U), TS = sigmoid(z_b), U = tanh(z_a) sigmoid(z_b), z = [z_a | z_b] from
    gate_preactivation.  XD: the conv input the launch stages (XD[l]; X[l] with dropout 0 and under wn_eval_fwd); bias = (bias[l], err[l]) of
    ref_gate_bias.  bound = (bound TS, bound U), in four steps:
      1. the accumulator: |z_dev - z| <= dz = K 2^-23 A + err(bias) (gate_preactivation), da / db its two halves;
      2. through the nonlinearities, exactly (Taylor with the Lagrange remainder): |tanh(z_a + da) - tanh(z_a)| <= (1 - t^2) da + da^2 sup|tanh''| / 2
         =: Dt, |sigmoid(z_b + db) - sigmoid(z_b)| <= s (1 - s) db + db^2 sup|sigmoid''| / 2 =: Ds (sup|tanh''| = 4 / (3 sqrt 3), sup|sigmoid''| =
         1 / (6 sqrt 3));
      3. fast_tanh / fast_sigmoid on the DEVICE's z (_fast_tanh_err, _fast_sigmoid_err, derived there from their instruction sequence), so
         they are evaluated at the upper ends |z| + dz, s + Ds, |t| + Dt, ...:  et = Dt + Et, es = Ds + Es;
         u = fl(t s): |du| <= s et + |t| es + et es, + 2^-24 of the product;
         second-order products of the relative errors inside Et / Es: every factor is below 2^-24 (4 |z| + 5) < 2^-10 for |z| < 2^11, and
         both functions are saturated to within 2^-126 long before (|z| > 89): the factor 1 + 2^-10 (SECOND_ORDER) covers them;
      4. the bf16 stores of TS and U: 2^-8 (|ref| + e).
    z_out: a list that receives z (for gate_start_leak's comparison)."""
    GH = W.w_dil[l].shape[-1] // 2
    z, dz = gate_preactivation(W, l, XD, cbt, bias, want_bound)
    if z_out is not None:
        z_out.append(z)
    za, zb = z[..., :GH], z[..., GH:]
    t, s = torch.tanh(za), torch.sigmoid(zb)
    u = t * s
    if not want_bound:
        return (s, u), None
    da, db = dz[..., :GH], dz[..., GH:]
    omt = 2.0 * torch.sigmoid(-2.0 * za)                           # 1 - tanh without cancellation
    oms = torch.sigmoid(-zb)                                       # 1 - sigmoid
    Dt = (1.0 - t * t) * da + 0.5 * TANH_D2 * da * da
    Ds = s * oms * db + 0.5 * SIGM_D2 * db * db
    Et = _fast_tanh_err(za.abs() + da, (t.abs() + Dt).clamp(max=1.0), (omt + Dt).clamp(max=2.0), (0.5 * (2.0 - omt + Dt)).clamp(max=1.0))
    Es = _fast_sigmoid_err(zb.abs() + db, (s + Ds).clamp(max=1.0), (oms + Ds).clamp(max=1.0))
    et, es = Dt + Et, Ds + Es
    du = s * et + t.abs() * es + et * es
    eu = du + U24 * (u.abs() + du)
    return (s, u), (_with_store(s, es, store), _with_store(u.abs(), eu, store))


def skip_bias_total(W):
    """csrc/wn_pack.hip wn_vecsum_kernel: a = 0; a = fl(a + c_l b_skip[l]) for l < L, (bias, err) [S]: every term passes through one product
    rounding (none under fma contraction) and at most L - 1 additions (0 + x is exact): L 2^-24 sum_l |c_l b_l|."""
    S = W.w_skip[0].shape[-1]
    b, a = torch.zeros(S, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)
    for l in range(W.L):
        if W.b_skip[l] is not None:
            b = b + W.skip_scale[l] * W.b_skip[l]
            a = a + abs(W.skip_scale[l]) * W.b_skip[l].abs()
    return b, W.L * U24 * a


def ref_r1(W, U_all, want_bound=False, store=True):
    """fwd_tail, the skip sum as ONE contraction (nrep = L) + EPI_STORE_BF16 with relu: R1 = relu(sum_l U[l] (c_l W_skip[l]) + skip_bias_total)
    (wavenet.py:706-719; W.w_skip[l] holds c_l W_skip, rounded as wn_pack_kernel rounds it).  U_all: an iterable of the L tensors U[l] [B, T, GH],
    consumed one at a time (a generator keeps one layer resident).  K = L GH + 1 (the bias is one more addend of the accumulator), + the error
    of the fp32 bias (skip_bias_total).  E = 0: the epilogue multiplies by scale = 1 (exact); ReLU is 1-Lipschitz, so the error of the
    accumulator carries over unchanged and no element near 0 needs excluding (a reference of 0 keeps its bound: the device may be a little
    above 0 there)."""
    b, eb = skip_bias_total(W)
    v, A, n = None, None, 0
    for l, U in enumerate(U_all):
        r = _mm(U, W.w_skip[l])
        v = r if v is None else v + r
        if want_bound:
            a = _mm(U.abs(), W.w_skip[l].abs())
            A = a if A is None else A + a
        n += 1
        K = n * U.shape[-1] + 1
    assert n == W.L, 'ref_r1 needs U of all %d layers (got %d)' % (W.L, n)
    ref = torch.relu(v + b)
    if not want_bound:
        return ref, None
    e = K * U23 * (A + b.abs()) + eb
    return ref, _with_store(ref, e, store)


def ref_h2(W, R1, want_bound=False, store=True):
    """fwd_tail, final_convolution_1 + EPI_STORE_BF16 with relu: H2 = relu(R1 fin1 + b) (wavenet.py:136-149).  K = S + 1, E = 0 (scale = 1; the
    fp32 bias is a parameter, read as stored)."""
    ref = torch.relu(_mm(R1, W.fin1) + W.b_fin1)
    if not want_bound:
        return ref, None
    e = (R1.shape[-1] + 1) * U23 * (_mm(R1.abs(), W.fin1.abs()) + W.b_fin1.abs())
    return ref, _with_store(ref, e, store)


def ref_yhat(W, H2, want_bound=False):
    """fwd_tail, final_convolution_2 + EPI_STORE_F32_BOT with M_valid = O: YHAT[b, o, t] = sum_s H2[b, t, s] fin2[s, o] + b[o], fp32, layout
    [B, O, T] (exactly O channels).  K = S; no bf16 store.  E: y = v * scale + bias with scale = 1 (exact product): ONE rounding of the sum (fma
    or not), 2^-24 (|v| + K 2^-23 A + |b|)."""
    v = _mm(H2, W.fin2)
    ref = (v + W.b_fin2).permute(0, 2, 1).contiguous()
    if not want_bound:
        return ref, None
    acc = H2.shape[-1] * U23 * _mm(H2.abs(), W.fin2.abs())
    e = acc + U24 * (v.abs() + acc + W.b_fin2.abs())
    return ref, e.permute(0, 2, 1).contiguous()


def _shift(x, s, dim):
    """y[..., i, ...] = x[..., i + s, ...] along dim, 0 outside."""
    n = x.shape[dim]
    y = torch.zeros_like(x)
    if abs(s) >= n:
        return y
    if s == 0:
        return x
    if s > 0:
        y.narrow(dim, 0, n - s).copy_(x.narrow(dim, s, n - s))
    else:
        y.narrow(dim, -s, n + s).copy_(x.narrow(dim, 0, n + s))
    return y


def ref_cup_level(params, cfg, i, inp, want_bound=False, rounded=True, w_ulps=0):
    """One level of the upsample net (csrc/wn_frontend.hip wn_up_fwd / wn_up_fwd_generic; modules.py:524-770) from the level's OWN input:
    inp [B, C, Tin] (level 0: c_in, level i: CUP[i-1]) -> CUP[i] [B, C, Tin s], s = upsample_scales[i], frequency padding pf = (fk - 1) / 2:
        NearestNeighbor (one level, s = hop)    out[f, t s + j] = in[f, t]                                                            exact copy
        2D        kernel [fk, s, 1, 1]          out[f, t s + j] = act(b + sum_kf in[f - kf + pf, t] K[kf, j])                         K = fk
        SubPixel  kernel [fk, 3, 1, s]          out[f, t s + j] = act(b[j] + sum_kf sum_kt in[f + kf - pf, t + kt - 1] K[kf, kt, j])  K = 3 fk
        Resize    kernel [fk, s, 1, 1]          out[f, to] = act(b + sum_kf sum_kt up[f + kf - pf, to + kt - (s - 1) / 2] K[kf, kt]),
                                                up[f, tu] = in[f, tu / s]                                                             K = fk s
        1D        kernel [1, s, C, C]           out[co, t s + j] = act(b[co] + sum_ci in[ci, t] K[j, co, ci])                         K = C
    (taps outside the frequency / time range are zero).  fp32 kernels, never rounded; rounded=True only takes leaky_alpha as the float32 the
    configuration struct carries.  Bound: v starts at the bias (exact) and takes K sequential v = fl(v + fl(in K)): K additions of partial
    sums that are at most A = |b| + sum |in| |K| each, and the products' own roundings, together at most A again: (K + 1) 2^-24 A; + 2^-24 |b|;
    LeakyRelu's alpha v is one more rounding, 2^-24 |ref|; every activation is 1-Lipschitz, so the rest carries over.  No bf16 store: CUP is
    fp32.  w_ulps: fp32 ulps by which the device's kernel may differ (weight normalisation, as in ref_x0)."""
    t = cfg.upsample_type
    x = inp.to(torch.float64)
    B, C, Tin = x.shape
    if t == 'NearestNeighbor':
        ref = torch.repeat_interleave(x, cfg.hop, dim=2)
        return ref, (torch.zeros_like(ref) if want_bound else None)
    eff = O.effective_params(params, cfg)
    s = cfg.upsample_scales[i]
    Kw = eff['local_conditioning_upsampling_%d/kernel' % (i + 1)].to(torch.float64)
    b = eff['local_conditioning_upsampling_%d/bias' % (i + 1)].to(torch.float64)
    fk = Kw.shape[0]
    pf = (fk - 1) // 2

    def run(xx, KK):
        if t == '2D':
            v = torch.zeros(B, C, Tin, s, dtype=torch.float64)
            for kf in range(fk):
                v = v + _shift(xx, pf - kf, 1)[..., None] * KK[kf, :, 0, 0]
            return v.reshape(B, C, Tin * s), fk
        if t == 'SubPixel':
            v = torch.zeros(B, C, Tin, s, dtype=torch.float64)
            for kf in range(fk):
                xf = _shift(xx, kf - pf, 1)
                for kt in range(3):
                    v = v + _shift(xf, kt - 1, 2)[..., None] * KK[kf, kt, 0, :]
            return v.reshape(B, C, Tin * s), 3 * fk
        if t == 'Resize':
            up = torch.repeat_interleave(xx, s, dim=2)
            pl = (s - 1) // 2
            v = torch.zeros(B, C, Tin * s, dtype=torch.float64)
            for kf in range(fk):
                xf = _shift(up, kf - pf, 1)
                for kt in range(s):
                    v = v + _shift(xf, kt - pl, 2) * KK[kf, kt, 0, 0]
            return v, fk * s
        if t == '1D':
            v = torch.einsum('bit,joi->botj', xx, KK[0])
            return v.reshape(B, C, Tin * s), C
        raise ValueError(t)

    v, K = run(x, Kw)
    if t == 'SubPixel':
        bb = b.repeat(Tin)                                         # b[j] at to = t s + j
    elif t == '1D':
        bb = b[:, None]
    else:
        bb = b
    v = v + bb
    act = cfg.upsample_activation
    alpha = float(np.float32(cfg.leaky_alpha)) if rounded else float(cfg.leaky_alpha)
    if act == 'Relu':
        ref = torch.relu(v)
    elif act == 'LeakyRelu':
        ref = torch.where(v > 0, v, alpha * v)
    else:
        assert act in (None, 'None')
        ref = v
    if not want_bound:
        return ref, None
    Ap, _ = run(x.abs(), Kw.abs())
    ba = (torch.zeros_like(v) + bb).abs()
    bound = (K + 1) * U24 * (Ap + ba) + U24 * ba + w_ulps * U24 * Ap
    if act == 'LeakyRelu':
        bound = bound + U24 * ref.abs()
    return ref, bound


def ref_cbt(CUP_last):
    """cbt, BIT-EXACT from the device's own last level: the bf16 rounding of CUP[last] [B, C, T], time-major [B, T, C] (the f2bf of the same
    fp32 value the kernel stores to CUP)."""
    return bf16(CUP_last).permute(0, 2, 1).contiguous()


def gate_start_leak(W, l, XD):
    """What z of layer l would GAIN if the taps read across the utterance start into the previous utterance's last rows (rows b T + t - (2 - j) d
    of the flat buffer with t < (2 - j) d, b > 0): [B, T, G], zero outside the first 2 d rows of the utterances b >= 1."""
    d = W.dil[l]
    B, T, R = XD.shape
    flat = rows(XD)
    out = torch.zeros(B, T, W.w_dil[l].shape[-1], dtype=torch.float64)
    for j in range(2):                                             # (the tap j = 2 has shift 0)
        sft = (2 - j) * d
        n = min(sft, T)
        for b in range(1, B):
            first = b * T - sft
            skip = max(0, -first)
            if n > skip:
                out[b, skip:n] += _mm(flat[first + skip: first + n], W.w_dil[l][j])
    return out
