"""Every launch of the training backward chain (and the forward launches that feed it) restated as ONE operation on stored buffers,
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
