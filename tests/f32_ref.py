"""float64 references of the fp32 training mode's kernels (csrc/wn_f32.hip), ONE launch each, written from the argument semantics of
SgemmArgs / WgradF32Args (the comments of those structs and of wgrad32), not from the kernel loops: plain torch on logical matrices.
The memory layout of an operand (pitch, offset, transposed strides) is the test's business; what a launch computes is stated here.

Rows are b * T + t for B utterances of T samples.  A row read through `shift` that falls outside [0, T) of ITS utterance is zero: a
tap never reads the neighbouring utterance.

Error bounds (nothing fitted; u = 2^-24 is half an ulp of fp32, 2 u = 2^-23 covers an adder that truncates):

  sgemm.  S = |alpha| keep sum_k |a_k| |w_k| over the products that take part, P = |prev| + |bias| + |add|.
    * the K products are rounded (u each) and summed in some order by at most K - 1 additions, each within 2 u of the partial sum's
      magnitude, which never exceeds sum |a_k||w_k|: together at most K 2^-23 sum |a||w|, in ANY order of summation;
    * keep_scale * a (or * v, on the output) and alpha * acc: one rounding each, u S each;
    * the epilogue: + prev, + bias, + add, * scale: four roundings of values no larger than S + P: 4 u (S + P) = 2^-22 (S + P);
    * second-order terms are below 2^-23 S for K <= 2^12.
    |dev - ref| <= |scale| ((K + 8) 2^-23 S + 2^-22 P): the first-order sum is (K + 1 + 2) 2^-23 S + 2^-22 P, the rest of the + 8 is slack for the
    second order.  ReLU and the mask are 1-Lipschitz / exact selections and add nothing; where the mask or a dropped OUTPUT element
    makes the result zero the bound is zero and the device must return exactly zero.
  wgrad.  The same with the N = B * T contracted rows in the place of K (the slab partial sums are further additions of the same sum:
    covered by "any order"), alpha applied once at the end:  |dev - ref| <= |alpha| (N + 8) 2^-23 keep sum_rows |a||b|.

With inputs of magnitude in [0.5, 1] one product is at least 0.25 keep |alpha scale|: `visible` below is the condition that a single
dropped or misplaced product moves an element by more than twice its bound (tests/test_f32_ref_cpu.py asserts it for every case)."""
import numpy as np
import torch

U23 = 2.0 ** -23
U22 = 2.0 ** -22


def shift_rows(x, B, T, s):
    """y[b * T + t] = x[b * T + t + s] when 0 <= t + s < T, else 0  (x [B * T, ch])."""
    x3 = x.reshape(B, T, -1)
    y = torch.zeros_like(x3)
    if abs(s) < T:
        if s >= 0:
            y[:, :T - s] = x3[:, s:]
        else:
            y[:, -s:] = x3[:, :T + s]
    return y.reshape(B * T, -1)


def to_bot(out, B, T):
    """[B * T, M] -> the y_hat layout [B, M, T] (out_bot = 1)."""
    return out.reshape(B, T, -1).permute(0, 2, 1).contiguous()


def ref_sgemm(In, W, B, T, shift=0, alpha=1.0, scale=1.0, prev=None, bias=None, add=None, relu=False, mask=None,
              keep_a=None, keep_out=None, keep_scale=1.0):
    """One sgemm launch.  In [B * T, K] (the K columns from col0 on), W [K, M] (logical: W[k][m] whatever its strides), prev the output
    buffer's earlier content when accumulate (else None), bias [M] or [B, M] (bias_bstride = M), add / mask [B * T, M], keep_a {0,1}
    [B * T, K]: the dropout keep mask of the A operand, indexed by the row that is READ; keep_out {0,1} [B * T, M]: drop_on_out.
    Epilogue order: alpha * acc, output dropout, + prev, + bias, + add, * scale, relu, mask.  Returns (ref, bound) [B * T, M] float64."""
    f = lambda t: None if t is None else t.to(torch.float64)      # noqa: E731
    In, W, prev, bias, add, mask, keep_a, keep_out = map(f, (In, W, prev, bias, add, mask, keep_a, keep_out))
    K = W.shape[0]
    assert In.shape == (B * T, K)
    A = In if keep_a is None else In * keep_a * keep_scale
    A = shift_rows(A, B, T, shift)
    v = alpha * (A @ W)
    S = abs(alpha) * (A.abs() @ W.abs())
    if keep_out is not None:
        v = v * keep_out * keep_scale
        S = S * keep_out * keep_scale
    P = torch.zeros_like(v)
    if prev is not None:
        v = v + prev; P = P + prev.abs()
    if bias is not None:
        bb = bias if bias.dim() == 1 else bias.repeat_interleave(T, dim=0)      # [B, M] -> one row per time row
        v = v + bb; P = P + bb.abs()
    if add is not None:
        v = v + add; P = P + add.abs()
    v = v * scale
    bound = abs(scale) * ((K + 8) * U23 * S + U22 * P)
    if relu:
        v = v.clamp_min(0.0)
    if mask is not None:
        on = mask > 0
        v = torch.where(on, v, torch.zeros_like(v))
        bound = torch.where(on, bound, torch.zeros_like(bound))
    return v, bound


def ref_wgrad(A, Bm, B, T, shift=0, alpha=1.0, keep_a=None, keep_scale=1.0):
    """One weight gradient.  A [B * T, K] or None (only the column sums), Bm [B * T, M], keep_a {0,1} [B * T, K] indexed by the row READ.
    Returns (dW [K, M] or None, bound, colsum [M] = alpha * column sums of Bm, its bound)."""
    Bm = Bm.to(torch.float64)
    N = B * T
    assert Bm.shape[0] == N
    cs = alpha * Bm.sum(0)
    cs_bound = abs(alpha) * (N + 8) * U23 * Bm.abs().sum(0)
    if A is None:
        return None, None, cs, cs_bound
    A = A.to(torch.float64)
    if keep_a is not None:
        A = A * keep_a.to(torch.float64) * keep_scale
    A = shift_rows(A, B, T, shift)
    dW = alpha * (A.t() @ Bm)
    bound = abs(alpha) * (N + 8) * U23 * (A.abs().t() @ Bm.abs())
    return dW, bound, cs, cs_bound


def ref_gate(Z, GU, dtype=torch.float64):
    """u = tanh(z_a) sigmoid(z_b); d z_a = gu s (1 - t^2), d z_b = gu t s (1 - s)  (Z [rows, 2 GH] = (z_a | z_b), GU [rows, GH]), evaluated in
    `dtype` with the formula as the kernels write it (1 / (1 + exp(-z)) for the sigmoid)."""
    Z = Z.to(dtype); GU = GU.to(dtype)
    GH = GU.shape[1]
    t = torch.tanh(Z[:, :GH])
    s = 1.0 / (1.0 + torch.exp(-Z[:, GH:]))
    U = t * s
    DZ = torch.cat([GU * s * (1.0 - t * t), GU * t * s * (1.0 - s)], dim=1)
    return U, DZ


def gate_bounds(Z, GU):
    """(U_ref, DZ_ref, U_bound, DZ_bound): float64 references and the per-element bound 8 x |float32 CPU evaluation - float64|, floored at
    2^-22 max(|ref|, |gu|) (|gu| = 1 for U): the yardstick is the same formula in the same precision on another implementation of tanh / exp."""
    U64, DZ64 = ref_gate(Z, GU, torch.float64)
    U32, DZ32 = ref_gate(Z, GU, torch.float32)
    g = GU.to(torch.float64).abs()
    ub = torch.maximum(8.0 * (U32.to(torch.float64) - U64).abs(), U22 * torch.maximum(U64.abs(), torch.ones_like(U64)))
    dzb = torch.maximum(8.0 * (DZ32.to(torch.float64) - DZ64).abs(), U22 * torch.maximum(DZ64.abs(), torch.cat([g, g], dim=1)))
    return U64, DZ64, ub, dzb


# ---------------------------------------------------------------------------------------------------------------- inputs
def exact_ints(gen, *shape):
    """integers in [-8, 8] as float64: exact in fp32 (and in bf16), so is every product and every partial sum below 2^24."""
    return torch.randint(-8, 9, shape, generator=gen).to(torch.float64)


def real_unit(gen, *shape):
    """magnitudes uniform in [0.5, 1] with random signs, rounded to float32 (the device reads these very values)."""
    m = 0.5 + 0.5 * torch.rand(*shape, generator=gen, dtype=torch.float64)
    s = torch.randint(0, 2, shape, generator=gen).to(torch.float64) * 2.0 - 1.0
    return (m * s).to(torch.float32).to(torch.float64)


def visible(bound, alpha=1.0, scale=1.0, keep_scale=1.0):
    """Does one dropped or misplaced product (>= 0.25 keep |alpha scale| with real_unit inputs) exceed twice the bound at every element,
    and is the bound at most 0.01?"""
    b = float(bound.max())
    return b <= 0.01 and 2.0 * b < 0.25 * keep_scale * abs(alpha * scale)


# ---------------------------------------------------------------------------------------------------------------- the cases
# sgemm: name -> dict(B, T, K, M, and what differs from the plain launch).  ld_in / ld_out / ldw (the pitch of plain weights) default to K / M / M; wm: transposed weights (wk = 1)
# with that pitch; drop = 'a' / 'out' with drop_ld; real = False: exact inputs only.  Named after the launch of wn_f32_forward /
# wn_f32_backward whose argument pattern the case copies; the others sweep one property at the smallest shape that reaches the branch.
def _sg(B, T, K, M, **kw):
    d = dict(B=B, T=T, K=K, M=M, ld_in=K, ld_out=M, ldw=M, shift=0, wm=0, accumulate=0, bias=0, add=0, alpha=1.0, scale=1.0, relu=0, mask=0, out_bot=0, drop=None, drop_ld=0)
    d.update(kw)
    return d


SGEMM_CASES = {
    # ---- the forward's launches
    'gate_tap0_gin':      _sg(3, 144, 136, 136, shift=-2, bias=2, drop='a', drop_ld=136),          # per-utterance bias (bias_bstride = G), dropout on A
    'gate_tap0':          _sg(3, 144, 24, 136, shift=-130, bias=1, drop='a', drop_ld=24),
    'gate_tap1':          _sg(3, 144, 136, 136, shift=-1, accumulate=1, drop='a', drop_ld=136),
    'gate_tap2':          _sg(1, 128, 16, 128, accumulate=1, drop='a', drop_ld=16),
    'gate_tap_scalar':    _sg(3, 5, 30, 30, ld_in=30, shift=-2, accumulate=1, drop='a', drop_ld=30),  # pitch 30: scalar A loads, scalar dropout words
    'gate_tap_drop_ld30': _sg(3, 144, 30, 136, ld_in=32, shift=-1, drop='a', drop_ld=30),            # aligned operand, drop_ld no multiple of 4
    'cin':                _sg(3, 144, 16, 136, accumulate=1),
    'skip_first':         _sg(3, 144, 136, 136, alpha=0.5),
    'skip_next':          _sg(3, 144, 136, 30, ld_out=32, ldw=32, alpha=0.25, accumulate=1),
    'out':                _sg(3, 144, 136, 136, bias=1, add=1, scale=0.5),
    'fin1':               _sg(3, 144, 136, 136, bias=1, relu=1),
    'fin2_o30':           _sg(3, 144, 136, 30, bias=1, out_bot=1, ld_out=0),
    'fin2_o2':            _sg(3, 144, 24, 2, bias=1, out_bot=1, ld_out=0),
    'fin2_o30_t5':        _sg(3, 5, 16, 30, bias=1, out_bot=1, ld_out=0),
    # ---- the backward's launches (transposed weights: wk = 1, wm = the forward's output width)
    'd_pre1_o30':         _sg(3, 144, 30, 136, ld_in=32, wm=30, mask=1),                             # K = O = 30 in a pitch of 32: scalar BT path, K tail
    'd_pre1_o2':          _sg(3, 144, 2, 136, ld_in=16, wm=2, mask=1),
    'd_skips':            _sg(3, 144, 136, 136, wm=136, mask=1),                                     # vector BT path with an 8-wide K tail
    'd_u_skip':           _sg(3, 144, 136, 128, wm=136, alpha=0.5),
    'd_u_out':            _sg(3, 144, 136, 128, wm=136, accumulate=1),
    'd_c':                _sg(3, 144, 136, 16, wm=136, accumulate=1),
    'd_h_tap0':           _sg(3, 144, 136, 136, wm=136, shift=2, scale=0.5, add=1, drop='out', drop_ld=136),
    'd_h_tap0_top':       _sg(3, 144, 136, 136, wm=136, shift=130, drop='out', drop_ld=136),
    'd_h_tap1':           _sg(3, 144, 136, 136, wm=136, shift=1, alpha=0.5, accumulate=1, drop='out', drop_ld=136),
    'd_h_tap2':           _sg(1, 128, 24, 30, wm=24, alpha=0.5, accumulate=1, drop='out', drop_ld=30),
    'd_h_tap_drop_ld30':  _sg(3, 5, 16, 30, wm=16, shift=1, accumulate=1, drop='out', drop_ld=30),
    # ---- one property each
    'shift_past_T':       _sg(3, 144, 16, 30, shift=-147, bias=1),                                   # every A row outside its utterance: the bias alone
    'shift_past_T_t5':    _sg(3, 5, 16, 30, shift=-8, accumulate=1),
    'shift_m130_t128':    _sg(3, 128, 16, 2, ld_out=16, shift=-130),
    'shift_p130_t144':    _sg(3, 144, 24, 30, ld_out=32, shift=130),
    'shift_p1_t5':        _sg(3, 5, 2, 2, ld_in=16, ld_out=16, shift=1),
    'k2_ld16':            _sg(1, 144, 2, 136, ld_in=16),
    'k30_ld32':           _sg(3, 128, 30, 128, ld_in=32, shift=-1),
    'k24':                _sg(1, 5, 24, 136, shift=-2),
    'm2':                 _sg(3, 144, 136, 2, ld_out=16, ldw=16),
    'm30':                _sg(1, 144, 16, 30, ld_out=32, ldw=32, bias=1, relu=1),
    'bt_wm30':            _sg(3, 144, 24, 136, wm=30, shift=-1),                                     # transposed, pitch no multiple of 4: scalar strided loads
    'bt_wm2':             _sg(1, 128, 2, 30, ld_in=16, ld_out=32, wm=2),
    'bt_wm136_m30':       _sg(3, 5, 136, 30, ld_out=32, wm=136, mask=1),
    'mask_relu_scale':    _sg(3, 144, 16, 136, bias=2, add=1, scale=0.5, relu=1, mask=1, accumulate=1),
    'out_bot_m2_t128':    _sg(3, 128, 16, 2, out_bot=1, ld_out=0, accumulate=1),
    'drop_a_kept_tail':   _sg(3, 144, 30, 30, ld_in=32, ld_out=32, shift=-1, drop='a', drop_ld=32),  # vector dropout words with a scalar K tail
}


def _wg(B, T, K, M, **kw):
    d = dict(B=B, T=T, K=K, M=M, lda=K, ldb=M, ldo=M, shift=0, alpha=1.0, biases=0, drop=0, colsum_only=0)
    d.update(kw)
    return d


# wgrad: K columns of A (the ones row is the launch's own), biases: 0 / 1 / 2 bias targets, drop: dropout on A (the engine's p = 0.5).
# Real inputs run where B * T <= 160 (the bound's condition); every case runs on exact inputs.
WGRAD_CASES = {
    'fin2':              _wg(3, 144, 136, 30, ldb=32, biases=1),                     # d W_fin2: Bm = DY in a pitch of 32
    'fin2_o2':           _wg(1, 144, 136, 2, ldb=16, biases=1),
    'fin1':              _wg(1, 144, 136, 136, biases=1),
    'skip':              _wg(3, 144, 128, 136, alpha=0.5, biases=1),                 # K = 128: the ones row is index 128, alone in the second k block
    'out_nobias':        _wg(3, 144, 128, 128, ldo=132),
    'taps_tap0':         _wg(3, 144, 136, 136, shift=-2, drop=1),
    'taps_tap1':         _wg(3, 50, 80, 128, shift=-1, drop=1),
    'taps_tap_d130':     _wg(3, 144, 16, 136, shift=-130, drop=1),
    'taps_tap_d130_b1':  _wg(1, 144, 24, 30, ldb=32, shift=-130, drop=1),
    'taps_scalar':       _wg(3, 5, 30, 30, ldb=32, shift=-2, drop=1),                # lda = 30: scalar A loads and dropout words
    'cin_two_biases':    _wg(3, 144, 16, 136, biases=2),
    'cin_k128_two':      _wg(1, 144, 128, 128, biases=2),
    'first_conv':        _wg(3, 144, 1, 136, biases=1),                              # A = the scalar input, lda = 1
    'first_conv_t5':     _wg(3, 5, 1, 30, ldb=32, biases=1),
    'colsum_only':       _wg(3, 144, 1, 136, biases=1, colsum_only=1),               # A == nullptr
    'colsum_only_m30':   _wg(1, 5, 1, 30, ldb=32, biases=2, colsum_only=1),
    'k80_m2':            _wg(1, 144, 80, 2, ldb=16, ldo=5, shift=-1),
    'k16_t5':            _wg(1, 5, 16, 128, shift=-2, biases=1),
    'k136_m136_b3_t50':  _wg(3, 50, 136, 136, shift=-2, biases=1, drop=1),
    'slab_2048':         _wg(1, 2048, 16, 30, ldb=32, shift=-1, biases=1),
    'slab_2049':         _wg(3, 2049, 16, 30, ldb=32, shift=-2, biases=1, drop=1),   # the second slab has one row
    'slab_2072':         _wg(3, 2072, 80, 2, ldb=16, shift=-130, biases=2),          # ... 24 rows
    'slab_2072_k136':    _wg(1, 2072, 136, 136, shift=-1, drop=1),
}


def case_seed(name):
    return int(np.frombuffer(name.encode().ljust(8, b'_')[:8], dtype=np.uint64)[0] % (2 ** 31))


def sgemm_operands(case, kind, gen):
    """The logical operands of one sgemm case as float64 tensors: exact integers or real_unit values."""
    c = case
    draw = exact_ints if kind == 'exact' else real_unit
    N = c['B'] * c['T']
    ops = dict(In=draw(gen, N, c['K']), W=draw(gen, c['K'], c['M']))
    ops['prev'] = draw(gen, N, c['M']) if c['accumulate'] else None
    ops['bias'] = None if not c['bias'] else draw(gen, c['M']) if c['bias'] == 1 else draw(gen, c['B'], c['M'])
    ops['add'] = draw(gen, N, c['M']) if c['add'] else None
    ops['mask'] = (torch.randint(-1, 2, (N, c['M']), generator=gen).to(torch.float64) * 0.5) if c['mask'] else None      # -0.5 / 0 / 0.5: > 0 keeps
    return ops


def wgrad_operands(case, kind, gen):
    c = case
    draw = exact_ints if kind == 'exact' else real_unit
    N = c['B'] * c['T']
    return dict(A=None if c['colsum_only'] else draw(gen, N, c['K']), Bm=draw(gen, N, c['M']))


# ---------------------------------------------------------------------------------------------------------------- a case's reference
DROP_P, DROP_SEED, DROP_LAYER = 0.5, 20240229, 3      # keep_scale = 2: a power of two, exact on integer inputs


def keep_mask(rows, ld):
    """the device's dropout keep mask of element row * ld + column, {0,1} float64 [rows, ld]  (tests/hip_util.py mirrors the hash)."""
    from hip_util import dropout_mask
    return torch.from_numpy(dropout_mask(DROP_SEED, DROP_LAYER, rows, ld, DROP_P)).to(torch.float64)


def sgemm_case_ref(case, ops):
    c = case
    N = c['B'] * c['T']
    keep_a = keep_out = None
    if c['drop'] == 'a':
        keep_a = keep_mask(N, c['drop_ld'])[:, :c['K']]
    elif c['drop'] == 'out':
        keep_out = keep_mask(N, c['drop_ld'])[:, :c['M']]
    return ref_sgemm(ops['In'], ops['W'], c['B'], c['T'], shift=c['shift'], alpha=c['alpha'], scale=c['scale'], prev=ops['prev'], bias=ops['bias'],
                     add=ops['add'], relu=bool(c['relu']), mask=ops['mask'], keep_a=keep_a, keep_out=keep_out, keep_scale=2.0 if c['drop'] else 1.0)


def wgrad_case_ref(case, ops):
    c = case
    keep_a = keep_mask(c['B'] * c['T'], c['lda'])[:, :c['K']] if c['drop'] else None
    return ref_wgrad(ops['A'], ops['Bm'], c['B'], c['T'], shift=c['shift'], alpha=c['alpha'], keep_a=keep_a, keep_scale=2.0 if c['drop'] else 1.0)


def wgrad_runs_real(case):
    return case['B'] * case['T'] <= 160
