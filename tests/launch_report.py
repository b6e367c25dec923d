"""The report of the launch-local parity tests (tests/test_hip_launch_local.py, tests/test_hip_reuse.py): collects the comparisons of one
engine against the float64 references of launch_ref.py, prints them compactly and fails with launch, layer, utterance, t and channel.

A plain helper, importable without a GPU (tests/test_launch_ref_cpu.py drives it on synthetic triples).  The rule that those CPU tests pin:
a device value that is not finite is a failure wherever it stands -- under a positive bound, where the bound is 0, inside a group, in a
weight-gradient tensor and in one whose reference is all zeros.  (A NaN compares false with everything: `ratio > 1` and `rel > tol` alone
let it through.)  A reference or a bound that is not finite is a mistake of the test itself and raises at once: it is never a pass."""
import os

import torch

WGRAD_FACTOR = 8.0
WGRAD_CAP = 1e-5
# The yardstick of a tensor with one or a few elements is ONE draw of a rounding error, not a scale: it can be arbitrarily close to 0, and it is
# exactly 0 when every float32 partial sum happens to be representable (measured on MI355X: 8.2e-9 .. 9.6e-9 for the one-element biases of the
# 2D upsample net, 0 for the out-conv bias of layer 5 of softmax_c1 at B = 1 x 112 -- where the unchanged kernels are at 7.8e-8 .. 1.6e-7 and
# 8.0e-9, i.e. one to three float32 ulps).  Every float32 result, the device's and the yardstick's own, carries the final rounding to float32:
# half an ulp, 2^-24 relative.  A yardstick below that is luck, so the yardstick is floored at the precision of the output format (DESIGN
# section 5).  The factor and the cap stay: the tolerance is never below 4.8e-7 and never above 1e-5.
WGRAD_YARD_FLOOR = 2.0 ** -24


def _finite_or_raise(what, kind, l, t):
    bad = ~torch.isfinite(t)
    assert not bool(bad.any()), 'the %s of %s layer %d has %d non-finite elements: a mistake of the test, not a result' % (what, kind, l, int(bad.sum()))


class Report:
    """Collects the comparisons of one engine and prints them compactly:
        kind err/bound rel-L2 @utterance:t:channel[e]      element-wise launches (e: the worst element is within 2d of an utterance end)
        tensor rel-L2/yardstick                            weight gradients (device against float64 / the float32 yardstick; dil = causal conv,
                                                           fin = final_convolution, in = input_convolution, up = upsample net, k / b = kernel / bias)
    detail=True: one line per layer and group (the benched geometries; every case with WN_LAUNCH_LOCAL_DETAIL=1); otherwise one line per
    engine with the worst layer of every launch kind (the 54 small sweep engines).  A failure always lists every offending launch, layer,
    utterance, t, channel and tile.  A device value that is not finite always is one."""

    def __init__(self, tag, B, T, detail):
        self.tag, self.B, self.T = tag, B, T
        self.detail = detail or os.environ.get('WN_LAUNCH_LOCAL_DETAIL') == '1'
        self.fail = []
        self.worst = {}          # kind -> (largest err / bound (weight gradients: rel-L2 / tolerance) over layers, layer, text)
        self.pending = []

    def _note(self, kind, l, ratio, text):
        self.pending.append(text)
        if kind not in self.worst or ratio >= self.worst[kind][0]:
            self.worst[kind] = (ratio, l, text)

    def flush(self, label):
        if self.detail and self.pending:
            print('[%s] %-8s %s' % (self.tag, label, ' | '.join(self.pending)))
        self.pending = []

    def elementwise(self, kind, l, dev, ref, bound, d=0, group=None):
        """dev / ref / bound [B, T, ch]: every element, bound 0 means exact.  group ([B, T, 1] of {0, 1}): report / assert on those rows only."""
        _finite_or_raise('reference', kind, l, ref)
        _finite_or_raise('bound', kind, l, bound)
        bad = ~torch.isfinite(dev)
        err = (dev - ref).abs()
        ratio = torch.where(bound > 0, err / torch.where(bound > 0, bound, torch.ones_like(bound)),
                            torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
        ratio = torch.where(bad, torch.full_like(ratio, float('inf')), ratio)      # (NaN / bound is NaN and NaN > 0 is false: neither branch above sees it)
        if group is not None:
            ratio = torch.where(group > 0, ratio, torch.zeros_like(ratio))
            bad = bad & (group > 0)
        worst = float(ratio.max())
        idx = int(ratio.argmax())
        b, rem = divmod(idx, ratio.shape[1] * ratio.shape[2])
        t, ch = divmod(rem, ratio.shape[2])
        nref = float(ref.norm())
        rel = float((dev - ref).norm()) / nref if nref > 0 else float((dev - ref).norm())
        nbad = int((ratio > 1.0).sum())
        nnf = int(bad.sum())
        near = d > 0 and (t >= self.T - 2 * d or t < 2 * d)
        self._note(kind, l, worst, '%s %.3f %.1e @%d:%d:%d%s' % (kind, worst, rel, b, t, ch, 'e' if near else ''))
        if nbad:
            self.fail.append('[%s] %s layer %d: err/bound %.3f, rel-L2 %.2e, %d of %d elements over the bound%s; worst at utterance %d t %d channel %d (row %d, tile %d%s): '
                             'dev %.6g ref %.6g bound %.3g' % (self.tag, kind, l, worst, rel, nbad, ratio.numel(), ' (%d of them not finite)' % nnf if nnf else '', b, t, ch,
                                                               b * self.T + t, (b * self.T + t) // 128, ', within 2d of an utterance end' if near else '',
                                                               float(dev[b, t, ch]), float(ref[b, t, ch]), float(bound[b, t, ch])))

    def exact(self, kind, l, dev, ref):
        _finite_or_raise('reference', kind, l, ref)
        diff = (dev != ref) | ~torch.isfinite(dev)
        nbad = int(diff.sum())
        self._note(kind, l, float(nbad), '%s %s' % (kind, 'bit-exact' if nbad == 0 else '%d differ' % nbad))
        if nbad:
            idx = int(diff.flatten().to(torch.int8).argmax())
            row, ch = divmod(idx, dev.shape[-1])
            self.fail.append('[%s] %s layer %d: %d elements differ, first at utterance %d t %d channel %d (tile %d): dev %.6g ref %.6g' % (
                self.tag, kind, l, nbad, row // self.T, row % self.T, ch, row // 128, float(dev.flatten()[idx]), float(ref.flatten()[idx])))

    def tensor(self, name, l, dev, ref, yard):
        """One weight-gradient tensor: rel-L2 of the device against float64, tolerance from the float32 yardstick of the same contraction."""
        dev, ref = dev.double().reshape(-1), ref.double().reshape(-1)
        _finite_or_raise('reference', 'wgrad ' + name, l, ref)
        assert yard == yard and abs(yard) != float('inf'), 'the yardstick of wgrad %s is %r: a mistake of the test, not a result' % (name, yard)
        short = '/'.join(p.replace('residual_block_', '').replace('local_conditioning_upsampling', 'up').replace('final_convolution', 'fin').replace('input_convolution', 'in')
                         .replace('causal_conv', 'dil').replace('_conv', '').replace('kernel', 'k').replace('bias', 'b') for p in name.split('/')[-2:])
        bad = ~torch.isfinite(dev)
        if bool(bad.any()):      # (before either branch below: a NaN makes rel NaN, and `rel > tol` false)
            first = int(bad.to(torch.int8).argmax())
            self._note('wgrad', l, float('inf'), '%s NOT FINITE' % short)
            self.fail.append('[%s] wgrad %s (layer %d): %d of %d elements are not finite, first at flat index %d: dev %.6g ref %.6g' % (
                self.tag, name, l, int(bad.sum()), dev.numel(), first, float(dev[first]), float(ref[first])))
            return
        nref = float(ref.norm())
        if nref == 0.0:
            nz = int((dev != 0).sum())
            self._note(short + ' (zero reference)', l, float(nz), '%s zeros' % short if nz == 0 else '%s %d NONZERO' % (short, nz))
            if nz:
                self.fail.append('[%s] wgrad %s: reference is all zeros, device has %d nonzero elements (max %.3e)' % (self.tag, name, nz, float(dev.abs().max())))
            return
        rel = float((dev - ref).norm()) / nref
        tol = min(WGRAD_FACTOR * max(yard, WGRAD_YARD_FLOOR), WGRAD_CAP)
        self._note('wgrad', l, rel / tol, '%s %.1e/%.1e' % (short, rel, yard))
        if not rel <= tol:
            self.fail.append('[%s] wgrad %s: rel-L2 %.3e > tolerance %.3e (8 x max(yardstick %.3e, 2^-24), cap 1e-5)' % (self.tag, name, rel, tol, yard))

    def finish(self):
        # the worst layer of every launch kind ("wgrad": the tensor closest to its tolerance, as rel-L2 / tolerance)
        print('[%s] worst    %s' % (self.tag, ' | '.join('%s (L%d%s)' % (v[2], v[1], ', %.2f of tolerance' % v[0] if k == 'wgrad' else '') for k, v in sorted(self.worst.items()))))
        assert not self.fail, '\n'.join(self.fail[:40])
