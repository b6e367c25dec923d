"""Existing synthesis paths, byte for byte, between two builds of the library (GPU): the parent commit's libwavenet_mi355.so (--parent-lib) against this
tree's, each loaded through WN_MI355_TEST_LIB in a child process of its own; SHA-256 over the bytes of samples and raw outputs.  Launch-per-layer path
(steps_per_graph = 24, T = 256, free running, caller noise) on three models of tests/synth_ref.py: wn_synthesize at 1 / 8 / 32 streams, a 3-slot session
(4-frame ticks), wn_synthesize_wide at 64 / 70 streams.  --out writes the table (profiles/wide_slots_identity.txt)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tacotron-2_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

MODELS, T, SPG = ('s6', 's6_softmax', 'w256'), 256, 24


def _sha(*ts):
    h = hashlib.sha256()
    n = 0
    for t in ts:
        b = t.cpu().contiguous().numpy().tobytes()
        h.update(b); n += len(b)
    return h.hexdigest()[:16], n


def child():
    if os.environ.get('WN_MI355_TEST_LIB'):
        from wide_timing import _tolerate_missing_wide_symbol
        _tolerate_missing_wide_symbol()
    import torch
    import synth_ref as SR
    from hip_util import upload_params
    from test_hip_synth import _noise
    from wavenet_vocoder import _ext
    res = {}
    for model in MODELS:
        hp, cfg, params, ti, wav, c, g = SR.make_case(model, 70, T)
        eng = _ext.Engine(hp, 70, T)
        eng.pack_weights(upload_params(eng, params))
        nz = _noise(cfg, T, 70, seed=4)[0]
        dt = torch.float32 if cfg.scalar_input else torch.int32
        for B in (1, 8, 32, 64, 70):
            out = torch.empty(B, T, dtype=dt, device='cuda'); raw = torch.empty(B, cfg.out_channels, T, device='cuda')
            run = eng.synthesize if B <= 32 else eng.synthesize_wide
            run(c[:B].contiguous().cuda(), nz[:, :B].contiguous().cuda(), out, raw, None, steps_per_graph=SPG)
            torch.cuda.synchronize(); eng.synth_check()
            assert eng.synth_path == 'graph'
            d, n = _sha(out, raw)
            res['%s %s B=%d samples+raw [%d bytes]' % (model, 'wn_synthesize' if B <= 32 else 'wn_synthesize_wide', B, n)] = d
        # a narrow slot session on the launch-per-layer path: 3 slots, 4-frame ticks, device noise
        eng.slots_begin(3, steps_per_graph=SPG)
        Tc, hop, parts = T // cfg.hop, cfg.hop, []
        for b in range(3):
            eng.slot_open(b, seed=11 + b)
        for f0 in range(0, Tc, 4):
            k = min(4, Tc - f0)
            out = torch.empty(3, k * hop, dtype=dt, device='cuda'); raw = torch.empty(3, cfg.out_channels, k * hop, device='cuda')
            eng.slots_push(c[:3, :, f0:f0 + k].contiguous().cuda(), [k] * 3, [f0 + k == Tc] * 3, out, raw)
            parts += [out, raw]
        torch.cuda.synchronize(); eng.synth_check()
        assert eng.synth_path == 'graph'
        res['%s 3-slot session (graph path, 4-frame ticks)' % model] = _sha(*parts)[0]
        eng.close()
    print('IDENT ' + json.dumps(res))


def _run(lib):
    env = dict(os.environ)
    env.pop('WN_MI355_TEST_LIB', None)
    if lib:
        env['WN_MI355_TEST_LIB'] = os.path.abspath(lib)
    p = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), '--child'], env=env, capture_output=True, text=True)
    line = [l for l in p.stdout.splitlines() if l.startswith('IDENT ')]
    if p.returncode != 0 or not line:
        raise RuntimeError('child (%s) failed (%d): %s' % (lib or 'this', p.returncode, p.stderr[-1500:]))
    return json.loads(line[-1][6:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.child:
        return child()
    parent, this = _run(a.parent_lib), _run(None)
    lines = ['Launch-per-layer path (steps_per_graph = %d, T = %d, free-running, caller noise; the session: device noise): the parent commit\'s library against this build,' % (SPG, T),
             'each loaded through WN_MI355_TEST_LIB in a process of its own; SHA-256 over the bytes of samples and raw outputs.', '']
    bad = 0
    for k in this:
        same = parent.get(k) == this[k]
        bad += not same
        lines.append('%-64s parent %s  this %s  %s' % (k, parent.get(k), this[k], 'identical' if same else 'DIFFERENT'))
    lines += ['', '%d of %d comparisons differ.' % (bad, len(this))]
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        open(a.out, 'w').write(text)
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
