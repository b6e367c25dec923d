"""wn_mel_run and wn_mel_peak, byte for byte, between two builds of the library (GPU): the parent commit's libwavenet_mi355.so (--parent-lib) against this
tree's, each loaded through WN_MI355_TEST_LIB in a child process of its own; SHA-256 over the bytes of the outputs.  The default geometry and every entry of
mel_util.CONFIGS x mel_util.TILES (WN_MEL_TF pins the frame tile), on the ragged boundary batch of that tile, both layouts, with pre-emphasis 0.97 and per-row
gains.  --out writes the table (profiles/mel_stream_identity.txt)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tacotron-2_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)


def _tolerate_missing_stream_symbols():
    """the parent build lacks wn_mel_stream_* : the binding resolves every name at load time, so give it stubs (nothing here calls them)"""
    import ctypes
    base = ctypes.CDLL

    class Lib(base):
        def __getattr__(self, name):
            try:
                return base.__getattr__(self, name)
            except AttributeError:
                if not name.startswith(('wn_mel_stream_', 'wn_test_mel_stream_')):
                    raise
                return ctypes.CFUNCTYPE(ctypes.c_int)(lambda *x: -4)
    ctypes.CDLL = Lib


def child():
    if os.environ.get('WN_MI355_TEST_LIB'):
        _tolerate_missing_stream_symbols()
    import numpy as np
    import torch
    import mel_util
    from wavenet_vocoder import _ext
    res = {}
    for label, over in [('default', {})] + list(mel_util.CONFIGS):
        hp = mel_util.mel_hparams(**over)
        for tf in mel_util.TILES:
            with mel_util.pinned_tile(tf):
                try:
                    probe = _ext.MelAnalyzer(hp, 1, 16)
                except _ext.WnError:
                    continue
                if probe.frame_tile != tf:      # the tile does not fit the LDS at this geometry: the library runs a smaller one, covered by its own row
                    probe.close()
                    continue
                probe.close()
                wavs = [w for _, w in mel_util.ragged_batch(hp, tf, max_frames=300)]
                lens = [len(w) for w in wavs]
                host = np.zeros((len(wavs), max(lens)), np.float32)
                for r, w in enumerate(wavs):
                    host[r, :lens[r]] = w
                dev = torch.from_numpy(host).cuda()
                gain = torch.tensor([0.5 + 0.1 * r for r in range(len(wavs))], dtype=torch.float32).cuda()
                an = _ext.MelAnalyzer(hp, len(wavs), max(lens), preemphasis=0.97)
                h, n = hashlib.sha256(), 0
                for t in (an.peak(dev, lens), an.run(dev, lens, gain=gain, channels_first=True), an.run(dev, lens, gain=None, channels_first=False)):
                    b = t.cpu().contiguous().numpy().tobytes()
                    h.update(b); n += len(b)
                torch.cuda.synchronize()
                an.close()
                res['%-12s TF=%-3d peak + run (both layouts) [%d bytes]' % (label, tf, n)] = h.hexdigest()[:16]
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
    lines = ['wn_mel_peak and wn_mel_run (pre-emphasis 0.97; channels-first with per-row gains, frames-first without) on the ragged boundary batch of each frame tile:',
             'the parent commit\'s library against this build, each loaded through WN_MI355_TEST_LIB in a process of its own; SHA-256 over the bytes of the outputs.', '']
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
