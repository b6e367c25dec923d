"""csrc/wn_frag.h on the host: the LDS addresses and lane maps of the LDS-DMA ring kernel for both MFMA shapes (tests/host/frag_main.cpp: its own main, built with
the host compiler under ASAN + UBSAN and run as an ordinary child process).  For every instantiated tile and every lane the program proves that staging followed by a
fragment read delivers the logical (row, k) of the instruction's operand map with every slot read exactly once, counts LDS bank conflicts of every fragment read with
the hardware's ds_read_b128 lane groups and bank rule (all 1-way), and follows accumulators -> LDS -> epilogue items over every (time, channel) of the tile."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fragment_layouts_of_both_mfma_shapes(tmp_path):
    exe = str(tmp_path / 'frag_main')
    r = subprocess.run(['hipcc', '-std=c++20', '-O1', '-g', '-Wall', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        '-I', os.path.join(ROOT, 'tacotron-2_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'frag_main.cpp'), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and 'frag ok' in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    cfgs = re.findall(r'cfg MT (\d) NT (\d) WM (\d) WN (\d) BK (\d+) MF (\d): reads (\d)-way, (\w+)', r.stdout)
    assert len(cfgs) == 8 and all(c[6] == '1' and c[7] == 'ok' for c in cfgs), r.stdout
    # both shapes of the two tiles that have them
    assert {c[:6] for c in cfgs} >= {('2', '2', '4', '2', '32', '0'), ('2', '2', '4', '2', '32', '1'), ('1', '2', '4', '2', '32', '0'), ('1', '2', '4', '2', '32', '1')}
    # the reason the 16x16x32 arm has its own swizzle: its read is 2-way conflicted on the 32x32x16 image of a 32-channel chunk
    assert '16x16x32 read on the 32x32x16 swizzle (BK 32): 2-way' in r.stdout
