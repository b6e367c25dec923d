"""Shared by tests/test_mel_stream_cpu.py and tests/test_hip_mel_stream.py: the streaming mel analysis' geometry, rule of readiness and counters written out
in plain Python (independent of csrc/wn_mel_stream.h), and the cut schedules both test files push rows under."""
import numpy as np

# n_fft, win_size, hop: the three of the issue, and one with an odd window, where Hl = 151 and Hr = 150 differ (in the others they are equal)
GEOMETRIES = {'default': (2048, 1100, 275), 'fft1024': (1024, 1024, 256), 'fft800': (800, 800, 200), 'odd_win': (512, 301, 64)}


def geometry(n_fft, win, hop):
    """(Hl, Hr): frame f reads the samples [f hop - Hl, f hop + Hr)"""
    off = (n_fft - win) // 2
    Hl = n_fft // 2 - off
    return Hl, win - Hl


def ready(n_fft, win, hop, S, final):
    """frames analysed of a row that has consumed S samples: by brute force over f"""
    if final:
        return 1 + S // hop
    Hr = geometry(n_fft, win, hop)[1]
    f = 0
    while f * hop + Hr <= S:
        f += 1
    return f


def fixed_cuts(n_fft, win, hop, max_push):
    Hr = geometry(n_fft, win, hop)[1]
    return [1, hop - 1, hop, hop + 1, Hr - 1, Hr, win, max_push]


class Row:
    """the counters of one row, as the header documents them"""

    def __init__(self, n_fft, win, hop):
        self.g = (n_fft, win, hop)
        self.Hl, self.Hr = geometry(n_fft, win, hop)
        self.S, self.F, self.ended = 0, 0, False

    def push(self, n, restart, final):
        """-> (status name, n_out, first_frame); a refused push changes nothing"""
        hop = self.g[2]
        active = n > 0 or final
        if active and self.ended and not restart:
            return 'state', 0, self.F
        if restart:
            self.S, self.F, self.ended = 0, 0, False
        first = self.F
        if not active:
            return 'ok', 0, first
        self.S += n
        F1 = ready(*self.g, self.S, final)
        n_out, self.F = F1 - self.F, F1
        self.ended = bool(final)
        return 'ok', n_out, first

    @property
    def tail_len(self):
        if self.ended:
            return 0
        return self.S - min(self.S, max(0, self.F * self.g[2] - self.Hl))


def random_schedule(rs, lens, max_push, cuts, p_zero=0.15, p_late_final=0.3, restart_mid=None):
    """Pushes [(n [B], restart [B], final [B])] that give row b exactly lens[b] samples: cuts drawn from `cuts` and from [0, max_push]; pushes of n = 0; some rows
    end with a final push of n = 0; rows end at different pushes.  restart_mid: {row: samples} -- that row is cut off after so many samples (no final) and
    restarted from its beginning."""
    B = len(lens)
    pos, done, started, late = [0] * B, [False] * B, [False] * B, [False] * B
    cut_off = dict(restart_mid or {})
    pushes = []
    while not all(done):
        n, r, f = [0] * B, [0] * B, [0] * B
        for b in range(B):
            if done[b]:
                continue
            if late[b]:
                f[b] = 1; done[b] = True
                continue
            c = 0 if rs.rand() < p_zero else int(cuts[rs.randint(len(cuts))] if rs.rand() < 0.5 else rs.randint(0, max_push + 1))
            c = min(c, max_push, lens[b] - pos[b])
            if b in cut_off and pos[b] + c >= cut_off[b] > 0:
                c = max(0, cut_off[b] - pos[b])
            r[b] = int(not started[b]); started[b] = True
            n[b] = c; pos[b] += c
            if b in cut_off and pos[b] == cut_off[b]:
                del cut_off[b]; pos[b] = 0; started[b] = False      # the next push restarts the row from sample 0
                continue
            if pos[b] == lens[b]:
                if rs.rand() < p_late_final:
                    late[b] = True
                else:
                    f[b] = 1; done[b] = True
        pushes.append((n, r, f))
    return pushes


def cycled_schedule(lens, max_push, cuts):
    """the fixed cut list cycled, row b starting b entries into it; a row's last push is final"""
    B = len(lens)
    pos, done, pushes, k = [0] * B, [False] * B, [], 0
    while not all(done):
        n, r, f = [0] * B, [0] * B, [0] * B
        for b in range(B):
            if done[b]:
                continue
            c = min(cuts[(k + b) % len(cuts)], max_push, lens[b] - pos[b])
            r[b] = int(pos[b] == 0 and k == 0)
            n[b] = c; pos[b] += c
            if pos[b] == lens[b]:
                f[b] = 1; done[b] = True
        pushes.append((n, r, f)); k += 1
    return pushes


def whole_schedule(lens, max_push):
    """every row in one push, whole and final; a row longer than max_push in pushes of max_push, the last one final"""
    return cycled_schedule(lens, max_push, [max_push])
