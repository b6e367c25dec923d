// Stand-alone host check of csrc/wn_frag.h: the LDS addresses and lane maps of the LDS-DMA ring kernel (csrc/wn_tile.h) for both MFMA shapes.
// For every instantiated (MT, NT, WM, WN, BK, MF) and every lane:
//   1. staging followed by a fragment read delivers exactly the logical element (row, k) of the instruction's operand map, and the reads of one
//      chunk take every 16-B slot of both images exactly once per wave row / column (a bijection onto the tile);
//   2. every fragment read (ds_read_b128) is free of LDS bank conflicts: lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32,
//      bank (a/4) mod 64 -- and the 16x16x32 read on the 32x32x16 swizzle of the 32-channel image is 2-way, which is why the swizzle differs;
//   3. accumulators -> LDS -> (row, 8 channels) items covers every (time, channel) of the workgroup tile exactly once, with the hardware's D map
//      written out here independently of the header.
// Built by tests/test_frag_layout_cpu.py with the host compiler (ASAN + UBSAN); no GPU.
#include "wn_frag.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } ++fails; } } while (0)

struct Cfg { int MT, NT, WM, WN, BK, MF, lds_epi, gate; };
// every wn_gemm_lds_kernel instantiation of wn_launch_gemm (lds_epi 0: the register epilogue of EPI_STORE_F32_BOT; gate 1: also launched as the gate)
static const Cfg CFGS[] = {
    {2, 1, 4, 2, 64, 0, 1, 0}, {2, 2, 4, 2, 32, 0, 1, 1}, {2, 2, 4, 2, 32, 1, 1, 1}, {1, 2, 4, 2, 32, 0, 1, 1}, {1, 2, 4, 2, 32, 1, 1, 1},
    {1, 3, 3, 2, 64, 0, 0, 0}, {1, 3, 3, 2, 32, 0, 0, 0}, {2, 2, 2, 4, 32, 0, 0, 0},
};

static const int GROUPS[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                  {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59}, {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
// worst N-way conflict of one ds_read_b128 (64 byte addresses, 16-B aligned): a 16-B read takes the 4 banks of its slot of the 256-B bank row
static int b128_ways(const int* addr) {
    int worst = 1;
    for (int g = 0; g < 4; ++g)
        for (int slot = 0; slot < 16; ++slot) {
            int distinct[16], n = 0;
            for (int q = 0; q < 16; ++q) {
                const int a = addr[GROUPS[g][q]];
                if (((a / 4) % 64) / 4 != slot) continue;
                bool seen = false;
                for (int d = 0; d < n; ++d) seen = seen || distinct[d] == a;
                if (!seen) distinct[n++] = a;
            }
            if (n > worst) worst = n;
        }
    return worst;
}

static int check_cfg(const Cfg& c) {
    const int MT = c.MT, NT = c.NT, WM = c.WM, WN = c.WN, BK = c.BK, MF = c.MF;
    const int KS = BK / 16, MTILE = WM * MT * 32, TTILE = WN * NT * 32;
    const int A_SLOTS = MTILE * BK / 8, B_SLOTS = TTILE * BK / 8;
    const int AI = MF ? 2 * MT : MT, AJ = MF ? 2 * NT : NT, KR = MF ? KS / 2 : KS;
    int worst = 1;
    // ---- 1a. weight image: slot -> (row, k) as the DMA leaves it
    std::vector<int> a_row(A_SLOTS, -1), a_k(A_SLOTS, -1), b_row(B_SLOTS, -1), b_k(B_SLOTS, -1);
    for (int f = 0; f < A_SLOTS / 64; ++f)
        for (int l = 0; l < 64; ++l) { a_row[f * 64 + l] = wn_frag_a_stage_row(BK, f, l); a_k[f * 64 + l] = wn_frag_a_stage_k(BK, f, l); }
    for (int p = 0; p < B_SLOTS / 64; ++p)
        for (int l = 0; l < 64; ++l) { b_row[p * 64 + l] = wn_frag_b_stage_row(BK, p, l); b_k[p * 64 + l] = wn_frag_b_stage_slot(BK, MF, p, l) * 8; }
    {   // the staged B image holds every (row, 8-channel group) once
        std::vector<int> seen(B_SLOTS, 0);
        for (int s = 0; s < B_SLOTS; ++s) {
            CHECK(b_row[s] >= 0 && b_row[s] < TTILE && b_k[s] >= 0 && b_k[s] < BK, "B stage out of range");
            if (b_row[s] >= 0 && b_row[s] < TTILE && b_k[s] >= 0 && b_k[s] < BK) ++seen[b_row[s] * (BK / 8) + b_k[s] / 8];
        }
        for (int s = 0; s < B_SLOTS; ++s) CHECK(seen[s] == 1, "B stage: (row %d, group %d) staged %d times", s / (BK / 8), s % (BK / 8), seen[s]);
    }
    // ---- 1b / 2. fragment reads
    std::vector<int> a_reads(A_SLOTS, 0), b_reads(B_SLOTS, 0);
    for (int wm = 0; wm < WM; ++wm)
        for (int i = 0; i < AI; ++i)
            for (int ks = 0; ks < KR; ++ks) {
                int addr[64];
                for (int l = 0; l < 64; ++l) {
                    const int a = addr[l] = wn_frag_a_read(MF, MT, KS, wm, i, ks, l);
                    CHECK(a >= 0 && a % 16 == 0 && a / 16 < A_SLOTS, "A read out of the image");
                    if (a < 0 || a % 16 || a / 16 >= A_SLOTS) continue;
                    ++a_reads[a / 16];
                    CHECK(a_row[a / 16] == wn_frag_a_row(MF, MT, wm, i, l) && a_k[a / 16] == wn_frag_a_k(MF, ks, l), "A read wm %d i %d ks %d lane %d: got (%d, %d) want (%d, %d)",
                          wm, i, ks, l, a_row[a / 16], a_k[a / 16], wn_frag_a_row(MF, MT, wm, i, l), wn_frag_a_k(MF, ks, l));
                    // the operand map of the instruction, written out: MF 0 row l&31, k 8(l>>5); MF 1 row l&15, k 8(l>>4)
                    const int want_row = MF ? wm * MT * 32 + i * 16 + (l & 15) : (wm * MT + i) * 32 + (l & 31), want_k = MF ? ks * 32 + 8 * (l >> 4) : ks * 16 + 8 * (l >> 5);
                    CHECK(a_row[a / 16] == want_row && a_k[a / 16] == want_k, "A operand map");
                }
                const int w = b128_ways(addr);
                if (w > worst) worst = w;
            }
    for (int wn = 0; wn < WN; ++wn)
        for (int j = 0; j < AJ; ++j)
            for (int ks = 0; ks < KR; ++ks) {
                int addr[64];
                for (int l = 0; l < 64; ++l) {
                    const int a = addr[l] = wn_frag_b_read(BK, MF, NT, wn, j, ks, l);
                    CHECK(a >= 0 && a % 16 == 0 && a / 16 < B_SLOTS, "B read out of the image");
                    if (a < 0 || a % 16 || a / 16 >= B_SLOTS) continue;
                    ++b_reads[a / 16];
                    const int want_row = MF ? wn * NT * 32 + j * 16 + (l & 15) : (wn * NT + j) * 32 + (l & 31), want_k = MF ? ks * 32 + 8 * (l >> 4) : ks * 16 + 8 * (l >> 5);
                    CHECK(b_row[a / 16] == want_row && b_k[a / 16] == want_k, "B read wn %d j %d ks %d lane %d: got (%d, %d) want (%d, %d)", wn, j, ks, l, b_row[a / 16], b_k[a / 16], want_row, want_k);
                    CHECK(want_row == wn_frag_b_row(MF, NT, wn, j, l), "B row helper");
                }
                const int w = b128_ways(addr);
                if (w > worst) worst = w;
            }
    for (int s = 0; s < A_SLOTS; ++s) CHECK(a_reads[s] == 1, "A slot %d read %d times", s, a_reads[s]);
    for (int s = 0; s < B_SLOTS; ++s) CHECK(b_reads[s] == 1, "B slot %d read %d times", s, b_reads[s]);
    CHECK(worst == 1, "fragment reads are %d-way conflicted", worst);
    // ---- 3. epilogue: accumulators -> staging -> items
    if (c.lds_epi) {
        const int PITCH = MTILE * 4 + 16, PROWS = WN * 32, NTH = WM * WN * 64;
        for (int gate = 0; gate <= c.gate; ++gate) {
            std::vector<int> out(TTILE * MTILE, 0);
            for (int jp = 0; jp < NT; ++jp) {
                std::vector<int> st_t(PROWS * MTILE, -1), st_m(PROWS * MTILE, -1);
                auto put = [&](int rl, int ml, int r, int t, int m) {
                    CHECK(rl >= 0 && rl < PROWS && ml >= 0 && ml % 4 == 0 && ml + r < MTILE && (rl * PITCH + ml * 4) % 16 == 0, "staging slot out of the pass or not a 16-B store");
                    if (!(rl >= 0 && rl < PROWS && ml >= 0 && ml + r < MTILE)) return;
                    CHECK(st_t[rl * MTILE + ml + r] == -1, "staging slot written twice");
                    st_t[rl * MTILE + ml + r] = t; st_m[rl * MTILE + ml + r] = m;
                };
                for (int wm = 0; wm < WM; ++wm) for (int wn = 0; wn < WN; ++wn) for (int l = 0; l < 64; ++l) {
                    if (MF == 0) {
                        for (int i = 0; i < MT; ++i) for (int reg = 0; reg < 16; ++reg)      // D of 32x32x16: col l&31, row 8(reg>>2) + 4(l>>5) + (reg&3)
                            put(wn_frag_acc_rl(0, wn, 0, l), wn_frag_acc_ml(0, MT, wm, i, reg >> 2, l), reg & 3,
                                (wn * NT + jp) * 32 + (l & 31), (wm * MT + i) * 32 + 8 * (reg >> 2) + 4 * (l >> 5) + (reg & 3));
                    } else {
                        for (int i = 0; i < AI; ++i) for (int jh = 0; jh < 2; ++jh) for (int reg = 0; reg < 4; ++reg)      // D of 16x16x32: col l&15, row 4(l>>4) + reg
                            put(wn_frag_acc_rl(1, wn, jh, l), wn_frag_acc_ml(1, MT, wm, i, 0, l), reg,
                                wn * NT * 32 + (2 * jp + jh) * 16 + (l & 15), wm * MT * 32 + i * 16 + 4 * (l >> 4) + reg);
                    }
                }
                const int C8 = (gate ? MTILE / 2 : MTILE) / 8, NIT = PROWS * C8 / NTH;
                CHECK(PROWS * C8 % NTH == 0 && NTH % C8 == 0, "item geometry");
                for (int tid = 0; tid < NTH; ++tid) for (int k = 0; k < NIT; ++k) {
                    const int rl = wn_frag_item_rl(NTH, C8, tid, k), tr = wn_frag_item_tr(NT, jp, rl), c8 = tid % C8;
                    CHECK(rl < PROWS && tr < TTILE, "item row");
                    if (rl >= PROWS || tr >= TTILE) continue;
                    for (int half = 0; half <= gate; ++half) for (int r = 0; r < 8; ++r) {
                        // gate: 64-row groups [32 tanh rows | 32 sigmoid rows]; the item reads channels ml .. ml + 7 and ml + 32 .. ml + 39
                        const int ml = gate ? ((c8 * 8) >> 5) * 64 + ((c8 * 8) & 31) + 32 * half + r : c8 * 8 + r;
                        CHECK(st_t[rl * MTILE + ml] == tr && st_m[rl * MTILE + ml] == ml, "item (tid %d, k %d) channel %d: staged (%d, %d), wants (%d, %d)", tid, k, ml, st_t[rl * MTILE + ml], st_m[rl * MTILE + ml], tr, ml);
                        ++out[tr * MTILE + ml];
                    }
                }
            }
            for (int s = 0; s < TTILE * MTILE; ++s) CHECK(out[s] == 1, "epilogue (gate %d): (time %d, channel %d) produced %d times", gate, s / MTILE, s % MTILE, out[s]);
        }
    }
    return worst;
}

int main() {
    for (const Cfg& c : CFGS) {
        const int before = fails, w = check_cfg(c);
        printf("cfg MT %d NT %d WM %d WN %d BK %d MF %d: reads %d-way, %s\n", c.MT, c.NT, c.WM, c.WN, c.BK, c.MF, w, fails == before ? "ok" : "FAILED");
    }
    {   // why MF = 1 has its own swizzle at BK = 32: the 16x16x32 B read on the 32x32x16 image
        int worst = 1;
        for (int wn = 0; wn < 2; ++wn) for (int j = 0; j < 4; ++j) {
            int addr[64];
            for (int l = 0; l < 64; ++l) { const int row = wn_frag_b_row(1, 2, wn, j, l); addr[l] = row * 64 + (((l >> 4) ^ wn_frag_swz(32, 0, row)) * 16); }
            const int w = b128_ways(addr);
            if (w > worst) worst = w;
        }
        printf("16x16x32 read on the 32x32x16 swizzle (BK 32): %d-way\n", worst);
        // and every permutation P of {0..3} applied to (row/4)%4: conflict-free for BOTH reads exactly when P[1] ^ P[2] == 1
        int perm_bad = 0;
        for (int code = 0; code < 256; ++code) {
            const int P[4] = {code & 3, (code >> 2) & 3, (code >> 4) & 3, (code >> 6) & 3};
            if ((1 << P[0] | 1 << P[1] | 1 << P[2] | 1 << P[3]) != 15) continue;
            int w16 = 1, w32 = 1;
            for (int j = 0; j < 8; ++j) {
                int a16[64], a32[64];
                for (int l = 0; l < 64; ++l) {
                    const int r16 = j * 16 + (l & 15), r32 = (j & 3) * 32 + (l & 31);
                    a16[l] = r16 * 64 + (((l >> 4) ^ P[(r16 >> 2) & 3]) * 16);
                    a32[l] = r32 * 64 + ((((j >> 2) * 2 + (l >> 5)) ^ P[(r32 >> 2) & 3]) * 16);
                }
                const int x = b128_ways(a16), y = b128_ways(a32);
                if (x > w16) w16 = x;
                if (y > w32) w32 = y;
            }
            if (((w16 == 1 && w32 == 1)) != ((P[1] ^ P[2]) == 1)) ++perm_bad;
        }
        CHECK(perm_bad == 0, "%d permutations contradict the rule P[1]^P[2] == 1", perm_bad);
    }
    if (fails) { printf("frag FAILED (%d checks)\n", fails); return 1; }
    printf("frag ok\n");
    return 0;
}
