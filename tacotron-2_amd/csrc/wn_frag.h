// LDS addresses and lane maps of the LDS-DMA ring kernel (wn_tile.h, wn_gemm_lds_body) for its two MFMA shapes, as constexpr functions of
// plain integers: the kernel's 16x16x32 arm calls them (its 32x32x16 arm spells the same MF = 0 expressions out, which keeps its compiled code what it was
// before this header existed), and tests/host/frag_main.cpp checks them on the host -- that staging followed by a fragment read
// delivers exactly the logical element the instruction's operand map asks for, that every fragment read is free of LDS bank conflicts, and that
// the accumulator -> LDS -> item path of the fused epilogues covers every (time, channel) of the tile once.
//
//   MF = 0   v_mfma_f32_32x32x16_bf16: lane l holds A[row l&31][k = 8(l>>5) + j], B[k = 8(l>>5) + j][col l&31];
//            D: col = l&31 (time), row = 8(reg>>2) + 4(l>>5) + (reg&3) (channel), 16 registers
//   MF = 1   v_mfma_f32_16x16x32_bf16: lane l holds A[row l&15][k = 8(l>>4) + j], B[k = 8(l>>4) + j][col l&15];
//            D: col = l&15 (time), row = 4(l>>4) + reg (channel), 4 registers
//
// A image (weights): the pack's fragment order [mtile32][kstep16][lane][8], one 1-KiB fragment per DMA, the same for both shapes.
// B image (activations): rows [t][BK channels], the 16-B slot index XORed with a function of the row (wn_frag_swz).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WN_FRAG_HD __host__ __device__ __attribute__((always_inline))      // inlined before any simplification: the kernels compile as if the expressions stood in them
#else
#define WN_FRAG_HD
#endif

// XOR term of the 16-B slot index of activation row `row` (applied to the DMA's source channel and to the fragment read alike).
// BK = 64 (128-B rows, 2 per bank line, 8 slots): (row/2) % 8, conflict-free for both shapes.  BK = 32 (64-B rows, 4 per bank line, 4 slots):
// MF = 0 keeps (row/4) % 4; the 16x16x32 read is 2-way conflicted on that image (rows r and r + 8 of a 16-lane group meet in one slot), so
// MF = 1 takes P[(row/4) % 4] with P = {0, 2, 3, 1} (any permutation with P[1] ^ P[2] == 1 is conflict-free for both reads).
WN_FRAG_HD constexpr int wn_frag_swz(int BK, int MF, int row) {
    const int RB = BK * 2, SPR = RB / 16, RPL = 256 / RB;       // row bytes, 16-B slots per row, rows per 256-B bank line
    return (BK == 64 || MF == 0) ? (row / RPL) % SPR : (0x78 >> (2 * ((row >> 2) & 3))) & 3;
}

// ---- staging (LDS-DMA destinations; lane `lane` of DMA piece `piece` lands at byte piece * 1024 + lane * 16 of its image)
// B: the row of the time tile and the LOGICAL 16-B slot (8 channels) this lane must fetch
WN_FRAG_HD constexpr int wn_frag_b_stage_row(int BK, int piece, int lane) { return piece * (1024 / (BK * 2)) + (lane * 16) / (BK * 2); }
WN_FRAG_HD constexpr int wn_frag_b_stage_slot(int BK, int MF, int piece, int lane) {
    return (lane % (BK * 2 / 16)) ^ wn_frag_swz(BK, MF, wn_frag_b_stage_row(BK, piece, lane));
}
// A: piece f = mt * KS + ks holds pack fragment (m-tile mt, 16-wide k-step ks); lane -> (row, first k) inside the workgroup's panel chunk
WN_FRAG_HD constexpr int wn_frag_a_stage_row(int BK, int piece, int lane) { return (piece / (BK / 16)) * 32 + (lane & 31); }
WN_FRAG_HD constexpr int wn_frag_a_stage_k(int BK, int piece, int lane) { return (piece % (BK / 16)) * 16 + (lane >> 5) * 8; }

// ---- fragment reads (byte offsets inside one ring slot's A / B image; one ds_read_b128 per lane)
// MF = 0: m-tile i (32 rows) of wave row wm, 16-wide k-step ks.  MF = 1: 16-row block i16 of wave row wm, 32-wide k-step ks32.
WN_FRAG_HD constexpr int wn_frag_a_read(int MF, int MT, int KS, int wm, int i, int ks, int lane) {
    return MF == 0 ? (wm * MT * KS * 64 + lane) * 16 + (i * KS + ks) * 1024
                   : ((wm * MT + (i >> 1)) * KS + 2 * ks + (lane >> 5)) * 1024 + (((lane >> 4) & 1) * 32 + (i & 1) * 16 + (lane & 15)) * 16;
}
// the logical (row of the workgroup's M tile, first k of the chunk) that read must deliver
WN_FRAG_HD constexpr int wn_frag_a_row(int MF, int MT, int wm, int i, int lane) {
    return MF == 0 ? (wm * MT + i) * 32 + (lane & 31) : wm * MT * 32 + i * 16 + (lane & 15);
}
WN_FRAG_HD constexpr int wn_frag_a_k(int MF, int ks, int lane) { return MF == 0 ? ks * 16 + (lane >> 5) * 8 : ks * 32 + (lane >> 4) * 8; }
// MF = 0: 32-row block j of wave column wn; MF = 1: 16-row block j16
WN_FRAG_HD constexpr int wn_frag_b_row(int MF, int NT, int wn, int j, int lane) {
    return MF == 0 ? (wn * NT + j) * 32 + (lane & 31) : wn * NT * 32 + j * 16 + (lane & 15);
}
WN_FRAG_HD constexpr int wn_frag_b_read(int BK, int MF, int NT, int wn, int j, int ks, int lane) {
    const int row = wn_frag_b_row(MF, NT, wn, j, lane);
    return row * (BK * 2) + (((MF == 0 ? ks * 2 + (lane >> 5) : ks * 4 + (lane >> 4)) ^ wn_frag_swz(BK, MF, row)) * 16);      // logical slot ^ swizzle
}

// ---- accumulators.  The epilogue stages pass jp (the jp-th 32 time rows of every wave column) as fp32 [rl][channel] rows of `pitch` bytes.
// MF = 0: fragment (i, jp), register group qd (4 registers = 4 consecutive channels).  MF = 1: fragment (i16, j16 = 2 jp + jh), all 4 registers.
WN_FRAG_HD constexpr int wn_frag_acc_rl(int MF, int wn, int jh, int lane) { return MF == 0 ? wn * 32 + (lane & 31) : wn * 32 + 16 * jh + (lane & 15); }
WN_FRAG_HD constexpr int wn_frag_acc_ml(int MF, int MT, int wm, int i, int qd, int lane) {
    return MF == 0 ? (wm * MT + i) * 32 + qd * 8 + (lane >> 5) * 4 : wm * MT * 32 + 16 * i + 4 * (lane >> 4);
}
// (the staged value of channel ml of row rl sits at byte rl * pitch + ml * 4)
// item (thread tid, step k) of a pass reads 8 channels (32 B) of staged row rl; its row inside the workgroup's time tile
WN_FRAG_HD constexpr int wn_frag_item_rl(int nth, int c8n, int tid, int k) { return tid / c8n + k * (nth / c8n); }
WN_FRAG_HD constexpr int wn_frag_item_tr(int NT, int jp, int rl) { return ((rl >> 5) * NT + jp) * 32 + (rl & 31); }
