// K-tile index arithmetic of the pipelined decode GEMVs (gemv.hip).
//
// A W row of k2 32-bit words (K/2, two bf16 each) is cut into 16-byte units of
// 4 words; K % 8 == 0 makes k2 a multiple of 4. 64 consecutive units (one per
// lane) form a unit-row. A wave walks the row in pieces of `depth` unit-rows:
// slot s of lane l in the piece that starts at unit-row r is unit
// (r + s) * 64 + l, so a lane meets its units in ascending K exactly as the
// one-load-per-trip loop does (l, l + 64, l + 128, ...).
//
// Pieces are as deep as the configured depth KU while that many whole
// unit-rows are left, then 4, 2, 1 deep as they fit into the remaining whole
// unit-rows — every slot of every such piece lies inside the row, so none of
// them needs a predicate. What is left after the whole unit-rows (K % 512 != 0
// only) is one partial unit-row in which lane l is live while its unit starts
// before k2.
//
// Plain C++ on purpose: tests/test_gemv_tail_math.py compiles these helpers
// into a host program under ASan/UBSan and sweeps every K and depth.
#pragma once

#if defined(__HIPCC__)
#define OA_GEMV_HD __host__ __device__ __forceinline__
#else
#define OA_GEMV_HD inline
#endif

#define GEMV_UNIT_WORDS 4  // one 16-byte load
#define GEMV_LANES 64

// whole unit-rows in a row of k2 words
OA_GEMV_HD int gemv_whole_rows(int k2) {
    return k2 / (GEMV_UNIT_WORDS * GEMV_LANES);
}

// Depth (in unit-rows) of the unpredicated piece that starts at unit-row r
// for configured depth ku (1, 2, 4 or 8); 0 when no whole unit-row is left.
OA_GEMV_HD int gemv_piece_depth(int k2, int ku, int r) {
    const int left = gemv_whole_rows(k2) - r;
    if (left >= ku) return ku;
    if (left >= 4) return 4;
    if (left >= 2) return 2;
    return left >= 1 ? 1 : 0;
}

// first word of slot `slot` of `lane` in the piece starting at unit-row r
OA_GEMV_HD int gemv_slot_word(int r, int slot, int lane) {
    return ((r + slot) * GEMV_LANES + lane) * GEMV_UNIT_WORDS;
}

// the partial unit-row after the whole ones: is this lane's unit in the row?
OA_GEMV_HD bool gemv_partial_live(int k2, int lane) {
    return gemv_slot_word(gemv_whole_rows(k2), 0, lane) < k2;
}
