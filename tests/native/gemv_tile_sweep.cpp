// Host-side sweep of the GEMV K-piece arithmetic (opsagent_amd/ops/csrc/
// gemv_tile.h), built with -fsanitize=address,undefined by
// tests/test_gemv_tail_math.py. It walks a row exactly as gemv_row_pieces in
// gemv.hip does and marks every 16-byte unit a lane would load in a heap array
// of exactly the row's unit count, so a unit past the row end is both asserted
// and an ASan heap-buffer-overflow.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gemv_tile.h"

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::fprintf(stderr, "FAIL k2=%d ku=%d: %s (line %d)\n", k2, ku,   \
                         #cond, __LINE__);                                     \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

static void mark(unsigned char* cover, int units, int word, int k2, int ku,
                 int* last_word_of_lane) {
    CHECK(word >= 0);
    CHECK(word % GEMV_UNIT_WORDS == 0);
    CHECK(word + GEMV_UNIT_WORDS <= k2);  // the whole 16-byte load is in the row
    CHECK(word > *last_word_of_lane);     // a lane walks K in ascending order
    *last_word_of_lane = word;
    const int u = word / GEMV_UNIT_WORDS;
    CHECK(u < units);
    cover[u]++;  // ASan-checked: `cover` has exactly `units` bytes
}

int main() {
    long pieces = 0, units_total = 0;
    const int depths[] = {1, 2, 4, 8};
    for (int k2 = 4; k2 <= 8192; k2 += 4) {  // K/2; K % 8 == 0
        for (int ku : depths) {
            const int units = k2 / GEMV_UNIT_WORDS;
            std::vector<unsigned char> cover_v(units, 0);
            unsigned char* cover = cover_v.data();
            int last[GEMV_LANES];
            for (int l = 0; l < GEMV_LANES; ++l) last[l] = -1;

            int r = 0;
            for (int d; (d = gemv_piece_depth(k2, ku, r)) > 0; r += d) {
                // the depths gemv_row_pieces has an instantiation for
                CHECK(d == ku || (d < ku && (d == 4 || d == 2 || d == 1)));
                CHECK(r + d <= gemv_whole_rows(k2));
                for (int lane = 0; lane < GEMV_LANES; ++lane)
                    for (int s = 0; s < d; ++s) {
                        // the kernel addresses slot s at slot 0 + s * 256 words
                        CHECK(gemv_slot_word(r, s, lane) ==
                              gemv_slot_word(r, 0, lane) + s * 256);
                        mark(cover, units, gemv_slot_word(r, s, lane), k2, ku,
                             &last[lane]);
                    }
                ++pieces;
            }
            CHECK(r == gemv_whole_rows(k2));
            if (gemv_slot_word(r, 0, 0) < k2) {  // the partial unit-row
                for (int lane = 0; lane < GEMV_LANES; ++lane)
                    if (gemv_partial_live(k2, lane))
                        mark(cover, units, gemv_slot_word(r, 0, lane), k2, ku,
                             &last[lane]);
            } else {
                CHECK(units % GEMV_LANES == 0);
            }
            for (int u = 0; u < units; ++u) CHECK(cover[u] == 1);
            units_total += units;
        }
    }
    std::printf("gemv_tile_sweep OK: %ld pieces, %ld units\n", pieces, units_total);
    return 0;
}
