// Stand-alone host program for the argument contracts of dh_beam_row_best and dh_beam_select_best: every call below must come back
// with DH_ERR_BAD_ARG before any HIP call is made, so it runs without a GPU.  Built with the host side under AddressSanitizer and
// UndefinedBehaviorSanitizer by tools/asan_beam_best.sh (the library's own sources, this main, no Python in the process).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/deephumor_hip.h"

static int failures = 0;
#define EXPECT_BAD(call) do { const int rc_ = (call); if (rc_ != DH_ERR_BAD_ARG) { std::printf("line %d: %s -> %d\n", __LINE__, #call, rc_); ++failures; } } while (0)

int main() {
    // host memory stands in for the device pointers: a rejected call dereferences none of them
    std::vector<float> logits(2 * 128), gmax(2 * 4), vals(6), pick_val(6 * 3);
    std::vector<int32_t> pick_idx(6 * 3), tokens(6 * 8), parent(6), hparent(6), end_step(2), src(6 * 9), first_pos(2), err(1);
    std::vector<uint8_t> ended(6), done(2);
    float* L = logits.data(); float* G = gmax.data(); int32_t* PI = pick_idx.data(); float* PV = pick_val.data(); int32_t* E = err.data();
    int32_t* FP = first_pos.data();
    // dh_beam_row_best(logits, ldl, V, group_max, gm_ld, n_groups, group_cols, rows, rows_per_img, beam, T, unk, step, first_pos, ...)
    EXPECT_BAD(dh_beam_row_best(nullptr, 128, 100, nullptr, 0, 0, 0, 6, 3, 3, 1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 6, 3, 3, 1.f, 1, 0, nullptr, nullptr, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 6, 3, 3, 1.f, 1, 0, nullptr, PI, nullptr, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 6, 3, 3, 1.f, 1, 0, nullptr, PI, PV, nullptr, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 0, 3, 3, 1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 6, 0, 3, 1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 0, nullptr, 0, 0, 0, 6, 3, 3, 1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 99, 100, nullptr, 0, 0, 0, 6, 3, 3, 1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 6, 3, 0, 1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 6, 3, DH_BEAM_MAX_BEAMS + 1, 1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 6, 3, 3, 0.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 6, 3, 3, -1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 6, 3, 3, NAN, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 6, 3, 3, INFINITY, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, G, 2, 1, 64, 6, 3, 3, 1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, G, 1, 2, 64, 6, 3, 3, 1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, G, 2, 2, 65, 6, 3, 3, 1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, G, 2, 2, 0, 6, 3, 3, 1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, G, 2000, 1025, 64, 6, 3, 3, 1.f, 1, 0, nullptr, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 6, 1, 3, 1.f, 1, 0, FP, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(L, 128, 100, nullptr, 0, 0, 0, 7, 3, 3, 1.f, 1, 0, FP, PI, PV, E, nullptr));
    EXPECT_BAD(dh_beam_row_best(nullptr, 0, 0, nullptr, 0, 0, 0, 0, 0, 0, 0.f, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
    // dh_beam_select_best(pick_idx, pick_val, tokens, tok_ld, vals, ended, src, src_ld, parent, hparent, done, end_step, n_img, beam,
    //                     first, first_pos, first_sets_ended, write_pos, t, step_index, eos_index, stream)
    int32_t* T = tokens.data(); float* VA = vals.data(); uint8_t* EN = ended.data(); int32_t* S = src.data(); int32_t* P = parent.data();
    int32_t* H = hparent.data(); uint8_t* D = done.data(); int32_t* ES = end_step.data();
    EXPECT_BAD(dh_beam_select_best(nullptr, PV, T, 8, VA, EN, nullptr, 0, P, H, D, ES, 2, 3, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, nullptr, T, 8, VA, EN, nullptr, 0, P, H, D, ES, 2, 3, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, nullptr, 8, VA, EN, nullptr, 0, P, H, D, ES, 2, 3, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 8, nullptr, EN, nullptr, 0, P, H, D, ES, 2, 3, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 8, VA, nullptr, nullptr, 0, P, H, D, ES, 2, 3, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 8, VA, EN, nullptr, 0, nullptr, H, D, ES, 2, 3, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 8, VA, EN, nullptr, 0, P, nullptr, D, ES, 2, 3, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 8, VA, EN, nullptr, 0, P, H, nullptr, ES, 2, 3, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 8, VA, EN, nullptr, 0, P, H, D, nullptr, 2, 3, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 8, VA, EN, nullptr, 0, P, H, D, ES, 0, 3, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 8, VA, EN, nullptr, 0, P, H, D, ES, 2, 0, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 8, VA, EN, nullptr, 0, P, H, D, ES, 2, DH_BEAM_MAX_BEAMS + 1, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 0, VA, EN, nullptr, 0, P, H, D, ES, 2, 3, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 8, VA, EN, nullptr, 0, P, H, D, ES, 2, 3, 0, nullptr, 1, 1, -1, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 8, VA, EN, S, 5, P, H, D, ES, 2, 3, 0, nullptr, 1, 1, 5, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 300, VA, EN, nullptr, 0, P, H, D, ES, 2, 64, 0, nullptr, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(PI, PV, T, 300, VA, EN, nullptr, 0, P, H, D, ES, 2, 64, 0, FP, 1, 1, 0, 1, 3, nullptr));
    EXPECT_BAD(dh_beam_select_best(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr,
                                   0, 0, 0, 0, 0, nullptr));
    std::printf(failures ? "%d argument checks FAILED\n" : "all argument checks of dh_beam_row_best / dh_beam_select_best hold (%d failures)\n", failures);
    return failures ? 1 : 0;
}
