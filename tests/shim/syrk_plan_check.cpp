// TEST INFRASTRUCTURE: the planners of sdpb_amd/csrc/syrk_stage.hpp (FxSyrk<FX>: syrk_plan, syrk_splits_for, q_window) on
// the host, without a device (tests/test_host_logic.py compiles it with -fsanitize=address,undefined and runs it).  For the
// image width of every compiled limb count it walks a grid of operand shapes, forced row splits and budgets and checks what
// FxSyrk::G and FxSyrk::G_windows rely on without checking it:
//   chunks      the chunks of the tile list cover it, and the last one is not empty;
//   row splits  at least one, and the last split owns a row -- also in a shorter last chunk, whose planes fit `part`;
//   budget      the partial planes stay inside a non-zero budget (or are the smallest chunk: one tile, one split);
//   windows     the input windows cover the rows, the last one is not empty, several windows are whole passes of the
//               product kernel, and the image stays inside its budget unless the plan says the bound is exceeded -- which it
//               says exactly when fewer rows than one pass fit.
// One line per limb count; exit status 1 if any line has failures.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "syrk_stage.hpp"

using namespace sdpb;
static long failures = 0;
#define CHECK(cond, ...)                                                                                                                             \
  do                                                                                                                                                 \
    if(!(cond))                                                                                                                                      \
      {                                                                                                                                              \
        if(++failures <= 20)                                                                                                                         \
          {                                                                                                                                          \
            std::printf("FAILED %s: ", #cond);                                                                                                       \
            std::printf(__VA_ARGS__);                                                                                                                \
            std::printf("\n");                                                                                                                       \
          }                                                                                                                                          \
      }                                                                                                                                              \
  while(0)

template <int NL> static bool check_width()
{
  constexpr int FX = fx_limbs<NL>();
  using S = FxSyrk<FX>;
  const long before = failures;
  long plans = 0, windows = 0;
  const int Ns[] = {1, 17, 33, 100, 150, 513, 2048};
  const unsigned rowss[] = {1, 9, 33, 300, 2560, 2561, 40000, 700000};
  const char *splits[] = {nullptr, "1", "2", "3", "32"};
  const size_t part_budgets[] = {0, 1, S::TILE_WORDS, 100000, 10000000, 1000000000};
  const char *image_bytes[] = {"4", "1000", "100000", "1000000", "100000000", "10000000000"};
  const S syrk(256); // the CU count of the MI355X
  constexpr size_t RB = S::SYRK_RB;
  auto last_split_owns_a_row = [](int nsplit, unsigned nrows) {
    const size_t rps = (size_t)cdiv(cdiv(nrows, nsplit), RB) * RB;
    return nsplit >= 1 && (size_t)(nsplit - 1) * rps < nrows;
  };
  for(int N : Ns)
    for(unsigned nrows : rowss)
      {
        const int tiles = (int)cdiv(N, S::SYRK_EDGE), ntile = tiles * (tiles + 1) / 2;
        for(const char *sp : splits)
          {
            if(sp)
              setenv("SDPB_HIP_SYRK_SPLITS", sp, 1);
            else
              unsetenv("SDPB_HIP_SYRK_SPLITS");
            for(size_t budget : part_budgets)
              {
                const SyrkPlan pl = syrk.syrk_plan(ntile, nrows, budget);
                ++plans;
#define WHERE "N %d rows %u splits %s budget %zu", N, nrows, sp ? sp : "-", budget
                CHECK(pl.ntile == ntile && pl.chunk_tiles >= 1 && pl.nchunk >= 1, WHERE);
                if(pl.chunk_tiles < 1 || pl.nchunk < 1)
                  continue;
                CHECK((long)pl.nchunk * pl.chunk_tiles >= ntile, WHERE);
                CHECK((long)(pl.nchunk - 1) * pl.chunk_tiles < ntile, WHERE);
                CHECK(last_split_owns_a_row(pl.nsplit_first, nrows), WHERE);
                CHECK(pl.part_words == (pl.uses_part ? (size_t)pl.nsplit_first * S::TILE_WORDS * pl.chunk_tiles : 0), WHERE);
                const int nt = ntile - (pl.nchunk - 1) * pl.chunk_tiles; // the last chunk
                if(nt != pl.chunk_tiles)
                  {
                    const int ns = std::min(pl.nsplit_first, syrk.syrk_splits_for(nt, nrows, pl.part_words));
                    CHECK(last_split_owns_a_row(ns, nrows), WHERE);
                    CHECK((size_t)ns * S::TILE_WORDS * nt <= pl.part_words, WHERE);
                  }
                if(budget && pl.uses_part)
                  CHECK(pl.part_words <= std::max(budget, S::TILE_WORDS), WHERE);
#undef WHERE
              }
          }
        unsetenv("SDPB_HIP_SYRK_SPLITS");
        for(const char *ib : image_bytes)
          {
            setenv("SDPB_HIP_SYRK_IMAGE_BYTES", ib, 1);
            const QWindow w = syrk.q_window(nrows, N);
            ++windows;
#define WHERE "N %d rows %u image bytes %s: %d windows of %u rows", N, nrows, ib, w.chunks, w.chunk_rows
            CHECK(w.budget_words == std::max<size_t>(1, (size_t)std::atof(ib) / 4), WHERE);
            CHECK(w.chunks >= 1 && (size_t)w.chunks * w.chunk_rows >= nrows, WHERE);
            CHECK((size_t)(w.chunks - 1) * w.chunk_rows < nrows, WHERE);
            CHECK(w.chunks == 1 || w.chunk_rows % RB == 0, WHERE);
            CHECK(w.image_words == S::image_words_for(w.chunk_rows, (size_t)N) && w.stride == S::image_stride(w.chunk_rows, (size_t)N), WHERE);
            CHECK(w.image_words <= w.budget_words || w.bound_exceeded, WHERE);
            // rows that fit, by the planner's own count of the image: per row its slots in every plane, + the pad and 4 words
            const size_t per_row = fx_row_slots<FX>((size_t)N) * fx_planes<FX>(), fixed = (size_t)64 * fx_planes<FX>() + 4;
            const size_t fit = w.budget_words > fixed ? (w.budget_words - fixed) / per_row : 0;
            const bool all_fit = S::image_words_for(nrows, (size_t)N) <= w.budget_words;
            CHECK(w.bound_exceeded == (!all_fit && fit < RB), WHERE);
#undef WHERE
          }
        unsetenv("SDPB_HIP_SYRK_IMAGE_BYTES");
      }
  std::printf("limbs %d FX %d: %ld plans, %ld windows, %ld failures\n", NL, FX, plans, windows, failures - before);
  return failures == before;
}

int main()
{
  bool ok = true;
  ok &= check_width<6>();
  ok &= check_width<10>();
  ok &= check_width<16>();
  ok &= check_width<18>();
  ok &= check_width<24>();
  ok &= check_width<26>();
  ok &= check_width<34>();
  ok &= check_width<42>();
  ok &= check_width<50>();
  ok &= check_width<66>();
  return ok ? 0 : 1;
}
