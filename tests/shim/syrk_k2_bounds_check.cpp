// TEST INFRASTRUCTURE: the carry schedule of k_syrk5_k2 (sdpb_amd/csrc/kernels.hpp) at the architectural bounds of the image
// words (tests/test_syrk_second_karatsuba.py compiles it with -fsanitize=address,undefined and runs it on the host).
// A real image never reaches xm = x0 + x1 = 2^29 - 2 (the largest evaluated value, p(3), is below 121 * 2^102), so the operator
// tests cannot load the 64-bit column sums to what the schedule is derived from.  This program runs the lane arithmetic the
// kernel is built from -- syrk5k2_mac_row, syrk5k2_pass_end (the cadence), syrk5k2_term (fold and combination) -- for the 64
// lanes of one tile with EVERY word at its bound (x0 = x1 = 2^28 - 1, xm = 2^29 - 2) over one sweep of 2560 rows:
//   sums     after every pass, c + d 2^32 of every output the instantiation computes is rows * w^2 exactly (a column sum that
//            wrapped, or a carry that lost a word, shows at the pass where it happens), and c < 2^32 right after a carry;
//   result   the three terms added mod 2^128, as the kernel's read-modify-write of the planes does, are
//            rows (x0 + x1 2^28)^2 = s0 + (sm - s0 - s1) 2^28 + s1 2^56, which is below 2^124.
// One line per pass length (16 and 32 rows); exit status 1 if any line has failures.
#include <cstdio>
#include <cstdlib>

#include "kernels.hpp"

using namespace sdpb;
typedef unsigned __int128 u128;
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

constexpr unsigned ROWS = 2560; // the rows of a planned split (syrk_stage.hpp: SYRK_SPLIT_ROWS)

// one tile, instantiation (PN, DIAG) of the row loop, passes of RBG rows
template <int RBG, int PN, bool DIAG> static void run_tile()
{
  const uint32_t bound[3] = {T5_MASK, T5_MASK, T5_XM_MAX};
  for(int lane = 0; lane < SYRK5_WG; ++lane)
    {
      const int li = lane & 7, lj = lane >> 3;
      u128 planes[4][4]; // the product's planes at the lane's outputs, written by t = 0 and added to by t = 1, 2
      for(int t = 0; t < 3; ++t)
        {
          uint64_t c[4][4], d[4][4];
          for(int p = 0; p < 4; ++p)
            for(int q = 0; q < 4; ++q)
              c[p][q] = d[p][q] = 0;
          unsigned since = 0;
          const uint32_t w = bound[t];
          const uint32_t a[4] = {w, w, w, w}, b[4] = {w, w, w, w};
          for(unsigned r0 = 0; r0 < ROWS; r0 += RBG)
            {
              for(int rr = 0; rr < RBG; ++rr)
                syrk5k2_mac_row<PN, DIAG>(c, a, b);
              const bool carries = since + RBG >= (t == 2 ? SYRK5_CARRY_ROWS_XM : SYRK5_CARRY_ROWS_X);
              syrk5k2_pass_end<RBG>(t, since, c, d);
              CHECK(carries == (since == 0), "RBG %d t %d row %u: the cadence", RBG, t, r0);
              for(int p = 0; p < 4; ++p)
                for(int q = 0; q < 4; ++q)
                  {
                    const bool computed = p < PN && (!DIAG || q <= p);
                    const u128 want = computed ? (u128)(r0 + RBG) * w * w : 0;
                    const u128 got = (u128)c[p][q] + ((u128)d[p][q] << 32);
                    CHECK(got == want, "RBG %d t %d row %u lane %d output (%d, %d): the column sum", RBG, t, r0 + RBG, lane, p, q);
                    if(carries)
                      CHECK(c[p][q] < ((uint64_t)1 << 32), "RBG %d t %d row %u: a carry leaves the low word", RBG, t, r0 + RBG);
                  }
            }
          for(int p = 0; p < 4; ++p)
            for(int q = 0; q < 4; ++q)
              planes[p][q] = (t > 0 ? planes[p][q] : 0) + syrk5k2_term(t, c[p][q], d[p][q]);
        }
      const u128 x = (u128)T5_MASK + ((u128)T5_MASK << T5_LB); // the largest two-limb piece: 2^56 - 1
      for(int p = 0; p < 4; ++p)
        for(int q = 0; q < 4; ++q)
          {
            const bool computed = p < PN && (!DIAG || q <= p);
            const u128 want = computed ? (u128)ROWS * x * x : 0;
            CHECK(planes[p][q] == want, "RBG %d lane (%d, %d) output (%d, %d): the combination", RBG, li, lj, p, q);
            CHECK((planes[p][q] >> 124) == 0, "RBG %d: the result fits 124 bits", RBG);
          }
    }
}

template <int RBG> static bool check_pass_length()
{
  const long before = failures;
  run_tile<RBG, 4, false>();
  run_tile<RBG, 4, true>();
  run_tile<RBG, 2, false>();
  run_tile<RBG, 2, true>();
  std::printf("%2d rows per pass, %u rows, 4 instantiations x 64 lanes x 3 sub-sweeps: %ld failures\n", RBG, ROWS, failures - before);
  return failures == before;
}

int main()
{
  bool ok = check_pass_length<16>();
  ok = check_pass_length<32>() && ok;
  return ok ? 0 : 1;
}
