// syrk_stage.hpp — host side of the exact fixed-point product Q' = P'^T P' of the Q stage (compute_Q.cxx:94-132).
//
// FxSyrk<FX> is the stage for images of FX limbs: the format constants the kernels are instantiated with, the budgets of
// its two windows, the planners (pure integer arithmetic: no device, only the CU count), the buffers of one operand shape
// (prepare) and the three launch sequences (column_sums, G, G_windows).  Solver<NL> keeps what depends on NL or on the
// iteration: the image of P' (k_normalize_fx), unbias + restore, the cross-rank sum, events and the chase.
// The budgets and the record of the latest call are ONE small record (SyrkRecord) per solver.  The solver's stage owns it;
// a workspace for another operand (op_syrk_Q, op_int_syrk, bench_op) is constructed from the solver's stage and shares the
// record, so an operator runs on its own buffers under the solver's budgets and what it did shows in sdpb_hip_memory_plan.
#pragma once
#include "kernels.hpp"

namespace sdpb
{
// Lower-triangle tiles of an N x N output, enumerated super-block by super-block
// (8x8 tiles) so that consecutive entries share operand panels.
// split_col > 0: the tiles that hold outputs of the columns [0, split_col) come first (super-block order inside each
// group), *count_left = how many they are; the tiles that hold outputs of the columns [split_col, N) follow -- the two
// launches of the chunked Q' take the two parts of the list.  Where split_col is not a multiple of the tile edge, the
// tiles of the straddling tile column are in BOTH parts (their products are computed twice; each part's finishing
// kernel reads only its own columns).
// edge: 16, or 32 for k_syrk_fx3 (super-blocks of 4x4 tiles then cover the same 128 columns)
inline std::vector<uint32_t> syrk_tile_order(int N, int split_col = 0, int *count_left = nullptr, int edge = 16)
{
  int SB = edge == 16 ? 8 : 4;
  if(const char *env = std::getenv("SDPB_HIP_SYRK_SB")) // tuning knob: super-block edge in tiles
    SB = std::max(1, std::atoi(env));
  const int tiles = (N + edge - 1) / edge, nsb = (tiles + SB - 1) / SB;
  std::vector<uint32_t> all;
  for(int bi = 0; bi < nsb; ++bi)
    for(int bj = 0; bj <= bi; ++bj)
      for(int ti = bi * SB; ti < std::min(tiles, (bi + 1) * SB); ++ti)
        for(int tj = bj * SB; tj < std::min(tiles, (bj + 1) * SB); ++tj)
          if(tj <= ti)
            all.push_back((uint32_t)ti << 16 | (uint32_t)tj);
  if(split_col <= 0)
    {
      if(count_left)
        *count_left = (int)all.size();
      return all;
    }
  std::vector<uint32_t> out;
  for(uint32_t t : all)
    if((int)(t & 0xffffu) * edge < split_col)
      out.push_back(t);
  if(count_left)
    *count_left = (int)out.size();
  for(uint32_t t : all)
    if(((int)(t & 0xffffu) + 1) * edge > split_col)
      out.push_back(t);
  return out;
}

// nsplit in [1, 32]: fewest splits within 2% of the best occupancy of the last round.  (Up to 16 until round 4: with
// N = 100 the output has 28 tiles, and 16 splits filled 448 of the chip's 768 workgroup slots — C3's product took
// 2.08 ms at 8 splits, 3.8 at 4, 15 at 1: profiles/r04k_syrk_row_splits.txt; the row floor of 64 passes per split
// still applies.)
// max_rows > 0 (k_syrk_fx3): at least so many splits that one has no more rows than that.  The workgroups of an XCD that
// stream the same operand panels drift apart by no more than a split's rows, so short splits are what lets them meet in
// that XCD's L2: on C4 (profiles/r04x_syrk3_fetch_vs_splits.txt) FETCH_SIZE per launch 99.7 M KB with 2 splits of 20 000
// rows, 78 with 8, 49 with 16 (2500 rows: same kernel time), 22 with 32 (+ 3.5 % time: the finishing kernel adds 32 x 105 planes).
constexpr int SYRK_MAX_SPLITS = 32;
inline int syrk_row_splits(int ntile, unsigned nrows, int slots, int rb, unsigned max_rows = 0)
{
  if(const char *env = std::getenv("SDPB_HIP_SYRK_SPLITS")) // tests force the split path on small inputs
    return std::max(1, std::min(SYRK_MAX_SPLITS, std::atoi(env)));
  int smin = 1;
  while(max_rows && smin < SYRK_MAX_SPLITS && nrows / (unsigned)smin > max_rows && nrows / (unsigned)(smin + 1) >= 64u * (unsigned)rb)
    ++smin;
  int best = smin;
  double best_eff = 0;
  for(int s = smin; s <= SYRK_MAX_SPLITS; ++s)
    {
      if(s > smin && nrows / (unsigned)s < 64u * (unsigned)rb)
        break;
      const double items = (double)ntile * s, rounds = std::ceil(items / slots), eff = items / (rounds * slots);
      if(eff > best_eff + 0.02)
        {
          best = s;
          best_eff = eff;
        }
    }
  return best;
}

// The plan of one G call: the tile list is walked in chunks; every chunk is one product launch + its finishing
// kernels over tile-packed partial planes (kernels.hpp: syrk_packed_decode) that fit `budget_words` of `part`.
// Analogue of the reference's output windows (bigint_syrk_blas.cxx:200-220: Q is computed window by window when the
// residues of the whole output do not fit --maxSharedMemory, BigInt_Shared_Memory_Syrk_Context.cxx:149-215).
struct SyrkPlan
{
  int ntile = 0, chunk_tiles = 0, nchunk = 0; // tiles of the call, tiles per chunk (a multiple of 8 unless one chunk), chunks
  int nsplit_first = 1;                       // row splits of the first chunk (all chunks but a shorter last one)
  size_t part_words = 0;                      // words of `part` the call needs
  bool uses_part = false;
};
// The INPUT window of the Q stage: the fixed-point image of P' is built for `chunk_rows` rows at a time (k_normalize_fx
// into ONE bounded buffer), each window's product is accumulated into Q' (k_acc_add_tri) -- the reference splits its
// input residue window by rows the same way when all rows do not fit --maxSharedMemory
// (BigInt_Shared_Memory_Syrk_Context.cxx:70-110,172-186: input_window_split_factor; bigint_syrk_blas.cxx:239-285 loops
// over the input windows).  Everything is exact integer arithmetic, so Q' keeps every bit whatever the split.
struct QWindow
{
  unsigned chunk_rows = 0; // rows per input window (a multiple of the product's 2560-row splits where there are that many rows)
  int chunks = 0;          // input windows per Q' (input_window_split_factor)
  size_t stride = 0;       // elements per group plane of the window's image
  size_t image_words = 0;  // words of the window's image buffer
  size_t budget_words = 0; // what the image was allowed
  bool bound_exceeded = false; // the budget is smaller than the smallest window (one pass of rows)
};
struct SyrkRecord
{
  size_t default_words = 0;    // window budget of the device, found by the first prepare() of the solver's stage
  size_t max_shared_bytes = 0; // sdpb_hip_set_max_shared_memory (0: not set)
  SyrkPlan last_plan;          // of the latest G call (sdpb_hip_memory_plan, the bench line)
  int last_windows = 1;        // of the latest G_windows call
};

template <int FX> class FxSyrk
{
public:
  static constexpr int ACCW = 2 * FX + 2;
  static constexpr bool SYRK_TOOM4 = fx_toom4<FX>();         // seven (FX/4)^2 products per row pair (k_syrk_fx2<.., true> + k_syrk4_finish)
  static constexpr bool SYRK_TOOM4K = fx_toom4k<FX>();       // ... and one Karatsuba level below them: 21 (FX/8)^2 products (k_syrk_fx3)
  static constexpr bool SYRK_TOOM5K = fx_toom5k<FX>();       // Toom-5 x two Karatsuba levels on 28-bit limbs, lazy carries: 27 products of three one-limb sub-sweeps (k_syrk5_k2 + k_syrk5_finish)
  static constexpr int SYRK_NPROD = fx_nprod<FX>();          // products per row pair of k_syrk_fx3 / k_syrk5_k2
  static constexpr int SYRK_EDGE = syrk_tile_edge<FX>();     // output tile of the syrk kernel in use
  static constexpr unsigned SYRK_SPLIT_ROWS = SYRK_TOOM4K ? 2560u : 0u; // rows per row split of k_syrk_fx3 at most (syrk_row_splits)
  static constexpr bool SYRK_TWO_LEVEL = fx_two_level<FX>() || SYRK_TOOM4; // piece-major image: nine (two Karatsuba levels) or seven pieces
  static constexpr int SYRK_PART_PLANES = SYRK_TOOM4K ? SYRK_NPROD * fx_part_limbs<FX>() : SYRK_TOOM4 ? 7 * (2 * (FX / 4) + 1) : ACCW; // planes one row split writes
  // words per column of the bias terms of the signed evaluation points (k_fx_colsum4_final / k_fx_colsum5_final), of a slice's column sums
  static constexpr size_t TOOMU_WORDS = SYRK_TOOM5K ? (size_t)3 * T5_Z : (size_t)2 * (2 * (FX / 4) + 2);
  static constexpr size_t COLSUM_WORDS = SYRK_TOOM5K ? 25 : FX + 8; // 5 x 5, or 2 (FX/2 + 2) / 4 (FX/4 + 2) limbs per column and slice
  // rows per LDS chunk: k_syrk_fx2 stages one piece group of 32 rows per pass; k_syrk_fx 3 FX/2 planes x RB rows
#ifndef SDPB_SYRK2_RBG
#define SDPB_SYRK2_RBG (FX >= 32 ? 16 : 32)
#endif
  static constexpr int SYRK_RB = SYRK_TWO_LEVEL ? SDPB_SYRK2_RBG : (FX <= 24 ? 16 : 8);
  static constexpr size_t TILE_WORDS = (size_t)SYRK_PART_PLANES * SYRK_EDGE * SYRK_EDGE; // partial planes of one tile in one row split
  static constexpr int SYRK5_ROWS = SDPB_SYRK5_ROWS; // rows per pass of k_syrk5_k2 (a divisor of SYRK_RB, which pads the image and aligns the splits)
  static_assert(!SYRK_TOOM5K || SYRK_RB % SYRK5_ROWS == 0, "a split begins and the image ends at whole passes of k_syrk5_k2");

  explicit FxSyrk(int num_cus) : num_cus_(num_cus), rec_(&own_) {}
  // a workspace for another operand under the budgets of the solver's stage, reporting its calls to it
  explicit FxSyrk(const FxSyrk *solver_stage) : num_cus_(solver_stage->num_cus_), rec_(solver_stage->rec_) {}

  // ---- budgets -------------------------------------------------------------------
  // The two windows of the stage -- the image (input window) and the partial planes of the product (output window) --
  // share one bound: sdpb_hip_set_max_shared_memory (--maxSharedMemory), else what prepare() found free on the device.
  void set_max_shared_memory(size_t bytes) { rec_->max_shared_bytes = bytes; }
  size_t window_budget_words() const { return rec_->max_shared_bytes ? std::max<size_t>(1, rec_->max_shared_bytes / sizeof(uint32_t)) : rec_->default_words; }
  // words of partial planes a G call may use: SDPB_HIP_SYRK_PART_BYTES (tests, shared GPUs), else what the window budget
  // leaves beside an image of `image_words`.  Never 0 ("unbounded") for a non-zero bound: at least one word, i.e.
  // one-tile chunks (round-5 advisor).
  size_t syrk_part_budget_words(size_t image_words) const
  {
    if(const char *e = std::getenv("SDPB_HIP_SYRK_PART_BYTES"))
      return std::max<size_t>(1, (size_t)std::max(1.0, std::atof(e)) / sizeof(uint32_t));
    const size_t w = window_budget_words();
    return std::max<size_t>(1, w - std::min(image_words, w / 2)); // (an image that could not be split -- chased Q' -- does not starve the planes)
  }
  size_t syrk_part_budget_words() const { return syrk_part_budget_words(win.image_words); }
  // words the image may take: SDPB_HIP_SYRK_IMAGE_BYTES (tests), else half of the window budget (the planes get the rest)
  size_t image_budget_words() const
  {
    if(const char *e = std::getenv("SDPB_HIP_SYRK_IMAGE_BYTES"))
      return std::max<size_t>(1, (size_t)std::max(1.0, std::atof(e)) / sizeof(uint32_t));
    return std::max<size_t>(1, window_budget_words() / 2);
  }
  // where the budget of the image / of the partial planes comes from (sdpb_hip_memory_plan)
  const char *budget_source(bool image) const
  {
    if(std::getenv(image ? "SDPB_HIP_SYRK_IMAGE_BYTES" : "SDPB_HIP_SYRK_PART_BYTES"))
      return image ? "SDPB_HIP_SYRK_IMAGE_BYTES" : "SDPB_HIP_SYRK_PART_BYTES";
    if(rec_->max_shared_bytes)
      return image ? "maxSharedMemory/2" : "maxSharedMemory";
    return image ? "device/2" : "device";
  }
  const SyrkRecord &record() const { return *rec_; }

  // ---- planners --------------------------------------------------------------------
  // the fixed-point image of a rows x cols operand: elements per group plane (kernels.hpp: fx_image_stride) and its words
  static size_t image_stride(size_t rows, size_t cols) { return std::max<size_t>(1, fx_image_stride<FX>(rows, cols, SYRK_RB)); }
  static size_t image_words_for(size_t rows, size_t cols) { return image_stride(rows, cols) * fx_planes<FX>() + 4; }
  static unsigned colsum_slices(size_t rows) { return (unsigned)std::min<size_t>(128, std::max<size_t>(1, cdiv(rows, 64))); }
  // k_syrk_fx3 / k_syrk5_k2: the 21 (27) products of a (tile, row split) in one workgroup (1), one Toom group each (7, 9), or one product each
  static int syrk_group_split()
  {
    if(!SYRK_TOOM4K)
      return 1;
    if(const char *e = std::getenv("SDPB_HIP_SYRK_GSPLIT"))
      {
        const int g = std::atoi(e);
        return g == 1 ? 1 : (g == 7 || g == 9) ? SYRK_NPROD / 3 : SYRK_NPROD;
      }
    return SYRK_NPROD; // (21 or 27: one product per workgroup) measured (profiles/r04s_syrk3_variants.txt): C4 101.6 ms against 102.8 with 7, C3 1.23 against 1.55 ms
  }
  // row splits of a launch over `tiles` tiles: the occupancy rule of syrk_row_splits, bounded by the partial planes
  // that fit `budget_words`, and no split without rows
  int syrk_splits_for(int tiles, unsigned nrows, size_t budget_words) const
  {
    // workgroups the chip holds at once: of four wavefronts, or the one-wave workgroups of k_syrk5_k2
    const int slots = num_cus_ * (SYRK_TOOM5K ? syrk5_wg_per_cu(SYRK5_ROWS) : syrk_waves_per_simd<FX>());
    int nsplit = syrk_row_splits(tiles * syrk_group_split(), nrows, slots, SYRK_RB, SYRK_SPLIT_ROWS);
    const size_t per_split = TILE_WORDS * tiles;
    if(budget_words && (size_t)nsplit * per_split > budget_words)
      nsplit = (int)std::max<size_t>(1, budget_words / per_split);
    while(nsplit > 1 && (size_t)(nsplit - 1) * (cdiv(cdiv(nrows, nsplit), SYRK_RB) * SYRK_RB) >= nrows)
      --nsplit; // (forced split counts on small inputs: the last split must own a row -- its planes are summed)
    return nsplit;
  }
  SyrkPlan syrk_plan(int ntile, unsigned nrows, size_t budget_words) const
  {
    SyrkPlan pl;
    pl.ntile = ntile;
    const int nsplit_all = syrk_splits_for(ntile, nrows, 0);
    pl.uses_part = nsplit_all > 1 || SYRK_TOOM4;
    pl.chunk_tiles = ntile;
    pl.nchunk = ntile ? 1 : 0;
    pl.nsplit_first = nsplit_all;
    if(!pl.uses_part || !ntile)
      return pl;
    const size_t need = (size_t)nsplit_all * TILE_WORDS * ntile;
    if(budget_words && need > budget_words)
      {
        // as few chunks as fit, of equal size: every launch stays far above the chip's resident workgroups
        const size_t bw = std::max(budget_words, TILE_WORDS); // one tile, one split: the smallest chunk
        int nchunk = (int)cdiv(need, bw);
        for(;; ++nchunk)
          {
            int ct = (int)cdiv(ntile, nchunk);
            if(ct >= 64)
              ct = (int)(cdiv(ct, 8) * 8); // whole rounds of the eight XCDs
            pl.chunk_tiles = std::min(ntile, ct);
            pl.nsplit_first = syrk_splits_for(pl.chunk_tiles, nrows, bw);
            if((size_t)pl.nsplit_first * TILE_WORDS * pl.chunk_tiles <= bw || pl.chunk_tiles <= 1)
              break;
          }
        pl.nchunk = (int)cdiv(ntile, pl.chunk_tiles);
      }
    pl.part_words = (size_t)pl.nsplit_first * TILE_WORDS * pl.chunk_tiles;
    return pl;
  }
  QWindow q_window(unsigned nrows, int N, bool one_chunk = false) const
  {
    QWindow w;
    w.budget_words = image_budget_words();
    const unsigned quantum = (unsigned)SYRK_RB;
    unsigned rows = std::max(nrows, 1u);
    if(!one_chunk && image_words_for(rows, (size_t)N) > w.budget_words)
      {
        // the most rows whose image fits, in whole passes of the product kernel
        const size_t per_row = fx_row_slots<FX>((size_t)N) * fx_planes<FX>();
        const size_t fixed = (size_t)64 * fx_planes<FX>() + 4;
        size_t fit = w.budget_words > fixed ? (w.budget_words - fixed) / per_row : 0;
        fit = fit / quantum * quantum;
        if(fit < quantum)
          {
            fit = quantum;
            w.bound_exceeded = true;
          }
        const unsigned f = (unsigned)cdiv(nrows, fit);
        // equal windows; whole row splits of the product kernel where that still fits
        unsigned cr = (unsigned)(cdiv(cdiv(nrows, f), quantum) * quantum);
        if(SYRK_SPLIT_ROWS && cr > SYRK_SPLIT_ROWS)
          {
            const unsigned up = (unsigned)(cdiv(cr, SYRK_SPLIT_ROWS) * SYRK_SPLIT_ROWS);
            if(up <= fit)
              cr = up;
          }
        rows = cr;
      }
    if(one_chunk && image_words_for(rows, (size_t)N) > w.budget_words)
      w.bound_exceeded = true;
    w.chunk_rows = rows;
    w.chunks = nrows ? (int)cdiv(nrows, rows) : 1;
    w.stride = image_stride((size_t)rows, (size_t)N);
    w.image_words = w.stride * fx_planes<FX>() + 4;
    return w;
  }

  // ---- the buffers of one operand shape ----------------------------------------------
  // image: ONE input window of the operand (k_normalize_fx / k_fx_from_int write its rows x cols elements only, the pad stays
  // zero); acc: cols x cols outputs + cols column sums (k_fx_colsum) in ACCW planes; acc2: the partial G of the input windows
  // after the first; part: the partial planes of one output window; zero_piece: what k_syrk_fx2 stages for rows/columns
  // outside the image
  DevBuf<uint32_t> image, acc, acc2, colsum_partial, toomU, tiles, part, zero_piece;
  QWindow win;
  size_t acc_stride = 0;
  struct Tiles { int first, count, col0, col1; }; // a range of the tile list and the columns of the lower triangle it covers
  Tiles all() const { return Tiles{0, ntile_, 0, cols_}; }
  Tiles left() const { return Tiles{0, ntile_left_, 0, split_col_}; }                        // of a chased Q': syrk_tile_order(N, split_col)
  Tiles right() const { return Tiles{ntile_left_, ntile_ - ntile_left_, split_col_, cols_}; }
  int plan_tiles() const { return std::max(ntile_left_, ntile_ - ntile_left_); }             // the larger launch

  // (Re)size everything for a rows x cols operand under the current budgets; buffers that already fit are kept.  one_chunk:
  // the image of all rows whatever the budget (chased Q', bench_op); split_col > 0: the tile list in two parts.
  // The windows are planned last and TOGETHER, against what is left of the device: the solver's stage is prepared when
  // everything else of the solver is allocated.  (The reference bounds the sum of its input and output residue windows by
  // --maxSharedMemory the same way: BigInt_Shared_Memory_Syrk_Context.cxx:149-215.)  Reserve for what comes later (the
  // exchange's buffers and RCCL's, operator scratch): 1/16 of the device + 1 GiB; never more than 1/8 of the device --
  // chunking costs nothing measurable while a chunk keeps thousands of workgroups (profiles/r05_syrk_chunks.txt,
  // r06_image_chunks.txt), and ranks that share a GPU (tests) each see the memory the others have not taken yet.
  // SDPB_HIP_SYRK_IMAGE_BYTES / SDPB_HIP_SYRK_PART_BYTES / sdpb_hip_set_max_shared_memory override.
  void prepare(size_t rows, int cols, hipStream_t stream, bool one_chunk = false, int split_col = 0)
  {
    auto fit = [](DevBuf<uint32_t> &b, size_t words) {
      if(b.n != std::max<size_t>(words, 1))
        b.alloc(words);
    };
    if(cols != cols_ || split_col != split_col_ || !tiles.p)
      {
        const std::vector<uint32_t> order = syrk_tile_order(cols, split_col, &ntile_left_, SYRK_EDGE);
        ntile_ = (int)order.size();
        tiles.upload(order);
      }
    rows_ = rows, cols_ = cols, split_col_ = split_col;
    acc_stride = (size_t)cols * cols + cols;
    fit(acc, acc_stride * ACCW);
    if(SYRK_TOOM4)
      fit(toomU, TOOMU_WORDS * cols);
    fit(colsum_partial, (size_t)colsum_slices(rows) * COLSUM_WORDS * cols);
    fit(zero_piece, 64);
    if(!rec_->default_words)
      {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        const size_t reserve = total_b / 16 + ((size_t)1 << 30);
        const size_t b = std::min(free_b > reserve ? free_b - reserve : 0, total_b / 8);
        rec_->default_words = std::max<size_t>(b, (size_t)64 << 20) / sizeof(uint32_t);
      }
    win = q_window((unsigned)rows, cols, one_chunk);
    if(image.n != win.image_words)
      {
        image.alloc(win.image_words);
        HIP_CHECK(hipMemsetAsync(image.p, 0, image.n * sizeof(uint32_t), stream));
      }
    if(win.chunks > 1)
      fit(acc2, acc_stride * ACCW);
    const size_t budget = syrk_part_budget_words();
    const size_t words = std::max(syrk_plan(ntile_left_, win.chunk_rows, budget).part_words, // (no split: every tile is "left")
                                  syrk_plan(ntile_ - ntile_left_, win.chunk_rows, budget).part_words);
    if(words)
      fit(part, words);
  }

  // ---- launches ----------------------------------------------------------------------
  // S_n = sum_r a'_rn behind the N x N block of acc (kernels.hpp: k_fx_colsum), all rows in one window
  void column_sums(hipStream_t stream) { column_sums(stream, acc.p, (unsigned)rows_); }
  // G = sum_r a'_ri a'_rj over the tiles `t` into acc, all rows in one window
  void G(hipStream_t stream, const Tiles &t) { G(stream, t, acc.p, (unsigned)rows_); }
  // Q' = sum over the input windows: `make(r0, rows)` writes the image of rows [r0, r0 + rows) into `image` (stride
  // win.stride); the first window's column sums and product go to acc, those of the others to acc2 and are added.  `mark`
  // is called once, after the first window's column sums (the HIP events that bracket the dominant kernel).
  template <class MakeImage, class Mark> void G_windows(hipStream_t stream, MakeImage &&make, Mark &&mark)
  {
    for(int c = 0; c < win.chunks; ++c)
      {
        const size_t r0 = (size_t)c * win.chunk_rows;
        const unsigned rows = (unsigned)std::min<size_t>(win.chunk_rows, rows_ - r0);
        if(c > 0 && rows < win.chunk_rows) // a shorter last window: the rows behind it still hold the previous window
          HIP_CHECK(hipMemsetAsync(image.p, 0, image.n * sizeof(uint32_t), stream));
        make(r0, rows);
        uint32_t *out = c == 0 ? acc.p : acc2.p;
        column_sums(stream, out, rows);
        if(c == 0)
          mark();
        G(stream, all(), out, rows);
        if(c > 0)
          launch(k_acc_add_tri<ACCW>, dim3(cdiv(acc_stride, WG)), dim3(WG), stream, acc.p, (const uint32_t *)acc2.p, acc_stride, cols_);
      }
    rec_->last_windows = win.chunks;
  }

private:
  int num_cus_;
  SyrkRecord own_, *rec_;
  size_t rows_ = 0;
  int cols_ = 0, split_col_ = 0, ntile_ = 0, ntile_left_ = 0;

  void column_sums(hipStream_t stream, uint32_t *out, unsigned nrows)
  {
    const unsigned slices = colsum_slices(nrows), rows_per_slice = cdiv(nrows, slices);
    const uint32_t *fx = image.p;
    uint32_t *partial = colsum_partial.p;
    const int N = cols_;
    const dim3 grid(cdiv(N, 64), slices), final_grid(cdiv(N, WG));
    // (the arms below are not all exclusive at compile time: which kernels a width instantiates stays as it has been)
    if constexpr(SYRK_TOOM4)
      {
        if constexpr(SYRK_TOOM5K)
          {
            launch(k_fx_colsum5<FX>, grid, dim3(WG), stream, fx, win.stride, nrows, N, rows_per_slice, partial);
            launch(k_fx_colsum5_final<FX>, final_grid, dim3(WG), stream, (const uint32_t *)partial, (int)slices, N, out, acc_stride, toomU.p,
                   (unsigned long long)nrows);
            return;
          }
        launch(k_fx_colsum2<FX, true>, grid, dim3(WG), stream, fx, win.stride, nrows, N, rows_per_slice, partial);
        launch(k_fx_colsum4_final<FX>, final_grid, dim3(WG), stream, (const uint32_t *)partial, (int)slices, N, out, acc_stride, toomU.p,
               (unsigned long long)nrows);
        return;
      }
    else if constexpr(SYRK_TWO_LEVEL)
      {
        launch(k_fx_colsum2<FX>, grid, dim3(WG), stream, fx, win.stride, nrows, N, rows_per_slice, partial);
        launch(k_fx_colsum2_final<FX>, final_grid, dim3(WG), stream, (const uint32_t *)partial, (int)slices, N, out, acc_stride);
        return;
      }
    launch(k_fx_colsum<FX>, grid, dim3(WG), stream, fx, win.stride, nrows, N, rows_per_slice, partial);
    launch(k_fx_colsum_final<FX>, final_grid, dim3(WG), stream, (const uint32_t *)partial, (int)slices, N, out, acc_stride);
  }
  // (kernels.hpp: k_syrk_fx) rows split over workgroups when that fills the last round of resident workgroups better;
  // `part` grows on demand (never beyond the budget)
  void G(hipStream_t stream, const Tiles &t, uint32_t *out_acc, unsigned nrows)
  {
    const int ntile = t.count, N = cols_, col0 = t.col0, col1 = t.col1;
    if(ntile == 0 || col1 <= col0)
      return;
    const int gsplit = syrk_group_split();
    // (the plan is made for the window's full height, so that a shorter last window reuses the same buffer)
    const SyrkPlan pl = syrk_plan(ntile, nrows, syrk_part_budget_words());
    if(pl.uses_part && part.n < pl.part_words)
      part.alloc(pl.part_words);
    rec_->last_plan = pl;
    const uint32_t *fx = image.p, *tu = toomU.p;
    constexpr size_t TW = (size_t)SYRK_EDGE * SYRK_EDGE;
    for(int t0 = 0; t0 < ntile; t0 += pl.chunk_tiles)
      {
        const int nt = std::min(pl.chunk_tiles, ntile - t0);
        const uint32_t *tl = tiles.p + t.first + t0;
        const int nsplit = nt == pl.chunk_tiles ? pl.nsplit_first : std::min(pl.nsplit_first, syrk_splits_for(nt, nrows, pl.part_words));
        const unsigned rps = cdiv(cdiv(nrows, nsplit), SYRK_RB) * SYRK_RB;
        const size_t ps = (size_t)nt * TW, total = ps; // plane stride of the chunk's partial planes = its packed words
        const bool packed = pl.uses_part;
        uint32_t *out = packed ? part.p : out_acc;
        const size_t os = packed ? ps : acc_stride;
        const dim3 grid(8 * cdiv((size_t)nt * nsplit, 8)), finish_grid(cdiv(total, WG));
        if constexpr(SYRK_TOOM4)
          {
            if constexpr(SYRK_TOOM5K)
              launch(k_syrk5_k2<FX, SYRK5_ROWS>, dim3(8 * cdiv((size_t)nt * nsplit * gsplit, 8)), dim3(SYRK5_WG), stream, fx, win.stride, nrows, N, out,
                     os, tl, nt, nsplit, rps, gsplit);
            else if constexpr(SYRK_TOOM4K)
              launch(k_syrk_fx3<FX, SYRK_RB>, dim3(8 * cdiv((size_t)nt * nsplit * gsplit, 8)), dim3(WG), stream, fx, win.stride, nrows, N, out, os, tl,
                     nt, nsplit, rps, gsplit);
            else
              launch(k_syrk_fx2<FX, SYRK_RB, true>, grid, dim3(WG), stream, fx, win.stride, nrows, N, out, os, tl, nt, nsplit, rps,
                     (const uint32_t *)zero_piece.p, 1);
            int nsum = nsplit;
            if constexpr(SYRK_TOOM4K)
              if(nsplit > 1)
                {
                  launch(k_syrk3_sum_splits<FX>, dim3(cdiv(total, WG), SYRK_NPROD), dim3(WG), stream, part.p, nsplit, ps, tl, total, N, col0, col1);
                  nsum = 1;
                }
            if constexpr(SYRK_TOOM5K)
              launch(k_syrk5_finish<FX>, finish_grid, dim3(WG), stream, (const uint32_t *)part.p, nsum, ps, tl, total, tu, out_acc, acc_stride, N,
                     col0, col1);
            else
              launch(k_syrk4_finish<FX>, finish_grid, dim3(WG), stream, (const uint32_t *)part.p, nsum, ps, tl, total, tu, out_acc, acc_stride, N,
                     col0, col1);
            continue;
          }
        else if constexpr(SYRK_TWO_LEVEL)
          launch(k_syrk_fx2<FX, SYRK_RB>, grid, dim3(WG), stream, fx, win.stride, nrows, N, out, os, tl, nt, nsplit, rps,
                 (const uint32_t *)zero_piece.p, (int)packed);
        else
          launch(k_syrk_fx<FX, SYRK_RB>, grid, dim3(WG), stream, fx, win.stride, nrows, N, out, os, tl, nt, nsplit, rps, (int)packed);
        if(packed)
          launch(k_syrk_reduce<FX>, finish_grid, dim3(WG), stream, (const uint32_t *)part.p, nsplit, ps, tl, total, out_acc, acc_stride, N, col0,
                 col1);
      }
  }
};
} // namespace sdpb
