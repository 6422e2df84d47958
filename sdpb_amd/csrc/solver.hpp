// solver.hpp — host driver of the device-resident interior-point iteration.
//
// Mirrors the reference's SDP_Solver (src/sdp_solve/SDP_Solver.hxx:28-112): state
// x, X, y, Y and the residues live in HBM for the whole run; iterate() is one pass
// of the loop body of SDP_Solver::run (run/run.cxx:380-467) including
// SDP_Solver::step (run/step/step.cxx:51-229).  Only a handful of scalars cross
// PCIe per iteration.  There is no CPU compute path: every matrix operation is a
// HIP kernel launch (kernels.hpp).
#pragma once
#include "kernels.hpp"
#include "syrk_stage.hpp"
#include "mw_host.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <utility>

namespace sdpb
{
struct SolverError : std::runtime_error
{
  int code; // 1 = Cholesky not PD, 4 = bad argument (include/sdpb_hip.h)
  SolverError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

// Collective callbacks supplied by the caller (one process per GPU; the Python
// launcher implements them with torch.distributed over RCCL, a C++ caller with RCCL
// or MPI directly).  Buffers are device pointers owned by the library.
struct Collectives
{
  // in-place SUM over ranks of `count` unsigned 64-bit integers
  int (*allreduce_sum_u64)(void *user, void *dev_ptr, size_t count) = nullptr;
  // gather `bytes` from every rank into recv (world*bytes), rank order
  int (*allgather_bytes)(void *user, const void *dev_send, void *dev_recv, size_t bytes) = nullptr;
  void *user = nullptr;
};

// Cross-rank exchange behind one interface: stream-ordered from the caller's point of view.
//   CallbackComm: host callbacks (MPI host, torch.distributed in the tests/launcher); the
//                 stream is synchronised around the call.
//   RcclComm:     RCCL inside the library (rccl_comm.hpp), enqueued on the library's stream —
//                 no host synchronisation at all.
struct Comm
{
  virtual ~Comm() {}
  virtual void allgather(const void *dev_send, void *dev_recv, size_t bytes, hipStream_t st) = 0;
  virtual void allreduce_sum_u64(void *dev_buf, size_t count, hipStream_t st) = 0;
  virtual const char *name() const = 0;
  virtual int ranks() const { return -1; } // size of the communicator as the transport reports it (-1: opaque callbacks)
  // in-place broadcast of `bytes` from rank `root`; false = not offered by this transport (the caller
  // then emulates it with an all-gather)
  virtual bool broadcast(void *, size_t, int, hipStream_t) { return false; }
  // asynchronous error state of the transport (RCCL: ncclCommGetAsyncError; 0 = none / not offered); safe to
  // call from another thread while the iteration thread waits on a stream (the bench watchdog does)
  virtual int async_error() const { return 0; }
};
struct CallbackComm : Comm
{
  Collectives c;
  explicit CallbackComm(const Collectives &cc) : c(cc) {}
  void allgather(const void *send, void *recv, size_t bytes, hipStream_t st) override
  {
    if(!c.allgather_bytes)
      throw SolverError(4, "world_size > 1 but no all-gather callback was registered (sdpb_hip_set_collectives)");
    HIP_CHECK(hipStreamSynchronize(st));
    if(c.allgather_bytes(c.user, send, recv, bytes) != 0)
      throw HipError(3, "allgather callback failed");
  }
  void allreduce_sum_u64(void *buf, size_t count, hipStream_t st) override
  {
    if(!c.allreduce_sum_u64)
      throw SolverError(4, "world_size > 1 but no all-reduce callback was registered (sdpb_hip_set_collectives)");
    HIP_CHECK(hipStreamSynchronize(st));
    if(c.allreduce_sum_u64(c.user, buf, count) != 0)
      throw HipError(3, "allreduce callback failed");
  }
  const char *name() const override { return "callbacks"; }
};

} // namespace sdpb
#include "rccl_comm.hpp"
namespace sdpb
{

enum TerminateReason // SDP_Solver_Terminate_Reason.hxx
{
  NotTerminated = -1,
  PrimalDualOptimal = 0,
  PrimalFeasible,
  DualFeasible,
  PrimalFeasibleJumpDetected,
  DualFeasibleJumpDetected,
  MaxComplementarityExceeded,
  MaxIterationsExceeded,
  MaxRuntimeExceeded,
  PrimalStepTooSmall,
  DualStepTooSmall,
  SIGTERM_Received
};
inline const char *terminate_string(int r)
{
  static const char *names[] = {"found primal-dual optimal solution",
                                "found primal feasible solution",
                                "found dual feasible solution",
                                "primal feasible jump detected",
                                "dual feasible jump detected",
                                "maxComplementarity exceeded",
                                "maxIterations exceeded",
                                "maxRuntime exceeded",
                                "primal step too small",
                                "dual step too small",
                                "SIGTERM signal received"};
  return (r < 0 || r > 10) ? "" : names[r];
}

// Static block -> GPU assignment: longest-processing-time greedy on an analytic
// cost (the quantities the reference measures into block_timings: cholesky_ +
// solve_ + syrk share, bigint_syrk/Readme.md:325-342; analogue of
// compute_block_grid_mapping.hxx:58-183).  Deterministic, identical on every rank.
// `measured`: per-block costs from an earlier run's block_timings file (read_block_costs.cxx:14-59);
// empty -> the analytic model.
inline std::vector<int> plan_block_owners(const std::vector<int> &dims, const std::vector<int> &num_points, int N, int world,
                                          const std::vector<long long> &measured = {})
{
  const int J = (int)dims.size();
  std::vector<double> cost(J);
  for(int j = 0; j < J; ++j)
    {
      const double m = dims[j], K = num_points[j], P = K * m * (m + 1) / 2;
      const double n0 = m * ((num_points[j] + 1) / 2), n1 = m * K - n0;
      cost[j] = P * P * P / 3 + P * P * N + P * (double)N * N / 2 + 8 * P * P + 5 * (n0 * n0 * n0 + n1 * n1 * n1);
    }
  if((int)measured.size() == J)
    for(int j = 0; j < J; ++j)
      cost[j] = (double)measured[j];
  std::vector<int> order(J), owner(J, 0);
  for(int j = 0; j < J; ++j)
    order[j] = j;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
  // least loaded rank; ties (a block_timings file may hold many zeros: blocks too small for the
  // file's resolution) go to the rank with the fewest blocks, so zero-cost blocks spread out
  // instead of piling up on rank 0
  std::vector<double> load(world, 0.0);
  std::vector<int> held(world, 0);
  for(int j : order)
    {
      int best = 0;
      for(int r = 1; r < world; ++r)
        if(load[r] < load[best] || (load[r] == load[best] && held[r] < held[best]))
          best = r;
      owner[j] = best;
      load[best] += cost[j];
      held[best] += 1;
    }
  return owner;
}

class SolverBase
{
public:
  virtual ~SolverBase() {}
  virtual void set_param(const std::string &name, const char *value) = 0;
  virtual void set_flags(long max_iterations, bool fpf, bool fdf, bool dpfj, bool ddfj) = 0;
  virtual void set_block(int j, const char *be, const char *bo, const char *B, const char *c) = 0;
  virtual void set_block_f64(int j, const char *be, const char *bo, const double *B, const double *c) = 0;
  virtual void set_objective(const char *b, const char *constant) = 0;
  // binary flavour: records in mpf_t layout (mw_host.hpp: from_mpf_record), limbs64 limbs each
  virtual void set_block_mpf(int j, int limbs64, const uint64_t *be, const uint64_t *bo, const uint64_t *B, const uint64_t *c) = 0;
  virtual void set_objective_mpf(int limbs64, const uint64_t *b, const uint64_t *constant) = 0;
  virtual size_t get_array_mpf(const std::string &which, int j, int parity, int limbs64, uint64_t *out, size_t capacity) = 0;
  virtual void set_array_mpf(const std::string &which, int j, int parity, int limbs64, const uint64_t *values, size_t count) = 0;
  virtual void init_state() = 0;
  virtual bool iterate() = 0;
  virtual void schur_solver_init() = 0;
  virtual void schur_solve() = 0;
  virtual int terminate_reason() const = 0;
  virtual std::string get_scalar(const std::string &name) = 0;
  virtual std::string get_array(const std::string &which, int j, int parity) = 0;
  virtual void set_array(const std::string &which, int j, int parity, const char *txt) = 0;
  virtual int block_owner(int j) const = 0;
  virtual void set_collectives(const Collectives &c) = 0;
  virtual void init_rccl(const void *unique_id, size_t id_bytes) = 0;
  virtual const char *comm_name() const = 0;
  virtual void set_profiling(bool on) = 0;
  virtual void set_max_runtime(double seconds) = 0;
  virtual void set_max_shared_memory(unsigned long long bytes) = 0;
  virtual std::string memory_plan_json() = 0;
  virtual void request_stop() = 0;
  virtual long host_syncs() const = 0;
  virtual void progress(unsigned long long out[8]) const = 0;
  virtual std::string timers_json() = 0;
  virtual int limbs() const = 0;
  virtual int fx_frac_bits() const = 0;
  virtual double bench_op(const std::string &op, int a, int b, int reps) = 0;
  virtual void block_timings(long long *microseconds) = 0;
  virtual void block_clock_ticks(unsigned long long *cholesky, unsigned long long *solve) = 0;
  // operator-level entry points for parity tests
  virtual std::string op_scalar(const std::string &op, const char *a, const char *b) = 0;
  virtual std::string op_int_syrk(int rows, int cols, const char *ints_colmajor) = 0;
  virtual std::string op_syrk_Q(int rows, int cols, const char *P_colmajor) = 0;
  virtual std::string op_min_eigenvalue(int n, const char *A_colmajor) = 0;
};

inline void split_numbers(const char *txt, std::vector<std::pair<const char *, const char *>> &out)
{
  out.clear();
  const char *p = txt;
  while(*p)
    {
      while(*p == ' ' || *p == '\n' || *p == '\t' || *p == ',' || *p == '\r')
        ++p;
      if(!*p)
        break;
      const char *q = p;
      while(*q && *q != ' ' && *q != '\n' && *q != '\t' && *q != ',' && *q != '\r')
        ++q;
      out.emplace_back(p, q);
      p = q;
    }
}

template <int NL> class Solver : public SolverBase
{
  using M = Mw<NL>;
  static constexpr int FX = fx_limbs<NL>(); // 32 (NL - 2) = GMP's rounded precision 64 (l - 1) (compute_Q.cxx:107), or the next multiple of four limbs
  static_assert(FX <= NL, "the image is cut from an NL-limb product");
  using Syrk = FxSyrk<FX>; // the exact product Q' = P'^T P' (syrk_stage.hpp): its formats, budgets, plans, buffers and launches

  // ---- problem shape -------------------------------------------------------
  int precision_, J_, N_, rank_, world_;
  std::vector<int> dims_, npts_, owner_;
  std::vector<int> local_; // global indices of the blocks this rank owns
  std::vector<BlockDesc> blk_;
  int Jl_ = 0;
  size_t Ptot_ = 0;        // local sum of P_j
  unsigned long long Ptot_global_ = 0; // sum over all ranks
  size_t psd_elems_ = 0, psd_rows_local_ = 0;
  long total_psd_rows_ = 0; // global (step.cxx:143)
  // stream_main_ is the library's stream; stream_ is the stream launches currently go to — normally the
  // same, for a scope one of the side streams (OnSideStream, the CU-masked stream beside Cholesky(Q)).  The
  // named streams themselves never change after construction.
  hipStream_t stream_main_ = nullptr, stream_ = nullptr;

  // ---- descriptors -----------------------------------------------------------
  DevBuf<BlockDesc> d_blk_;
  DevBuf<MatDesc> d_Et_;
  DevBuf<MatDesc> d_basesT_, d_scaled_, d_psd_, d_bases_, d_E_, d_pair_, d_schur_, d_bt_, d_vecP_, d_vecn_, d_Q_, d_vecQ_;
  std::vector<MatDesc> h_Et_;
  std::vector<MatDesc> h_basesT_, h_scaled_, h_psd_, h_bases_, h_E_, h_pair_, h_schur_, h_bt_, h_vecP_, h_vecn_;
  // blocked Cholesky(Q): per panel descriptors
  DevBuf<MatDesc> d_qdiag_, d_rowP_; // diagonal blocks of Q; dx as 1 x P row vectors
  int q_nb_ = 0, q_panels_ = 0;
  int max_n_ = 0, max_q_ = 0, max_P_ = 0, max_pairs_ = 1;
  size_t max_scaled_ = 0;

  // ---- device arrays ---------------------------------------------------------
  DevArray X_, Y_, Xc_, Yc_, dX_, dY_, PR_, mXY_, R_, Z_, W_;
  DevArray basesT_, scaled_, bases_, E_, Et_, T_, YQ_, AX_, AY_, S_, BT_, PT_;
  DevArray c_, x_, dx_, dres_, invdS_, invdX_, invdY_, eigD_, eigE_, eigD2_, eigE2_, cmby_;
  DevArray LiX_, LiY_, LiS_, LiQ_, qtmpv_; // inverted diagonal blocks of the Cholesky factors
  DevArray part2_; // partial sums of the column norms (the Q chain may run beside the predictor, which uses part_)
  DevArray b_, y_, dy_, rp_, norms_, invnorms_, Q_, invdQ_, part_, red_, red2_, lam_, lam2_, ratio_, scal_;
  // P = L^{-1} B with the trailing updates as fixed-point tile dot products (kernels.hpp: k_td_image_L, k_trsm_rlt_panel_td):
  // images of the tiles of every L_j below its diagonal blocks, their row exponents and limb sums, tile offsets per block
  bool use_td_ = false;
  DevBuf<int> td_tile_off_;
  DevBuf<uint32_t> td_img_, td_sum_;
  DevBuf<int32_t> td_exp_;
  int td_max_tiles_ = 0;
  int num_cus_;
  Syrk syrk_; // the iteration's stage: all local rows of P' x N
  DevBuf<double> eigF_, eigF2_;
  DevBuf<unsigned long long> acc64_;
  DevBuf<int> flags_; // [0..2Jl) chol fail per psd (X) matrix, then Q fail, Q diag fail
  DevBuf<int> flags2_; // chol fail of Y (factored on the side stream concurrently with X)
  DevBuf<int> flags3_; // chol fail of the Schur blocks S_j
  // Per-block measured cost (kernels.hpp: WgClock): [0, Jl) Cholesky(S_j), [Jl, 2 Jl) P_j = L_j^{-1} B_j, in
  // ticks of the 100 MHz wall clock summed over the workgroups that worked on the block; accumulated over
  // the profiled iterations only (compute_Q.cxx:40-53 cholesky_/solve_ timers)
  DevBuf<unsigned long long> blk_cycles_;
  // Result block (kernels.hpp: XOp): R_COUNT numbers + X_EXTRA words.  Reductions deposit their
  // results here; the host reads the whole block with one copy at each of the three
  // synchronisation points of an iteration (fetch()).
  enum ResSlot
  {
    R_CX = 0,
    R_BY,
    R_DERR,
    R_PERR_P,
    R_PERR_p,
    R_TRACE,
    R_RERR,
    R_FROB,
    R_LAMX,
    R_LAMY,
    R_COND,
    R_QCOND,
    R_COUNT
  };
  static_assert(R_COUNT <= X_MAXSLOTS, "result block too large for XOps");
  static constexpr size_t RES_WORDS = (size_t)(NL + 1) * R_COUNT + X_EXTRA;
  DevBuf<uint32_t> qpanel_msg_, qpanel_gather_; // panel message of the distributed Cholesky(Q) (+ all-gather emulation of its broadcast)
  // Cholesky(Q) distributed over the ranks (1-D block-cyclic over column panels, one broadcast per panel:
  // SURVEY.md §8e; the reference factors Q over all ranks too, initialize_schur_complement_solver.cxx:95-103)
  // instead of replicated.  Opt-in with SDPB_HIP_DIST_CHOLQ=1 (worthwhile from N ~ 1536 up, where the N^3/3
  // trailing updates outweigh the per-panel broadcasts: C5-class); replicated otherwise.
  bool dist_cholq_ = false;
  // Q' in two column chunks, Cholesky(Q) chasing it (initialize_schur_complement_solver): the left chunk_cA_ columns are
  // multiplied, finished, reduced over the ranks and restored first; panels [0, chase_hA_) are factored on the side
  // streams while the main stream multiplies the right chunk
  bool q_chase_ = false;
  int chase_hA_ = 0, chase_cA_ = 0;
  hipEvent_t ev_chunk_ = nullptr, ev_syrk2_ = nullptr, ev_syrk3_ = nullptr;
  bool syrk_events2_pending_ = false;
  long xc_broadcast_calls_ = 0;
  double xc_broadcast_bytes_ = 0;
  DevBuf<uint32_t> resbuf_, xgather_;
  std::vector<M> res_host_ = std::vector<M>(R_COUNT);
  uint32_t xw_host_[X_EXTRA] = {0xffffffffu, 0, 0, 0, 0, 0, 0};
  std::unique_ptr<Comm> comm_;
  // Collective-sequence self-check and progress record (kernels.hpp: XW_SEQ_LO).  Every collective this rank
  // hands to the transport is folded into a running 64-bit FNV-1a hash of (kind, bytes, root); the hash
  // travels in the result block and k_combine_slots compares the ranks' values at every synchronisation
  // point.  The atomics are also what sdpb_hip_progress reads from a watchdog thread while the iteration
  // thread sits in a stream synchronisation behind a collective that never completes.
  enum CollKind : unsigned
  {
    COLL_ALLGATHER = 1,
    COLL_ALLREDUCE = 2,
    COLL_BROADCAST = 3
  };
  std::atomic<unsigned long long> seq_hash_{0xcbf29ce484222325ull}, seq_count_{0}, seq_last_kind_{0}, seq_last_bytes_{0},
    seq_last_root_{0}, prog_iteration_{0}, prog_syncs_{0};
  // Q substitution with lane-parallel exact sums (k_qsolve_panel3, round 4); SDPB_HIP_QSOLVE_SUM_LANES=0 runs the
  // round-3 kernel (k_qsolve_panel2: 8 + 4 dependent aligned adds per sum) for A/B measurements
  bool qsolve_sum_lanes_ = true;
  bool tridiag_wide_ = true; // SDPB_HIP_TRIDIAG_WIDE=0: TRI_T lanes per matrix whatever the rank owns (A/B)
  unsigned long long launches_ = 0; // kernels launched by this solver's init_state / iterate / schur_* (LaunchScope)
  DevBuf<int> tri_ids_;      // PSD matrices by size bucket for k_tridiag: the tri_count_large_ with more than TRI_SMALL_N rows first
  int tri_count_large_ = 0, tri_lanes_small_ = TRI_T, tri_lanes_large_ = TRI_T;
  static constexpr int TRI_SMALL_N = 24;
  int seq_fault_rank_ = -1; // SDPB_HIP_TEST_SEQ_FAULT=r: rank r perturbs its hash (test of the mismatch path)
  void note_collective(unsigned kind, size_t bytes, int root)
  {
    unsigned long long h = seq_hash_.load(std::memory_order_relaxed);
    const unsigned long long words[3] = {kind, (unsigned long long)bytes, (unsigned long long)(root + 1)};
    for(unsigned long long w : words)
      for(int b = 0; b < 8; ++b)
        {
          h ^= (w >> (8 * b)) & 0xffu;
          h *= 0x100000001b3ull;
        }
    seq_hash_.store(h, std::memory_order_relaxed);
    seq_last_kind_.store(kind, std::memory_order_relaxed);
    seq_last_bytes_.store(bytes, std::memory_order_relaxed);
    seq_last_root_.store((unsigned long long)(root + 1), std::memory_order_relaxed);
    seq_count_.fetch_add(1, std::memory_order_release);
  }
  // what this rank handed to the exchange (bench.py: proof that N ranks exchanged, and how much)
  long xc_allgather_calls_ = 0, xc_allreduce_calls_ = 0;
  double xc_allgather_bytes_ = 0, xc_allreduce_bytes_ = 0;
  long host_syncs_ = 0;
  bool profile_ = false;
  // SDPB_HIP_OVERLAP_SYRK=1 moves the Q chain to the side stream (experiment, measured on C4: the VALU-bound
  // syrk slows by 8 ms when it shares the CUs, the step by 4 ms: profiles/r02d_overlap_syrk.txt) -> off
  bool overlap_syrk_ = false;
  long profiled_iterations_ = 0;
  double max_runtime_s_ = std::numeric_limits<double>::infinity();
  std::chrono::steady_clock::time_point start_time_;
  bool started_ = false;
  std::atomic<int> stop_requested_{0};

  // ---- parameters (Solver_Parameters.hxx:13-30) --------------------------------
  M duality_gap_threshold_, primal_error_threshold_, dual_error_threshold_, initial_matrix_scale_primal_,
    initial_matrix_scale_dual_, feasible_centering_parameter_, infeasible_centering_parameter_, step_length_reduction_,
    max_complementarity_, min_primal_step_, min_dual_step_;
  long max_iterations_ = 500;
  bool find_primal_feasible_ = false, find_dual_feasible_ = false, detect_primal_feasible_jump_ = false,
       detect_dual_feasible_jump_ = false;

  // ---- scalars (SDP_Solver.hxx:44-74, print_iteration.cxx:91-104) ---------------
  M objective_const_, primal_objective_, dual_objective_, duality_gap_, primal_error_P_, primal_error_p_, dual_error_,
    R_error_, mu_, beta_corrector_, primal_step_length_, dual_step_length_, Q_cond_number_, max_block_cond_number_;
  std::string max_block_cond_number_name_;
  long iteration_ = 0;
  int terminate_reason_ = NotTerminated;
  Collectives coll_;
  hipStream_t stream_q_ = nullptr; // Cholesky(Q) runs here, concurrently with stream_
  hipEvent_t ev_q_ready_ = nullptr, ev_q_done_ = nullptr, ev_la_strip_ = nullptr, ev_la_bulk_ = nullptr;
  hipStream_t stream_q2_ = nullptr; // bulk updates of the look-ahead Cholesky(Q)
  // While the factorisation of Q is pending, the main stream's work (residues, the predictor's Q-independent
  // part) is throughput work that fills every CU, and the chain's single workgroups then wait for wavefront
  // slots and LDS (0.75 instead of 0.41 ms per panel).  That stretch of the main stream therefore runs on a
  // stream whose CU mask leaves R compute units free (hipExtStreamCreateWithCUMask); the syrk and everything
  // after the join stay on the unmasked stream.  Measured on C4 (profiles/r02l_beside_cus.txt), R = 0 / 16 /
  // 32 / 64 / 128: wait at the join 5.5 / 3.1 / 2.0 / 0.55 / 0.02 ms, iteration 281.5 / 280.4 / 280.4 / 279.5 /
  // 281.1 ms.  Default R = a quarter of the CUs with one rank; with several ranks (collectives inside the
  // stretch, less work to hide) only on request: SDPB_HIP_BESIDE_CUS=R, 0 switches it off.
  hipStream_t stream_beside_ = nullptr;
  hipEvent_t ev_beside_ = nullptr;
  bool beside_active_ = false;
  bool q_pending_ = false;
  bool single_stream_ = false;
  hipEvent_t ev_syrk0_ = nullptr, ev_syrk1_ = nullptr;
  bool syrk_events_pending_ = false;
  double syrk_kernel_ms_ = 0;
  long syrk_launches_ = 0;
  std::map<std::string, double> timers_ms_;
  std::vector<std::pair<std::string, double>> timer_order_;

  enum ScalSlot
  {
    S_MU = 0,
    S_BETAMU,
    S_ALPHA_P,
    S_ALPHA_D,
    S_COUNT
  };

public:
  Solver(int precision_bits, const std::vector<int> &dims, const std::vector<int> &num_points, int N, int rank, int world,
         const std::vector<long long> &block_costs = {})
      : precision_(precision_bits), J_((int)dims.size()), N_(N), rank_(rank), world_(world), dims_(dims), npts_(num_points),
        num_cus_(device_cus(N, (int)dims.size())), syrk_(num_cus_)
  {
    owner_ = plan_block_owners(dims, num_points, N, world, block_costs);
    HIP_CHECK(hipStreamCreate(&stream_main_));
    stream_ = stream_main_;
    {
      // The side stream carries latency-bound dependent chains (Cholesky(Q): 1000 pivots in a row)
      // next to throughput work on the main stream: at high priority its small launches are
      // dispatched as soon as they are ready instead of queueing behind full-chip kernels.
      int least = 0, greatest = 0;
      HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
      int prio = greatest;
      if(const char *e = std::getenv("SDPB_HIP_SIDE_PRIORITY")) // 0: same priority as the main stream (A/B)
        prio = std::atoi(e) ? greatest : 0;
      // SDPB_HIP_SINGLE_STREAM=1: everything on the main stream (debugging aid; a GPU test asserts that
      // the concurrent schedule gives bit-identical iterations, i.e. no ordering is left to chance)
      if(const char *e = std::getenv("SDPB_HIP_SINGLE_STREAM"))
        single_stream_ = std::atoi(e) != 0;
      if(single_stream_)
        stream_q_ = stream_q2_ = stream_main_;
      else
        {
          HIP_CHECK(hipStreamCreateWithPriority(&stream_q_, hipStreamNonBlocking, prio));
          HIP_CHECK(hipStreamCreateWithPriority(&stream_q2_, hipStreamNonBlocking, prio));
        }
    }
    {
      int reserve = world_ == 1 ? num_cus_ / 4 : 0;
      if(const char *e = std::getenv("SDPB_HIP_BESIDE_CUS"))
        reserve = std::atoi(e);
      if(reserve > 0 && reserve < num_cus_ && !single_stream_)
        {
          std::vector<uint32_t> mask((num_cus_ + 31) / 32, 0u);
          for(int cu = 0; cu < num_cus_; ++cu)
            if((cu * 37) % num_cus_ >= reserve) // the reserved ones are spread over the XCDs
              mask[cu / 32] |= 1u << (cu % 32);
          // an optimisation only: a runtime that refuses the mask leaves the schedule as it was
          if(hipExtStreamCreateWithCUMask(&stream_beside_, (uint32_t)mask.size(), mask.data()) != hipSuccess)
            {
              (void)hipGetLastError();
              stream_beside_ = nullptr;
            }
          else
            HIP_CHECK(hipEventCreateWithFlags(&ev_beside_, hipEventDisableTiming));
        }
    }
    HIP_CHECK(hipEventCreateWithFlags(&ev_la_strip_, hipEventDisableTiming));
    HIP_CHECK(hipEventCreateWithFlags(&ev_la_bulk_, hipEventDisableTiming));
    HIP_CHECK(hipEventCreate(&ev_q_ready_));
    HIP_CHECK(hipEventCreate(&ev_q_done_));
    HIP_CHECK(hipEventCreate(&ev_syrk0_));
    HIP_CHECK(hipEventCreate(&ev_syrk1_));
    HIP_CHECK(hipEventCreate(&ev_syrk2_));
    HIP_CHECK(hipEventCreate(&ev_syrk3_));
    HIP_CHECK(hipEventCreateWithFlags(&ev_chunk_, hipEventDisableTiming));
    build_layout();
    set_default_params();
  }
  static int device_cus(int N, int J) // the argument check comes first: bad arguments throw without touching the device
  {
    if(N <= 0 || J <= 0)
      throw SolverError(4, "sdpb_hip_create: need at least one block and N >= 1");
    int dev = 0;
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    return prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  ~Solver() override
  {
    if(ev_q_ready_)
      (void)hipEventDestroy(ev_q_ready_);
    if(ev_q_done_)
      (void)hipEventDestroy(ev_q_done_);
    if(ev_la_strip_)
      (void)hipEventDestroy(ev_la_strip_);
    if(ev_la_bulk_)
      (void)hipEventDestroy(ev_la_bulk_);
    leave_beside_stream();
    if(ev_beside_)
      (void)hipEventDestroy(ev_beside_);
    if(stream_beside_)
      (void)hipStreamDestroy(stream_beside_);
    if(stream_q2_ && !single_stream_)
      (void)hipStreamDestroy(stream_q2_);
    if(stream_q_ && !single_stream_)
      (void)hipStreamDestroy(stream_q_);
    if(ev_syrk0_)
      (void)hipEventDestroy(ev_syrk0_);
    if(ev_syrk1_)
      (void)hipEventDestroy(ev_syrk1_);
    if(ev_syrk2_)
      (void)hipEventDestroy(ev_syrk2_);
    if(ev_syrk3_)
      (void)hipEventDestroy(ev_syrk3_);
    if(ev_chunk_)
      (void)hipEventDestroy(ev_chunk_);
    if(stream_main_)
      (void)hipStreamDestroy(stream_main_);
  }
  int limbs() const override { return NL; }
  int fx_frac_bits() const override { return sdpb::fx_frac_bits<FX>(); }
  int block_owner(int j) const override { return owner_.at(j); }
  void set_collectives(const Collectives &c) override
  {
    coll_ = c;
    comm_.reset(new CallbackComm(c));
  }
  void init_rccl(const void *unique_id, size_t id_bytes) override
  {
    if(world_ == 1)
      return;
    comm_.reset(make_rccl_comm(unique_id, id_bytes, rank_, world_));
  }
  const char *comm_name() const override { return world_ == 1 ? "none" : (comm_ ? comm_->name() : "unset"); }
  void set_profiling(bool on) override { profile_ = on; }
  void set_max_runtime(double seconds) override { max_runtime_s_ = seconds; }
  // --maxSharedMemory (the reference bounds the shared-memory window of the Q stage with it, run.cxx:79-181,
  // BigInt_Shared_Memory_Syrk_Context.cxx:70-215): here the two windows of the Q stage TOGETHER -- the fixed-point image
  // of P' (input window: at most half of the bound, built for as many rows at a time as fit) and the partial planes of
  // the product (output window: the rest); 0 = the default plan
  void set_max_shared_memory(unsigned long long bytes) override
  {
    syrk_.set_max_shared_memory((size_t)bytes);
    HIP_CHECK(hipStreamSynchronize(stream_main_));
    prepare_syrk();
  }
  // bytes per array class on this rank + the plan of the syrk's partial planes
  std::string memory_plan_json() override
  {
    auto da = [](std::initializer_list<const DevArray *> l) {
      size_t b = 0;
      for(const DevArray *a : l)
        if(a->base)
          b += a->bytes();
      return b;
    };
    auto db = [](std::initializer_list<size_t> l) {
      size_t b = 0;
      for(size_t x : l)
        b += x;
      return b;
    };
    const QWindow &qwin = syrk_.win;
    const SyrkRecord &rec = syrk_.record();
    const size_t part_budget = syrk_.syrk_part_budget_words();
    const SyrkPlan pl = syrk_.syrk_plan(syrk_.plan_tiles(), qwin.chunk_rows, part_budget);
    const SyrkPlan unbounded = syrk_.syrk_plan(syrk_.plan_tiles(), (unsigned)Ptot_, 0);
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    std::ostringstream o;
    o << "{\"rank\": " << rank_ << ", \"limbs\": " << NL << ", \"owned_blocks\": " << Jl_ << ", \"rows\": " << Ptot_ << ", \"N\": " << N_
      << ", \"bytes\": {"
      << "\"psd_state_and_scratch\": " << da({&X_, &Y_, &Xc_, &Yc_, &dX_, &dY_, &PR_, &mXY_, &R_, &Z_, &W_, &LiX_, &LiY_})
      << ", \"bases_and_pairings\": " << da({&bases_, &basesT_, &scaled_, &E_, &Et_, &T_, &YQ_, &AX_, &AY_})
      << ", \"schur_blocks\": " << da({&S_, &LiS_})
      << ", \"B\": " << da({&BT_}) << ", \"P\": " << da({&PT_})
      << ", \"P_fixed_point_image\": " << syrk_.image.n * sizeof(uint32_t)
      << ", \"Q\": " << da({&Q_, &LiQ_}) + db({syrk_.acc.n * sizeof(uint32_t), syrk_.acc2.n * sizeof(uint32_t), acc64_.n * sizeof(unsigned long long), qpanel_msg_.n * sizeof(uint32_t)})
      << ", \"syrk_partial_planes\": " << syrk_.part.n * sizeof(uint32_t)
      << ", \"vectors_and_small\": "
      << da({&c_, &x_, &dx_, &dres_, &invdS_, &invdX_, &invdY_, &eigD_, &eigE_, &eigD2_, &eigE2_, &b_, &y_, &dy_, &rp_, &norms_, &invnorms_, &invdQ_,
             &qtmpv_, &part_, &part2_, &red_, &red2_, &lam_, &lam2_, &ratio_, &scal_, &cmby_})
           + db({syrk_.colsum_partial.n * sizeof(uint32_t), syrk_.toomU.n * sizeof(uint32_t), xgather_.n * sizeof(uint32_t)})
      << "}, \"syrk\": {\"tile_edge\": " << Syrk::SYRK_EDGE << ", \"tiles\": " << pl.ntile << ", \"chunks\": " << pl.nchunk
      << ", \"tiles_per_chunk\": " << pl.chunk_tiles << ", \"row_splits\": " << pl.nsplit_first
      << ", \"rows_per_split\": " << (pl.nsplit_first ? cdiv(qwin.chunk_rows, pl.nsplit_first) : 0) << ", \"planes_per_split\": " << Syrk::SYRK_PART_PLANES
      << ", \"partial_bytes\": " << pl.part_words * sizeof(uint32_t) << ", \"partial_bytes_unbounded\": " << unbounded.part_words * sizeof(uint32_t)
      << ", \"partial_bytes_full_square_layout\": "
      << (size_t)unbounded.nsplit_first * Syrk::SYRK_PART_PLANES * ((size_t)N_ * N_ + N_) * sizeof(uint32_t) * (unbounded.uses_part ? 1 : 0)
      << ", \"budget_bytes\": " << part_budget * sizeof(uint32_t) << ", \"budget_source\": \"" << syrk_.budget_source(false)
      << "\", \"bound_exceeded_min_chunk\": " << (pl.uses_part && pl.part_words > part_budget ? "true" : "false")
      << ", \"min_chunk_bytes\": " << Syrk::TILE_WORDS * sizeof(uint32_t) << "}"
      // the input window (BigInt_Shared_Memory_Syrk_Context.cxx:70-110: input_window_split_factor)
      << ", \"image\": {\"image_chunks\": " << qwin.chunks << ", \"rows_per_chunk\": " << qwin.chunk_rows << ", \"rows\": " << Ptot_
      << ", \"image_bytes\": " << qwin.image_words * sizeof(uint32_t) << ", \"image_bytes_unbounded\": " << Syrk::image_words_for(std::max<size_t>(Ptot_, 1), (size_t)N_) * sizeof(uint32_t)
      << ", \"budget_bytes\": " << qwin.budget_words * sizeof(uint32_t) << ", \"budget_source\": \"" << syrk_.budget_source(true)
      << "\", \"bound_exceeded_min_chunk\": " << (qwin.bound_exceeded ? "true" : "false") << ", \"accumulator_bytes\": " << syrk_.acc2.n * sizeof(uint32_t)
      << ", \"last_call_windows\": " << rec.last_windows << "}"
      << ", \"window_budget_bytes\": " << syrk_.window_budget_words() * sizeof(uint32_t)
      << ", \"last_syrk_call\": {\"tiles\": " << rec.last_plan.ntile << ", \"chunks\": " << rec.last_plan.nchunk
      << ", \"tiles_per_chunk\": " << rec.last_plan.chunk_tiles << ", \"row_splits\": " << rec.last_plan.nsplit_first
      << ", \"partial_bytes\": " << rec.last_plan.part_words * sizeof(uint32_t) << "}"
      << ", \"device\": {\"free_bytes\": " << free_b << ", \"total_bytes\": " << total_b << "}}";
    return o.str();
  }
  void request_stop() override { stop_requested_.store(1); } // async-signal-safe: a SIGTERM handler may call it
  long host_syncs() const override { return host_syncs_; }
  // [0] iteration, [1] host synchronisation points passed, [2] collectives enqueued, [3] sequence hash,
  // [4] kind of the last collective (1 all-gather, 2 all-reduce, 3 broadcast), [5] its bytes, [6] its root + 1
  // (0 = rootless), [7] the transport's asynchronous error code.  Lock-free: callable from any thread.
  void progress(unsigned long long out[8]) const override
  {
    out[0] = prog_iteration_.load();
    out[1] = prog_syncs_.load();
    out[2] = seq_count_.load(std::memory_order_acquire);
    out[3] = seq_hash_.load();
    out[4] = seq_last_kind_.load();
    out[5] = seq_last_bytes_.load();
    out[6] = seq_last_root_.load();
    out[7] = comm_ ? (unsigned long long)comm_->async_error() : 0ull;
  }
  int terminate_reason() const override { return terminate_reason_; }

private:
  // ==========================================================================
  // layout
  // ==========================================================================
  void build_layout()
  {
    size_t off_scaled = 0, off_psd = 0, off_bases = 0, off_E = 0, off_pair = 0, off_schur = 0, off_bt = 0, off_vecn = 0;
    for(int j = 0; j < J_; ++j)
      {
        const int m = dims_[j], K = npts_[j];
        const int n0 = m * ((K + 1) / 2), n1 = m * K - n0;
        total_psd_rows_ += n0 + n1;
        Ptot_global_ += (unsigned long long)K * m * (m + 1) / 2;
        if(owner_[j] != rank_)
          continue;
        local_.push_back(j);
        BlockDesc bd;
        bd.m = m;
        bd.K = K;
        bd.P = K * m * (m + 1) / 2;
        const int d = K - 1;
        bd.rows[0] = d / 2 + 1;
        bd.rows[1] = (d + 1) / 2;
        bd.n[0] = n0;
        bd.n[1] = n1;
        bd.voff = Ptot_;
        bd.global_index = j;
        blk_.push_back(bd);
        for(int b = 0; b < 2; ++b)
          {
            const int n = bd.n[b], q = m * K;
            h_psd_.push_back(MatDesc{off_psd, n, n, n, K});
            h_vecn_.push_back(MatDesc{off_vecn, n, 1, n, K});
            h_bases_.push_back(MatDesc{off_bases, bd.rows[b], K, bd.rows[b], K});
            h_basesT_.push_back(MatDesc{off_bases, K, bd.rows[b], K, K});
            const int pr = m * (m + 1) / 2;
            h_scaled_.push_back(MatDesc{off_scaled, K, pr * bd.rows[b], K, K});
            off_scaled += (size_t)K * pr * bd.rows[b];
            max_scaled_ = std::max(max_scaled_, (size_t)K * pr * bd.rows[b]);
            h_E_.push_back(MatDesc{off_E, n, q, n, K});
            h_Et_.push_back(MatDesc{off_E, q, n, q, K});
            h_pair_.push_back(MatDesc{off_pair, q, q, q, K});
            off_psd += (size_t)n * n;
            off_vecn += n;
            off_bases += (size_t)bd.rows[b] * K;
            off_E += (size_t)n * q;
            off_pair += (size_t)q * q;
            max_n_ = std::max(max_n_, n);
            max_q_ = std::max(max_q_, q);
          }
        h_schur_.push_back(MatDesc{off_schur, bd.P, bd.P, bd.P, K});
        h_bt_.push_back(MatDesc{off_bt, N_, bd.P, N_, K});
        h_vecP_.push_back(MatDesc{(unsigned long long)Ptot_, bd.P, 1, bd.P, K});
        off_schur += (size_t)bd.P * bd.P;
        off_bt += (size_t)N_ * bd.P;
        Ptot_ += bd.P;
        max_P_ = std::max(max_P_, bd.P);
        max_pairs_ = std::max(max_pairs_, m * (m + 1) / 2);
      }
    Jl_ = (int)local_.size();
    psd_elems_ = off_psd;
    psd_rows_local_ = off_vecn;

    d_blk_.upload(blk_);
    d_psd_.upload(h_psd_);
    d_vecn_.upload(h_vecn_);
    d_bases_.upload(h_bases_);
    d_basesT_.upload(h_basesT_);
    d_scaled_.upload(h_scaled_);
    d_E_.upload(h_E_);
    d_Et_.upload(h_Et_);
    d_pair_.upload(h_pair_);
    d_schur_.upload(h_schur_);
    d_bt_.upload(h_bt_);
    d_vecP_.upload(h_vecP_);
    d_Q_.upload(std::vector<MatDesc>{MatDesc{0, N_, N_, N_, 0}});
    d_vecQ_.upload(std::vector<MatDesc>{MatDesc{0, N_, 1, N_, 0}});

    // Q is processed in panels of PB columns (kernels.hpp)
    q_nb_ = PB;
    q_panels_ = (N_ + q_nb_ - 1) / q_nb_;
    std::vector<MatDesc> qd;
    for(int p = 0; p < q_panels_; ++p)
      {
        const int k0 = p * q_nb_, nb = std::min(q_nb_, N_ - k0);
        qd.push_back(MatDesc{(unsigned long long)k0 + (unsigned long long)k0 * N_, nb, nb, N_, 0});
      }
    d_qdiag_.upload(qd);
    {
      std::vector<MatDesc> rows;
      for(const MatDesc &v : h_vecP_)
        rows.push_back(MatDesc{v.off, 1, v.rows, 1, v.aux});
      d_rowP_.upload(rows);
    }

    for(DevArray *a : {&X_, &Y_, &Xc_, &Yc_, &dX_, &dY_, &PR_, &mXY_, &R_, &Z_, &W_, &LiX_, &LiY_})
      a->alloc(off_psd, NL);
    bases_.alloc(off_bases, NL);
    basesT_.alloc(off_bases, NL);
    scaled_.alloc(off_scaled, NL);
    for(DevArray *a : {&E_, &Et_, &T_, &YQ_})
      a->alloc(off_E, NL);
    AX_.alloc(off_pair, NL);
    AY_.alloc(off_pair, NL);
    S_.alloc(off_schur, NL);
    LiS_.alloc(off_schur, NL);
    BT_.alloc(off_bt, NL);
    PT_.alloc(off_bt, NL);
    for(DevArray *a : {&c_, &x_, &dx_, &dres_, &invdS_})
      a->alloc(Ptot_, NL);
    for(DevArray *a : {&invdX_, &invdY_, &eigD_, &eigE_, &eigD2_, &eigE2_})
      a->alloc(off_vecn, NL);
    for(DevArray *a : {&b_, &y_, &dy_, &rp_, &norms_, &invnorms_, &invdQ_})
      a->alloc(N_, NL);
    Q_.alloc((size_t)N_ * N_, NL);
    eigF_.alloc(2 * (off_vecn + 1));
    eigF2_.alloc(2 * (off_vecn + 1));
    LiQ_.alloc((size_t)N_ * N_, NL);
    qtmpv_.alloc(N_, NL);
    part_.alloc((size_t)std::max(Jl_, 1) * N_, NL);
    red_.alloc(1024, NL);
    red2_.alloc(4, NL);
    lam_.alloc(std::max(2 * Jl_, 1), NL);
    lam2_.alloc(std::max(2 * Jl_, 1), NL);
    ratio_.alloc((size_t)5 * std::max(Jl_, 1) + 1, NL);
    scal_.alloc(S_COUNT, NL);
    if constexpr(td_trsm_enabled<NL>())
      {
        // SDPB_HIP_TILEDOT=0: the float path everywhere (A/B measurements, parity comparisons)
        use_td_ = true;
        if(const char *e = std::getenv("SDPB_HIP_TILEDOT"))
          use_td_ = std::atoi(e) != 0;
        std::vector<int> off;
        size_t tiles = 0;
        for(const BlockDesc &bd : blk_)
          {
            off.push_back((int)tiles);
            const int nt = td_tiles_of(bd.P);
            tiles += nt;
            td_max_tiles_ = std::max(td_max_tiles_, nt);
          }
        use_td_ = use_td_ && tiles > 0;
        if(use_td_)
          {
            constexpr size_t WT = td::limbs<NL>();
            td_tile_off_.upload(off);
            td_img_.alloc(tiles * PB * PB * WT);
            td_sum_.alloc(tiles * PB * WT);
            td_exp_.alloc(tiles * PB);
          }
      }
    // (the buffers of the exact product Q' = P'^T P' are planned last: prepare_syrk())
    if(world_ > 1)
      acc64_.alloc(((size_t)N_ * (N_ + 1) / 2 + N_) * Syrk::ACCW);
    flags_.alloc((size_t)2 * std::max(Jl_, 1) + 4);
    flags2_.alloc((size_t)2 * std::max(Jl_, 1));
    flags3_.alloc((size_t)std::max(Jl_, 1));
    resbuf_.alloc(RES_WORDS);
    if(world_ > 1)
      xgather_.alloc(std::max(RES_WORDS, (size_t)(NL + 1) * N_) * world_);
    if(const char *e = std::getenv("SDPB_HIP_PROFILE"))
      profile_ = std::atoi(e) != 0;
    if(const char *e = std::getenv("SDPB_HIP_OVERLAP_SYRK"))
      overlap_syrk_ = std::atoi(e) != 0;
    if(const char *e = std::getenv("SDPB_HIP_TEST_SEQ_FAULT"))
      seq_fault_rank_ = std::atoi(e);
    if(const char *e = std::getenv("SDPB_HIP_QSOLVE_SUM_LANES"))
      qsolve_sum_lanes_ = std::atoi(e) != 0;
    if(const char *e = std::getenv("SDPB_HIP_TRIDIAG_WIDE"))
      tridiag_wide_ = std::atoi(e) != 0;
    {
      std::vector<int> ids;
      for(int pass = 0; pass < 2; ++pass)
        for(int q = 0; q < 2 * Jl_; ++q)
          if((h_psd_[q].rows > TRI_SMALL_N) == (pass == 0))
            ids.push_back(q);
      tri_count_large_ = 0;
      for(int q = 0; q < 2 * Jl_; ++q)
        tri_count_large_ += h_psd_[q].rows > TRI_SMALL_N;
      tri_ids_.upload(ids);
      if(const char *e = std::getenv("SDPB_HIP_TRI_T_SMALL"))
        tri_lanes_small_ = std::max(64, std::atoi(e));
      if(const char *e = std::getenv("SDPB_HIP_TRI_T_LARGE"))
        tri_lanes_large_ = std::max(64, std::atoi(e));
    }
    // opt-in (round-3 advisor): the production transport of its panel messages, ncclBroadcast, has not yet
    // run with more than one rank on hardware; the replicated factorisation uses no collective at all
    dist_cholq_ = false;
    if(const char *e = std::getenv("SDPB_HIP_DIST_CHOLQ"))
      dist_cholq_ = world_ > 1 && std::atoi(e) != 0;
    if(dist_cholq_)
      qpanel_msg_.alloc(((size_t)N_ * PB + (size_t)PB * PB + PB) * (NL + 1) + 2);
    part2_.alloc((size_t)std::max(Jl_, 1) * N_, NL);
    {
      // Chased Q' (opt-in: SDPB_HIP_Q_CHASE=1): the split column is a panel boundary and a tile boundary near the middle.
      // Built for the ranks of a multi-GPU job, where the chain of diagonal blocks of the replicated Cholesky(Q) is
      // what every rank waits for; measured (profiles/r04g_*, r04h_*): the product's workgroups hold every VGPR of their
      // SIMDs, so the chain's single workgroups wait for a workgroup of the product to retire before each of their 3 x 16
      // launches -- the wait at the join does not shrink for a rank of eight (8.5 -> 9.0 ms, step 54.2 -> 55.4 ms), and
      // on one rank the 2 ms won at the join (4.1 -> 1.9 ms) cost 0.9 ms of product time.  Not the default anywhere.
      const int panels = (int)cdiv(N_, PB), step = PB % 16 == 0 ? 1 : (PB % 8 == 0 ? 2 : (PB % 4 == 0 ? 4 : (PB % 2 == 0 ? 8 : 16)));
      bool want = false;
      if(const char *e = std::getenv("SDPB_HIP_Q_CHASE"))
        want = std::atoi(e) != 0;
      chase_hA_ = std::max(step, (panels / 2) / step * step);
      chase_cA_ = PB * chase_hA_;
      q_chase_ = want && !dist_cholq_ && !(overlap_syrk_ && world_ == 1) && chase_hA_ < panels && chase_cA_ < N_; // the same decision on every rank
    }
    // (where the chunk boundary of a chased Q' is not a tile boundary the straddling tile column is in both parts of the tile list)
    prepare_syrk();
  }
  // (re)size the buffers of the Q stage under the current budget: after everything else of this solver is allocated
  void prepare_syrk() { syrk_.prepare(Ptot_, N_, stream_, /*one_chunk=*/q_chase_, q_chase_ ? chase_cA_ : 0); }

  void set_default_params()
  {
    // Solver_Parameters.cxx:10-157
    set_param("dualityGapThreshold", "1e-30");
    set_param("primalErrorThreshold", "1e-30");
    set_param("dualErrorThreshold", "1e-30");
    set_param("initialMatrixScalePrimal", "1e20");
    set_param("initialMatrixScaleDual", "1e20");
    set_param("feasibleCenteringParameter", "0.1");
    set_param("infeasibleCenteringParameter", "0.3");
    set_param("stepLengthReduction", "0.7");
    set_param("maxComplementarity", "1e100");
    set_param("minPrimalStep", "0");
    set_param("minDualStep", "0");
  }

  // ---- batches -----------------------------------------------------------------
  Batch psd(const DevArray &a) const { return Batch{a.ptr(), d_psd_.p, 2 * Jl_}; }
  Batch vecn(const DevArray &a) const { return Batch{a.ptr(), d_vecn_.p, 2 * Jl_}; }
  Batch basesB() const { return Batch{bases_.ptr(), d_bases_.p, 2 * Jl_}; }
  Batch basesTB() const { return Batch{basesT_.ptr(), d_basesT_.p, 2 * Jl_}; }
  Batch scaledB() const { return Batch{scaled_.ptr(), d_scaled_.p, 2 * Jl_}; }
  Batch eB(const DevArray &a) const { return Batch{a.ptr(), d_E_.p, 2 * Jl_}; }
  Batch etB(const DevArray &a) const { return Batch{a.ptr(), d_Et_.p, 2 * Jl_}; }
  Batch pairB(const DevArray &a) const { return Batch{a.ptr(), d_pair_.p, 2 * Jl_}; }
  Batch schurB() const { return Batch{S_.ptr(), d_schur_.p, Jl_}; }
  Batch btB(const DevArray &a) const { return Batch{a.ptr(), d_bt_.p, Jl_}; }
  Batch vecPB(const DevArray &a) const { return Batch{a.ptr(), d_vecP_.p, Jl_}; }
  Batch QB() const { return Batch{Q_.ptr(), d_Q_.p, 1}; }
  Batch vecQB(const DevArray &a) const { return Batch{a.ptr(), d_vecQ_.p, 1}; }

  // ---- timers (names follow the reference's Scoped_Timer hierarchy, §5) -----------
  struct Timer
  {
    Solver *s;
    std::string name;
    std::chrono::steady_clock::time_point t0;
    // Stage timers synchronise the stream, so they exist only when profiling is requested
    // (SDPB_HIP_PROFILE=1 / sdpb_hip_set_profiling); the reference pays for its timers at
    // --verbosity >= 2 only.  Unprofiled iterations queue their launches ahead of the GPU.
    Timer(Solver *s_, const char *n) : s(s_)
    {
      if(!s->profile_)
        return;
      name = n;
      t0 = std::chrono::steady_clock::now();
    }
    ~Timer()
    {
      if(!s->profile_ || name.empty())
        return;
      (void)hipStreamSynchronize(s->stream_);
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if(!s->timers_ms_.count(name))
        s->timer_order_.emplace_back(name, 0.0);
      s->timers_ms_[name] += ms;
    }
  };

public:
  std::string timers_json() override
  {
    HIP_CHECK(hipStreamSynchronize(stream_));
    resolve_syrk_events();
    std::ostringstream ss;
    ss << "{";
    bool first = true;
    for(auto &kv : timer_order_)
      {
        ss << (first ? "" : ", ") << "\"" << kv.first << "\": " << timers_ms_.at(kv.first);
        first = false;
      }
    // dominant kernel: HIP-event time, launches, algorithmic bytes and limb MACs per launch
    const double fx_bytes = (double)Ptot_ * N_ * (FX + 1) * 4.0, acc_bytes = (double)N_ * (N_ + 1) / 2 * Syrk::ACCW * 4.0;
    ss << (first ? "" : ", ") << "\"kernel.k_syrk_fx.ms\": " << syrk_kernel_ms_ << ", \"kernel.k_syrk_fx.launches\": " << syrk_launches_
       << ", \"kernel.k_syrk_fx.algorithmic_bytes\": " << (fx_bytes + acc_bytes)
       << ", \"kernel.k_syrk_fx.limb_macs\": "
       << (double)Ptot_ * N_ * (N_ + 1) / 2 * FX * FX * (Syrk::SYRK_TOOM5K ? 81.0 / 256 : Syrk::SYRK_TOOM4K ? 21.0 / 64 : Syrk::SYRK_TOOM4 ? 7.0 / 16 : Syrk::SYRK_TWO_LEVEL ? 9.0 / 16 : 0.75) // executed: 81 (27 x 3 one-limb), 21 (FX/8)^2, 7 or 9 (FX/4)^2, or 3 (FX/2)^2 per product
       << ", \"kernel.k_syrk_fx.karatsuba_levels\": " << (Syrk::SYRK_TOOM4 ? 0 : Syrk::SYRK_TWO_LEVEL ? 2 : 1) << ", \"kernel.k_syrk_fx.toom4\": " << (Syrk::SYRK_TOOM4 ? 1 : 0) << ", \"kernel.k_syrk_fx.toom4k\": " << (Syrk::SYRK_TOOM4K ? 1 : 0) << ", \"kernel.k_syrk_fx.toom5k_lazy_carries\": " << (Syrk::SYRK_TOOM5K ? 1 : 0)
       << ", \"host_syncs\": " << host_syncs_ << ", \"launches\": " << launches_
       << ", \"iterations\": " << iteration_ << ", \"comm.world\": " << world_ << ", \"comm.ranks\": " << (comm_ ? comm_->ranks() : (world_ == 1 ? 1 : 0))
       << ", \"comm.owned_blocks\": " << Jl_ << ", \"comm.owned_rows\": " << Ptot_ << ", \"comm.allgather_calls\": " << xc_allgather_calls_
       << ", \"comm.allgather_bytes\": " << xc_allgather_bytes_ << ", \"comm.allreduce_calls\": " << xc_allreduce_calls_
       << ", \"comm.allreduce_bytes\": " << xc_allreduce_bytes_ << ", \"comm.broadcast_calls\": " << xc_broadcast_calls_
       << ", \"comm.broadcast_bytes\": " << xc_broadcast_bytes_ << ", \"comm.cholesky_Q\": " << (dist_cholq_ ? "\"distributed\"" : "\"replicated\"") << ", \"comm.q_chase\": " << (q_chase_ ? 1 : 0)
       << ", \"comm.collectives\": " << seq_count_.load() << ", \"comm.sequence_hash\": \"" << std::hex << seq_hash_.load() << std::dec << "\"";
    ss << "}";
    return ss.str();
  }

  // ==========================================================================
  // inputs
  // ==========================================================================
  void set_param(const std::string &n, const char *value) override
  {
    const M v = mw::from_decimal<NL>(value);
    if(n == "dualityGapThreshold") duality_gap_threshold_ = v;
    else if(n == "primalErrorThreshold") primal_error_threshold_ = v;
    else if(n == "dualErrorThreshold") dual_error_threshold_ = v;
    else if(n == "initialMatrixScalePrimal") initial_matrix_scale_primal_ = v;
    else if(n == "initialMatrixScaleDual") initial_matrix_scale_dual_ = v;
    else if(n == "feasibleCenteringParameter") feasible_centering_parameter_ = v;
    else if(n == "infeasibleCenteringParameter") infeasible_centering_parameter_ = v;
    else if(n == "stepLengthReduction") step_length_reduction_ = v;
    else if(n == "maxComplementarity") max_complementarity_ = v;
    else if(n == "minPrimalStep") min_primal_step_ = v;
    else if(n == "minDualStep") min_dual_step_ = v;
    else throw SolverError(4, "unknown parameter " + n);
  }
  void set_flags(long max_iterations, bool fpf, bool fdf, bool dpfj, bool ddfj) override
  {
    max_iterations_ = max_iterations;
    find_primal_feasible_ = fpf;
    find_dual_feasible_ = fdf;
    detect_primal_feasible_jump_ = dpfj;
    detect_dual_feasible_jump_ = ddfj;
  }

  std::vector<M> parse_list(const char *txt, size_t expect, const char *what)
  {
    std::vector<std::pair<const char *, const char *>> tok;
    split_numbers(txt, tok);
    if(tok.size() != expect)
      throw SolverError(4, std::string("wrong element count for ") + what + ": got " + std::to_string(tok.size())
                             + ", expected " + std::to_string(expect));
    std::vector<M> v(expect);
    for(size_t i = 0; i < expect; ++i)
      v[i] = mw::from_decimal<NL>(tok[i].first, tok[i].second);
    return v;
  }
  int local_index(int j) const
  {
    for(int l = 0; l < Jl_; ++l)
      if(local_[l] == j)
        return l;
    return -1;
  }

  // Text blobs in the JSON's row-major order (Json_Block_Data_Parser.hxx:26-36).
  // Blocks owned by other ranks are ignored (every rank may be fed the whole SDP).
  void set_block(int j, const char *be, const char *bo, const char *B, const char *c) override
  {
    const int l = set_block_bases(j, be, bo);
    if(l < 0)
      return;
    const BlockDesc &bd = blk_[l];
    // B[p][n] row-major is exactly B^T (N x P) column-major: element (n,p) at n + p*N
    upload<NL>(BT_, h_bt_[l].off, parse_list(B, (size_t)bd.P * N_, "B"));
    upload<NL>(c_, bd.voff, parse_list(c, bd.P, "c"));
  }
  // Same, with B (row-major P x N) and c given as doubles (exact conversion): bulk
  // synthetic inputs whose entries are dyadic rationals.
  void set_block_f64(int j, const char *be, const char *bo, const double *B, const double *c) override
  {
    const int l = set_block_bases(j, be, bo);
    if(l < 0)
      return;
    const BlockDesc &bd = blk_[l];
    std::vector<M> v((size_t)bd.P * N_);
    for(size_t i = 0; i < v.size(); ++i)
      v[i] = mw::from_double<NL>(B[i]);
    upload<NL>(BT_, h_bt_[l].off, v);
    v.resize(bd.P);
    for(int i = 0; i < bd.P; ++i)
      v[i] = mw::from_double<NL>(c[i]);
    upload<NL>(c_, bd.voff, v);
  }
  static std::vector<M> records(const uint64_t *rec, size_t count, int limbs64)
  {
    if(!rec || limbs64 < 1)
      throw SolverError(4, "mpf records: null pointer or limbs64 < 1");
    std::vector<M> v(count);
    try
      {
        for(size_t i = 0; i < count; ++i)
          v[i] = mw::from_mpf_record<NL>(rec + i * (size_t)(limbs64 + 2), limbs64);
      }
    catch(std::exception &e)
      {
        throw SolverError(4, e.what());
      }
    return v;
  }
  // Same as set_block with every number given as an mpf_t-layout record (row-major like the JSON)
  void set_block_mpf(int j, int limbs64, const uint64_t *be, const uint64_t *bo, const uint64_t *B, const uint64_t *c) override
  {
    if(j < 0 || j >= J_)
      throw SolverError(4, "set_block: block index out of range");
    const int l = local_index(j);
    if(l < 0)
      return;
    const BlockDesc &bd = blk_[l];
    const std::vector<M> e = records(be, (size_t)bd.rows[0] * bd.K, limbs64), o = records(bo, (size_t)bd.rows[1] * bd.K, limbs64);
    set_block_bases_values(l, e, o);
    upload<NL>(BT_, h_bt_[l].off, records(B, (size_t)bd.P * N_, limbs64));
    upload<NL>(c_, bd.voff, records(c, bd.P, limbs64));
  }
  void set_objective_mpf(int limbs64, const uint64_t *b, const uint64_t *constant) override
  {
    upload<NL>(b_, 0, records(b, N_, limbs64));
    objective_const_ = records(constant, 1, limbs64)[0];
  }
  int set_block_bases(int j, const char *be, const char *bo)
  {
    if(j < 0 || j >= J_)
      throw SolverError(4, "set_block: block index out of range");
    const int l = local_index(j);
    if(l < 0)
      return -1;
    const BlockDesc &bd = blk_[l];
    set_block_bases_values(l, parse_list(be, (size_t)bd.rows[0] * bd.K, "bilinear_bases"), parse_list(bo, (size_t)bd.rows[1] * bd.K, "bilinear_bases"));
    return l;
  }
  // bases given row-major (rows[b] x K) for the two parities of local block l
  void set_block_bases_values(int l, const std::vector<M> &even, const std::vector<M> &odd)
  {
    const BlockDesc &bd = blk_[l];
    const std::vector<M> *src[2] = {&even, &odd};
    for(int b = 0; b < 2; ++b)
      {
        const int rs = bd.rows[b];
        const std::vector<M> &v = *src[b];
        std::vector<M> cm((size_t)rs * bd.K);
        for(int r = 0; r < rs; ++r)
          for(int k = 0; k < bd.K; ++k)
            cm[(size_t)k * rs + r] = v[(size_t)r * bd.K + k];
        upload<NL>(bases_, h_bases_[2 * l + b].off, cm);
        upload<NL>(basesT_, h_basesT_[2 * l + b].off, v); // K x rs, sample index fastest = the row-major input
      }
    // bases_blocks (set_bases_blocks.cxx:3-22) for this block's two parities
    Batch bb = basesB(), ee = eB(E_), et = etB(Et_);
    bb.d += 2 * l;
    ee.d += 2 * l;
    et.d += 2 * l;
    bb.count = ee.count = et.count = 2;
    const size_t mx = std::max((size_t)bd.n[0] * bd.m * bd.K, (size_t)bd.n[1] * bd.m * bd.K);
    launch(k_build_bases_block<NL>, dim3(cdiv(mx, WG), 2), dim3(WG), stream_, bb, ee, et, d_blk_.p + l);
    HIP_CHECK(hipStreamSynchronize(stream_));
  }
  void set_objective(const char *b, const char *constant) override
  {
    upload<NL>(b_, 0, parse_list(b, N_, "b"));
    objective_const_ = mw::from_decimal<NL>(constant);
  }

  // SDP_Solver.cxx:23-38
  void init_state() override
  {
    LaunchScope launches_of_this_solver(&launches_);
    for(DevArray *a : {&X_, &Y_, &x_, &y_, &dx_, &dy_, &dX_, &dY_})
      HIP_CHECK(hipMemsetAsync(a->base, 0, a->bytes(), stream_));
    upload_scalar(S_ALPHA_P, initial_matrix_scale_primal_);
    upload_scalar(S_ALPHA_D, initial_matrix_scale_dual_);
    add_diagonal(X_, S_ALPHA_P);
    add_diagonal(Y_, S_ALPHA_D);
    iteration_ = 0;
    started_ = false;
    terminate_reason_ = NotTerminated;
    primal_step_length_ = mw::zero<NL>();
    dual_step_length_ = mw::zero<NL>();
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

private:
  // ==========================================================================
  // small device helpers
  // ==========================================================================
  mw::Ptr res() const { return mw::Ptr{resbuf_.p, (size_t)R_COUNT}; }
  uint32_t *xwords() const { return resbuf_.p + (size_t)(NL + 1) * R_COUNT; }
  // a host scalar travels as a kernel argument: stream ordered, no copy, no synchronisation
  void store_scalar(mw::Ptr p, size_t idx, const M &v) { launch(k_store_scalar<NL>, dim3(1), dim3(64), stream_, p, idx, v); }
  void upload_scalar(int slot, const M &v) { store_scalar(scal_.ptr(), (size_t)slot, v); }

  template <class F> void foreach(size_t count, F f)
  {
    if(!count)
      return;
    launch(k_foreach<F>, dim3(std::min<unsigned>(cdiv(count, WG), 4096)), dim3(WG), stream_, count, f);
  }
  // two-stage reduction into result slot `slot` (no synchronisation).  Empty range -> `empty`.
  template <int OP, class F> void reduce_to(int slot, size_t count, F f, const M &empty = mw::zero<NL>())
  {
    if(!count)
      {
        store_scalar(res(), (size_t)slot, empty);
        return;
      }
    const unsigned g = std::min<unsigned>(cdiv(count, WG), 512);
    launch(k_reduce<NL, OP, F>, dim3(g), dim3(WG), stream_, count, f, red_.ptr());
    mw::CPtr rp = red_.cptr();
    auto ld = [rp] __device__(size_t i) { return mw::load<NL>(rp, i); };
    launch(k_reduce<NL, OP, decltype(ld)>, dim3(1), dim3(WG), stream_, (size_t)g, ld, mw::Ptr{resbuf_.p + slot, (size_t)R_COUNT});
  }
  Comm &comm()
  {
    if(!comm_)
      throw SolverError(4, "world_size > 1 but no collectives were registered (sdpb_hip_set_collectives / sdpb_hip_rccl_init)");
    return *comm_;
  }
  // All-gather the result blocks of every rank and combine slot by slot in rank order (every rank
  // ends with identical bits, so ranks stay in lock-step).  One message per synchronisation point.
  void exchange(std::initializer_list<std::pair<int, int>> slot_ops)
  {
    if(world_ == 1)
      return;
    XOps ops;
    for(int &o : ops.op)
      o = X_KEEP;
    for(auto &so : slot_ops)
      ops.op[so.first] = so.second;
    xc_allgather_calls_ += 1;
    xc_allgather_bytes_ += (double)(RES_WORDS * sizeof(uint32_t));
    note_collective(COLL_ALLGATHER, RES_WORDS * sizeof(uint32_t), -1);
    {
      unsigned long long h = seq_hash_.load();
      if(seq_fault_rank_ == rank_)
        h ^= 1ull;
      launch(k_store_words2<0>, dim3(1), dim3(64), stream_, xwords() + XW_SEQ_LO, (uint32_t)h, (uint32_t)(h >> 32));
    }
    comm().allgather(resbuf_.p, xgather_.p, RES_WORDS * sizeof(uint32_t), stream_);
    launch(k_combine_slots<NL>, dim3(1), dim3(64), stream_, (const uint32_t *)xgather_.p, world_, (int)R_COUNT, ops, resbuf_.p);
  }
  // THE synchronisation point: one copy of the result block, then the host decides.
  void fetch(unsigned max_stage = FAIL_Q)
  {
    uint32_t h[RES_WORDS];
    HIP_CHECK(hipMemcpyAsync(h, resbuf_.p, sizeof h, hipMemcpyDeviceToHost, stream_));
    HIP_CHECK(hipStreamSynchronize(stream_));
    host_syncs_ += 1;
    prog_syncs_.store((unsigned long long)host_syncs_);
    for(int i = 0; i < R_COUNT; ++i)
      {
        const uint32_t hd = h[i];
        res_host_[i].neg = hd >> 31;
        res_host_[i].e = hd ? (int32_t)((hd & 0x7fffffffu) - mw::EBIAS) : mw::EZERO;
        for(int k = 0; k < NL; ++k)
          res_host_[i].m[k] = h[(size_t)(k + 1) * R_COUNT + i];
      }
    for(int k = 0; k < X_EXTRA; ++k)
      xw_host_[k] = h[(size_t)(NL + 1) * R_COUNT + k];
    throw_if_failed(max_stage);
  }
  // the reference's RUNTIME_ERRORs, from the smallest failure tag of all ranks
  void throw_if_failed(unsigned max_stage)
  {
    if(world_ > 1 && xw_host_[XW_SEQBAD])
      {
        // the ranks did not enqueue the same collectives: whatever was exchanged since the last agreeing
        // synchronisation point is meaningless; every rank sees the same words and raises the same error
        (void)hipStreamSynchronize(stream_q_);
        (void)hipStreamSynchronize(stream_q2_);
        q_pending_ = false;
        std::ostringstream ss;
        ss << "collective sequence mismatch: rank " << (xw_host_[XW_SEQBAD] - 1) << " and rank 0 enqueued different (kind, bytes, root) "
           << "sequences on the exchange before synchronisation point " << host_syncs_ << " of iteration " << iteration_
           << " (this rank: " << seq_count_.load() << " collectives)";
        throw HipError(3, ss.str());
      }
    const uint32_t tag = xw_host_[XW_FAIL];
    if(tag == 0xffffffffu || (tag >> 27) > max_stage)
      return;
    // leave the streams quiet before unwinding (the side streams may still be busy)
    (void)hipStreamSynchronize(stream_q_);
    (void)hipStreamSynchronize(stream_q2_);
    q_pending_ = false;
    const unsigned stage = tag >> 27, code = tag & ((1u << 27) - 1u);
    std::ostringstream ss;
    switch(stage)
      {
      case FAIL_X:
      case FAIL_Y: // cholesky_decomposition.cxx:22-25
        ss << "Error when computing Cholesky decomposition of Block_Diagonal_Matrix " << (stage == FAIL_X ? "X" : "Y")
           << ", block index = " << code / 2 << ", parity = " << code % 2 << ": A was not numerically HPD";
        break;
      case FAIL_S: // compute_Q.cxx:36-38
        ss << "Error when computing Cholesky decomposition of block_" << code << ": A was not numerically HPD";
        break;
      case FAIL_QDIAG: // compute_Q.cxx:65-91
        ss << "Normalized Q should have ones on diagonal. For i = " << code;
        break;
      default: // initialize_schur_complement_solver.cxx:95-103
        ss << "Error when computing Cholesky(Q): A was not numerically HPD";
      }
    throw SolverError(1, ss.str());
  }
  // Sum an N-vector held in a device array (stride == count) across ranks: gathered and added in
  // rank order by every rank (bit-identical results everywhere), entirely on the device.
  void allreduce_vec_sum(DevArray &a, size_t count)
  {
    if(world_ == 1)
      return;
    if(a.n != count)
      throw SolverError(4, "allreduce_vec_sum: array stride differs from the vector length");
    const size_t words = (size_t)(NL + 1) * count;
    if(xgather_.n < words * world_)
      {
        HIP_CHECK(hipDeviceSynchronize());
        xgather_.alloc(words * world_);
      }
    xc_allgather_calls_ += 1;
    xc_allgather_bytes_ += (double)(words * sizeof(uint32_t));
    note_collective(COLL_ALLGATHER, words * sizeof(uint32_t), -1);
    comm().allgather(a.base, xgather_.p, words * sizeof(uint32_t), stream_);
    launch(k_combine_vec<NL>, dim3(cdiv(count, WG)), dim3(WG), stream_, (const uint32_t *)xgather_.p, world_, (int)count, a.ptr());
  }
  // launches go to the side stream for a scope (exception safe; restores whatever was current)
  struct OnSideStream
  {
    Solver *s;
    hipStream_t prev;
    explicit OnSideStream(Solver *s_) : s(s_), prev(s_->stream_) { s->stream_ = s->stream_q_; }
    ~OnSideStream() { s->stream_ = prev; }
  };
  void resolve_syrk_events()
  {
    if(!syrk_events_pending_)
      return;
    syrk_events_pending_ = false;
    float ms = 0, ms2 = 0;
    const bool two = syrk_events2_pending_;
    syrk_events2_pending_ = false;
    if(hipEventElapsedTime(&ms, ev_syrk0_, ev_syrk1_) == hipSuccess && (!two || hipEventElapsedTime(&ms2, ev_syrk2_, ev_syrk3_) == hipSuccess))
      {
        syrk_kernel_ms_ += ms + ms2; // the two column chunks of a chased Q' count as one launch of the product
        syrk_launches_ += 1;
      }
  }

  void copy(const DevArray &src, DevArray &dst)
  {
    HIP_CHECK(hipMemcpyAsync(dst.base, src.base, src.bytes(), hipMemcpyDeviceToDevice, stream_));
  }
  // Block_Diagonal_Matrix::add_diagonal (Block_Diagonal_Matrix.hxx:63-69); c = scal_[slot]
  void add_diagonal(DevArray &A, int slot)
  {
    const MatDesc *d = d_vecn_.p;
    const MatDesc *dp = d_psd_.p;
    mw::Ptr a = A.ptr();
    mw::CPtr sc = scal_.cptr();
    const int nq = 2 * Jl_;
    // one lane per diagonal element: walk the (small) descriptor table to find the matrix
    foreach(psd_rows_local_, [=] __device__(size_t i) {
      int q = 0;
      while(q + 1 < nq && d[q + 1].off <= i)
        ++q;
      const int r = (int)(i - d[q].off);
      const size_t e = (size_t)dp[q].off + (size_t)r * (dp[q].ld + 1);
      mw::store<NL>(a, e, mw::add(mw::load<NL>(a, e), mw::load<NL>(sc, slot)));
    });
  }
  // A = (A + A^T)/2, optionally negated (Block_Diagonal_Matrix::symmetrize :95-109)
  void symmetrize(DevArray &A, bool negate)
  {
    launch(k_symmetrize<NL>, dim3(cdiv((size_t)max_n_ * max_n_, WG), 2 * Jl_), dim3(WG), stream_, psd(A), (int)negate);
  }
  // A = L L^T in place for a batch (lower factor; Li receives the inverted diagonal blocks)
  void blocked_cholesky(const Batch &A, const Batch &invd, const Batch &Li, int max_n, int *fail, hipStream_t st = nullptr,
                        unsigned long long *cyc = nullptr)
  {
    if(!st)
      st = stream_;
    const int panels = cdiv(max_n, PB);
    for(int p = 0; p < panels; ++p)
      {
        launch(k_chol_inv_lds<NL>, dim3(A.count), dim3(CI_T), st, A, invd, Li, p, fail, cyc);
        const int below = max_n - PB * (p + 1), above = PB * p;
        const int rows = std::max(below, above);
        if(rows > 0)
          launch(k_chol_panel_solve<NL>, dim3(cdiv(rows, TR), A.count), dim3(WG), st, A, Li, p, 0, cyc);
        if(below > 0)
          {
            const unsigned tiles = cdiv(below, 16);
            launch(k_chol_syrk_down<NL>, dim3(tiles * (tiles + 1) / 2, A.count), dim3(WG), st, A, p, 0, cyc, 0, std::numeric_limits<int>::max());
          }
      }
  }
  // The same factorisation of ONE matrix with a one-panel look-ahead on two streams: the
  // diagonal block p+1 (a long dependent chain on a single CU) only needs the first PB
  // rows of panel p and the leading PB x PB block of the trailing update, so those go
  // first on `st`; the rest of panel p and of the update run on `st2` while block p+1 is
  // being factored.  Entry: the work before is ordered on st; exit: everything is
  // ordered on st.
  // Panels [p0, p1) only, the trailing updates confined to the columns below col_hi (the chased Cholesky(Q): the left
  // chunk of Q is factored before the right one exists; chol_deferred_updates() then brings the right chunk up to date
  // and a second call takes the remaining panels).  Entry for p0 > 0: diagonal block p0 is up to date on st.
  void blocked_cholesky_lookahead(const Batch &A, const Batch &invd, const Batch &Li, int n, int *fail, hipStream_t st, hipStream_t st2,
                                  int p0 = 0, int p1 = -1, int col_hi = std::numeric_limits<int>::max())
  {
    const int panels = p1 < 0 ? (int)cdiv(n, PB) : p1;
    constexpr int STRIP_ROW_TILES = PB / TR, STRIP_TILES = (PB / 16) * (PB / 16 + 1) / 2;
    unsigned long long *const cyc = nullptr; // Q is not an SDP block
    launch(k_chol_inv_lds<NL>, dim3(1), dim3(CI_T), st, A, invd, Li, p0, fail, cyc);
    for(int p = p0; p < panels; ++p)
      {
        // here: diagonal block p is queued on st, and st has joined the bulk of step p-1
        const int below = n - PB * (p + 1), above = PB * p;
        const int row_tiles = cdiv(std::max(below, above), TR);
        const unsigned tiles = below > 0 ? cdiv(below, 16) : 0;
        const int ntile = (int)(tiles * (tiles + 1) / 2);
        const int strip_rows = below > 0 ? std::min(row_tiles, STRIP_ROW_TILES) : 0;
        const int strip_tiles = std::min(ntile, STRIP_TILES);
        if(strip_rows > 0) // the PB rows below the diagonal block (+ zeroing of rows [0, PB) above it)
          launch(k_chol_strip_solve<NL>, dim3(std::min(strip_rows * TR, std::max(below, above))), dim3(WG), st, A, Li, p);
        HIP_CHECK(hipEventRecord(ev_la_strip_, st));
        HIP_CHECK(hipStreamWaitEvent(st2, ev_la_strip_, 0));
        if(row_tiles > strip_rows)
          launch(k_chol_panel_solve<NL>, dim3(row_tiles - strip_rows, 1), dim3(WG), st2, A, Li, p, strip_rows, cyc);
        if(ntile > strip_tiles && PB * (p + 1) < col_hi)
          launch(k_chol_syrk_down<NL>, dim3(ntile - strip_tiles, 1), dim3(WG), st2, A, p, strip_tiles, cyc, 0, col_hi);
        HIP_CHECK(hipEventRecord(ev_la_bulk_, st2));
        // (the last panel of a range that ends before the matrix does leaves the next diagonal block to the deferred updates)
        if(strip_tiles > 0 && p + 1 < panels) // leading PB x PB block of the trailing update
          launch(k_chol_strip_update<NL>, dim3(cdiv((size_t)PB * (PB + 1) / 2, WG / (PB <= WG ? WG / PB : 1))), dim3(WG), st, A, p);
        if(p + 1 < panels)
          launch(k_chol_inv_lds<NL>, dim3(1), dim3(CI_T), st, A, invd, Li, p + 1, fail, cyc); // overlaps the bulk of step p
        HIP_CHECK(hipStreamWaitEvent(st, ev_la_bulk_, 0));
      }
  }
  // Panels [0, h) applied to the columns from col_lo = PB h on, in the order and with the kernels the look-ahead
  // factorisation itself would have used (every entry sees the same operations: the factor is bit-identical), on st2.
  void chol_deferred_updates(const Batch &A, int n, int h, hipStream_t st2)
  {
    constexpr int STRIP_TILES = (PB / 16) * (PB / 16 + 1) / 2;
    unsigned long long *const cyc = nullptr;
    const int col_lo = PB * h;
    for(int p = 0; p < h; ++p)
      {
        const int below = n - PB * (p + 1);
        const unsigned tiles = below > 0 ? cdiv(below, 16) : 0;
        const int ntile = (int)(tiles * (tiles + 1) / 2);
        const int strip_tiles = std::min(ntile, STRIP_TILES);
        if(p + 1 == h && strip_tiles > 0)
          launch(k_chol_strip_update<NL>, dim3(cdiv((size_t)PB * (PB + 1) / 2, WG / (PB <= WG ? WG / PB : 1))), dim3(WG), st2, A, p);
        if(ntile > strip_tiles)
          launch(k_chol_syrk_down<NL>, dim3(ntile - strip_tiles, 1), dim3(WG), st2, A, p, strip_tiles, cyc, col_lo, std::numeric_limits<int>::max());
      }
  }
  // X := X L^{-T} (rows of X are the right-hand sides)
  // src: an array with X's layout that holds the right-hand sides (nullptr: X itself, the solve in place)
  void trsm_rlt(const Batch &L, const Batch &Li, const Batch &X, int max_rows, int max_n, unsigned long long *cyc = nullptr,
                const DevArray *src = nullptr)
  {
    const mw::CPtr s = src ? src->cptr() : mw::CPtr(X.p.base, X.p.stride);
    for(int p = 0; p < (int)cdiv(max_n, PB); ++p)
      launch(k_trsm_rlt_panel<NL>, dim3(cdiv(max_rows, TR), X.count), dim3(WG), stream_, L, Li, X, s, p, cyc);
  }
  // the same for the Schur blocks (P = L^{-1} B): trailing updates as fixed-point tile dot products where the build has them
  void trsm_rlt_schur(const Batch &L, const Batch &Li, const Batch &X, int max_rows, int max_n, unsigned long long *cyc, const DevArray *src)
  {
    if constexpr(td_trsm_enabled<NL>())
      if(use_td_)
        {
          const mw::CPtr s = src ? src->cptr() : mw::CPtr(X.p.base, X.p.stride);
          launch(k_td_image_L<NL>, dim3(td_max_tiles_, X.count), dim3(WG), stream_, L, Li, (const int *)td_tile_off_.p, td_img_.p, td_exp_.p, td_sum_.p);
          for(int p = 0; p < (int)cdiv(max_n, PB); ++p)
            launch(k_trsm_rlt_panel_td<NL>, dim3(cdiv(max_rows, TR), X.count), dim3(WG), stream_, L, Li, X, s, p, cyc, (const int *)td_tile_off_.p,
                   (const uint32_t *)td_img_.p, (const int32_t *)td_exp_.p, (const uint32_t *)td_sum_.p);
          return;
        }
    trsm_rlt(L, Li, X, max_rows, max_n, cyc, src);
  }
  // X := X L^{-1}
  void trsm_rln(const Batch &L, const Batch &Li, const Batch &X, int max_rows, int max_n)
  {
    for(int p = (int)cdiv(max_n, PB) - 1; p >= 0; --p)
      launch(k_trsm_rln_panel<NL>, dim3(cdiv(max_rows, TR), X.count), dim3(WG), stream_, L, Li, X, p);
  }

  // C = (+/-) A B (+ C) on the PSD-shaped batch; sub != nullptr fuses "- sub"; trans_out
  // stores the transpose
  void gemm_psd(const DevArray &A, const DevArray &B, DevArray &C, bool alpha_neg, bool beta_one, const DevArray *sub = nullptr,
                bool trans_out = false)
  {
    const unsigned tiles = cdiv(max_n_, 16) * cdiv(max_n_, 16);
    launch(k_gemm<NL, false, false>, dim3(tiles, 2 * Jl_), dim3(WG), stream_, psd(A), psd(B), psd(C), (int)alpha_neg, (int)beta_one, 0,
           psd(sub ? *sub : C), sub ? 1 : 0, (int)trans_out);
  }
  // cholesky_solve.cxx:4-13 on a transposed operand: At := At Xc^{-T} Xc^{-1}, i.e.
  // (Xc^{-T} Xc^{-1} A)^T; one lane per row, every load coalesced
  void cholesky_solve_X_transposed(DevArray &At)
  {
    trsm_rlt(psd(Xc_), psd(LiX_), psd(At), max_n_, max_n_);
    trsm_rln(psd(Xc_), psd(LiX_), psd(At), max_n_, max_n_);
  }

  // ==========================================================================
  // the iteration
  // ==========================================================================
  // compute_objectives.cxx:6-29, dot.cxx:4-22: the two dot products (combined on the host after fetch())
  void queue_objectives()
  {
    Timer t(this, "objectives");
    mw::CPtr c = c_.cptr(), x = x_.cptr(), b = b_.cptr(), y = y_.cptr();
    reduce_to<RED_SUM>(R_CX, Ptot_, [=] __device__(size_t i) { return mw::mul(mw::load<NL>(c, i), mw::load<NL>(x, i)); });
    reduce_to<RED_SUM>(R_BY, (size_t)N_, [=] __device__(size_t i) { return mw::mul(mw::load<NL>(b, i), mw::load<NL>(y, i)); });
  }

  // compute_bilinear_pairings.cxx:17-31
  void compute_bilinear_pairings()
  {
    Timer t(this, "bilinear_pairings");
    compute_A_X_inv();
    // A_Y and the factor of Y were queued on the side stream by factor_X_and_Y()
    HIP_CHECK(hipStreamWaitEvent(stream_, ev_q_done_, 0));
    if(Jl_)
      launch(k_fail_tags<0>, dim3(cdiv(2 * Jl_, WG)), dim3(WG), stream_, (const int *)flags2_.p, 2 * Jl_, (unsigned)FAIL_Y, 2, d_blk_.p, xwords() + XW_FAIL);
  }
  // A_X_inv = (Xc^{-1} E)^T (Xc^{-1} E)      compute_A_X_inv.cxx:18-29
  // computed on the transpose: Tt = E^T Xc^{-T} (row solves), A_X_inv = Tt Tt^T
  void compute_A_X_inv()
  {
    const unsigned tiles_q = cdiv(max_q_, 16) * cdiv(max_q_, 16);
    copy(Et_, T_);
    trsm_rlt(psd(Xc_), psd(LiX_), etB(T_), max_q_, max_n_);
    launch(k_gemm<NL, false, true>, dim3(tiles_q, 2 * Jl_), dim3(WG), stream_, etB(T_), etB(T_), pairB(AX_), 0, 0, 1, pairB(AX_), 0, 0);
  }
  // A_Y = E^T (Y E)                           compute_A_Y.cxx:30-45
  void compute_A_Y()
  {
    const unsigned tiles_q = cdiv(max_q_, 16) * cdiv(max_q_, 16);
    launch(k_gemm<NL, false, false>, dim3(cdiv(max_n_, 16) * cdiv(max_q_, 16), 2 * Jl_), dim3(WG), stream_, psd(Y_), eB(E_), eB(YQ_), 0, 0,
           0, eB(YQ_), 0, 0);
    // E^T comes from the stored transpose: lanes of a tile then read consecutive rows of Et (coalesced)
    // instead of 16 columns of E a row stride apart, whose 19 limb planes overflow the CU's L1
    // (3.6 ms -> the same products, same order, same bits).
    launch(k_gemm<NL, false, false>, dim3(tiles_q, 2 * Jl_), dim3(WG), stream_, etB(Et_), eB(YQ_), pairB(AY_), 0, 0, 1, pairB(AY_), 0, 0);
  }
  // cholesky_decomposition.cxx:5-28 for X and Y (run.cxx:386-387).  The factor of a batch of
  // small matrices is a latency-bound chain of pivots, so Y's factor and A_Y (which needs
  // only Y) go to the side stream while X's factor and A_X_inv run on the main stream.  A
  // failed factorisation is recorded as a failure tag and raised at the next fetch().
  void factor_X_and_Y()
  {
    Timer t(this, "choleskyDecomposition");
    HIP_CHECK(hipMemsetAsync(flags_.p, 0, flags_.n * sizeof(int), stream_));
    HIP_CHECK(hipMemsetAsync(flags2_.p, 0, flags2_.n * sizeof(int), stream_));
    HIP_CHECK(hipMemsetAsync(flags3_.p, 0, flags3_.n * sizeof(int), stream_));
    HIP_CHECK(hipEventRecord(ev_q_ready_, stream_));
    HIP_CHECK(hipStreamWaitEvent(stream_q_, ev_q_ready_, 0));
    {
      OnSideStream side(this);
      copy(Y_, Yc_);
      blocked_cholesky(psd(Yc_), vecn(invdY_), psd(LiY_), max_n_, flags2_.p);
      compute_A_Y();
      HIP_CHECK(hipEventRecord(ev_q_done_, stream_));
    }
    copy(X_, Xc_);
    blocked_cholesky(psd(Xc_), vecn(invdX_), psd(LiX_), max_n_, flags_.p);
    if(Jl_)
      launch(k_fail_tags<0>, dim3(cdiv(2 * Jl_, WG)), dim3(WG), stream_, (const int *)flags_.p, 2 * Jl_, (unsigned)FAIL_X, 2, d_blk_.p, xwords() + XW_FAIL);
  }

  void max_abs_to(int slot, const DevArray &a, size_t count)
  {
    mw::CPtr p = a.cptr();
    reduce_to<RED_MAX>(slot, count, [=] __device__(size_t i) { return mw::abs(mw::load<NL>(p, i)); });
  }

  // compute_dual_residues_and_error.cxx:7-66
  void compute_dual_residues_and_error()
  {
    Timer t(this, "computeDualResidues");
    launch(k_dual_residues<NL>, dim3(cdiv(max_P_, WG), Jl_), dim3(WG), stream_, pairB(AY_), c_.cptr(), dres_.ptr(), d_blk_.p);
    launch(k_gemv_n<NL>, dim3(cdiv(max_P_, 4), Jl_), dim3(WG), stream_, btB(BT_), y_.cptr(), dres_.ptr(), d_blk_.p, N_, -1);
    max_abs_to(R_DERR, dres_, Ptot_);
  }
  // constraint_matrix_weighted_sum.cxx:14-66 (+ the add/subtract that follows it)
  void constraint_matrix_weighted_sum(const DevArray &a, DevArray &out, const DevArray &addend, int sign)
  {
    // scaled_ is scratch shared by the calls: they are all queued on the main stream, in order
    launch(k_scale_bases<NL>, dim3(cdiv(max_scaled_, WG), 2 * Jl_), dim3(WG), stream_, basesB(), a.cptr(), scaledB(), d_blk_.p);
    launch(k_constraint_weighted_sum<NL>, dim3(cdiv((size_t)max_n_ * max_n_, WG), 2 * Jl_), dim3(WG), stream_, basesB(), scaledB(),
           psd(out), psd(addend), sign, d_blk_.p);
  }
  // compute_primal_residues_and_error_P_Ax_X.cxx:5-14
  void compute_primal_residues_P()
  {
    Timer t(this, "computePrimalResidues");
    constraint_matrix_weighted_sum(x_, PR_, X_, -1);
    max_abs_to(R_PERR_P, PR_, psd_elems_);
  }
  // out[n] = base[n] + sign * sum_blocks (M_j^T v_j)[n], summed over all ranks
  template <bool SQUARE> void gemv_t_all(const DevArray &MT, const DevArray &v, const DevArray *base, int sign, DevArray &out)
  {
    gemv_t_all<SQUARE>(MT, v, base, sign, out, part_);
  }
  template <bool SQUARE>
  void gemv_t_all(const DevArray &MT, const DevArray &v, const DevArray *base, int sign, DevArray &out, DevArray &part)
  {
    launch(k_gemv_t_partial<NL, SQUARE>, dim3(cdiv(N_, WG), Jl_), dim3(WG), stream_, btB(MT), v.cptr(), part.ptr(), d_blk_.p, N_);
    if(world_ == 1)
      {
        launch(k_sum_partials<NL>, dim3(cdiv(N_, SP_ROWS)), dim3(WG), stream_, part.cptr(), Jl_, N_, base ? base->cptr() : out.cptr(),
               base ? 1 : 0, sign, out.ptr());
        return;
      }
    // local sum, cross-rank sum, then base + sign*sum
    launch(k_sum_partials<NL>, dim3(cdiv(N_, SP_ROWS)), dim3(WG), stream_, part.cptr(), Jl_, N_, out.cptr(), 0, 1, out.ptr());
    allreduce_vec_sum(out, N_);
    launch(k_base_plus_signed<NL>, dim3(cdiv(N_, WG)), dim3(WG), stream_, out.ptr(), base ? base->cptr() : out.cptr(), base ? 1 : 0, sign, N_);
  }
  // compute_primal_residues_and_error_p_b_Bx.cxx:9-86
  void compute_primal_residue_p()
  {
    Timer t(this, "computePrimalResidue_p");
    gemv_t_all<false>(BT_, x_, &b_, -1, rp_);
    max_abs_to(R_PERR_p, rp_, N_);
  }

  // compute_feasible_and_termination.cxx:4-71; `time_up` is rank 0's wall-clock test
  // (":66-69 Time varies between cores, so follow the decision of the root")
  bool compute_feasible_and_termination(bool &feasible, bool time_up)
  {
    const M perr = mw::max(primal_error_P_, primal_error_p_);
    const bool dualf = mw::lt(dual_error_, dual_error_threshold_), primf = mw::lt(perr, primal_error_threshold_);
    feasible = primf && dualf;
    const bool optimal = mw::lt(duality_gap_, duality_gap_threshold_);
    const M one = mw::from_u32<NL>(1);
    if(feasible && optimal)
      terminate_reason_ = PrimalDualOptimal;
    else if(dualf && find_dual_feasible_)
      terminate_reason_ = DualFeasible;
    else if(primf && find_primal_feasible_)
      terminate_reason_ = PrimalFeasible;
    else if(mw::cmp(dual_step_length_, one) == 0 && detect_dual_feasible_jump_)
      terminate_reason_ = DualFeasibleJumpDetected;
    else if(mw::cmp(primal_step_length_, one) == 0 && detect_primal_feasible_jump_)
      terminate_reason_ = PrimalFeasibleJumpDetected;
    else if(iteration_ > max_iterations_)
      terminate_reason_ = MaxIterationsExceeded;
    else if(time_up)
      terminate_reason_ = MaxRuntimeExceeded;
    else if(iteration_ > 1 && mw::lt(primal_step_length_, min_primal_step_))
      terminate_reason_ = PrimalStepTooSmall;
    else if(iteration_ > 1 && mw::lt(dual_step_length_, min_dual_step_))
      terminate_reason_ = DualStepTooSmall;
    else
      return false;
    return true;
  }

  // initialize_schur_complement_solver.cxx:62-104
  void initialize_schur_complement_solver()
  {
    {
      Timer t(this, "initializeSchurComplementSolver.schur_complement");
      const unsigned strips = cdiv((size_t)max_P_ * (max_P_ + 1) / 2, WG); // lower triangle, packed
      launch(k_schur_complement<NL>, dim3(8 * cdiv(Jl_, 8) * strips), dim3(WG), stream_, pairB(AX_), pairB(AY_), schurB(), d_blk_.p,
             (int)strips);
    }
    {
      // compute_Q.cxx:9-61 : L = chol(S) in place, P^T = B^T L^{-T}
      Timer t(this, "initializeSchurComplementSolver.Q.cholesky");
      blocked_cholesky(schurB(), vecPB(invdS_), Batch{LiS_.ptr(), d_schur_.p, Jl_}, max_P_, flags3_.p, nullptr, block_clock(0));
      if(Jl_)
        launch(k_fail_tags<0>, dim3(cdiv(Jl_, WG)), dim3(WG), stream_, (const int *)flags3_.p, Jl_, (unsigned)FAIL_S, 1, d_blk_.p, xwords() + XW_FAIL);
    }
    {
      Timer t(this, "initializeSchurComplementSolver.Q.solve");
      trsm_rlt_schur(schurB(), Batch{LiS_.ptr(), d_schur_.p, Jl_}, btB(PT_), N_, max_P_, block_clock(1), &BT_); // reads B, writes P
    }
    // Optional (off, see overlap_syrk_): with one rank the whole Q chain — norms, fixed-point image,
    // syrk, restore, Cholesky(Q) — can run on the side stream while the main stream goes on to the
    // Q-independent part of the predictor (R, Z, the Schur right-hand side, L^{-1} dx, P^T dx).
    // (With several ranks the chain contains collectives, which stay ordered on the one stream the
    // communicator is used from.)
    const bool side = overlap_syrk_ && world_ == 1;
    if(side)
      {
        HIP_CHECK(hipEventRecord(ev_q_ready_, stream_));
        HIP_CHECK(hipStreamWaitEvent(stream_q_, ev_q_ready_, 0));
      }
    {
      std::unique_ptr<OnSideStream> on_side;
      if(side)
        on_side.reset(new OnSideStream(this));
      // syrk_Q, compute_Q.cxx:94-132
      Timer t(this, "initializeSchurComplementSolver.Q.syrk");
      gemv_t_all<true>(PT_, x_, nullptr, 1, norms_, side ? part2_ : part_); // norms_ = column norms^2 (Matrix_Normalizer.cxx:75-137)
      norms_to_inverse(norms_.ptr(), invnorms_.ptr(), (size_t)N_);
      const size_t cnt = Ptot_ * (size_t)N_;
      // image of the rows [r0, r0 + rows) of P' (one input window; all rows unless the window is split: q_window())
      auto make_image = [&](size_t r0, unsigned rows) {
        const size_t n = (size_t)rows * N_;
        launch(k_normalize_fx<NL, FX>, dim3(cdiv(n, WG)), dim3(WG), stream_, mw::offset(PT_.cptr(), r0 * (size_t)N_), n, N_, // one element per lane: streams at HBM rate
               invnorms_.cptr(), syrk_.image.p, syrk_.win.stride);
      };
      uint32_t *const acc = syrk_.acc.p;
      const size_t acc_stride = syrk_.acc_stride, acc_bytes = syrk_.acc.n * sizeof(uint32_t);
      if(cnt && q_chase_)
        make_image(0, (unsigned)Ptot_);
      int *qflags = flags_.p + 2 * std::max(Jl_, 1);
      HIP_CHECK(hipMemsetAsync(qflags, 0, 4 * sizeof(int), stream_));
      // unbias + un-normalise the columns [c0, c1) of the lower triangle into Q (check of the diagonal included)
      auto finish_Q_columns = [&](int c0, int c1) {
        const size_t idx0 = (size_t)c0 * N_, idx1 = (size_t)c1 * N_;
        launch(k_syrk_unbias<FX>, dim3(cdiv(idx1 - idx0, WG)), dim3(WG), stream_, acc, acc_stride, N_, Ptot_global_, idx0, idx1);
        launch(k_restore_Q<NL, FX>, dim3(cdiv(idx1 - idx0, WG)), dim3(WG), stream_, (const uint32_t *)acc, acc_stride, N_, norms_.cptr(),
               Q_.ptr(), qflags + 1, idx0, idx1);
      };
      if(q_chase_)
        {
          // Q' in two column chunks with Cholesky(Q) chasing it: while the main stream multiplies (and, with several
          // ranks, reduces) the right chunk, the side streams factor the panels of the left one -- half of the chain
          // of diagonal blocks, the part of Cholesky(Q) that no number of GPUs shortens, moves behind the product.
          // Every rank issues the same collectives in the same order (two all-reduces instead of one).
          const int cA = chase_cA_;
          if(cnt)
            {
              syrk_.column_sums(stream_);
              resolve_syrk_events();
              HIP_CHECK(hipEventRecord(ev_syrk0_, stream_));
              syrk_.G(stream_, syrk_.left());
              HIP_CHECK(hipEventRecord(ev_syrk1_, stream_));
            }
          else
            HIP_CHECK(hipMemsetAsync(acc, 0, acc_bytes, stream_));
          if(world_ > 1)
            reduce_Q_accumulators(0, cA, true);
          finish_Q_columns(0, cA);
          cholesky_Q_chase_left();
          if(cnt)
            {
              HIP_CHECK(hipEventRecord(ev_syrk2_, stream_));
              syrk_.G(stream_, syrk_.right());
              HIP_CHECK(hipEventRecord(ev_syrk3_, stream_));
              syrk_events_pending_ = syrk_events2_pending_ = true;
            }
          if(world_ > 1)
            reduce_Q_accumulators(cA, N_, false);
          finish_Q_columns(cA, N_);
          cholesky_Q_chase_right();
          return;
        }
      if(cnt)
        {
          // HIP events on the launch stream bracket the dominant kernel (bench.py roofline); they are
          // read back lazily, after a later synchronisation point has passed them.  (With the image in several
          // input windows they also span the images and column sums of the windows after the first.)
          syrk_.G_windows(stream_, make_image, [&] {
            resolve_syrk_events();
            HIP_CHECK(hipEventRecord(ev_syrk0_, stream_));
          });
          HIP_CHECK(hipEventRecord(ev_syrk1_, stream_));
          syrk_events_pending_ = true;
        }
      else
        HIP_CHECK(hipMemsetAsync(acc, 0, acc_bytes, stream_));
      if(world_ > 1)
        reduce_Q_accumulators();
      finish_Q_columns(0, N_);
      if(side)
        {
          // Cholesky(Q) follows on the same (side) stream, look-ahead bulk on the third one
          blocked_cholesky_lookahead(QB(), vecQB(invdQ_), Batch{LiQ_.ptr(), d_Q_.p, 1}, N_, qflags, stream_, stream_q2_);
          HIP_CHECK(hipEventRecord(ev_q_done_, stream_));
          q_pending_ = true;
        }
    }
    if(dist_cholq_)
      cholesky_Q_distributed();
    else if(!side)
      cholesky_Q_async();
  }
  unsigned long long *block_clock(int stage)
  {
    if(!profile_ || !Jl_)
      return nullptr;
    if(blk_cycles_.n < (size_t)2 * Jl_)
      {
        blk_cycles_.alloc((size_t)2 * Jl_);
        HIP_CHECK(hipMemsetAsync(blk_cycles_.p, 0, blk_cycles_.n * sizeof(unsigned long long), stream_));
      }
    return blk_cycles_.p + (size_t)stage * Jl_;
  }
  // norms^2 -> norms (in place) and 1/norm (Matrix_Normalizer.cxx:133-136); a zero column keeps 0
  void norms_to_inverse(mw::Ptr nr, mw::Ptr inv, size_t n)
  {
    foreach(n, [=] __device__(size_t i) {
      const M n2 = mw::load<NL>(nr, i);
      if(mw::is_zero(n2))
        {
          mw::store<NL>(inv, i, n2);
          return;
        }
      const M r = mw::rsqrt(n2);
      M s = mw::mul(n2, r);
      s = mw::add(s, mw::mul_2exp(mw::mul(r, mw::sub(n2, mw::mul(s, s))), -1));
      mw::store<NL>(nr, i, s);
      mw::store<NL>(inv, i, mw::mul(r, mw::sub(mw::from_u32<NL>(2), mw::mul(s, r))));
    });
  }
  // exact cross-GPU sum of the fixed-point Q' images
  void reduce_Q_accumulators(int c0 = 0, int c1 = -1, bool with_sums = true)
  {
    // lower triangle of the columns [c0, c1) (+ the N column sums): entries x ACCW planes of 64-bit lanes
    if(c1 < 0)
      c1 = N_;
    const size_t T = tri_packed_offset(N_, c1) - tri_packed_offset(N_, c0) + (with_sums ? (size_t)N_ : 0);
    const dim3 grid(cdiv(N_, WG), c1 - c0 + (with_sums ? 1 : 0));
    launch(k_widen_tri_u64<0>, grid, dim3(WG), stream_, (const uint32_t *)syrk_.acc.p, syrk_.acc_stride, N_, (int)Syrk::ACCW, acc64_.p, c0, c1, (int)with_sums);
    xc_allreduce_calls_ += 1;
    xc_allreduce_bytes_ += (double)(T * Syrk::ACCW * 8);
    note_collective(COLL_ALLREDUCE, T * Syrk::ACCW * 8, -1);
    comm().allreduce_sum_u64(acc64_.p, T * Syrk::ACCW, stream_);
    launch(k_narrow_tri_carry<0>, grid, dim3(WG), stream_, (const unsigned long long *)acc64_.p, N_, (int)Syrk::ACCW, syrk_.acc.p, syrk_.acc_stride, c0, c1,
           (int)with_sums);
  }
  // in-place broadcast on the main stream through whatever the exchange runs on
  void xbroadcast(uint32_t *buf, size_t words, int root)
  {
    const size_t bytes = words * sizeof(uint32_t);
    xc_broadcast_calls_ += 1;
    xc_broadcast_bytes_ += (double)bytes;
    note_collective(COLL_BROADCAST, bytes, root);
    if(comm().broadcast(buf, bytes, root, stream_))
      return;
    if(qpanel_gather_.n < words * world_)
      {
        HIP_CHECK(hipStreamSynchronize(stream_));
        qpanel_gather_.alloc(words * world_);
      }
    comm().allgather(buf, qpanel_gather_.p, bytes, stream_);
    if(root != rank_)
      HIP_CHECK(hipMemcpyAsync(buf, qpanel_gather_.p + (size_t)root * words, bytes, hipMemcpyDeviceToDevice, stream_));
  }
  // Cholesky(Q) over all ranks (the reference factors Q over COMM_WORLD too, initialize_schur_complement_solver.cxx:
  // 95-103): column panel p belongs to rank p % world.  Step p: the owner factors and inverts the diagonal block,
  // solves the rows below it and broadcasts the finished panel (with the inverted block and its failure flag);
  // every rank then applies the panel to the column panels IT owns.  Each rank ends with the whole factor (it
  // received every panel), so the Q solves stay as they are.  The N^3/3 trailing updates divide by the number of
  // ranks; the chain of diagonal blocks does not.
  //
  // One-panel look-ahead on two side streams (round 4; the shape of blocked_cholesky_lookahead):
  //   chain stream S (stream_q_):  broadcast(p) -> unpack(p) -> [owner of p+1: update panel p+1 with panel p,
  //                                factor + invert its diagonal block, solve its rows, pack(p+1)] -> broadcast(p+1) ...
  //   bulk stream B (stream_q2_):  wait panel p -> update the other owned panels q > p with panel p
  // so the diagonal block of panel p+1 (a dependent chain on one CU) is factored while this rank's bulk of step p
  // runs, and the main stream goes on with the residues and the Q-independent part of the predictor until
  // join_cholesky_Q().  Panel p+1 at step p needs the updates of panels < p, which ran on B: S waits for B's
  // event of step p-1.  Every panel is computed by its owner only, so all ranks hold identical bits.  The
  // broadcasts are issued from S; the host issues every collective of the iteration in the same program order on
  // every rank, which is what the one communicator requires (RCCL orders its kernels in issue order across the
  // streams it is used from; the callback transport synchronises S and calls the host collective at once).
  void cholesky_Q_distributed()
  {
    int *qflags = flags_.p + 2 * std::max(Jl_, 1);
    const Batch A = QB(), invd = vecQB(invdQ_), Li{LiQ_.ptr(), d_Q_.p, 1};
    const int panels = cdiv(N_, PB);
    constexpr int TPP = PB >= 16 ? PB / 16 : 1;
    hipStream_t S = stream_q_, B = stream_q2_;
    HIP_CHECK(hipEventRecord(ev_q_ready_, stream_));
    HIP_CHECK(hipStreamWaitEvent(S, ev_q_ready_, 0));
    HIP_CHECK(hipStreamWaitEvent(B, ev_q_ready_, 0));
    auto factor_and_pack = [&](int p) { // the owner's part of panel p, on S
      const int k0 = PB * p, nb = std::min(PB, N_ - k0), rows = N_ - k0;
      const size_t cnt = (size_t)rows * nb + (size_t)nb * nb + nb;
      launch(k_chol_inv_lds<NL>, dim3(1), dim3(CI_T), S, A, invd, Li, p, qflags, (unsigned long long *)nullptr);
      const int below = N_ - PB * (p + 1), above = PB * p;
      if(std::max(below, above) > 0)
        launch(k_chol_panel_solve<NL>, dim3(cdiv(std::max(below, above), TR), 1), dim3(WG), S, A, Li, p, 0, (unsigned long long *)nullptr);
      launch(k_qpanel_pack<NL>, dim3(cdiv(cnt, WG)), dim3(WG), S, A, Li, invd, p, (const int *)qflags, qpanel_msg_.p);
    };
    if(rank_ == 0)
      factor_and_pack(0);
    for(int p = 0; p < panels; ++p)
      {
        const int owner = p % world_, k0 = PB * p, nb = std::min(PB, N_ - k0), rows = N_ - k0;
        const size_t cnt = (size_t)rows * nb + (size_t)nb * nb + nb, words = cnt * (NL + 1) + 1;
        {
          OnSideStream on_chain(this); // stream_ = S for the message
          xbroadcast(qpanel_msg_.p, words, owner);
        }
        if(owner != rank_)
          launch(k_qpanel_unpack<NL>, dim3(cdiv(std::max(cnt, (size_t)k0 * nb), WG)), dim3(WG), S, A, Li, invd, p, qflags, (const uint32_t *)qpanel_msg_.p);
        HIP_CHECK(hipEventRecord(ev_la_strip_, S)); // panel p is in place on this rank
        const int Mrows = N_ - (k0 + nb);
        const bool own_next = p + 1 < panels && (p + 1) % world_ == rank_;
        if(own_next)
          {
            if(p >= 1)
              HIP_CHECK(hipStreamWaitEvent(S, ev_la_bulk_, 0)); // panels < p have been applied to panel p+1 (on B)
            launch(k_chol_syrk_cols<NL>, dim3(cdiv(Mrows, 16), TPP), dim3(WG), S, A, p, p + 1, world_, 1);
            factor_and_pack(p + 1);
          }
        HIP_CHECK(hipStreamWaitEvent(B, ev_la_strip_, 0));
        // the other owned panels q > p: q = rank (mod world)
        int q0 = p + 1;
        while(q0 % world_ != rank_)
          ++q0;
        if(own_next)
          q0 += world_;
        if(q0 < panels)
          {
            const int count = (panels - 1 - q0) / world_ + 1;
            launch(k_chol_syrk_cols<NL>, dim3(cdiv(Mrows, 16), count * TPP), dim3(WG), B, A, p, q0, world_, count);
          }
        HIP_CHECK(hipEventRecord(ev_la_bulk_, B));
      }
    // B has waited for the last panel on S and S queues nothing after it: B's tail orders the whole factor
    HIP_CHECK(hipEventRecord(ev_q_done_, B));
    q_pending_ = true;
  }
  // El::Cholesky(UPPER,Q) (initialize_schur_complement_solver.cxx:95-103), stored here
  // as the lower factor L = U^T (blocked, see kernels.hpp).  The factorisation is a long
  // dependent chain that occupies a handful of CUs, so it runs on its own stream while
  // the main stream goes on with -XY, mu, R-error and the part of the predictor that does
  // not need Q (R, Z, the Schur right-hand side, L^{-1} dx, P^T dx); join_cholesky_Q()
  // joins before the first Q solve.
  // The chased Cholesky(Q), first half: panels [0, chase_hA_) of the left chunk on the side streams (the main stream
  // goes on with the right chunk of Q').  Second half: the left panels applied to the right chunk, then the rest.
  void cholesky_Q_chase_left()
  {
    int *qflags = flags_.p + 2 * std::max(Jl_, 1);
    HIP_CHECK(hipEventRecord(ev_q_ready_, stream_));
    HIP_CHECK(hipStreamWaitEvent(stream_q_, ev_q_ready_, 0));
    blocked_cholesky_lookahead(QB(), vecQB(invdQ_), Batch{LiQ_.ptr(), d_Q_.p, 1}, N_, qflags, stream_q_, stream_q2_, 0, chase_hA_, chase_cA_);
  }
  void cholesky_Q_chase_right()
  {
    int *qflags = flags_.p + 2 * std::max(Jl_, 1);
    HIP_CHECK(hipEventRecord(ev_chunk_, stream_)); // the right chunk of Q is in place
    HIP_CHECK(hipStreamWaitEvent(stream_q2_, ev_chunk_, 0));
    chol_deferred_updates(QB(), N_, chase_hA_, stream_q2_); // in order behind the left half's own bulk updates
    HIP_CHECK(hipEventRecord(ev_la_bulk_, stream_q2_));
    HIP_CHECK(hipStreamWaitEvent(stream_q_, ev_la_bulk_, 0));
    blocked_cholesky_lookahead(QB(), vecQB(invdQ_), Batch{LiQ_.ptr(), d_Q_.p, 1}, N_, qflags, stream_q_, stream_q2_, chase_hA_);
    HIP_CHECK(hipEventRecord(ev_q_done_, stream_q_));
    q_pending_ = true;
    if(stream_beside_ && !beside_active_)
      {
        HIP_CHECK(hipEventRecord(ev_beside_, stream_));
        HIP_CHECK(hipStreamWaitEvent(stream_beside_, ev_beside_, 0));
        stream_ = stream_beside_;
        beside_active_ = true;
      }
  }
  void cholesky_Q_async()
  {
    int *qflags = flags_.p + 2 * std::max(Jl_, 1);
    HIP_CHECK(hipEventRecord(ev_q_ready_, stream_));
    HIP_CHECK(hipStreamWaitEvent(stream_q_, ev_q_ready_, 0));
    blocked_cholesky_lookahead(QB(), vecQB(invdQ_), Batch{LiQ_.ptr(), d_Q_.p, 1}, N_, qflags, stream_q_, stream_q2_);
    HIP_CHECK(hipEventRecord(ev_q_done_, stream_q_));
    q_pending_ = true;
    if(stream_beside_ && !beside_active_)
      {
        HIP_CHECK(hipEventRecord(ev_beside_, stream_));
        HIP_CHECK(hipStreamWaitEvent(stream_beside_, ev_beside_, 0));
        stream_ = stream_beside_;
        beside_active_ = true;
      }
  }
  // back to the unmasked main stream, ordered after what the masked one was given (no-throw: also
  // called from the destructor and at the start of an iteration that follows an exception)
  void leave_beside_stream() noexcept
  {
    if(!beside_active_)
      return;
    (void)hipEventRecord(ev_beside_, stream_beside_);
    stream_ = stream_main_;
    (void)hipStreamWaitEvent(stream_main_, ev_beside_, 0);
    beside_active_ = false;
  }
  // the main stream waits for the factor of Q (device-side); failures become tags
  void join_cholesky_Q()
  {
    leave_beside_stream();
    if(!q_pending_)
      return;
    q_pending_ = false;
    Timer t(this, "initializeSchurComplementSolver.Cholesky_Q(join)");
    HIP_CHECK(hipStreamWaitEvent(stream_, ev_q_done_, 0));
    launch(k_fail_tags_q<0>, dim3(1), dim3(64), stream_, (const int *)(flags_.p + 2 * std::max(Jl_, 1)), xwords() + XW_FAIL);
  }

  // solve_schur_complement_equation.cxx:16-79
  void solve_schur_complement_equation()
  {
    {
      Timer t(this, "searchDirection.solve.dx_Linv");
      // dx := L^{-1} dx, one workgroup per block runs all panels (k_vec_trsm)
      launch(k_vec_trsm<NL, false>, dim3(Jl_), dim3(WG), stream_, schurB(), Batch{LiS_.ptr(), d_schur_.p, Jl_}, Batch{dx_.ptr(), d_rowP_.p, Jl_});
    }
    {
      Timer t(this, "searchDirection.solve.dy_PTdx");
      gemv_t_all<false>(PT_, dx_, &rp_, -1, dy_); // dy = p - sum_j P_j^T dx_j
    }
    join_cholesky_Q();
    {
      Timer t(this, "searchDirection.solve.dy_Qinv");
      // El::cholesky::SolveAfter with the blocked factor: forward (dy -> qtmpv_), then
      // backward (qtmpv_ -> dy); one launch per panel, one lane per (row, column) of the panel
      static_assert(PB * PB <= 1024, "the Q-substitution kernels take a PB x PB panel per workgroup");
      for(int p = 0; p < q_panels_; ++p)
        {
          const int k0 = p * q_nb_, nb = std::min(q_nb_, N_ - k0), rest = N_ - k0 - nb;
          Batch iv{LiQ_.ptr(), d_qdiag_.p + p, 1};
          if(qsolve_sum_lanes_)
            launch(k_qsolve_panel3<NL, false>, dim3(std::max(1u, cdiv(rest, PB))), dim3(QS2_T), stream_, QB(), iv, dy_.ptr(), qtmpv_.ptr(), k0);
          else
            launch(k_qsolve_panel2<NL, false>, dim3(std::max(1u, cdiv(rest, PB))), dim3(QS2_T), stream_, QB(), iv, dy_.ptr(), qtmpv_.ptr(), k0);
        }
      for(int p = q_panels_ - 1; p >= 0; --p)
        {
          const int k0 = p * q_nb_;
          Batch iv{LiQ_.ptr(), d_qdiag_.p + p, 1};
          if(qsolve_sum_lanes_)
            launch(k_qsolve_panel3<NL, true>, dim3(std::max(1u, cdiv(k0, PB))), dim3(QS2_T), stream_, QB(), iv, qtmpv_.ptr(), dy_.ptr(), k0);
          else
            launch(k_qsolve_panel2<NL, true>, dim3(std::max(1u, cdiv(k0, PB))), dim3(QS2_T), stream_, QB(), iv, qtmpv_.ptr(), dy_.ptr(), k0);
        }
    }
    {
      Timer t(this, "searchDirection.solve.dx_Pdy");
      launch(k_gemv_n<NL>, dim3(cdiv(max_P_, 4), Jl_), dim3(WG), stream_, btB(PT_), dy_.cptr(), dx_.ptr(), d_blk_.p, N_, 1);
    }
    {
      Timer t(this, "searchDirection.solve.dx_LTinv");
      // dx := L^{-T} dx
      launch(k_vec_trsm<NL, true>, dim3(Jl_), dim3(WG), stream_, schurB(), Batch{LiS_.ptr(), d_schur_.p, Jl_}, Batch{dx_.ptr(), d_rowP_.p, Jl_});
    }
  }

  // compute_search_direction.cxx:44-90
  void compute_search_direction(const M &beta, bool corrector)
  {
    {
      // R = beta mu I - XY (- dX dY)
      Timer t(this, "searchDirection.R");
      copy(mXY_, R_);
      if(corrector)
        gemm_psd(dX_, dY_, R_, true, true);
      upload_scalar(S_BETAMU, mw::mul(beta, mu_));
      add_diagonal(R_, S_BETAMU);
    }
    {
      // Z = Symmetrize(X^{-1} (PrimalResidues Y - R))
      Timer t(this, "searchDirection.Z");
      gemm_psd(PR_, Y_, Z_, false, false, &R_, true); // Z^T = (PR Y - R)^T
      cholesky_solve_X_transposed(Z_);
      symmetrize(Z_, false);
    }
    {
      // dx = -d - Tr(A_p Z) ; dy = p
      Timer t(this, "searchDirection.schur_RHS");
      launch(k_schur_rhs2<NL>, dim3(max_pairs_, Jl_), dim3(WG), stream_, basesTB(), psd(Z_), dres_.cptr(), dx_.ptr(), d_blk_.p);
    }
    solve_schur_complement_equation();
    {
      // dX = PrimalResidues + sum_p A_p dx[p]
      Timer t(this, "searchDirection.dX");
      constraint_matrix_weighted_sum(dx_, dX_, PR_, +1);
    }
    {
      // dY = Symmetrize(X^{-1} (R - dX Y))
      Timer t(this, "searchDirection.dY");
      gemm_psd(dX_, Y_, dY_, false, false, &R_, true); // dY^T = (dX Y - R)^T
      cholesky_solve_X_transposed(dY_);
      symmetrize(dY_, true);
    }
  }
  // frobenius_product_of_sums.cxx:6-31: sum (X+dX).(Y+dY) into R_FROB
  void queue_frobenius_product()
  {
    mw::CPtr X = X_.cptr(), dX = dX_.cptr(), Y = Y_.cptr(), dY = dY_.cptr();
    reduce_to<RED_SUM>(R_FROB, psd_elems_, [=] __device__(size_t i) {
      return mw::mul(mw::add(mw::load<NL>(X, i), mw::load<NL>(dX, i)), mw::add(mw::load<NL>(Y, i), mw::load<NL>(dY, i)));
    });
  }
  // corrector_centering_parameter.cxx:12-31 from the fetched Frobenius product
  M corrector_centering_parameter(bool feasible)
  {
    const M r = mw::div(res_host_[R_FROB], mw::mul(mu_, mw::from_u32<NL>((uint32_t)total_psd_rows_)));
    const M one = mw::from_u32<NL>(1);
    const M beta = mw::lt(r, one) ? mw::mul(r, r) : r;
    if(feasible)
      return mw::min(mw::max(feasible_centering_parameter_, beta), one);
    return mw::max(infeasible_centering_parameter_, beta);
  }

  // step_length.cxx:27-46
  // lambda_min(L^{-1} dM L^{-T}) of every local PSD block into lam (step_length.cxx:27-46 up to the
  // reduction), enqueued on stream_
  void enqueue_min_eigenvalues(const DevArray &Lc, const DevArray &Li, const DevArray &dM, DevArray &W, DevArray &D, DevArray &E,
                               DevBuf<double> &F, DevArray &lam)
  {
    copy(dM, W);
    // W = L^{-1} dM L^{-T} (lower_triangular_inverse_congruence.cxx:4-16): W1 = dM L^{-T}, then
    // W = (W1^T L^{-T}) since the result is symmetric — both solves run on rows
    trsm_rlt(psd(Lc), psd(Li), psd(W), max_n_, max_n_);
    launch(k_transpose<NL>, dim3(cdiv((size_t)max_n_ * max_n_, WG), 2 * Jl_), dim3(WG), stream_, psd(W));
    trsm_rlt(psd(Lc), psd(Li), psd(W), max_n_, max_n_);
    // lanes per matrix (kernels.hpp, k_tridiag; the result has the same bits for every choice): per size bucket -- the
    // rank-2 update of a Householder step has w (w + 1) / 2 entries, 190 at n = 20 and 780 at n = 40 -- and wider where
    // the rank owns so few matrices that all of them are resident anyway (the launch then lasts as long as the
    // Householder chain of the largest one: a rank of an 8-GPU job)
    const int mats = 2 * Jl_, slots = num_cus_ * (2048 / 4 / TRI_T); // workgroups of TRI_T lanes resident at 2 waves / SIMD
    const int widen = !tridiag_wide_ ? 1 : (mats * 4 <= slots ? 4 : (mats * 2 <= slots ? 2 : 1));
    auto tridiag = [&](int lanes, const int *ids, int count) {
      if(!count)
        return;
      lanes = std::min(512, lanes * widen);
      // (above 66 limbs the tree image of 512 lanes no longer fits the CU's 160 KB of LDS: 256 lanes there.  A 98-limb
      // build -- 3072 bits, 50 minutes of hipcc for the one object -- was tried in round 5: every kernel fits, but the step
      // lengths and the block condition numbers agree with the oracle to 2^-64 only; not shipped, profiles/r05w_*.log)
      constexpr bool T512 = 512 * sizeof(TriSlot<NL>) + sizeof(Mw<NL>) <= 160 * 1024;
      if constexpr(T512)
        {
          if(lanes >= 512)
            {
              launch(k_tridiag<NL, 512>, dim3(count), dim3(512), stream_, psd(W), vecn(D), vecn(E), ids);
              return;
            }
        }
      if(lanes >= 256)
        launch(k_tridiag<NL, 256>, dim3(count), dim3(256), stream_, psd(W), vecn(D), vecn(E), ids);
      else if(lanes >= 128)
        launch(k_tridiag<NL, 128>, dim3(count), dim3(128), stream_, psd(W), vecn(D), vecn(E), ids);
      else
        launch(k_tridiag<NL, 64>, dim3(count), dim3(64), stream_, psd(W), vecn(D), vecn(E), ids);
    };
    // ONE launch (the matrices with the long chains first in `ids`) unless the buckets are given different widths: two
    // launches on a stream run one after the other, and the second bucket would idle behind the tail of the first
    // (measured: + 0.8 ms per iteration on C4, profiles/r05_tridiag_lanes.txt)
    if(tri_lanes_small_ == tri_lanes_large_)
      tridiag(tri_lanes_large_, (const int *)tri_ids_.p, mats);
    else
      {
        tridiag(tri_lanes_large_, (const int *)tri_ids_.p, tri_count_large_);
        tridiag(tri_lanes_small_, (const int *)tri_ids_.p + tri_count_large_, mats - tri_count_large_);
      }
    launch(k_tridiag_min<NL>, dim3(cdiv(2 * Jl_, EIG_T)), dim3(EIG_T), stream_, vecn(D), vecn(E), F.p, F.p + psd_rows_local_ + 1, lam.ptr());
  }
  // The primal and the dual step length are two independent latency-bound chains (Householder
  // steps, one-lane Newton): they run concurrently, X on the main stream and Y on the stream
  // Cholesky(Q) used earlier in the iteration (Z is free by now and serves as Y's work matrix).
  // The smallest eigenvalues land in R_LAMX / R_LAMY (a rank without blocks contributes +huge).
  void queue_step_lengths()
  {
    Timer t(this, "stepLength");
    if(Jl_)
      {
        HIP_CHECK(hipEventRecord(ev_q_ready_, stream_));
        HIP_CHECK(hipStreamWaitEvent(stream_q_, ev_q_ready_, 0));
        enqueue_min_eigenvalues(Xc_, LiX_, dX_, W_, eigD_, eigE_, eigF_, lam_);
        {
          OnSideStream side(this);
          enqueue_min_eigenvalues(Yc_, LiY_, dY_, Z_, eigD2_, eigE2_, eigF2_, lam2_);
          HIP_CHECK(hipEventRecord(ev_q_done_, stream_));
        }
        HIP_CHECK(hipStreamWaitEvent(stream_, ev_q_done_, 0));
      }
    M huge = mw::from_u32<NL>(1);
    huge.e = 1 << 28;
    mw::CPtr lp = lam_.cptr(), lp2 = lam2_.cptr();
    reduce_to<RED_MIN>(R_LAMX, (size_t)2 * Jl_, [=] __device__(size_t i) { return mw::load<NL>(lp, i); }, huge);
    reduce_to<RED_MIN>(R_LAMY, (size_t)2 * Jl_, [=] __device__(size_t i) { return mw::load<NL>(lp2, i); }, huge);
  }
  M step_length_from(const M &lambda)
  {
    const M &gamma = step_length_reduction_;
    if(mw::gt(lambda, mw::neg(gamma)))
      return mw::from_u32<NL>(1);
    return mw::div(mw::neg(gamma), lambda);
  }

  // update_cond_numbers.hxx:16-110: the ratios and the winner are found on the device
  void queue_cond_numbers()
  {
    Timer t(this, "condition_numbers");
    const int J1 = std::max(Jl_, 1);
    if(Jl_)
      {
        launch(k_diag_ratio<NL>, dim3(Jl_), dim3(DR_T), stream_, schurB(), ratio_.ptr(), (size_t)0);
        launch(k_diag_ratio<NL>, dim3(2 * Jl_), dim3(DR_T), stream_, psd(Xc_), ratio_.ptr(), (size_t)J1);
        launch(k_diag_ratio<NL>, dim3(2 * Jl_), dim3(DR_T), stream_, psd(Yc_), ratio_.ptr(), (size_t)3 * J1);
      }
    launch(k_diag_ratio<NL>, dim3(1), dim3(DR_T), stream_, QB(), res(), (size_t)R_QCOND);
    launch(k_cond_best<NL>, dim3(1), dim3(WG), stream_, ratio_.cptr(), Jl_, (const BlockDesc *)d_blk_.p, res(), (size_t)R_COND, xwords() + XW_TAG);
  }
  void finish_cond_numbers()
  {
    Q_cond_number_ = mw::mul(res_host_[R_QCOND], res_host_[R_QCOND]);
    max_block_cond_number_ = mw::mul(res_host_[R_COND], res_host_[R_COND]);
    const uint32_t tag = xw_host_[XW_TAG];
    std::ostringstream ss;
    if(tag)
      {
        const uint32_t code = tag - 1u;
        const int g = (int)(code / 8u), kind = (int)((code % 8u) / 2u), parity = (int)(code % 2u);
        if(kind == 0)
          ss << "schur_complement_cholesky.block_" << g;
        else
          ss << (kind == 1 ? "X" : "Y") << "_cholesky.block_" << g << "_" << parity;
      }
    else
      ss << "schur_complement_cholesky.block_-1";
    max_block_cond_number_name_ = ss.str();
  }

  // -XY and its trace (scale_multiply_add.cxx:4-13, step.cxx:137-144); only X and Y enter, so
  // it is queued with the residues and mu reaches the host at the first synchronisation point
  void queue_minus_XY_and_trace()
  {
    Timer t(this, "XY");
    gemm_psd(X_, Y_, mXY_, true, false);
    const MatDesc *dv = d_vecn_.p, *dp = d_psd_.p;
    mw::CPtr a = mXY_.cptr();
    const int nq = 2 * Jl_;
    reduce_to<RED_SUM>(R_TRACE, psd_rows_local_, [=] __device__(size_t i) {
      int q = 0;
      while(q + 1 < nq && dv[q + 1].off <= i)
        ++q;
      const int r = (int)(i - dv[q].off);
      return mw::load<NL>(a, (size_t)dp[q].off + (size_t)r * (dp[q].ld + 1));
    });
  }
  // compute_R_error.hxx:9-29 : max |(-XY) + mu I| into R_RERR (mu is scal_[S_MU])
  void queue_R_error()
  {
    Timer t(this, "R_error");
    const MatDesc *dp = d_psd_.p;
    mw::CPtr a = mXY_.cptr(), sc = scal_.cptr();
    const int nq = 2 * Jl_;
    reduce_to<RED_MAX>(R_RERR, psd_elems_, [=] __device__(size_t i) {
      int q = 0;
      while(q + 1 < nq && dp[q + 1].off <= i)
        ++q;
      const size_t e = i - (size_t)dp[q].off;
      const int n = dp[q].rows;
      M v = mw::load<NL>(a, i);
      if(e % n == e / n)
        v = mw::add(v, mw::load<NL>(sc, S_MU));
      return mw::abs(v);
    });
  }

  // step.cxx:51-229 (mu and the termination tests were settled by iterate())
  void step(bool feasible)
  {
    upload_scalar(S_MU, mu_);
    queue_R_error();
    {
      Timer t(this, "computeSearchDirection(betaPredictor)");
      const M beta_predictor = feasible ? mw::zero<NL>() : infeasible_centering_parameter_; // predictor_centering_parameter.cxx:4-9
      compute_search_direction(beta_predictor, false);
    }
    // ---- synchronisation point 2: the corrector's centering parameter needs sum (X+dX).(Y+dY)
    queue_frobenius_product();
    exchange({{R_FROB, X_SUM}, {R_RERR, X_MAX}});
    fetch(); // raises Cholesky failures of S_j and Q
    R_error_ = res_host_[R_RERR];
    {
      Timer t(this, "computeSearchDirection(betaCorrector)");
      beta_corrector_ = corrector_centering_parameter(feasible);
      compute_search_direction(beta_corrector_, true);
    }
    queue_cond_numbers();
    queue_step_lengths();
    // ---- synchronisation point 3: step lengths (and the condition numbers for the log)
    exchange({{R_LAMX, X_MIN}, {R_LAMY, X_MIN}, {R_COND, X_ARGMAX}});
    fetch();
    finish_cond_numbers();
    primal_step_length_ = step_length_from(res_host_[R_LAMX]);
    dual_step_length_ = step_length_from(res_host_[R_LAMY]);
    if(feasible)
      {
        primal_step_length_ = mw::min(primal_step_length_, dual_step_length_);
        dual_step_length_ = primal_step_length_;
      }
    {
      // step.cxx:208-224; queued, not waited for: the next synchronisation point covers it
      Timer t(this, "update");
      upload_scalar(S_ALPHA_P, primal_step_length_);
      upload_scalar(S_ALPHA_D, dual_step_length_);
      axpy_scalar(S_ALPHA_P, dx_, x_, Ptot_);
      axpy_scalar(S_ALPHA_P, dX_, X_, psd_elems_);
      axpy_scalar(S_ALPHA_D, dy_, y_, (size_t)N_);
      axpy_scalar(S_ALPHA_D, dY_, Y_, psd_elems_);
    }
  }
  void axpy_scalar(int slot, const DevArray &d, DevArray &v, size_t count)
  {
    mw::CPtr sc = scal_.cptr(), dd = d.cptr();
    mw::Ptr vv = v.ptr();
    foreach(count, [=] __device__(size_t i) {
      mw::store<NL>(vv, i, mw::add(mw::load<NL>(vv, i), mw::mul(mw::load<NL>(sc, slot), mw::load<NL>(dd, i))));
    });
  }

public:
  // One pass of run.cxx:322-467.  Returns true when the loop terminates.  Three host
  // synchronisation points (fetch()): the termination test, the corrector's centering parameter,
  // the step lengths; everything else is queued ahead of the GPU.
  bool iterate() override
  {
    LaunchScope launches_of_this_solver(&launches_);
    if(!started_)
      {
        started_ = true;
        start_time_ = std::chrono::steady_clock::now();
      }
    iteration_ += 1;
    prog_iteration_.store((unsigned long long)iteration_);
    leave_beside_stream();
    Timer whole(this, "iteration");
    if(profile_)
      profiled_iterations_ += 1;
    {
      // failure tag, rank 0's wall-clock verdict, SIGTERM seen on this rank
      const double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - start_time_).count();
      launch(k_store_words4<0>, dim3(1), dim3(64), stream_, xwords(), 0xffffffffu, elapsed >= max_runtime_s_ ? 1u : 0u,
             stop_requested_.load() ? 1u : 0u, 0u);
    }
    // ---- synchronisation point 1: everything the termination test needs (run.cxx:380-435) and mu
    queue_objectives();
    factor_X_and_Y();
    compute_bilinear_pairings();
    // The Schur complement solver (step.cxx:117-127) needs only X and Y, so it is queued BEFORE the
    // residues and the termination test: Cholesky(Q), the dependent chain that follows the syrk on
    // the side streams, then runs beside the residues as well as beside the predictor's
    // Q-independent part.  On the (last) iteration that terminates here the work is discarded — S, P, Q
    // are scratch — and a failure in it is not raised (the reference would not have computed it).
    initialize_schur_complement_solver();
    compute_dual_residues_and_error();
    compute_primal_residues_P();
    compute_primal_residue_p();
    queue_minus_XY_and_trace();
    exchange({{R_CX, X_SUM}, {R_DERR, X_MAX}, {R_PERR_P, X_MAX}, {R_TRACE, X_SUM}});
    fetch(FAIL_Y); // raises Cholesky failures of X and Y only
    if(xw_host_[XW_OR])
      {
        join_cholesky_Q();
        terminate_reason_ = SIGTERM_Received; // run.cxx:332-355: any rank, graceful exit
        return true;
      }
    primal_objective_ = mw::add(objective_const_, res_host_[R_CX]);
    dual_objective_ = mw::add(objective_const_, res_host_[R_BY]);
    const M denom = mw::max(mw::add(mw::abs(primal_objective_), mw::abs(dual_objective_)), mw::from_u32<NL>(1));
    duality_gap_ = mw::div(mw::abs(mw::sub(primal_objective_, dual_objective_)), denom);
    dual_error_ = res_host_[R_DERR];
    primal_error_P_ = res_host_[R_PERR_P];
    primal_error_p_ = res_host_[R_PERR_p];
    bool feasible = false;
    if(compute_feasible_and_termination(feasible, xw_host_[XW_STOP] != 0))
      {
        join_cholesky_Q();
        return true;
      }
    Timer t(this, "step");
    mu_ = mw::div(mw::neg(res_host_[R_TRACE]), mw::from_u32<NL>((uint32_t)total_psd_rows_));
    if(mw::gt(mu_, max_complementarity_)) // step.cxx:145-153 (after the Schur complement solver, as here)
      {
        join_cholesky_Q();
        terminate_reason_ = MaxComplementarityExceeded;
        return true;
      }
    step(feasible);
    return false;
  }

  // The piece of the step that approx_objective and outer_limits reuse (approx_objective/
  // setup_solver.cxx:204-220, outer_limits/compute_optimal.cxx:188-215): from the current X and Y,
  //   L_j = chol(S_j)            -> get_array("L", j)        schur_complement_cholesky
  //   P_j = L_j^{-1} B_j         -> get_array("PT", j)       schur_off_diagonal (stored transposed, N x P_j)
  //   chol(Q), Q = sum P_j^T P_j -> get_array("Q")           lower factor = (El::Cholesky UPPER)^T
  // without touching x, X, y, Y.  Raises the same errors as the iteration.
  void schur_solver_init() override
  {
    LaunchScope launches_of_this_solver(&launches_);
    launch(k_store_words4<0>, dim3(1), dim3(64), stream_, xwords(), 0xffffffffu, 0u, 0u, 0u);
    factor_X_and_Y();
    compute_bilinear_pairings();
    initialize_schur_complement_solver();
    join_cholesky_Q();
    exchange({});
    fetch();
  }
  // solve_schur_complement_equation.cxx:16-79 with that solver: in dx (set_array "dx", per block)
  // and dy (set_array "dy"), out the solution in the same arrays
  void schur_solve() override
  {
    LaunchScope launches_of_this_solver(&launches_);
    copy(dy_, rp_);
    solve_schur_complement_equation();
    HIP_CHECK(hipStreamSynchronize(stream_));
  }

  // ==========================================================================
  // outputs
  // ==========================================================================
  std::string get_scalar(const std::string &n) override
  {
    const M *v = nullptr;
    M pe;
    if(n == "mu") v = &mu_;
    else if(n == "P-obj" || n == "primalObjective") v = &primal_objective_;
    else if(n == "D-obj" || n == "dualObjective") v = &dual_objective_;
    else if(n == "gap" || n == "dualityGap") v = &duality_gap_;
    else if(n == "P-err") v = &primal_error_P_;
    else if(n == "p-err") v = &primal_error_p_;
    else if(n == "D-err" || n == "dualError") v = &dual_error_;
    else if(n == "R-err") v = &R_error_;
    else if(n == "P-step") v = &primal_step_length_;
    else if(n == "D-step") v = &dual_step_length_;
    else if(n == "beta") v = &beta_corrector_;
    else if(n == "Q_cond_number") v = &Q_cond_number_;
    else if(n == "max_block_cond_number") v = &max_block_cond_number_;
    else if(n == "primalError") { pe = mw::max(primal_error_P_, primal_error_p_); v = &pe; }
    else if(n == "block_name") return max_block_cond_number_name_;
    else if(n == "iteration") return std::to_string(iteration_);
    else throw SolverError(4, "unknown scalar " + n);
    return mw::to_decimal<NL>(*v);
  }

  struct ArrayRef
  {
    DevArray *a;
    size_t off, count;
  };
  ArrayRef locate(const std::string &w, int j, int parity)
  {
    if(w == "y") return {&y_, 0, (size_t)N_};
    if(w == "dy") return {&dy_, 0, (size_t)N_};
    if(w == "primal_residue_p") return {&rp_, 0, (size_t)N_};
    if(w == "Q") return {&Q_, 0, (size_t)N_ * N_};
    if(w == "b") return {&b_, 0, (size_t)N_};
    const int l = local_index(j);
    if(l < 0)
      throw SolverError(4, "block " + std::to_string(j) + " is not owned by this rank");
    const BlockDesc &bd = blk_[l];
    if(w == "x") return {&x_, (size_t)bd.voff, (size_t)bd.P};
    if(w == "dx") return {&dx_, (size_t)bd.voff, (size_t)bd.P};
    if(w == "c") return {&c_, (size_t)bd.voff, (size_t)bd.P};
    if(w == "dual_residues") return {&dres_, (size_t)bd.voff, (size_t)bd.P};
    if(w == "c_minus_By")
      {
        // save_c_minus_By.hxx:18-47: c - B y of the current y, all local blocks at once
        if(cmby_.n < Ptot_)
          cmby_.alloc(Ptot_, NL);
        copy(c_, cmby_);
        launch(k_gemv_n<NL>, dim3(cdiv(max_P_, 4), Jl_), dim3(WG), stream_, btB(BT_), y_.cptr(), cmby_.ptr(), d_blk_.p, N_, -1);
        return {&cmby_, (size_t)bd.voff, (size_t)bd.P};
      }
    if(w == "S" || w == "L") return {&S_, (size_t)h_schur_[l].off, (size_t)bd.P * bd.P};
    if(w == "BT") return {&BT_, (size_t)h_bt_[l].off, (size_t)bd.P * N_};
    if(w == "PT") return {&PT_, (size_t)h_bt_[l].off, (size_t)bd.P * N_};
    const int q = 2 * l + (parity ? 1 : 0);
    const size_t nn = (size_t)bd.n[parity ? 1 : 0] * bd.n[parity ? 1 : 0], qq = (size_t)bd.m * bd.K * bd.m * bd.K;
    if(w == "X") return {&X_, (size_t)h_psd_[q].off, nn};
    if(w == "Y") return {&Y_, (size_t)h_psd_[q].off, nn};
    if(w == "dX") return {&dX_, (size_t)h_psd_[q].off, nn};
    if(w == "dY") return {&dY_, (size_t)h_psd_[q].off, nn};
    if(w == "Xc") return {&Xc_, (size_t)h_psd_[q].off, nn};
    if(w == "Yc") return {&Yc_, (size_t)h_psd_[q].off, nn};
    if(w == "primal_residues") return {&PR_, (size_t)h_psd_[q].off, nn};
    if(w == "AXinv") return {&AX_, (size_t)h_pair_[q].off, qq};
    if(w == "AY") return {&AY_, (size_t)h_pair_[q].off, qq};
    throw SolverError(4, "unknown array " + w);
  }
  // column-major, newline separated decimals
  std::string get_array(const std::string &which, int j, int parity) override
  {
    const ArrayRef r = locate(which, j, parity);
    join_cholesky_Q();
    HIP_CHECK(hipStreamSynchronize(stream_));
    std::vector<M> v = download<NL>(*r.a, r.off, r.count);
    std::string out;
    for(auto &e : v)
      {
        out += mw::to_decimal<NL>(e);
        out += "\n";
      }
    return out;
  }
  // binary flavours: column-major mpf_t-layout records (exact when limbs64 >= NL/2 + 1)
  size_t get_array_mpf(const std::string &which, int j, int parity, int limbs64, uint64_t *out, size_t capacity) override
  {
    const ArrayRef r = locate(which, j, parity);
    if(!out || capacity < r.count)
      return r.count;
    if(limbs64 < 1)
      throw SolverError(4, "get_array_mpf: limbs64 < 1");
    join_cholesky_Q();
    HIP_CHECK(hipStreamSynchronize(stream_));
    const std::vector<M> v = download<NL>(*r.a, r.off, r.count);
    for(size_t i = 0; i < v.size(); ++i)
      mw::to_mpf_record<NL>(v[i], out + i * (size_t)(limbs64 + 2), limbs64);
    return r.count;
  }
  void set_array_mpf(const std::string &which, int j, int parity, int limbs64, const uint64_t *values, size_t count) override
  {
    if(which != "x" && which != "X" && which != "y" && which != "Y" && which != "dx" && which != "dy" && which != "c")
      throw SolverError(4, "set_array: only x, X, y, Y (state), dx, dy (right-hand sides of schur_solve) and c (after set_block_f64) can be set");
    if(which != "y" && which != "dy" && local_index(j) < 0)
      return;
    const ArrayRef r = locate(which, j, parity);
    if(count != r.count)
      throw SolverError(4, "set_array_mpf: wrong element count for " + which);
    upload<NL>(*r.a, r.off, records(values, count, limbs64));
  }
  // checkpoint-style state injection (x, X, y, Y): column-major decimals
  void set_array(const std::string &which, int j, int parity, const char *txt) override
  {
    if(which != "x" && which != "X" && which != "y" && which != "Y" && which != "dx" && which != "dy" && which != "c")
      throw SolverError(4, "set_array: only x, X, y, Y (state), dx, dy (right-hand sides of schur_solve) and c (after set_block_f64) can be set");
    if(which != "y" && which != "dy" && local_index(j) < 0)
      return;
    const ArrayRef r = locate(which, j, parity);
    upload<NL>(*r.a, r.off, parse_list(txt, r.count, which.c_str()));
  }

  // ==========================================================================
  // operator-level entry points (parity tests call the device arithmetic and the
  // fixed-point syrk kernel in isolation through the C ABI)
  // ==========================================================================
  std::string op_scalar(const std::string &op, const char *a, const char *b) override
  {
    int code = op == "add" ? 0 : op == "sub" ? 1 : op == "mul" ? 2 : op == "div" ? 3 : op == "sqrt" ? 4 : -1;
    if(code < 0)
      throw SolverError(4, "op_scalar: unknown op " + op);
    DevArray io;
    io.alloc(3, NL);
    upload<NL>(io, 0, std::vector<M>{mw::from_decimal<NL>(a), mw::from_decimal<NL>(b)});
    mw::Ptr p = io.ptr();
    // one kernel per operation: with all five inlined behind a switch the kernel needs the whole register
    // file at 50 limbs (256 VGPRs + 255 AGPRs + scratch) and does not return on gfx950
    switch(code)
      {
      case 0: foreach(1, [=] __device__(size_t) { mw::store<NL>(p, 2, mw::add(mw::load<NL>(p, 0), mw::load<NL>(p, 1))); }); break;
      case 1: foreach(1, [=] __device__(size_t) { mw::store<NL>(p, 2, mw::sub(mw::load<NL>(p, 0), mw::load<NL>(p, 1))); }); break;
      case 2: foreach(1, [=] __device__(size_t) { mw::store<NL>(p, 2, mw::mul(mw::load<NL>(p, 0), mw::load<NL>(p, 1))); }); break;
      case 3: foreach(1, [=] __device__(size_t) { mw::store<NL>(p, 2, mw::div(mw::load<NL>(p, 0), mw::load<NL>(p, 1))); }); break;
      default: foreach(1, [=] __device__(size_t) { mw::store<NL>(p, 2, mw::sqrt(mw::load<NL>(p, 0))); }); break;
      }
    HIP_CHECK(hipStreamSynchronize(stream_));
    return mw::to_decimal<NL>(download<NL>(io, 2, 1)[0]);
  }

  // Per-block cost in microseconds per iteration, the quantity the reference measures into
  // block_timings: the block's own Cholesky and Trsm (compute_Q.cxx:40-53 cholesky_<j> + solve_<j>)
  // plus its share of the syrk, which the reference too can only split by block size because all
  // blocks are processed together (bigint_syrk/Readme.md:325-342).  Blocks run batched on the GPU, so
  // "the time of block j" is measured as the residence time of the workgroups that worked on it
  // (kernels.hpp: WgClock, 100 MHz wall clock, profiled iterations only); the measured wall time of
  // the stage is divided among the local blocks in proportion to those MEASURED times — a block that
  // is cheaper than its size suggests (zeros short-cut the multi-word products) shows up as cheaper.
  // Blocks of other ranks get 0 (the caller sums over ranks).
  void block_timings(long long *us) override
  {
    for(int j = 0; j < J_; ++j)
      us[j] = 0;
    auto stage = [&](const char *name) {
      auto it = timers_ms_.find(name);
      return it == timers_ms_.end() ? 0.0 : it->second;
    };
    const double t_chol = stage("initializeSchurComplementSolver.Q.cholesky"), t_solve = stage("initializeSchurComplementSolver.Q.solve"),
                 t_syrk = stage("initializeSchurComplementSolver.Q.syrk");
    if(profiled_iterations_ == 0 || stage("iteration") <= 0)
      throw SolverError(4, "block_timings: no profiled iteration yet (sdpb_hip_set_profiling, then iterate)");
    if(!Jl_)
      return;
    HIP_CHECK(hipStreamSynchronize(stream_));
    const std::vector<unsigned long long> cyc = blk_cycles_.download();
    if(cyc.size() < (size_t)2 * Jl_)
      throw SolverError(4, "block_timings: the profiled iterations did not reach the Schur complement stage");
    double s_chol = 0, s_solve = 0, s_rows = 0;
    for(int l = 0; l < Jl_; ++l)
      {
        s_chol += (double)cyc[l];
        s_solve += (double)cyc[Jl_ + l];
        s_rows += blk_[l].P;
      }
    for(int l = 0; l < Jl_; ++l)
      {
        const double ms = (s_chol > 0 ? t_chol * (double)cyc[l] / s_chol : 0.0) + (s_solve > 0 ? t_solve * (double)cyc[Jl_ + l] / s_solve : 0.0)
                          + t_syrk * blk_[l].P / s_rows;
        us[local_[l]] = (long long)std::llround(1000.0 * ms / (double)profiled_iterations_);
      }
  }
  // the raw counters behind block_timings (tests): ticks of Cholesky(S_j) and of P_j = L_j^{-1} B_j per local block
  void block_clock_ticks(unsigned long long *cholesky, unsigned long long *solve) override
  {
    for(int j = 0; j < J_; ++j)
      cholesky[j] = solve[j] = 0;
    HIP_CHECK(hipStreamSynchronize(stream_));
    if(blk_cycles_.n < (size_t)2 * Jl_ || !Jl_)
      return;
    const std::vector<unsigned long long> cyc = blk_cycles_.download();
    for(int l = 0; l < Jl_; ++l)
      {
        cholesky[local_[l]] = cyc[l];
        solve[local_[l]] = cyc[Jl_ + l];
      }
  }

  // sdpb_hip_bench_op: average HIP-event time of one kernel on synthetic operands (ms)
  double bench_op(const std::string &op, int a, int b, int reps) override
  {
    if(op == "trsm")
      {
        // P = L^{-1} B with the solver's own blocks and the factors of the last iteration (a = b = 0)
        if(iteration_ == 0)
          throw SolverError(4, "bench_op trsm: run an iteration first");
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        float total = 0;
        for(int r = 0; r < std::max(reps, 1); ++r)
          {
            HIP_CHECK(hipEventRecord(e0, stream_));
            trsm_rlt_schur(schurB(), Batch{LiS_.ptr(), d_schur_.p, Jl_}, btB(PT_), N_, max_P_, nullptr, &BT_);
            HIP_CHECK(hipEventRecord(e1, stream_));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            total += ms;
          }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        return total / std::max(reps, 1);
      }
    if(op != "syrk" || a <= 0 || b <= 0)
      throw SolverError(4, "bench_op: unknown op " + op);
    const int rows = a, cols = b;
    Syrk ws(&syrk_); // the whole image in one window; column terms of the Toom-4 image zero: the timing does not depend on them
    ws.prepare((size_t)rows, cols, stream_, /*one_chunk=*/true);
    {
      // pseudo-random limbs with the top bit of every word clear (valid pieces of every image layout)
      uint32_t *p = ws.image.p;
      foreach(ws.win.stride * fx_planes<FX>(), [=] __device__(size_t i) {
        uint64_t z = (uint64_t)i * 0x9E3779B97F4A7C15ull + 0x1234567ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        p[i] = (uint32_t)(z >> (Syrk::SYRK_TOOM5K ? 37 : 33)); // (limbs of the lazy-carry image are < 2^28)
      });
    }
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    ws.G(stream_, ws.all()); // warm-up
    HIP_CHECK(hipEventRecord(e0, stream_));
    for(int r = 0; r < std::max(reps, 1); ++r)
      ws.G(stream_, ws.all());
    HIP_CHECK(hipEventRecord(e1, stream_));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ms / std::max(reps, 1);
  }

  // syrk_Q as an operator (compute_Q.cxx:94-132): column norms, normalise-and-shift, the exact
  // integer syrk, the diagonal check and the restore, on a rows x cols matrix P given column-major as
  // decimals — the reference's own unit test of this stage is calculate_matrix_square.test.cxx
  // (random P, compare with plain P^T P to p/2 bits).  Returns the lower triangle of Q = P^T P
  // (cols x cols column-major, upper part zero).  Same kernels, same order as the iteration.
  std::string op_syrk_Q(int rows, int cols, const char *txt) override
  {
    if(rows <= 0 || cols <= 0)
      throw SolverError(4, "op_syrk_Q: rows and cols must be positive");
    const size_t cnt = (size_t)rows * cols;
    const std::vector<M> in = parse_list(txt, cnt, "P");
    // P^T (cols x rows column-major): element (r, n) at r*cols + n, the layout of PT_
    std::vector<M> pt(cnt);
    for(int c = 0; c < cols; ++c)
      for(int r = 0; r < rows; ++r)
        pt[(size_t)r * cols + c] = in[(size_t)c * rows + r];
    DevArray PT, part, nrm, inv, Q;
    PT.alloc(cnt, NL);
    part.alloc(cols, NL);
    nrm.alloc(cols, NL);
    inv.alloc(cols, NL);
    Q.alloc((size_t)cols * cols, NL);
    upload<NL>(PT, 0, pt);
    BlockDesc bd{};
    bd.P = rows;
    bd.voff = 0;
    DevBuf<BlockDesc> dbd;
    dbd.upload(std::vector<BlockDesc>{bd});
    DevBuf<MatDesc> dmd;
    dmd.upload(std::vector<MatDesc>{MatDesc{0, cols, rows, cols, 0}});
    launch(k_gemv_t_partial<NL, true>, dim3(cdiv(cols, WG), 1), dim3(WG), stream_, Batch{PT.ptr(), dmd.p, 1}, PT.cptr(), part.ptr(),
           (const BlockDesc *)dbd.p, cols);
    launch(k_sum_partials<NL>, dim3(cdiv(cols, SP_ROWS)), dim3(WG), stream_, part.cptr(), 1, cols, nrm.cptr(), 0, 1, nrm.ptr());
    norms_to_inverse(nrm.ptr(), inv.ptr(), (size_t)cols);
    DevBuf<int> qf;
    Syrk ws(&syrk_); // the same input windows as the iteration (SDPB_HIP_SYRK_IMAGE_BYTES, --maxSharedMemory)
    ws.prepare((size_t)rows, cols, stream_);
    const size_t as = ws.acc_stride;
    DevBuf<uint32_t> &acc = ws.acc;
    ws.G_windows(
      stream_,
      [&](size_t r0, unsigned nr) {
        const size_t n = (size_t)nr * cols;
        launch(k_normalize_fx<NL, FX>, dim3(cdiv(n, WG)), dim3(WG), stream_, mw::offset(PT.cptr(), r0 * (size_t)cols), n, cols, inv.cptr(), ws.image.p,
               ws.win.stride);
      },
      [] {});
    qf.alloc(4);
    HIP_CHECK(hipMemsetAsync(qf.p, 0, 4 * sizeof(int), stream_));
    launch(k_syrk_unbias<FX>, dim3(cdiv((size_t)cols * cols, WG)), dim3(WG), stream_, acc.p, as, cols, (unsigned long long)rows, (size_t)0,
           (size_t)cols * cols);
    launch(k_restore_Q<NL, FX>, dim3(cdiv((size_t)cols * cols, WG)), dim3(WG), stream_, (const uint32_t *)acc.p, as, cols, nrm.cptr(),
           Q.ptr(), qf.p + 1, (size_t)0, (size_t)cols * cols);
    HIP_CHECK(hipStreamSynchronize(stream_));
    const std::vector<int> flags = qf.download();
    if(flags[1]) // compute_Q.cxx:65-91
      throw SolverError(1, "Normalized Q should have ones on diagonal. For i = " + std::to_string(flags[1] - 1));
    std::string out;
    for(const M &e : download<NL>(Q, 0, (size_t)cols * cols))
      {
        out += mw::to_decimal<NL>(e);
        out += "\n";
      }
    return out;
  }

  // min_eigenvalue.cxx:8-33 as an operator: the smallest eigenvalue of a symmetric n x n matrix (column-major decimals) with
  // the kernels of the step length -- Householder tridiagonalisation (k_tridiag), then fp64 bisection + multi-word Newton on the
  // shifted tridiagonal matrix (k_tridiag_min).  The reference calls El::HermitianEig and takes El::Min.
  std::string op_min_eigenvalue(int n, const char *txt) override
  {
    if(n <= 0)
      throw SolverError(4, "op_min_eigenvalue: n must be positive");
    DevArray A, D, E, lam;
    A.alloc((size_t)n * n, NL);
    D.alloc(n, NL);
    E.alloc(n, NL);
    lam.alloc(1, NL);
    upload<NL>(A, 0, parse_list(txt, (size_t)n * n, "A"));
    DevBuf<MatDesc> dm, dv;
    dm.upload(std::vector<MatDesc>{MatDesc{0, n, n, n, 0}});
    dv.upload(std::vector<MatDesc>{MatDesc{0, n, 1, n, 0}});
    DevBuf<int> ids;
    ids.upload(std::vector<int>{0});
    DevBuf<double> F;
    F.alloc(2 * ((size_t)n + 1));
    const Batch Ab{A.ptr(), dm.p, 1}, Db{D.ptr(), dv.p, 1}, Eb{E.ptr(), dv.p, 1};
    launch(k_tridiag<NL, 128>, dim3(1), dim3(128), stream_, Ab, Db, Eb, (const int *)ids.p);
    launch(k_tridiag_min<NL>, dim3(1), dim3(EIG_T), stream_, Db, Eb, F.p, F.p + n + 1, lam.ptr());
    HIP_CHECK(hipStreamSynchronize(stream_));
    return mw::to_decimal<NL>(download<NL>(lam, 0, 1)[0]);
  }

  // Exact integer syrk of a rows x cols integer matrix (column-major decimal
  // integers, |v| < 2^(32 FX)); returns the lower triangle of P^T P (cols x cols,
  // column-major, upper part zero) as decimal integers.  Same kernel as syrk_Q.
  std::string op_int_syrk(int rows, int cols, const char *txt) override
  {
    std::vector<std::pair<const char *, const char *>> tok;
    split_numbers(txt, tok);
    if((int)tok.size() != rows * cols)
      throw SolverError(4, "op_int_syrk: wrong element count");
    const size_t cnt = (size_t)rows * cols;
    std::vector<uint32_t> h(cnt * (FX + 1), 0); // plane 0 = sign, planes 1..FX = magnitude
    for(int c = 0; c < cols; ++c)
      for(int r = 0; r < rows; ++r)
        {
          const char *s = tok[(size_t)c * rows + r].first, *e = tok[(size_t)c * rows + r].second;
          bool negative = false;
          if(*s == '-')
            {
              negative = true;
              ++s;
            }
          mw::BigNat n;
          for(; s < e; ++s)
            {
              if(*s < '0' || *s > '9')
                throw SolverError(4, "op_int_syrk: not an integer");
              if(n.w.empty())
                {
                  if(*s != '0')
                    n.w.push_back((uint32_t)(*s - '0'));
                }
              else
                n.mul_small(10, (uint32_t)(*s - '0'));
            }
          if(n.w.size() > (size_t)FX || (n.w.size() == (size_t)FX && (n.w[FX - 1] >> (sdpb::fx_frac_bits<FX>() % 32)) != 0))
            throw SolverError(4, "op_int_syrk: |value| >= 2^" + std::to_string(sdpb::fx_frac_bits<FX>()));
          const size_t idx = (size_t)r * cols + c; // fx element (r, n) at r*N + n
          for(size_t k = 0; k < n.w.size(); ++k)
            h[(k + 1) * cnt + idx] = n.w[k];
          h[idx] = (negative && !n.w.empty()) ? 1u : 0u;
        }
    DevBuf<uint32_t> staged;
    staged.upload(h);
    Syrk ws(&syrk_); // the same input windows as the iteration (SDPB_HIP_SYRK_IMAGE_BYTES, --maxSharedMemory)
    ws.prepare((size_t)rows, cols, stream_);
    const size_t as = ws.acc_stride;
    DevBuf<uint32_t> &acc = ws.acc;
    ws.G_windows(
      stream_,
      [&](size_t r0, unsigned nr) {
        const size_t n = (size_t)nr * cols;
        launch(k_fx_from_int<FX>, dim3(cdiv(n, WG)), dim3(WG), stream_, (const uint32_t *)staged.p + r0 * (size_t)cols, cnt, n, cols, ws.image.p,
               ws.win.stride);
      },
      [] {});
    launch(k_syrk_unbias<FX>, dim3(cdiv((size_t)cols * cols, WG)), dim3(WG), stream_, acc.p, as, cols, (unsigned long long)rows, (size_t)0,
           (size_t)cols * cols);
    HIP_CHECK(hipStreamSynchronize(stream_));
    std::vector<uint32_t> a = acc.download();
    std::string out;
    for(int j = 0; j < cols; ++j)
      for(int i = 0; i < cols; ++i)
        {
          const size_t idx = (size_t)i + (size_t)j * cols;
          if(i < j)
            {
              out += "0\n";
              continue;
            }
          mw::BigNat n;
          n.w.resize(Syrk::ACCW);
          for(int k = 0; k < Syrk::ACCW; ++k)
            n.w[k] = a[(size_t)k * as + idx];
          const bool negative = n.w[Syrk::ACCW - 1] >> 31;
          if(negative)
            {
              uint64_t carry = 1;
              for(auto &w : n.w)
                {
                  const uint64_t s = (uint64_t)(~w) + carry;
                  w = (uint32_t)s;
                  carry = s >> 32;
                }
            }
          n.trim();
          std::string dig;
          while(!n.is_zero())
            {
              uint32_t rem = n.div_small(1000000000u);
              for(int k = 0; k < 9; ++k)
                {
                  dig.push_back((char)('0' + rem % 10));
                  rem /= 10;
                }
            }
          while(!dig.empty() && dig.back() == '0')
            dig.pop_back();
          if(dig.empty())
            dig = "0";
          else if(negative)
            dig.push_back('-');
          out.append(dig.rbegin(), dig.rend());
          out += "\n";
        }
    return out;
  }
};

// one factory per compiled limb count (solver_nl.hip is built once per SDPB_NL)
__attribute__((weak)) SolverBase *make_solver_6(int, const std::vector<int> &, const std::vector<int> &, int, int, int, const std::vector<long long> &);
__attribute__((weak)) SolverBase *make_solver_10(int, const std::vector<int> &, const std::vector<int> &, int, int, int, const std::vector<long long> &);
__attribute__((weak)) SolverBase *make_solver_16(int, const std::vector<int> &, const std::vector<int> &, int, int, int, const std::vector<long long> &);
__attribute__((weak)) SolverBase *make_solver_18(int, const std::vector<int> &, const std::vector<int> &, int, int, int, const std::vector<long long> &);
__attribute__((weak)) SolverBase *make_solver_24(int, const std::vector<int> &, const std::vector<int> &, int, int, int, const std::vector<long long> &);
__attribute__((weak)) SolverBase *make_solver_26(int, const std::vector<int> &, const std::vector<int> &, int, int, int, const std::vector<long long> &);
__attribute__((weak)) SolverBase *make_solver_34(int, const std::vector<int> &, const std::vector<int> &, int, int, int, const std::vector<long long> &);
__attribute__((weak)) SolverBase *make_solver_42(int, const std::vector<int> &, const std::vector<int> &, int, int, int, const std::vector<long long> &);
__attribute__((weak)) SolverBase *make_solver_50(int, const std::vector<int> &, const std::vector<int> &, int, int, int, const std::vector<long long> &);
__attribute__((weak)) SolverBase *make_solver_66(int, const std::vector<int> &, const std::vector<int> &, int, int, int, const std::vector<long long> &);
} // namespace sdpb
