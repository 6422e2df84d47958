"""Host logic of the iteration driver on the CPU emulation build: the three synchronisation
points, --maxRuntime inside the termination test, graceful stop, and errors that every rank
raises identically.  (The gfx950 library runs the same host code; see tests/test_gpu_parity*.py.)"""
import os
import sys

import pytest

from sdpb_amd.solver import SDPBError, SDPSolver
from tests import libs, parity


def _solver(name="1d-constraints", **kw):
    sdp, meta, iters, out = parity.load_case(name)
    return sdp, SDPSolver(sdp, meta["precision"], meta["params"], lib_path=libs.emu_lib(), **kw), iters


def test_three_host_synchronisation_points_per_iteration():
    _, s, _ = _solver()
    for _ in range(4):
        assert not s.iterate()
    assert s.host_syncs == 3 * 4
    s.close()


def test_max_runtime_is_tested_inside_the_iteration_before_the_step():
    """compute_feasible_and_termination.cxx:51-56: the state the run ends with is the one the
    objectives in out.txt were computed from (no step after the test)."""
    _, s, _ = _solver()
    for _ in range(2):
        assert not s.iterate()
    x_before = s.array("x", 0)
    s.set_max_runtime(0.0)
    assert s.iterate()
    assert s.terminate_reason == "maxRuntime exceeded"
    assert s.array("x", 0) == x_before
    s.close()


def test_max_iterations_takes_precedence_over_max_runtime():
    sdp, meta, _, _ = parity.load_case("1d")
    s = SDPSolver(sdp, meta["precision"], dict(meta["params"], maxIterations=2), lib_path=libs.emu_lib())
    s.set_max_runtime(0.0)
    s.set_max_runtime(1e9)
    assert not s.iterate() and not s.iterate()
    s.set_max_runtime(0.0)
    assert s.iterate()
    assert s.terminate_reason == "maxIterations exceeded"
    s.close()


def test_request_stop_ends_the_run_gracefully_with_the_sigterm_reason():
    _, s, _ = _solver()
    assert not s.iterate()
    y_before = s.array("y")
    s.request_stop()
    assert s.iterate()
    assert s.terminate_reason == "SIGTERM signal received"
    assert s.array("y") == y_before
    s.close()


def test_profiling_timers_are_off_by_default_and_named_like_the_reference():
    _, s, _ = _solver()
    assert not s.iterate()
    t = s.timers()
    assert "initializeSchurComplementSolver.Q.syrk" not in t and t["host_syncs"] == 3
    s.set_profiling(True)
    assert not s.iterate()
    t = s.timers()
    for k in ("choleskyDecomposition", "initializeSchurComplementSolver.Q.syrk", "computeSearchDirection(betaCorrector)",
              "stepLength"):
        assert k in t, k
    s.close()


def _failing_rank_worker(rank, world, port, lib, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, libs.ROOT)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from sdpb_amd.distributed import make_collectives
        sdp, meta, _, _ = parity.load_case("1d-constraints")
        s = SDPSolver(sdp, meta["precision"], meta["params"], rank=rank, world_size=world, lib_path=lib)
        s.set_collectives(*make_collectives(torch.device("cpu")))
        assert not s.iterate()
        # make Y of block 1 indefinite on its owner only: the OTHER rank must raise the same error
        # instead of running on into the next collective
        owner = s.block_owner(1)
        if owner == rank:
            n = len(s.array("Y", 1, 1))
            s.set_array("Y", ["-1"] + ["0"] * (n - 1), 1, 1)
        try:
            s.iterate()
            q.put((rank, owner, None))
        except SDPBError as e:
            q.put((rank, owner, (e.code, str(e))))
        s.close()
    finally:
        dist.destroy_process_group()


def test_a_cholesky_failure_on_one_rank_is_raised_by_every_rank():
    import torch.multiprocessing as mp
    from tests.test_multirank_gpu import _free_port
    lib = libs.emu_lib()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_failing_rank_worker, args=(r, 2, port, lib, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, _, e0), (_, _, e1) = results
    assert e0 is not None and e0 == e1, (e0, e1)
    assert e0[0] == 1 and "Block_Diagonal_Matrix Y, block index = 1, parity = 1" in e0[1]


def _schur_hook(lib):
    """sdpb_hip_schur_solver_init rebuilds, from a loaded (x, X, y, Y), exactly the Schur solver the
    iteration builds from that state; sdpb_hip_schur_solve solves with it."""
    import mpmath
    name = "1d-constraints"
    sdp, meta, _, _ = parity.load_case(name)
    a = SDPSolver(sdp, meta["precision"], meta["params"], lib_path=lib)
    for _ in range(2):
        assert not a.iterate()
    # the state travels as mpf records: bit exact (decimal text is not)
    state = {(w, j, b): a.array_mpf(w, j, b) for w in ("X", "Y") for j in range(sdp.J) for b in (0, 1)}
    state.update({("x", j, 0): a.array_mpf("x", j) for j in range(sdp.J)})
    y = a.array_mpf("y")
    X00 = a.array("X", 0, 0)
    assert not a.iterate()          # builds its Schur solver from that state (then moves on)
    b = SDPSolver(sdp, meta["precision"], meta["params"], lib_path=lib)
    for (w, j, par), v in state.items():
        b.set_array_mpf(w, v, j, par)
    b.set_array_mpf("y", y)
    b.schur_solver_init()
    for j in range(sdp.J):
        assert b.array("L", j) == a.array("L", j)
        assert b.array("PT", j) == a.array("PT", j)
    assert b.array("X", 0, 0) == X00                          # state untouched
    assert b.array("Q") == a.array("Q")
    # solve S-system for a known solution: rhs built from (dx*, dy*) must give it back.
    # Equation (solve_schur_complement_equation.cxx): with L L^T = S, P = L^{-1} B, Q = P^T P:
    #   dx <- L^{-1} dx ; dy <- Q^{-1}(dy - P^T dx) ... checked here through linearity instead:
    r1 = [["1"] * len(b.array("dx", j)) for j in range(sdp.J)]
    for scale in ("1", "3"):
        for j in range(sdp.J):
            b.set_array("dx", [scale] * len(r1[j]), j)
        b.set_array("dy", [scale] * sdp.N)
        b.schur_solve()
        sol = [mpmath.mpf(v) for j in range(sdp.J) for v in b.array("dx", j)] + [mpmath.mpf(v) for v in b.array("dy")]
        if scale == "1":
            base = sol
        else:
            for u, v in zip(base, sol):
                assert abs(3 * u - v) <= mpmath.mpf(2) ** -(meta["precision"] - 40) * (abs(v) + 1)
    a.close()
    b.close()


def test_schur_solver_hook_for_approx_objective():
    _schur_hook(libs.emu_lib())


@pytest.mark.gpu
def test_schur_solver_hook_for_approx_objective_on_the_device():
    _schur_hook(libs.product_lib())


def test_schur_solver_hook_matches_the_oracle():
    assert parity.check_schur_hook_against_oracle(libs.emu_lib()) <= -384


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["singlet_cT", "1d-constraints"])
def test_schur_solver_hook_matches_the_oracle_on_the_device(name):
    assert parity.check_schur_hook_against_oracle(libs.product_lib(), name) <= -384


def test_block_timings_are_written_read_and_balance_the_ranks(tmp_path):
    """the timing run writes <checkpointDir>/block_timings (write_timing.cxx:34-68), the
    next run reads it (read_block_costs.cxx:14-59) and plans the blocks on those costs."""
    import ctypes
    from sdpb_amd import run
    from sdpb_amd.solver import load_library
    sdp_dir = os.path.join(parity.GOLDEN, "dfibo", "sdp")
    sdp, meta, _, _ = parity.load_case("dfibo")
    ck = tmp_path / "ck"
    argv = ["-s", sdp_dir, "-o", str(tmp_path / "out"), "-c", str(ck), "--precision", str(meta["precision"]), "--lib",
            libs.emu_lib(), "--maxIterations", "3", "--verbosity", "0"]
    run.solve(argv)
    with open(ck / "block_timings") as f:
        costs = [int(t) for t in f.read().split()]
    assert len(costs) == sdp.J and all(c >= 0 for c in costs) and sum(costs) > 0
    # larger blocks cost more (dfibo mixes num_points 1 and 4); the costs are measurements (host clock in
    # the emulation build), so compare the groups, not every pair
    big = [c for c, k in zip(costs, sdp.num_points) if k == max(sdp.num_points)]
    small = [c for c, k in zip(costs, sdp.num_points) if k == min(sdp.num_points)]
    assert sum(big) / len(big) > sum(small) / len(small)
    # the plan on measured costs is a balanced partition
    L = load_library(libs.emu_lib())
    owners = (ctypes.c_int * sdp.J)()
    assert L.sdpb_hip_plan_blocks_with_costs(sdp.J, (ctypes.c_longlong * sdp.J)(*costs), 4, owners) == 0
    loads = [sum(c for c, o in zip(costs, owners) if o == r) for r in range(4)]
    assert set(owners) == {0, 1, 2, 3} and max(loads) - min(loads) <= max(costs)
    # a solver created with those costs uses exactly that plan
    s = SDPSolver(sdp, meta["precision"], meta["params"], rank=1, world_size=4, lib_path=libs.emu_lib(), block_costs=costs)
    assert [s.block_owner(j) for j in range(sdp.J)] == list(owners)
    s.close()
    # second run: the file is consumed (no timing run, file untouched), results unchanged
    before = os.path.getmtime(ck / "block_timings")
    run.solve(argv[:3] + [str(tmp_path / "out2")] + argv[4:])
    assert os.path.getmtime(ck / "block_timings") == before
    with open(tmp_path / "out" / "out.txt") as a, open(tmp_path / "out2" / "out.txt") as b:
        strip = lambda t: [ln for ln in t.splitlines() if not ln.startswith("Solver runtime")]  # noqa: E731
        assert strip(a.read()) == strip(b.read())
    with pytest.raises(SDPBError, match="Incompatible number of entries"):
        SDPSolver(sdp, meta["precision"], lib_path=libs.emu_lib(), block_costs=costs[:-1])


def _measured_block_costs(lib, strict):
    """SURVEY §8f row 2 as a MEASUREMENT (compute_Q.cxx:40-53 times every block): the per-block device
    clocks see what an operation-count model cannot — a block whose free-variable matrix B_j is zero
    short-cuts the multi-word products of P_j = L_j^{-1} B_j and is measured cheaper than a block of the
    same shape with a dense B_j; the Cholesky clocks order the blocks by size."""
    import numpy as np
    from sdpb_amd import synthetic
    dims, npts, N = [2, 2, 1, 1, 2, 1], [12] * 6, 40
    sdp, src = synthetic.make_lazy(dims, npts, N, 512, seed=9)

    def source(j):
        be, bo, B, c = src(j)
        return (be, bo, np.zeros_like(B), c) if j == 0 else (be, bo, B, c)   # block 0: same shape as block 1, B = 0
    s = SDPSolver(sdp, 512, parity.DEFAULT_PARAMS, lib_path=lib, block_source=source)
    assert not s.iterate()
    s.set_profiling(True)
    for _ in range(2):
        assert not s.iterate()
    s.set_profiling(False)
    chol, solve = s.block_clock_ticks()
    costs = s.block_timings()
    s.close()
    assert all(t > 0 for t in chol) and all(t > 0 for t in solve[1:]) and all(c > 0 for c in costs)
    big, small = [chol[j] for j in (0, 1, 4)], [chol[j] for j in (2, 3, 5)]        # P = 36 blocks vs P = 12 blocks
    assert sum(big) / 3 > sum(small) / 3
    if strict:   # device clocks; the emulation's host clock mostly measures its fibre switches
        assert solve[0] < 0.6 * solve[1], (solve[0], solve[1])      # measured, not modelled: the zero block is cheaper
        assert min(big) > max(small)
        assert costs[0] < costs[1]
    return chol, solve, costs


def test_block_costs_are_measured_per_block():
    _measured_block_costs(libs.emu_lib(), strict=False)


@pytest.mark.gpu
def test_block_costs_are_measured_per_block_on_the_device():
    chol, solve, costs = _measured_block_costs(libs.product_lib(), strict=True)
    print("cholesky ticks", chol, "solve ticks", solve, "block_timings us", costs)


@pytest.mark.gpu
def test_block_timings_are_written_read_and_balance_the_ranks_on_the_device(tmp_path):
    """GPU twin of test_block_timings_are_written_read_and_balance_the_ranks: the timing run of the
    sdpb-compatible driver writes <checkpointDir>/block_timings from the device clocks, the next run
    consumes it; the plan on the measured costs is a balanced partition."""
    import ctypes
    from sdpb_amd import run
    from sdpb_amd.solver import load_library
    sdp_dir = os.path.join(parity.GOLDEN, "singlet_cT", "sdp")
    sdp, meta, _, _ = parity.load_case("singlet_cT")
    ck = tmp_path / "ck"
    argv = ["-s", sdp_dir, "-o", str(tmp_path / "out"), "-c", str(ck), "--precision", str(meta["precision"]), "--maxIterations", "4",
            "--verbosity", "0"]
    run.solve(argv)
    with open(ck / "block_timings") as f:
        costs = [int(t) for t in f.read().split()]
    assert len(costs) == sdp.J and all(c > 0 for c in costs)
    # singlet_cT: K = 24 ... 31; the largest blocks are measured dearer than the smallest
    order = sorted(range(sdp.J), key=lambda j: sdp.num_points[j])
    assert costs[order[-1]] > costs[order[0]]
    L = load_library(libs.product_lib())
    owners = (ctypes.c_int * sdp.J)()
    assert L.sdpb_hip_plan_blocks_with_costs(sdp.J, (ctypes.c_longlong * sdp.J)(*costs), 2, owners) == 0
    loads = [sum(c for c, o in zip(costs, owners) if o == r) for r in range(2)]
    assert set(owners) == {0, 1} and abs(loads[0] - loads[1]) <= max(costs)
    before = os.path.getmtime(ck / "block_timings")
    run.solve(argv[:3] + [str(tmp_path / "out2")] + argv[4:])
    assert os.path.getmtime(ck / "block_timings") == before


def test_zero_costs_do_not_pile_up_on_rank_zero():
    """A reference-written block_timings file holds milliseconds: small blocks read 0.  Ties between equally
    loaded ranks go to the rank with fewer blocks."""
    import ctypes
    from sdpb_amd.solver import load_library
    L = load_library(libs.emu_lib())
    J, world = 12, 4
    owners = (ctypes.c_int * J)()
    assert L.sdpb_hip_plan_blocks_with_costs(J, (ctypes.c_longlong * J)(*([0] * J)), world, owners) == 0
    assert sorted(list(owners).count(r) for r in range(world)) == [3, 3, 3, 3]
    # two dear blocks take a rank each; the free ones are shared by the two unloaded ranks
    costs = [0] * 8 + [5, 5, 0, 0]
    assert L.sdpb_hip_plan_blocks_with_costs(J, (ctypes.c_longlong * J)(*costs), world, owners) == 0
    assert sorted(list(owners).count(r) for r in range(world)) == [1, 1, 5, 5] and owners[8] != owners[9]
    with pytest.raises(SDPBError, match="Incompatible number of entries"):
        sdp, meta, _, _ = parity.load_case("dfibo")
        SDPSolver(sdp, meta["precision"], lib_path=libs.emu_lib(), block_costs=[1] * (sdp.J + 3))


def test_tile_dot_products_are_exact_against_gmp(tmp_path):
    """sdpb_amd/csrc/tiledot.hpp (the fixed-point tile dot products behind the trailing updates of P = L^-1 B: radix 2^27,
    biased images, carry-free 64-bit column sums) against exact GMP integers on the host (tests/shim/tiledot_check.cpp): the
    image is the exact floor, the tile sum misses only the columns that are not formed (< 2^(27 cut + 37)), and the float
    accumulator ends within 2^-(32 NL - 4) of the exact sum relative to its largest term while the spread of the tile stays
    inside the spare bits -- for 6, 10, 16, 18, 24 limbs with 32-term tiles and 26 limbs with 16-term tiles."""
    import subprocess
    exe = tmp_path / "tiledot_check"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(libs.ROOT, "sdpb_amd", "csrc"), "-I/opt/conda/include",
                        os.path.join(libs.ROOT, "tests", "shim", "tiledot_check.cpp"), "-o", str(exe), "-l:libgmp.so.10"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count(" 0 failures") == 8, r.stdout + r.stderr


def test_syrk_planners_keep_what_the_launches_rely_on(tmp_path):
    """sdpb_amd/csrc/syrk_stage.hpp (FxSyrk<FX>: syrk_plan, syrk_splits_for, q_window) on the host, without a device and under
    AddressSanitizer + UBSan (tests/shim/syrk_plan_check.cpp): for the image width of each of the ten compiled limb counts,
    over N = 1 ... 2048, 1 ... 700 000 rows, forced row splits and budgets from nothing to 10^10 bytes, the chunks of the tile
    list cover it and none is empty, the last row split of every chunk (a shorter last one included) owns a row and its planes
    fit the buffer, the planes stay inside a non-zero budget or are one tile in one split, the input windows cover the rows in
    whole passes of the product kernel, and the image stays inside its budget unless the plan says the bound is exceeded."""
    import subprocess
    exe = tmp_path / "syrk_plan_check"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-I" + os.path.join(libs.ROOT, "tests", "emu", "include"),
                        "-I" + os.path.join(libs.ROOT, "sdpb_amd", "csrc"), "-DSDPB_NO_RCCL", "-Wno-unknown-pragmas", "-Wno-attributes",
                        os.path.join(libs.ROOT, "tests", "shim", "syrk_plan_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count(" 0 failures") == 10 and not r.stderr, r.stdout + r.stderr
