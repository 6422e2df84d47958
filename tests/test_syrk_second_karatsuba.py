"""The second Karatsuba level of the lazy-carry syrk (kernels.hpp: k_syrk5_k2, 512 bits).  Every two-limb piece (x0, x1) of
the Toom-5 x Karatsuba image carries xm = x0 + x1 as a third one-word plane (81 planes), and a product of two pieces is three
one-limb sub-sweeps combined as s0 + (sm - s0 - s1) 2^28 + s1 2^56 -- 81 multiply-adds per row pair.  A lane owns the 4 x 4
outputs (i0 + 8 p, j0 + 8 q) of a 32 x 32 tile, and the image keeps column c of a tile in slot 4 (c % 8) + c / 8.

Every GPU / emulation case drives SDPSolver.op_int_syrk and compares every entry of the lower triangle with exact Python
integers; the reference of a shape is computed once and shared by the row splits and the two libraries.  The carry schedule
at the bounds of the image words, which no real image reaches (xm = 2^29 - 2 needs p(3) >= 121 * 2^102), is checked by a
stand-alone host program under AddressSanitizer + UBSan (tests/shim/syrk_k2_bounds_check.cpp)."""
import functools
import os
import random
import subprocess

import pytest

from sdpb_amd.solver import SDPSolver
from tests import libs, parity

PRECISION = 512  # the only width that takes the lazy-carry path (FX = 16)
FB = 509
LIBS = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]
# the limb boundaries inside each of the five 102-bit Toom pieces: x0 | x1 of the low half, low | high half, x0 | x1 of the high half
BOUNDARY_BITS = [102 * k + b for k in range(5) for b in (28, 55, 83)]


def _solver(kind):
    sdp, _, _, _ = parity.load_case("1d")
    lib = libs.product_lib() if kind == "gpu" else libs.emu_lib()
    s = SDPSolver(sdp, PRECISION, {}, lib_path=lib)
    assert s.fx_frac_bits == FB, "512 bits is the lazy-carry image"
    return s


def _boundary_value(rng):
    """A value at or next to the limb boundaries: a few of the bits 102 k + {28, 55, 83}, each as 2^b, 2^b - 1 (ones all
    the way down: every limb below at its maximum) or 2^b + 1, of either sign."""
    v = 0
    for b in rng.sample(BOUNDARY_BITS, rng.choice((1, 1, 2, 3, 15))):
        v += 2 ** b + rng.choice((-1, 0, 1))
    return v if rng.random() < 0.5 else -v


@functools.lru_cache(maxsize=None)
def _case(rows, cols):
    """Column-major rows x cols entries -- boundary values, every single boundary pattern of both signs, and full-range random
    entries among them -- and the exact lower triangle of Q' = A^T A, computed once per shape."""
    rng = random.Random(7000 * rows + cols)
    vals = [_boundary_value(rng) if rng.random() < 0.8 else rng.randrange(-(2 ** FB) + 1, 2 ** FB) for _ in range(rows * cols)]
    singles = [s * (2 ** b + d) for b in BOUNDARY_BITS for d in (-1, 0, 1) for s in (1, -1)]
    for n, v in enumerate(singles):  # spread over the columns, wrapping around the operand
        vals[(n * 37) % (rows * cols)] = v
    col = [vals[c * rows:(c + 1) * rows] for c in range(cols)]
    want = {(i, j): sum(a * b for a, b in zip(col[i], col[j])) for j in range(cols) for i in range(j, cols)}
    return tuple(vals), want


def _compare(got, want, cols):
    for j in range(cols):
        for i in range(cols):
            g = got[i + j * cols]
            if i < j:
                assert g == 0, (i, j)
            else:
                assert g == want[(i, j)], f"Q'({i},{j}) is wrong"


# cols 8, 9: a diagonal-only output of one and of two 8-column groups; 24, 25: three groups, and the first column of the
# fourth (the row loop of at most 16 rows against the full one); 40: a ragged last tile row of 8 columns with an
# off-diagonal tile; 72: a full off-diagonal tile and ragged tiles both on and off the diagonal.
# rows 33: two passes, the second one row long; 150: the 64-row and the 128-row carry fire; 300: both fire several times.
@pytest.mark.parametrize("kind", LIBS)
@pytest.mark.parametrize("splits", ["1", "2"])
@pytest.mark.parametrize("rows", [33, 150, 300])
@pytest.mark.parametrize("cols", [8, 9, 24, 25, 40, 72])
def test_limb_boundary_values_are_bit_exact(cols, rows, splits, kind, monkeypatch):
    monkeypatch.setenv("SDPB_HIP_SYRK_SPLITS", splits)
    vals, want = _case(rows, cols)
    s = _solver(kind)
    _compare(s.op_int_syrk(rows, cols, list(vals)), want, cols)
    s.close()


@pytest.mark.parametrize("kind", LIBS)
def test_every_entry_at_the_largest_magnitude(kind, monkeypatch):
    """parity.check_int_syrk_extremes over one sweep of 300 rows on a ragged 50-column operand: the largest words a real image
    holds, through both carry cadences."""
    monkeypatch.setenv("SDPB_HIP_SYRK_SPLITS", "1")
    s = _solver(kind)
    parity.check_int_syrk_extremes(s, 300, 50)
    s.close()


def test_carry_schedule_at_the_bounds_of_the_image_words(tmp_path):
    """tests/shim/syrk_k2_bounds_check.cpp: the lane arithmetic the kernel is built from (multiply-adds, the carry cadence,
    the fold and the combination of the three sub-sweeps) with EVERY image word at its architectural bound -- x0 = x1 =
    2^28 - 1, xm = 2^29 - 2 -- over one 2560-row sweep of one tile, against the closed form in unsigned __int128; host code
    under AddressSanitizer + UBSan, for both pass lengths and all four instantiations of the row loop."""
    exe = tmp_path / "syrk_k2_bounds_check"
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(libs.ROOT, "tests", "emu", "include"), "-I" + os.path.join(libs.ROOT, "sdpb_amd", "csrc"),
                        "-DSDPB_NO_RCCL", "-Wno-unknown-pragmas", "-Wno-attributes",
                        os.path.join(libs.ROOT, "tests", "shim", "syrk_k2_bounds_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count(" 0 failures") == 2 and not r.stderr, r.stdout + r.stderr
