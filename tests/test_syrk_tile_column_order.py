"""The tile column order of the lazy-carry image (kernels.hpp: fx_col_slot, 512 bits): inside every group of 32 columns the
image keeps column c in slot 2 (c % 16) + (c % 32) / 16, so that k_syrk_fx3 reads a lane's two pieces of an operand with one
128-bit LDS read.  Everything that writes or indexes image columns (k_fx_from_int / k_normalize_fx, k_fx_colsum5, the
staging and the row loop of k_syrk_fx3) has to agree on that order, and on the rows padded to whole groups of 32 slots.

Every case drives SDPSolver.op_int_syrk and compares every entry of the lower triangle with exact Python integers.  The
same cases run on the gfx950 library (marked gpu) and on the CPU emulation build of the same sources."""
import functools
import random

import pytest

from sdpb_amd.solver import SDPSolver
from tests import libs, parity

PRECISION = 512  # the only width that takes the lazy-carry path (FX = 16)
LIBS = [pytest.param("emu", id="emu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


def _solver(kind):
    sdp, _, _, _ = parity.load_case("1d")
    lib = libs.product_lib() if kind == "gpu" else libs.emu_lib()
    s = SDPSolver(sdp, PRECISION, {}, lib_path=lib)
    assert s.fx_frac_bits == 509, "512 bits is the lazy-carry image"
    return s


def _exact(rows, cols, vals):
    """Lower triangle of Q' = A^T A for the column-major rows x cols integers `vals`: {(i, j): Q'(i, j), i >= j}."""
    col = [vals[c * rows:(c + 1) * rows] for c in range(cols)]
    return {(i, j): sum(a * b for a, b in zip(col[i], col[j])) for j in range(cols) for i in range(j, cols)}


@functools.lru_cache(maxsize=None)
def _random_case(rows, cols):
    """Random full-range entries (with the extremes and zero among them) and their exact product, computed once per shape."""
    fb = 509
    rng = random.Random(1000 * rows + cols)
    vals = [rng.randrange(-(2 ** fb) + 1, 2 ** fb) for _ in range(rows * cols)]
    vals[0], vals[1], vals[2], vals[-1], vals[-2] = 0, 2 ** fb - 1, -(2 ** fb) + 1, 2 ** fb - 1, -(2 ** fb) + 1
    return tuple(vals), _exact(rows, cols, vals)


def _compare(got, want, cols, name=False):
    """Every entry of the lower triangle against `want`, zeros above it; name: say which column pairs own a wrong value."""
    owners = {}
    if name:
        for k, v in want.items():
            owners.setdefault(v, []).append(k)
    for j in range(cols):
        for i in range(cols):
            g = got[i + j * cols]
            if i < j:
                assert g == 0, (i, j)
            elif g != want[(i, j)]:
                raise AssertionError(f"Q'({i},{j}) is wrong" + (f": it holds the entry of the column pair(s) {owners.get(g)}" if name else ""))


@pytest.mark.parametrize("kind", LIBS)
def test_every_entry_names_its_column_pair(kind, monkeypatch):
    """Column c is the constant 3^(c % 20) + c (a few rows negated, which leaves Q' alone): Q'(i, j) = rows v_i v_j names
    its column pair (2624 different integers for the 2628 pairs), so a slot mix-up anywhere shows as a wrong entry and says
    whose it holds."""
    rows, cols = 33, 72
    monkeypatch.setenv("SDPB_HIP_SYRK_SPLITS", "1")
    v = [3 ** (c % 20) + c for c in range(cols)]
    sign = [-1 if r in (0, 7, 31, 32) else 1 for r in range(rows)]
    vals = [sign[r] * v[c] for c in range(cols) for r in range(rows)]
    want = {(i, j): rows * v[i] * v[j] for j in range(cols) for i in range(j, cols)}
    s = _solver(kind)
    _compare(s.op_int_syrk(rows, cols, vals), want, cols, name=True)
    s.close()


# cols 37: a last tile row with fewer than 17 columns (quadrant masks 1 and 5); 50: 17 ... 31 columns (masks 15 and 11 on a
# ragged tile); 72: a full off-diagonal tile and an edge of 8 columns.  rows 33: two passes, the second one row long;
# 150: five passes (both carry cadences fire), no multiple of 32.
@pytest.mark.parametrize("kind", LIBS)
@pytest.mark.parametrize("splits", ["1", "2"])
@pytest.mark.parametrize("rows", [33, 150])
@pytest.mark.parametrize("cols", [37, 50, 72])
def test_tile_shapes_are_bit_exact(cols, rows, splits, kind, monkeypatch):
    monkeypatch.setenv("SDPB_HIP_SYRK_SPLITS", splits)
    vals, want = _random_case(rows, cols)
    s = _solver(kind)
    _compare(s.op_int_syrk(rows, cols, list(vals)), want, cols)
    s.close()


@pytest.mark.parametrize("kind", LIBS)
def test_every_entry_at_the_largest_magnitude(kind, monkeypatch):
    """parity.check_int_syrk_extremes over one sweep of 150 rows on a ragged 50-column operand: the carry schedule of the
    column accumulators does not depend on the column order."""
    monkeypatch.setenv("SDPB_HIP_SYRK_SPLITS", "1")
    s = _solver(kind)
    parity.check_int_syrk_extremes(s, 150, 50)
    s.close()


@pytest.mark.parametrize("kind", LIBS)
def test_column_sums_remove_the_biases_of_permuted_columns(kind, monkeypatch):
    """Negative entries put the biases of the three signed evaluation points in play; k_fx_colsum5 has to sum slot
    fx_col_slot(c) into column c for k_syrk5_finish to remove them exactly.  Columns of one sign, of the other, and mixed,
    with different magnitudes from column to column, on 50 columns (a ragged second group)."""
    rows, cols, fb = 40, 50, 509
    monkeypatch.setenv("SDPB_HIP_SYRK_SPLITS", "1")
    rng = random.Random(50)
    vals = []
    for c in range(cols):
        top = 2 ** (fb - 3 * c)  # a different size per column: a sum that lands on the wrong column cannot cancel
        for r in range(rows):
            m = rng.randrange(1, top)
            vals.append(-m if c % 3 == 0 or (c % 3 == 1 and rng.random() < 0.5) else m)
    want = _exact(rows, cols, vals)
    s = _solver(kind)
    _compare(s.op_int_syrk(rows, cols, vals), want, cols)
    s.close()
