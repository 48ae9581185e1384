"""boundary.field = Open without a GPU: the numpy restatement of the two kernels (tests/open_boundary_reference.py) against what
the operation approximates -- the free-space potential summed source by source --, and the C ABI's declaration."""
import ctypes
import os

import numpy as np
import pytest

from tests import open_boundary_reference as R

LD = np.longdouble
CENTRED = ((-4.0, -4.0), (4.0, 4.0))
OFF_CENTRE = ((-3.0, -5.5), (6.5, 3.5))      # 9.5 x 9.0
# each wall in turn the nearest to the expansion point x = y = 0 (8.5 x 9.5 or 9.5 x 8.5: dx != dy on the grids used)
WALL_BOXES = {
    "low x": ((-2.5, -5.0), (6.0, 4.5)),
    "high x": ((-6.0, -4.5), (2.5, 5.0)),
    "low y": ((-5.0, -2.5), (4.5, 6.0)),
    "high y": ((-4.5, -6.0), (5.0, 2.5)),
}
CASES = {"centred square": (64, 64) + CENTRED, "off-centre rectangle": (96, 80) + OFF_CENTRE}
CASES.update({"nearest wall " + k: (96, 80) + v for k, v in WALL_BOXES.items()})


def edge_mask(ny, nx):
    m = np.zeros((ny, nx), bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    return m


def test_wall_boxes_put_each_wall_nearest():
    for name, (lo, hi) in WALL_BOXES.items():
        d = {"low x": -lo[0], "high x": hi[0], "low y": -lo[1], "high y": hi[1]}
        assert min(d, key=d.get) == name and sorted(d.values())[1] > 1.5 * d[name]


@pytest.mark.parametrize("case", sorted(CASES))
def test_expansion_is_the_free_space_potential_of_compact_sources(case):
    """expansion (order 18) against direct (no multipoles), both in longdouble, on sources within rho <= 0.25: they differ by the
    remainder of the series, pref/h^2 sum|s| (2/19) rho^19/(1 - rho) (5e-13 sum|s| at rho = 0.25), and by the longdouble rounding
    of both (twice rounding_bound at longdouble's eps, orders below).  A wrong sign of an imaginary part, a wrong odd moment, a
    missing scale, h^2 or a target index of the wrong wall: all of them are O(1) here."""
    nx, ny, lo, hi = CASES[case]
    planes = R.compact_source(nx, ny, lo, hi, nbatch=2, seed=11)
    assert all(12 <= np.count_nonzero(p) <= 36 for p in planes)
    g = R.geometry(nx, ny, lo, hi)
    for p in planes:      # mixed sign, and symmetric about neither axis: the odd moments of either parity are there
        x, y = R.cell_positions(g, np.float64)
        assert p.min() < 0.0 < p.max()
        assert abs((p * x[None, :]).sum()) > 0.05 * np.abs(p * x[None, :]).sum()
        assert abs((p * y[:, None]).sum()) > 0.05 * np.abs(p * y[:, None]).sum()
    rho, trunc = R.truncation_bound(planes, nx, ny, lo, hi)
    assert 0.1 < rho <= 0.25
    rnd, S = R.rounding_bound(planes, nx, ny, lo, hi, eps=np.finfo(LD).eps)
    got, want = R.expansion(planes, nx, ny, lo, hi, 0, LD), R.direct(planes, nx, ny, lo, hi)
    edge = edge_mask(ny, nx)
    assert np.array_equal(got[:, ~edge], planes[:, ~edge]) and np.array_equal(want[:, ~edge], planes[:, ~edge])
    err = np.abs(got - want)[:, edge]
    tol = (trunc + 2 * rnd)[:, edge]
    print(f"{case}: rho {float(rho):.3f}, worst |expansion - direct| / bound {float((err / tol).max()):.3f}, "
          f"/ S {float((err / S[:, edge]).max()):.2e}")
    assert np.all(err <= tol)
    assert np.all(np.abs(want - planes)[:, edge] > 1e3 * tol)      # the correction is there, far above what is allowed


def test_monopole_mask_drops_only_the_logarithm():
    nx, ny, (lo, hi) = 48, 40, OFF_CENTRE
    planes = R.compact_source(nx, ny, lo, hi, nbatch=3, seed=5)
    free, masked = R.correction(planes, nx, ny, lo, hi, 0), R.correction(planes, nx, ny, lo, hi, 0b010)
    assert np.array_equal(free[0], masked[0]) and np.array_equal(free[2], masked[2])
    g = R.geometry(nx, ny, lo, hi)
    px, py, tj, ti, hh = R.edge_points(g, LD)
    inside = ~(R.cutoff_r2(g, LD)[0] > g.cutoff_sq)
    log = np.zeros((ny, nx), LD)
    np.add.at(log, (tj, ti), -LD(g.pref) * planes[1][inside].astype(LD).sum() * np.log((px * px + py * py) * LD(g.scale) ** 2) / hh)
    edge = edge_mask(ny, nx)
    assert np.allclose((free[1] - masked[1])[edge].astype(float), log[edge].astype(float), rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("case", sorted(CASES))
def test_float64_restatement_stays_within_the_counted_bound(case):
    """the float64 expansion against the longdouble one on a dense source: within eps (K S + DSRC T + DEDGE U), the bound the
    kernels are held to (a bound the restatement alone broke would be a wrong bound)"""
    nx, ny, lo, hi = CASES[case]
    for ring in ("zero", "random"):
        planes = R.dense_source(nx, ny, lo, hi, nbatch=2, seed=3, ring=ring)
        bound, S = R.rounding_bound(planes, nx, ny, lo, hi, 0b10)
        eps = np.finfo(np.float64).eps
        edge = edge_mask(ny, nx)
        f64, ref = R.expansion(planes, nx, ny, lo, hi, 0b10, np.float64), R.expansion(planes, nx, ny, lo, hi, 0b10, LD)
        err = np.abs(f64 - ref)[:, edge]
        tol = (bound + eps * np.abs(planes))[:, edge]      # (the add onto a random ring rounds to the ring's size)
        print(f"{case}, {ring} ring: worst deviation {float((err / (eps * S[:, edge])).max()):.2f} eps S")
        assert np.all(err <= tol)


def test_library_exports_hps_open_boundary_as_declared():
    from hipace_amd import _lib
    _lib.build()
    L = ctypes.CDLL(_lib.SO)
    C = ctypes
    assert hasattr(L, "hps_open_boundary")
    res, sig = _lib._SIGS["hps_open_boundary"]
    assert res is C.c_int
    assert sig == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint, C.c_void_p]
    hdr = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "hpslice.h")).read()
    flat = " ".join(hdr.split())
    assert ("int hps_open_boundary (double* staging_dev, int nbatch, int nx, int ny, const double lo[2], const double hi[2], "
            "unsigned no_monopole_mask, void* stream);") in flat
