"""boundary.field = Open on the GPU, off the 64 x 64 centred box: k_multipole_moments + k_open_boundary_apply through
hps_open_boundary (the engine's own launches, hipace_amd/csrc/open_boundary.hip) against the numpy restatement in longdouble and against
the free-space potential itself (tests/open_boundary_reference.py), and the engine on an off-centre rectangular box against the
oracle.

The bound.  Every edge cell is held to eps (K S + DSRC T + DEDGE U), S, T, U per edge cell from the sources' absolute moments
(open_boundary_reference.terms).  K = 180 is counted from the kernels' longest chain of roundings, the order-18 term, in unit
roundoffs u = eps/2, every product and sum rounded on its own:
    z'^18 by 18 complex products (2 sqrt2 u each) 51; per component s z'^n 1, the thread's sum of up to 16 cells 15, 43 LDS
    entries per thread 43, the six-way tree 3, 43 of the 256 parts per thread 43, its tree 3 = 108, on the modulus 153;
    1/z (|z|^2 2, the division 1, on the modulus, to the 18th power) 77; 17 complex products 48; M_n z^-n 2; 2/n and its product 2;
    the 19 sums of the series 19; the logarithm and its product 3; pref, h^2 and the division 3; the atomic add, two at a corner, 2
    = 360 u = 180 eps.
DSRC = 4 and DEDGE = 9 are the roundings of the positions (i dx + xoff) scale of a source cell and of a wall point, in eps of the
scaled coordinates (derived next to the constants in open_boundary_reference.py).  They cannot be folded into K: i dx + xoff
cancels, the error is absolute, and S loses its monopole term where ln|z|^2 crosses 0.  None of the three was tuned on a GPU's
output; the float64 restatement is held to the same bound in the same test.  Observed on an MI355X with dense sources, the
worst edge cell of a shape over its boxes and rings, in units of eps S: 24x20 0.32, 64x64 0.08, 65x63 0.05, 300x280 0.02, 730x724
0.009, 1024x1024 0.006 (the float64 restatement: 0.40, 0.11, 0.05, 0.03, 0.010, 0.004); the whole bound is 214 - 228 eps S there.
The count is a worst case over 360 roundings of one sign, the sources are random: the kernels use a thousandth of it.
"""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from hipace_amd import decks
from tests import open_boundary_reference as R
from tests.util import rel_err

LD = np.longdouble
EPS = np.finfo(np.float64).eps
gpu = pytest.mark.gpu

CENTRED = ((-4.0, -4.0), (4.0, 4.0))
OFF_CENTRE = ((-3.0, -5.5), (6.5, 3.5))       # 9.5 x 9.0: dx != dy on every grid below
BOXES = {"centred": CENTRED, "off-centre": OFF_CENTRE}
# on 24 x 20 only: each wall in turn the nearest to the expansion point
WALL_BOXES = {
    "low-x": ((-2.5, -5.0), (6.0, 4.5)),
    "high-x": ((-6.0, -4.5), (2.5, 5.0)),
    "low-y": ((-5.0, -2.5), (4.5, 6.0)),
    "high-y": ((-4.5, -6.0), (5.0, 2.5)),
}
ALL_BOXES = dict(BOXES, **WALL_BOXES)

# nx, ny: what of the two kernels the size reaches (asserted in test_shapes_reach_what_they_are_named_for)
SHAPES = [
    (24, 20),        # 88 boundary points: one partial workgroup in apply; most moment workgroups are empty
    (64, 64),        # the case of every deck so far: the anchor
    (65, 63),        # odd sizes, nx != ny
    (300, 280),      # above 65 536 cells: load slots u = 0, 1 carry data; five apply workgroups, the last partial
    (730, 724),      # 528 520 > 524 288 cells: every slot, and the second trip of the loop, ragged
    (1024, 1024),    # the production size, once
]
DENSE = [(nx, ny, box, ring) for nx, ny in SHAPES[:-1] for box in BOXES for ring in ("zero", "random")]
DENSE += [(24, 20, box, "zero") for box in WALL_BOXES] + [(1024, 1024, "off-centre", "zero")]
COMPACT = [(nx, ny, box) for nx, ny in SHAPES for box in BOXES] + [(24, 20, box) for box in WALL_BOXES]


def test_shapes_reach_what_they_are_named_for():
    src = open(os.path.join(os.path.dirname(__file__), "..", "hipace_amd", "csrc", "open_boundary.hip")).read()
    order, parts = map(int, re.search(r"constexpr int OPEN_ORDER = (\d+), OPEN_PARTS = (\d+);", src).groups())
    assert order == R.ORDER
    assert "hipLaunchKernelGGL(k_multipole_moments, dim3(OPEN_PARTS, nbatch), dim3(256)" in src
    assert "hipLaunchKernelGGL(k_open_boundary_apply, dim3(ceil_div(2*nx + 2*ny, 256), nbatch), dim3(256)" in src
    slots = int(re.search(r"c0 \+= (\d+)\*stride", src).group(1))
    threads, wg = parts * 256, 256
    assert (threads, slots) == (65536, 8)
    points = lambda nx, ny: 2 * nx + 2 * ny      # noqa: E731
    cells = lambda nx, ny: nx * ny               # noqa: E731
    assert points(24, 20) == 88 < wg and cells(24, 20) < 2 * wg                         # 254 of the 256 moment workgroups see no cell
    assert points(64, 64) == wg and cells(64, 64) <= threads
    assert 65 % 2 == 63 % 2 == 1 and cells(65, 63) <= threads
    assert threads < cells(300, 280) <= 2 * threads                                    # slots 0 and 1
    assert -(-points(300, 280) // wg) == 5 and points(300, 280) % wg != 0
    assert cells(730, 724) == 528520 > slots * threads == 524288                       # a second trip ...
    assert cells(730, 724) - slots * threads < threads                                 # ... in which some threads have no cell
    assert cells(1024, 1024) == 2 * slots * threads
    assert threads < cells(288, 264) <= 2 * threads and points(288, 264) == 1104       # the engine's large case below
    for nx, ny in SHAPES:
        for lo, hi in BOXES.values():
            g = R.geometry(nx, ny, lo, hi)
            assert g.dx != g.dy or ((lo, hi) == CENTRED and nx == ny)
            # the cells whose membership in the cutoff disc one rounding could decide are taken out of every source: few
            assert R.cutoff_border(nx, ny, lo, hi).mean() <= 1e-3
    for name, (lo, hi) in WALL_BOXES.items():
        d = {"low-x": -lo[0], "high-x": hi[0], "low-y": -lo[1], "high-y": hi[1]}
        assert min(d, key=d.get) == name
        assert R.geometry(24, 20, lo, hi).dx != R.geometry(24, 20, lo, hi).dy


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


def run(api, planes, lo, hi, mask=0):
    import torch
    t = torch.tensor(np.ascontiguousarray(planes), dtype=torch.float64, device="cuda")
    assert api.open_boundary(t, lo, hi, mask) is t
    return t.cpu().numpy()


def edge_mask(ny, nx):
    m = np.zeros((ny, nx), bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    return m


@functools.lru_cache(maxsize=None)
def dense_case(nx, ny, box, ring, nbatch=1, mask=0):
    """(planes, longdouble restatement, bound, S), computed once and never written to"""
    lo, hi = ALL_BOXES[box]
    planes = R.dense_source(nx, ny, lo, hi, nbatch=nbatch, seed=nx + ny, ring=ring)
    assert R.cutoff_border(nx, ny, lo, hi).mean() <= 1e-3
    bound, S = R.rounding_bound(planes, nx, ny, lo, hi, mask)
    ref = R.expansion(planes, nx, ny, lo, hi, mask, LD)
    for a in (planes, ref, bound, S):
        a.setflags(write=False)
    return planes, ref, bound, S


@gpu
@pytest.mark.parametrize("nx,ny,box,ring", DENSE, ids=lambda v: str(v))
def test_dense_source_against_the_longdouble_restatement(api, nx, ny, box, ring):
    """Assertion 1 of the module's docstring: every edge cell within eps (K S + DSRC T + DEDGE U) of the longdouble restatement
    (plus eps |s| of the cell where the ring is left random: the add onto it rounds to its size); the float64 restatement within
    the same bound; the interior bit-unchanged.  Cells beyond the cutoff are 1e6 times larger: one of them in the moments, or a
    moment short of a cell, is 1e6 / 1e13 times the bound."""
    lo, hi = ALL_BOXES[box]
    planes, ref, bound, S = dense_case(nx, ny, box, ring)
    got = run(api, planes, lo, hi)
    edge = edge_mask(ny, nx)
    assert np.array_equal(got[:, ~edge], planes[:, ~edge])
    tol = (bound + EPS * np.abs(planes))[:, edge]
    err = np.abs(got - ref)[:, edge]
    err64 = np.abs(R.expansion(planes, nx, ny, lo, hi, 0, np.float64) - ref)[:, edge]
    print(f"open boundary {nx}x{ny} {box} {ring}-ring: worst deviation {float((err / (EPS * S[:, edge])).max()):.3f} eps S "
          f"(float64 restatement {float((err64 / (EPS * S[:, edge])).max()):.3f}); bound / (eps S) = "
          f"{float((tol / (EPS * S[:, edge])).max()):.0f}")
    assert np.all(err64 <= tol)
    assert np.all(err <= tol)
    if ring == "zero":      # the correction is there and is read without cancellation
        assert np.all(np.abs(got[:, edge]) > 0.0) and np.abs(ref[:, edge]).max() > 1e6 * tol.max()
    else:                   # added onto the ring, not stored over it: a store would be off by the ring's own O(1) values
        assert np.median(np.abs(planes[:, edge])) > 1e6 * np.median(tol)


@gpu
@pytest.mark.parametrize("nx,ny,box", COMPACT, ids=lambda v: str(v))
def test_compact_source_against_the_free_space_potential(api, nx, ny, box):
    """Assertion 2: on sources within rho <= 0.25 the kernels give -phi/h^2 of phi(r) = dx dy/(4 pi) sum s ln(|r - r'|^2 scale^2),
    summed source by source in longdouble, to the remainder of an order-18 series, pref/h^2 sum|s| (2/19) rho^19/(1 - rho), plus
    the rounding bound: an error shared by the kernels and their restatement fails here."""
    lo, hi = ALL_BOXES[box]
    planes = R.compact_source(nx, ny, lo, hi, nbatch=2, seed=11)
    # (a few dozen cells where the grid has them; 24 x 20 has a handful within rho <= 0.25, off both axes all the same)
    assert all(np.count_nonzero(p) >= (30 if nx >= 64 else 1) for p in planes)
    rho, trunc = R.truncation_bound(planes, nx, ny, lo, hi)
    assert rho <= 0.25
    bound, S = R.rounding_bound(planes, nx, ny, lo, hi)
    want = R.direct(planes, nx, ny, lo, hi)
    got = run(api, planes, lo, hi)
    edge = edge_mask(ny, nx)
    assert np.array_equal(got[:, ~edge], planes[:, ~edge])
    err, tol = np.abs(got - want)[:, edge], (trunc + bound)[:, edge]
    print(f"open boundary {nx}x{ny} {box} compact: rho {float(rho):.3f}, worst |kernels - direct| {float((err / (EPS * S[:, edge])).max()):.3f} "
          f"eps S, {float((err / tol).max()):.4f} of the bound")
    assert np.all(err <= tol)
    assert np.abs(want[:, edge]).min() > 1e3 * tol.max()


@gpu
@pytest.mark.parametrize("nx,ny,box", [(65, 63, "off-centre"), (300, 280, "centred")], ids=lambda v: str(v))
def test_batches_and_monopole_masks(api, nx, ny, box):
    """Assertion 4: nbatch = 1 .. 4 of different planes under the masks 0, 0x6 (the engine's Psi/Ez/Bz call), 0x1 (SALAME's) and 0xF:
    every plane of a batch is its own single-plane result bit for bit, a masked plane is the restatement with M_0 = 0, and on a
    plane of zero net source inside the cutoff the mask changes nothing beyond the rounding bound."""
    lo, hi = ALL_BOXES[box]
    planes = R.dense_source(nx, ny, lo, hi, nbatch=4, seed=7, ring="zero").copy()
    g = R.geometry(nx, ny, lo, hi)
    r2, c = R.cutoff_r2(g)
    inside = ~(r2 > c)
    # plane 2: zero net source inside the cutoff (one cell takes minus the correctly rounded sum of the others)
    jc, ic = np.argwhere(inside)[len(np.argwhere(inside)) // 2]
    planes[2, jc, ic] = 0.0
    planes[2, jc, ic] = -math.fsum(planes[2][inside])
    assert abs(math.fsum(planes[2][inside])) <= EPS * abs(planes[2, jc, ic])
    single = {(b, m): run(api, planes[b:b + 1], lo, hi, m)[0] for b in range(4) for m in (0, 1)}
    edge = edge_mask(ny, nx)
    for nbatch in (1, 2, 3, 4):
        for mask in (0x0, 0x6, 0x1, 0xF):
            got = run(api, planes[:nbatch], lo, hi, mask)
            for b in range(nbatch):
                assert np.array_equal(got[b], single[b, (mask >> b) & 1]), (nbatch, hex(mask), b)
    for m in (0, 1):
        ref = R.expansion(planes, nx, ny, lo, hi, 0xF * m, LD)
        bound, S = R.rounding_bound(planes, nx, ny, lo, hi, 0xF * m)
        for b in range(4):
            assert np.array_equal(single[b, m][~edge], planes[b][~edge])
            assert np.all(np.abs(single[b, m] - ref[b])[edge] <= bound[b][edge]), (b, m)
    # the monopole matters where there is one, and not on plane 2
    bound, S = R.rounding_bound(planes, nx, ny, lo, hi, 0)
    assert np.abs(single[0, 0] - single[0, 1])[edge].max() > 1e6 * bound[0][edge].max()
    assert np.all(np.abs(single[2, 0] - single[2, 1])[edge] <= 2 * bound[2][edge])


@gpu
@pytest.mark.parametrize("nx,ny", SHAPES, ids=lambda v: str(v))
def test_two_calls_give_bit_identical_planes(api, nx, ny):
    """Assertion 5: the kernels promise a fixed order of summation (no atomics but the two adds of a corner, which commute)."""
    lo, hi = OFF_CENTRE
    planes = R.dense_source(nx, ny, lo, hi, nbatch=3, seed=1, ring="zero")
    first, second = run(api, planes, lo, hi, 0x6), run(api, planes, lo, hi, 0x6)
    assert np.array_equal(first, second)
    assert not np.array_equal(first, planes)


REFUSED = {
    "nbatch 5": (dict(shape=(5, 8, 8)), "nbatch must be 1..4"),
    "nx 1": (dict(shape=(1, 8, 1)), "nx and ny must be at least 2"),
    "ny 1": (dict(shape=(1, 1, 8)), "nx and ny must be at least 2"),
    "hi = lo in x": (dict(lo=(-1.0, -4.0), hi=(-1.0, 4.0)), "hi > lo"),
    "hi < lo in y": (dict(lo=(-4.0, 4.0), hi=(4.0, -4.0)), "hi > lo"),
    "not a number": (dict(lo=(-4.0, -4.0), hi=(4.0, float("nan"))), "hi > lo"),
    "origin on the low x wall": (dict(lo=(0.0, -4.0), hi=(8.0, 4.0)), "x = y = 0 inside the box"),
    "origin on the high y wall": (dict(lo=(-4.0, -8.0), hi=(4.0, 0.0)), "x = y = 0 inside the box"),
    "origin outside": (dict(lo=(1.0, -8.0), hi=(17.0, 8.0)), "x = y = 0 inside the box"),
}


@gpu
@pytest.mark.parametrize("case", sorted(REFUSED))
def test_bad_arguments_are_refused_by_message(api, case):
    import torch
    from hipace_amd._lib import HpsError
    args, message = REFUSED[case]
    t = torch.ones(args.get("shape", (2, 8, 8)), dtype=torch.float64, device="cuda")
    with pytest.raises(HpsError, match=re.escape(message)):
        api.open_boundary(t, args.get("lo", CENTRED[0]), args.get("hi", CENTRED[1]))
    assert bool((t == 1.0).all())


@gpu
def test_null_pointers_and_nbatch_0_are_refused_by_message(api):
    import torch
    from hipace_amd import _lib
    t = torch.ones((1, 8, 8), dtype=torch.float64, device="cuda")
    lo, hi = (C.c_double * 2)(-4.0, -4.0), (C.c_double * 2)(4.0, 4.0)
    call = _lib.lib().hps_open_boundary
    for args, message in [((None, 1, 8, 8, lo, hi, 0, None), "null argument"), ((C.c_void_p(t.data_ptr()), 1, 8, 8, None, hi, 0, None), "null argument"),
                          ((C.c_void_p(t.data_ptr()), 1, 8, 8, lo, None, 0, None), "null argument"),
                          ((C.c_void_p(t.data_ptr()), 0, 8, 8, lo, hi, 0, None), "nbatch must be 1..4")]:
        assert call(*args) == 1      # HPS_ERR_ARG
        assert message in _lib.lib().hps_last_error().decode()
    with pytest.raises(ValueError, match="contiguous CUDA float64"):
        api.open_boundary(t.float(), CENTRED[0], CENTRED[1])
    assert bool((t == 1.0).all())


# ---- the engine on such a box ------------------------------------------------------------------------------------------
def _open_wall_deck(solver, **grid):
    base = decks.blowout_wake()
    base.update(nz=20, n_steps=1, lo=(-3.0, -5.0, 1.2), hi=(5.0, 4.0, 6.0), nx=80, ny=72, beam_pos_mean=(0.6, -0.4, 0.0), field_bc=1)
    base.update(grid)
    return decks.predictor_corrector(base, 1.0e-4, 7, 0.0635) if solver else base


def _engine_against_oracle(api, oracle, deck, solver):      # (the comparison of test_open_field_boundary_slice_by_slice_vs_oracle)
    from hipace_amd._lib import COMPS, COMPS_PC
    names = COMPS_PC if solver else COMPS
    ge = api.SliceEngine(deck, tile_size=16, sort_period=5)
    ge.set_diagnostics(True)
    oe = oracle.Engine(deck)
    ge.begin_step()
    oe.begin_step()
    wall = 0.0
    for isl in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
        if isl % 5 == 0:
            gs, os_ = ge.slab(), oe.slab()
            for c in range(ge.ncomp):
                assert rel_err(gs[c], os_[c]) < 1e-9, (isl, names[c], rel_err(gs[c], os_[c]))
            g = (gs.shape[1] - deck["ny"]) // 2
            ipsi = list(names).index("Psi")
            wall = max(wall, np.abs(gs[ipsi][g, g:-g]).max() / np.abs(gs[ipsi]).max())
    gc, oc = ge.checksums(), oe.checksums()
    for k, v in oc.items():
        if v:
            assert abs(gc[k] - v) <= 1e-9 * abs(v), (k, gc[k], v)
    if solver:
        assert ge.pc_stats()[0] == oe.pc_stats()[0]
    else:
        assert ge.stats()["vcycles"] == oe.vcycles()
    return wall


@gpu
@pytest.mark.parametrize("solver", [0, 1], ids=["explicit", "predictor-corrector"])
def test_engine_on_an_off_centre_rectangular_box_vs_oracle(api, oracle, solver):
    """The deck of test_open_field_boundary_slice_by_slice_vs_oracle (tests/test_gpu_parity.py) on lo = (-3, -5), hi = (5, 4) with
    80 x 72 cells (dx = 0.1, dy = 0.125; the low-x wall the nearest) and 20 slices, under both Bx/By solvers with tile_size = 16:
    every slab component every fifth slice and the checksums against the oracle at 1e-9, equal V-cycle counts (explicit) and loop
    iterations (predictor-corrector)."""
    wall = _engine_against_oracle(api, oracle, _open_wall_deck(solver), solver)
    assert wall > 1e-3, wall      # the walls are open: Psi at the wall is not 0


@gpu
def test_engine_above_65536_cells_vs_oracle(api, oracle):
    """the same box at 288 x 264 cells, 4 slices, explicit solver: 76 032 cells (a second load slot in the moments) and 1104
    boundary points (five apply workgroups) inside the engine"""
    _engine_against_oracle(api, oracle, _open_wall_deck(0, nx=288, ny=264, nz=4), 0)
