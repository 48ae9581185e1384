"""Every kernel the size dispatch of hps_poisson_create can pick, against a numpy DST-I solve (tests/util.py, independent of the
oracle), up to 2047^2.

The dispatch chooses twice.  Along x: an own DST kernel of length N = nx + 1 (OWN_X, the lengths of g_dst_impls in
poisson.hip), else the dense product for nx <= 512 and ny <= 512, else rocFFT.  Along y: k_tridiag_y<M, ..> by ny (TRI_ROWS,
find_tri_impl), and rocFFT for ny > 2048 whatever nx is.  Every solve states the kernels it reaches through
FFTPoissonSolver.info(), and test_every_kernel_of_the_dispatch_is_reached holds the table to the two lists, so a change of the
dispatch fails here instead of leaving a kernel without a test.

Tolerance 1e-12 relative to the largest value of the reference, as test_poisson: the reference and the kernels are both
O(log n) eps transforms; the tall anisotropic grids are the ones where LU factors of the y solve rounded from double
instead of long double lose three digits (1.5e-11 at 64 x 2000, dy/dx = 1/50)."""
import ctypes as C

import numpy as np
import pytest

from tests.util import G2, poisson_dirichlet_ref, rel_err

pytestmark = pytest.mark.gpu

# g_dst_impls: own DST lengths N = nx + 1 and their kernel (k_dst_rows_sym<N1, N2> / k_dst_rows_pow2<log2 N>)
OWN_X = {1025: "own-sym", 513: "own-sym", 129: "own-sym", 65: "own-sym", 33: "own-sym", 99: "own-sym", 77: "own-sym",
         2048: "own-pow2", 1024: "own-pow2", 512: "own-pow2", 256: "own-pow2", 128: "own-pow2", 64: "own-pow2"}
# find_tri_impl: largest ny of each k_tridiag_y<M, ..>, and its M
TRI_ROWS = {256: 4, 512: 8, 1024: 16, 2048: 32}

D, A1, A50 = (0.25, 0.2), (1.0, 0.02), (0.02, 1.0)          # (dx, dy): the suite's default cell, dy/dx = 1/50 and 50
# (nx, ny, (dx, dy), expected info(): backend, x_len, tri_rows)
SINGLE = [
    # own symmetric kernels: every length, every tridiagonal shape
    (1024, 1025, D, ("own-sym", 1025, 32)), (1024, 2000, D, ("own-sym", 1025, 32)), (512, 513, D, ("own-sym", 513, 16)),
    (128, 257, D, ("own-sym", 129, 8)), (64, 2048, D, ("own-sym", 65, 32)), (32, 31, D, ("own-sym", 33, 4)),
    (98, 40, D, ("own-sym", 99, 4)), (98, 1024, D, ("own-sym", 99, 16)), (76, 76, D, ("own-sym", 77, 4)),
    (76, 512, D, ("own-sym", 77, 8)),
    # own power-of-two kernels
    (2047, 2047, (16 / 2047, 16 / 2047), ("own-pow2", 2048, 32)), (2047, 3, D, ("own-pow2", 2048, 4)),
    (1023, 1024, D, ("own-pow2", 1024, 16)), (511, 512, D, ("own-pow2", 512, 8)), (255, 256, D, ("own-pow2", 256, 4)),
    (127, 513, D, ("own-pow2", 128, 16)), (63, 2, D, ("own-pow2", 64, 4)), (63, 1025, D, ("own-pow2", 64, 32)),
    # dense product (no own length, nx <= 512, ny <= 512): tiny grids, K and M, N not multiples of the 32-deep slabs
    (2, 2, D, ("dense", 0, 4)), (3, 7, D, ("dense", 0, 4)), (2, 300, D, ("dense", 0, 8)), (33, 33, D, ("dense", 0, 4)),
    (33, 257, D, ("dense", 0, 8)), (300, 256, D, ("dense", 0, 4)), (300, 512, D, ("dense", 0, 8)),
    (510, 97, D, ("dense", 0, 4)), (510, 510, D, ("dense", 0, 8)),
    # rocFFT: past the dense limits, and ny > 2048 with an own length along x
    (300, 513, D, ("rocfft", 0, 0)), (513, 64, D, ("rocfft", 0, 0)), (600, 520, D, ("rocfft", 0, 0)),
    (63, 2049, D, ("rocfft", 0, 0)), (64, 2100, D, ("rocfft", 0, 0)),
    # anisotropic cells: the LU factors of the y solve depend on (dy/dx)^2
    (98, 40, A1, ("own-sym", 99, 4)), (98, 40, A50, ("own-sym", 99, 4)),
    (255, 256, A1, ("own-pow2", 256, 4)), (255, 256, A50, ("own-pow2", 256, 4)),
    (300, 300, A1, ("dense", 0, 8)), (300, 300, A50, ("dense", 0, 8)),
    (64, 2000, A1, ("own-sym", 65, 32)), (64, 2000, (1.0, 0.01), ("own-sym", 65, 32)), (64, 2000, A50, ("own-sym", 65, 32)),
    (600, 520, A1, ("rocfft", 0, 0)),
]


def _id(case):
    nx, ny, (dx, dy), _ = case
    return f"{nx}x{ny}" + ("" if (dx, dy) == D else f"-dx{dx:g}-dy{dy:g}")


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


def _sentinel_slab(rng, ncomp, ny, nx, ng):
    """A slab whose every value is random: anything the solve writes outside its targets shows."""
    return rng.standard_normal((ncomp, ny + 2 * ng, nx + 2 * ng))


def _check_targets(out, before, comps, refs, ng, tol=1e-12):
    """Interior of comps[b] equal to refs[b]; its guard cells and every other component bit-equal to `before`."""
    errs = []
    for c, ref in zip(comps, refs):
        interior = (slice(ng, -ng), slice(ng, -ng))
        errs.append(rel_err(out[c][interior], ref))
        g_out, g_in = out[c].copy(), before[c].copy()
        g_out[interior] = 0
        g_in[interior] = 0
        assert np.array_equal(g_out, g_in), f"component {c}: a guard cell was written"
    others = [c for c in range(out.shape[0]) if c not in comps]
    assert np.array_equal(out[others], before[others]), "a component that is not a target was written"
    assert max(errs) < tol, errs
    return max(errs)


@pytest.mark.parametrize("case", SINGLE, ids=_id)
def test_single_solve_vs_numpy_dst(api, case):
    import torch
    nx, ny, (dx, dy), expect = case
    rng = np.random.default_rng(nx * 10007 + ny)
    rhs = rng.standard_normal((ny, nx))
    ps = api.FFTPoissonSolver(nx, ny, dx, dy)
    assert ps.info() == expect
    ps.StagingArea().copy_(torch.as_tensor(rhs))
    before = _sentinel_slab(rng, 3, ny, nx, G2)
    f = api.Fields(nx, ny, G2, 3, data=before)
    ps.SolvePoissonEquation(f, 1)
    torch.cuda.synchronize()
    err = _check_targets(f.numpy(), before, [1], [poisson_dirichlet_ref(rhs, dx, dy)], G2)
    print(f"{_id(case)} {expect} rel. error {err:.2e}")


# (expected backend, nx, ny): an odd and an even ny per back-end -- with odd ny the own kernels' two-row transforms pair the
# last row of one plane with the first row of the next
BATCH = [("own-sym", 98, 41), ("own-sym", 64, 48), ("own-pow2", 127, 65), ("own-pow2", 63, 64),
         ("dense", 33, 31), ("dense", 300, 40), ("rocfft", 600, 33), ("rocfft", 520, 48)]
BATCH_COMPS = [6, 2, 4, 0]      # out of order, no two adjacent


def _solve_batch(api, ps, nb, staging, f, comps):
    from hipace_amd import _lib
    cc = (C.c_int * len(comps))(*comps)
    return _lib.lib().hps_poisson_solve_batch(ps._h, nb, C.c_void_p(staging.data_ptr()), f.struct(), cc, None)


@pytest.mark.parametrize("nb", [1, 2, 3, 4])
@pytest.mark.parametrize("backend,nx,ny", BATCH, ids=[f"{b}-{nx}x{ny}" for b, nx, ny in BATCH])
def test_batched_solves_vs_numpy_dst(api, backend, nx, ny, nb):
    """hps_poisson_solve_batch: nb planes into components out of order, slabs with guard width 1 or 3; every plane equal
    to its own single-plane reference, everything else untouched."""
    import torch
    from hipace_amd import _lib
    ng = 1 if nb % 2 else 3
    dx, dy = 0.3, 0.2
    rng = np.random.default_rng(1000 * nb + nx + 7 * ny)
    rhs = rng.standard_normal((nb, ny, nx))
    ps = api.FFTPoissonSolver(nx, ny, dx, dy)
    assert ps.info()[0] == backend
    st = torch.as_tensor(rhs).cuda().contiguous()
    before = _sentinel_slab(rng, 7, ny, nx, ng)
    f = api.Fields(nx, ny, ng, 7, data=before)
    comps = BATCH_COMPS[:nb]
    _lib.check(_solve_batch(api, ps, nb, st, f, comps))
    torch.cuda.synchronize()
    err = _check_targets(f.numpy(), before, comps, [poisson_dirichlet_ref(r, dx, dy) for r in rhs], ng)
    print(f"batch {backend} {nx}x{ny} nb={nb} ng={ng} {ps.info()} rel. error {err:.2e}")


@pytest.mark.parametrize("backend,nx,ny", BATCH[::2], ids=[b for b, _, _ in BATCH[::2]])
def test_batch_of_0_or_5_planes_is_refused(api, backend, nx, ny):
    import torch
    from hipace_amd import _lib
    ps = api.FFTPoissonSolver(nx, ny, 0.3, 0.2)
    assert ps.info()[0] == backend
    st = torch.ones((5, ny, nx), dtype=torch.float64, device="cuda")
    before = _sentinel_slab(np.random.default_rng(5), 7, ny, nx, G2)
    f = api.Fields(nx, ny, G2, 7, data=before)
    for nb in (0, 5):
        assert _solve_batch(api, ps, nb, st, f, [6, 2, 4, 0, 1]) != 0
        assert "1..4" in _lib.lib().hps_last_error().decode()
    torch.cuda.synchronize()
    assert np.array_equal(f.numpy(), before)


def test_every_kernel_of_the_dispatch_is_reached(api):
    """The table above reaches every own x length, every tridiagonal shape on both sides of its threshold, the dense
    product in each y band it takes, and rocFFT both ways -- as the solvers report it, not as the table claims."""
    reached = {}
    for nx, ny, (dx, dy), _ in SINGLE:
        reached[(nx, ny)] = api.FFTPoissonSolver(nx, ny, dx, dy).info()
    got = set(reached.values())
    assert {(b, n) for b, n, _ in got if n} == {(b, n) for n, b in OWN_X.items()}
    assert {m for _, _, m in got} == set(TRI_ROWS.values()) | {0}
    assert {b for b, _, _ in got} == {"own-sym", "own-pow2", "dense", "rocfft"}
    assert {m for b, _, m in got if b == "dense"} == {TRI_ROWS[256], TRI_ROWS[512]}
    limits = sorted(TRI_ROWS)
    for i, lim in enumerate(limits):
        above = TRI_ROWS[limits[i + 1]] if i + 1 < len(limits) else 0
        assert any(ny == lim and r[2] == TRI_ROWS[lim] for (nx, ny), r in reached.items()), lim
        assert any(ny == lim + 1 and r[2] == above for (nx, ny), r in reached.items()), lim + 1
    assert any(r[0] == "rocfft" and nx + 1 in OWN_X for (nx, ny), r in reached.items())      # ny > 2048 beats an own length
    assert any(r[0] == "rocfft" and nx > 512 and nx + 1 not in OWN_X for (nx, ny), r in reached.items())
