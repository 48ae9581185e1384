"""Every kernel the size dispatch of hps_mg_create / hps_mg2_create can pick, against the oracle and against a plain float64
numpy restatement of hpmg's equation (tests/util.py, independent of the oracle).

hps_mg_create chooses per grid:
- the lower V (LOWV): k_lower_v3 from the first cell-centred level of at most 64 x 64 cells whose coarser levels fit 32 x 32,
  else k_lower_v<CC> from the first level of at most LOWV_MAX_CELLS, all levels below it in one workgroup's LDS; where that
  does not fit (no level is small enough, the coarsest one is large), the generic bottom: the coarsest level swept in global
  memory, the reference's CPU branch;
- the down-leg smoother of each level above it (TILES): TileSmall up to SMALL_TILE_CELLS cells, TileBig above; node-centred
  levels that form their right-hand side from the finer residual themselves on TileSmall or TileMid;
- the coefficient pyramid: k_acf_pyramid / k_nodal_acf_pyramid<np> for np = min(lowv_begin, NPYR_MAX) levels, k_restrict below.
Each case states what MultiGrid.info() must report, and test_every_kernel_of_the_dispatch_is_reached holds the table to the
lists below, so a change of the dispatch fails here instead of leaving a kernel without a test.

What a solve must match (each case cold and warm): the oracle's V-cycle count, solution to 1e-10 relative, resnorm to 1e-6;
rhs and chi bit-equal, the solution's guard cells equal to the oracle's.  Independently of the oracle: the returned resnorm is
max|r(phi)| of the returned solution (solve_doit copies cor[0], the iterate whose residual it measured, into sol:
HpMultiGrid.cpp:1380-1427) and meets the stopping target; and, up to DIRECT_MAX_CELLS, both phi and GSRB^4(phi) lie within
||A^-1|| ||r|| of the sparse direct solution."""
import numpy as np
import pytest

from tests.util import (G2, helmholtz1_direct, helmholtz1_gsrb4, helmholtz1_residual, rel_err)

pytestmark = pytest.mark.gpu

# what multigrid.hip can launch: the lower-V kinds, the down-leg tiles, the pyramid depths (both centrings), and its thresholds
LOWV = ("v3", "v-cc", "v-nodal", "bottom")
TILES = ("TileSmall", "TileBig", "TileSmall-pull", "TileMid-pull")
LOWV_MAX_CELLS, SMALL_TILE_CELLS, NPYR_MAX = 34 * 34, 300 * 300, 5
# multigrid2.hip
MG2_BOTTOMS = ("lower-v", "per-sweep")          # single-block: only a grid that cannot coarsen once reached it, now refused
MG2_TILES = ("single-block", "32x16", "64x32")
LOW2_MAX_CELLS, BIG_TILE_CELLS = 256, 256 * 256
DIRECT_MAX_CELLS = 300 * 300

S, B, SP, MP = TILES


def _i(lowv, nlev, lb, lds, tiles, pyr, restricts):
    return dict(nlev=nlev, lowv_begin=lb, lowv=lowv, lowv_lds=lds, tiles=tiles, pyramid=pyr, restricts=restricts)


def _expect(nx, ny, e):
    """the full info() of a table row: the centring by parity; node-centred level 1 pulls whenever it is a smoother level"""
    cc = nx % 2 == 0
    return dict(e, cc=cc, nodal_pull1=(not cc) and e["lowv_begin"] > 1)


# (dx, dy): the default cell, dy/dx = 1/4 and 4 (with point smoothing, cell-centred grids of smaller such cells take more
# than 200 V-cycles to 1e-4, in the reference as here)
D, AY, AX = (0.1, 0.1), (0.4, 0.1), (0.1, 0.4)
# (nx, ny, (dx, dy), expected info())
CASES = [
    # k_lower_v3: top level exactly 64 x 64 (128^2, 256^2) or 32 x 32 (64^2); lowv_begin 6 (k_restrict + k_level_cinv below
    # the pyramid); 640 x 576 has level 1 at 320 x 288 cells (TileBig), 600^2 below has it at exactly 300^2 (TileSmall)
    (64, 64, D, _i("v3", 6, 1, 24480, (S,), 1, 0)),
    (128, 128, D, _i("v3", 7, 1, 87072, (S,), 1, 0)),
    (256, 256, D, _i("v3", 8, 2, 87072, (S, S), 2, 0)),
    (512, 512, D, _i("v3", 9, 3, 87072, (B, S, S), 3, 0)),
    (640, 576, D, _i("v3", 7, 4, 31072, (B, B, S, S), 4, 0)),
    (4096, 2048, D, _i("v3", 11, 6, 45984, (B, B, B, B, S, S), 5, 1)),
    # k_lower_v<true>: coarsening stops at 66 x 33; 64 B under the LDS limit; 1-cell-wide coarse levels
    (132, 66, D, _i("v-cc", 2, 1, 139392, (S,), 1, 0)),
    (426, 24, D, _i("v-cc", 2, 1, 163584, (S,), 1, 0)),
    (2048, 16, D, _i("v-cc", 4, 3, 32768, (S, S, S), 3, 0)),
    (4, 2048, D, _i("v-cc", 2, 1, 131072, (S,), 1, 0)),
    # k_lower_v<false>: pyramid depths 1 .. 5, and 5 + k_restrict (2047^2); 13 x 637 needs exactly 163 840 B
    (7, 7, D, _i("v-nodal", 2, 1, 1600, (S,), 1, 0)),
    (9, 9, D, _i("v-nodal", 2, 1, 2304, (S,), 1, 0)),
    (15, 15, D, _i("v-nodal", 3, 1, 6784, (S,), 1, 0)),
    (127, 127, D, _i("v-nodal", 6, 2, 94976, (S, SP), 2, 0)),
    (255, 127, D, _i("v-nodal", 6, 3, 48576, (S, SP, SP), 3, 0)),
    (255, 255, D, _i("v-nodal", 7, 3, 94976, (S, SP, SP), 3, 0)),
    (511, 511, D, _i("v-nodal", 8, 4, 94976, (B, SP, SP, SP), 4, 0)),
    (1023, 1023, D, _i("v-nodal", 9, 5, 94976, (B, MP, SP, SP, SP), 5, 0)),
    (2047, 2047, (16 / 2047, 16 / 2047), _i("v-nodal", 10, 6, 94976, (B, MP, B, SP, SP, SP), 5, 1)),
    (13, 637, D, _i("v-nodal", 2, 1, 163840, (S,), 1, 0)),
    (63, 67, D, _i("v-nodal", 3, 1, 93504, (S,), 1, 0)),      # level 1: 33 x 35 = 1155 nodes, one under LOWV_MAX_CELLS
    # the generic bottom: 64 B over the limit (394 x 26), coarsening that stops early in either centring; level 0 at
    # exactly 300^2 cells (TileSmall) and above (302 x 300, 299^2 nodes); node-centred level 1 at 299^2 nodes (595^2:
    # TileSmall, pulling) and 301^2 (599^2: TileMid)
    (394, 26, D, _i("bottom", 2, 1, 0, (S,), 1, 0)),
    (300, 300, D, _i("bottom", 3, 2, 0, (S, S), 2, 0)),
    (302, 300, D, _i("bottom", 2, 1, 0, (B,), 1, 0)),
    (600, 600, D, _i("bottom", 4, 3, 0, (B, S, S), 3, 0)),
    (1000, 1000, D, _i("bottom", 4, 3, 0, (B, B, S), 3, 0)),
    (1000, 512, D, _i("bottom", 4, 3, 0, (B, B, S), 3, 0)),
    (129, 129, D, _i("bottom", 2, 1, 0, (S,), 1, 0)),
    (257, 257, D, _i("bottom", 2, 1, 0, (S,), 1, 0)),
    (297, 297, D, _i("bottom", 2, 1, 0, (S,), 1, 0)),
    (299, 299, D, _i("bottom", 3, 2, 0, (B, SP), 2, 0)),
    (513, 513, D, _i("bottom", 2, 1, 0, (B,), 1, 0)),
    (595, 595, D, _i("bottom", 3, 2, 0, (B, SP), 2, 0)),
    (599, 599, D, _i("bottom", 4, 3, 0, (B, MP, SP), 3, 0)),
    # anisotropic cells on one shape of v3, v-nodal and bottom
    (128, 128, AY, _i("v3", 7, 1, 87072, (S,), 1, 0)), (128, 128, AX, _i("v3", 7, 1, 87072, (S,), 1, 0)),
    (255, 127, AY, _i("v-nodal", 6, 3, 48576, (S, SP, SP), 3, 0)), (255, 127, AX, _i("v-nodal", 6, 3, 48576, (S, SP, SP), 3, 0)),
    (300, 300, AY, _i("bottom", 3, 2, 0, (S, S), 2, 0)), (300, 300, AX, _i("bottom", 3, 2, 0, (S, S), 2, 0)),
]
COLD_ONLY = {(4096, 2048), (2047, 2047)}      # (the oracle takes seconds per solve; test_multigrid_solve1 has 2047^2 warm)
# one shape of each lower-V kind for the coefficient edges and the back-to-back solves
ONE_OF_EACH = {"v3": (128, 128, "v3"), "v-cc": (132, 66, "v-cc"), "v-nodal": (255, 127, "v-nodal"), "bottom": (300, 300, "bottom"),
               "bottom-nodal": (129, 129, "bottom")}


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


def make_slab(nx, ny, seed, chi="uniform", guess=None):
    """(5, ny + 2g, nx + 2g): sol (random guard cells: the solve must neither read nor write them), rhs, chi.  chi "uniform":
    [0.5, 1.5] as test_multigrid_solve1; "zero": a pure Poisson solve; "wide": log-uniform over 1e-3 .. 1e3."""
    g = G2
    rng = np.random.default_rng(seed)
    slab = np.zeros((5, ny + 2 * g, nx + 2 * g))
    slab[0:2] = rng.standard_normal((2, ny + 2 * g, nx + 2 * g))
    slab[0:2, g:-g, g:-g] = 0.0 if guess is None else guess
    slab[2:4] = rng.standard_normal((2, ny + 2 * g, nx + 2 * g))
    slab[4] = {"uniform": lambda: 0.5 + rng.random((ny + 2 * g, nx + 2 * g)),
               "zero": lambda: np.zeros((ny + 2 * g, nx + 2 * g)),
               "wide": lambda: 10.0 ** rng.uniform(-3, 3, (ny + 2 * g, nx + 2 * g))}[chi]()
    return slab


def oracle_solve(oracle, slab, nx, ny, dx, dy, tol_rel=1e-4):
    sol = np.ascontiguousarray(slab[0:2]).copy()
    it, rn = oracle.mg_solve1(sol, np.ascontiguousarray(slab[2:4]), np.ascontiguousarray(slab[4]), nx, ny, G2, dx, dy, tol_rel=tol_rel)
    assert it >= 0, "the oracle did not converge"
    return it, rn, sol


_DIRECT = {}


def check_solve(out, slab, it, rn, ref, nx, ny, dx, dy, tol_rel=1e-4, tol_abs=2.2250738585072014e-308):
    """The GPU's result `out` of a solve of `slab` (returned it, rn) against the oracle's `ref` = (it, rn, sol) and against
    hpmg's equation in numpy.  Returns (error vs the oracle, error vs the direct solve or None)."""
    g = G2
    it_ref, rn_ref, sol_ref = ref
    cc = nx % 2 == 0
    inner = (slice(None), slice(g, -g), slice(g, -g))
    assert it == it_ref, (it, it_ref)
    err = rel_err(out[0:2][inner], sol_ref[inner])
    assert err < 1e-10, err
    assert abs(rn - rn_ref) <= 1e-6 * rn_ref, (rn, rn_ref)
    assert np.array_equal(out[2:5], slab[2:5]), "rhs or chi was written"
    gs, go = sol_ref.copy(), out[0:2].copy()
    gs[inner] = 0
    go[inner] = 0
    assert np.array_equal(go, gs), "a guard cell of the solution differs from the oracle's"
    phi, rhs, acf, phi0 = out[0:2][inner], slab[2:4][inner], slab[4][g:-g, g:-g], slab[0:2][inner]
    # the stopping rule of solve_doit on the numpy operator: resnorm is the residual of the returned iterate
    r = np.abs(helmholtz1_residual(phi, rhs, acf, dx, dy, cc)).max()
    r0 = np.abs(helmholtz1_residual(helmholtz1_gsrb4(phi0, rhs, acf, dx, dy, cc), rhs, acf, dx, dy, cc)).max()
    target = max(tol_abs, tol_rel * max(np.abs(rhs).max(), r0))
    assert abs(r - rn) <= 1e-6 * rn, (r, rn)
    assert r <= target * (1 + 1e-9), (r, target)
    derr = None
    if nx * ny <= DIRECT_MAX_CELLS:
        key = (nx, ny, dx, dy, rhs.tobytes(), acf.tobytes())
        if key not in _DIRECT:
            _DIRECT.clear()
            _DIRECT[key] = helmholtz1_direct(rhs, acf, dx, dy, cc)
        exact, ainv = _DIRECT[key]
        x4 = helmholtz1_gsrb4(phi, rhs, acf, dx, dy, cc)
        for x in (phi, x4):
            bound = ainv * np.abs(helmholtz1_residual(x, rhs, acf, dx, dy, cc)).max()
            e = np.abs(x - exact).max()
            assert e <= bound * (1 + 1e-9), (e, bound)
        derr = rel_err(phi, exact)
    return err, derr


def gpu_solve(api, slab, nx, ny, dx, dy, mg=None, tol_rel=1e-4):
    f = api.Fields(nx, ny, G2, 5, data=slab)
    it, rn = (mg or api.MultiGrid(nx, ny, dx, dy)).solve1(f, 0, 2, 4, tol_rel=tol_rel)
    return f.numpy(), it, rn


@pytest.mark.parametrize("case,warm", [(c, w) for c in CASES for w in (False, True) if not (w and c[:2] in COLD_ONLY)],
                         ids=[_id(c) + ("-warm" if w else "-cold") for c in CASES for w in (False, True) if not (w and c[:2] in COLD_ONLY)])
def test_solve_on_every_dispatch_path(api, oracle, case, warm):
    nx, ny, (dx, dy), e = case
    mg = api.MultiGrid(nx, ny, dx, dy)
    assert mg.info() == _expect(nx, ny, e)
    rng = np.random.default_rng(nx + 7 * ny)
    slab = make_slab(nx, ny, nx * 31 + ny, guess=0.05 * rng.standard_normal((2, ny, nx)) if warm else None)
    ref = oracle_solve(oracle, slab, nx, ny, dx, dy)
    assert ref[0] >= 1
    out, it, rn = gpu_solve(api, slab, nx, ny, dx, dy, mg)
    err, derr = check_solve(out, slab, it, rn, ref, nx, ny, dx, dy)
    print(f"{_id(case)} {e['lowv']} {'warm' if warm else 'cold'} V-cycles {it} vs oracle {err:.1e}"
          + ("" if derr is None else f" vs direct {derr:.1e}"))


@pytest.mark.parametrize("chi", ["zero", "wide", "converged"])
@pytest.mark.parametrize("kind", list(ONE_OF_EACH))
def test_coefficient_edges(api, oracle, kind, chi):
    """chi = 0 (the vacuum ahead of a beam: a pure Poisson solve), chi over six decades, and a warm start from the oracle's
    converged solution, which takes 0 V-cycles: solve1_finish copies cor[0], the smoothed initial guess (k_copy2)."""
    nx, ny, lowv = ONE_OF_EACH[kind]
    dx, dy = D
    mg = api.MultiGrid(nx, ny, dx, dy)
    assert mg.info()["lowv"] == lowv
    slab = make_slab(nx, ny, nx + ny, chi="uniform" if chi == "converged" else chi)
    if chi == "converged":
        slab[0:2] = oracle_solve(oracle, slab, nx, ny, dx, dy)[2]
    ref = oracle_solve(oracle, slab, nx, ny, dx, dy)
    assert (ref[0] == 0) == (chi == "converged")
    out, it, rn = gpu_solve(api, slab, nx, ny, dx, dy, mg)
    err, derr = check_solve(out, slab, it, rn, ref, nx, ny, dx, dy)
    print(f"{kind} {nx}x{ny} chi={chi} V-cycles {it} vs oracle {err:.1e} vs direct {derr:.1e}")


@pytest.mark.parametrize("kind", list(ONE_OF_EACH))
def test_one_handle_back_to_back(api, oracle, kind):
    """A hard solve (1e-8), an easy one (1e-4 from a nearby guess), one converged on entry, on one handle: the speculation depth
    is the previous solve's V-cycle count, so the later solves enqueue V-cycles they do not need -- those must change nothing."""
    nx, ny, lowv = ONE_OF_EACH[kind]
    dx, dy = D
    mg = api.MultiGrid(nx, ny, dx, dy)
    assert mg.info()["lowv"] == lowv
    hard = make_slab(nx, ny, 3 * nx + ny)
    ref_hard = oracle_solve(oracle, hard, nx, ny, dx, dy, tol_rel=1e-8)
    easy = make_slab(nx, ny, 5 * nx + ny)
    near = oracle_solve(oracle, easy, nx, ny, dx, dy, tol_rel=1e-3)[2]
    easy[0:2] = near + 1e-3 * np.random.default_rng(nx).standard_normal(near.shape)
    ref_easy = oracle_solve(oracle, easy, nx, ny, dx, dy)
    done = make_slab(nx, ny, 7 * nx + ny)
    done[0:2] = oracle_solve(oracle, done, nx, ny, dx, dy, tol_rel=1e-6)[2]
    ref_done = oracle_solve(oracle, done, nx, ny, dx, dy)
    its = []
    for slab, ref, tol in ((hard, ref_hard, 1e-8), (easy, ref_easy, 1e-4), (done, ref_done, 1e-4)):
        out, it, rn = gpu_solve(api, slab, nx, ny, dx, dy, mg, tol_rel=tol)
        check_solve(out, slab, it, rn, ref, nx, ny, dx, dy, tol_rel=tol)
        its.append(it)
    assert its[0] > its[1] > its[2] == 0, its
    print(f"{kind} {nx}x{ny} V-cycles {its}")


@pytest.mark.parametrize("nx,ny", [(300, 300), (129, 129)])
def test_solve1_fabs_on_the_generic_bottom(api, oracle, nx, ny):
    """hps_mg_solve1_fabs with guard widths 1 (sol), 3 (rhs) and 2 (acoef) on grids whose coarsest level is swept in global
    memory."""
    import torch
    dx, dy = D
    mg = api.MultiGrid(nx, ny, dx, dy)
    assert mg.info()["lowv"] == "bottom"
    slab = make_slab(nx, ny, nx, guess=0.05 * np.random.default_rng(nx).standard_normal((2, ny, nx)))
    slab[0:2] = np.pad(slab[0:2, G2:-G2, G2:-G2], ((0, 0), (G2, G2), (G2, G2)))
    ref = oracle_solve(oracle, slab, nx, ny, dx, dy)
    gs, gr = 1, 3
    fs = api.Fields(nx, ny, gs, 2)
    fs.t[:, gs:-gs, gs:-gs] = torch.tensor(slab[0:2, G2:-G2, G2:-G2], device="cuda")
    fr = api.Fields(nx, ny, gr, 2)
    fr.t[:, gr:-gr, gr:-gr] = torch.tensor(slab[2:4, G2:-G2, G2:-G2], device="cuda")
    fa = api.Fields(nx, ny, G2, 1, data=slab[4:5])
    it, rn = mg.solve1_fabs(fs, fr, fa)
    out = np.zeros_like(slab)
    out[0:2] = slab[0:2]
    out[0:2, G2:-G2, G2:-G2] = fs.numpy()[:, gs:-gs, gs:-gs]
    out[2:5] = slab[2:5]
    check_solve(out, slab, it, rn, ref, nx, ny, dx, dy)
    assert np.all(fs.numpy()[:, 0] == 0) and np.all(fs.numpy()[:, :, -1] == 0)      # guard cells untouched
    assert np.array_equal(fr.numpy()[:, gr:-gr, gr:-gr], slab[2:4, G2:-G2, G2:-G2])


def test_refusals(api):
    """Grids hps_mg_create refuses, as the reference asserts: parity mismatch, too small to coarsen once, and planes beyond
    the 32-bit byte offsets of the kernels (refused before anything is allocated)."""
    def refused(nx, ny, needle):
        with pytest.raises(RuntimeError) as ei:
            api.MultiGrid(nx, ny, 0.1, 0.1)
        assert needle in str(ei.value), str(ei.value)
    refused(64, 63, "parity")
    for n in (2, 3, 5):
        refused(n, n, "too small to coarsen")
    refused(11570, 11570, "2^27")      # (11570 + 16)^2 > 2^27: the kernels would need 7.5 GB of planes
    for nx, ny in ((2, 2), (6, 2), (2, 4096)):
        with pytest.raises(RuntimeError) as ei:
            api.MultiGrid2(nx, ny, 0.1, 0.1)
        assert "too small to coarsen" in str(ei.value)


# ---- system type 2 (multigrid2.hip) ------------------------------------------------------------------------------------
# (nx, ny, expected info(): low_top, bottom, tiles of the levels above the bottom part)
CASES2 = [
    (96, 64, dict(nlev=6, low_top=3, bottom="lower-v", tiles=("32x16", "32x16", "32x16"))),
    (16, 16, dict(nlev=4, low_top=1, bottom="lower-v", tiles=("single-block",))),
    (256, 256, dict(nlev=8, low_top=4, bottom="lower-v", tiles=("32x16", "32x16", "32x16", "32x16"))),
    (258, 256, dict(nlev=2, low_top=-1, bottom="per-sweep", tiles=("64x32",))),
    (512, 256, dict(nlev=8, low_top=5, bottom="lower-v", tiles=("64x32", "32x16", "32x16", "32x16", "32x16"))),
    (300, 300, dict(nlev=3, low_top=-1, bottom="per-sweep", tiles=("64x32", "32x16"))),
    (4, 512, dict(nlev=2, low_top=-1, bottom="per-sweep", tiles=("32x16",))),
]


@pytest.mark.parametrize("nx,ny,expect", CASES2, ids=[f"{nx}x{ny}" for nx, ny, _ in CASES2])
def test_multigrid2_dispatch_vs_oracle(api, oracle, nx, ny, expect):
    """As test_multigrid2_solve2_vs_oracle, on both sides of BIG_TILE_CELLS and on the generic bottom (one k2_sweeps launch
    per sweep).  No accepted grid reaches the single-block generic bottom: a coarsest level of at most LOW2_MAX_CELLS always
    fits k2_lower_v once the grid coarsens at least once."""
    import torch
    mg = api.MultiGrid2(nx, ny, 0.11, 0.13)
    assert mg.info() == expect
    rng = np.random.default_rng(nx + ny)
    rhs = rng.standard_normal((2, ny, nx))
    ar = 3.0 + rng.random((ny, nx))
    sol = 0.02 * rng.standard_normal((2, ny, nx))
    want = sol.copy()
    it_ref, rn_ref = oracle.mg_solve2(want, rhs, ar, -7.5, 0.11, 0.13, tol_rel=1e-6)
    assert it_ref >= 1
    t = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda").contiguous()
    tsol = t(sol)
    it, rn = mg.solve2(tsol, t(rhs), t(ar), t(np.array([-7.5])), tol_rel=1e-6)
    assert it == it_ref
    assert rel_err(tsol.cpu().numpy(), want) < 1e-10
    assert abs(rn - rn_ref) <= 1e-6 * rn_ref
    print(f"mg2 {nx}x{ny} {expect['bottom']} V-cycles {it}")


def test_every_kernel_of_the_dispatch_is_reached(api):
    """The tables above reach every lower-V kind, every down-leg tile, every pyramid depth of both centrings with and without
    trailing k_restrict launches, both sides of LOWV's LDS limit and of SMALL_TILE_CELLS -- as the solvers report it."""
    got = {}
    for nx, ny, (dx, dy), _ in CASES:
        got[(nx, ny)] = api.MultiGrid(nx, ny, dx, dy).info()
    assert {i["lowv"] for i in got.values()} == set(LOWV)
    assert {t for i in got.values() for t in i["tiles"]} == set(TILES)
    for cc in (True, False):
        assert {i["pyramid"] for i in got.values() if i["cc"] == cc} == set(range(1, NPYR_MAX + 1)), cc
        assert any(i["restricts"] > 0 for i in got.values() if i["cc"] == cc), cc
    assert any(i["lowv"] == "v3" and i["lowv_begin"] > NPYR_MAX for i in got.values())      # k_level_cinv
    assert {i["lowv"] for i in got.values() if not i["cc"]} >= {"v-nodal", "bottom"}
    assert {i["lowv"] for i in got.values() if i["cc"]} >= {"v3", "v-cc", "bottom"}
    lds = [i["lowv_lds"] for i in got.values() if i["lowv"] in ("v-cc", "v-nodal")]
    assert max(lds) == 163840 and 163584 in lds
    # level 0 on both sides of SMALL_TILE_CELLS (exactly 300^2 cells; 302 x 300; 299^2 and 301^2 nodes), then level 1
    assert [got[s]["tiles"][0] for s in ((300, 300), (302, 300), (297, 297), (299, 299))] == ["TileSmall", "TileBig"] * 2
    assert got[(600, 600)]["tiles"][1] == "TileSmall" and got[(640, 576)]["tiles"][1] == "TileBig"
    assert got[(595, 595)]["tiles"][1] == "TileSmall-pull" and got[(599, 599)]["tiles"][1] == "TileMid-pull"
    got2 = {(nx, ny): api.MultiGrid2(nx, ny, 0.1, 0.1).info() for nx, ny, _ in CASES2}
    assert {i["bottom"] for i in got2.values()} == set(MG2_BOTTOMS)
    assert {t for i in got2.values() for t in i["tiles"]} == set(MG2_TILES)


@pytest.mark.parametrize("tile_size", [0, 16])
@pytest.mark.parametrize("n", [300, 129])
def test_engine_on_a_grid_with_the_generic_bottom(api, oracle, n, tile_size):
    """blowout_wake at n x n cells, whose Bx/By multigrid takes the generic bottom, slice by slice against the oracle as
    test_engine_slice_by_slice_vs_oracle: fields to 1e-9, equal V-cycle counts.  A component the oracle has exactly 0 (the
    transverse fields ahead of the beam, where the neutral plasma's deposits cancel: the GPU's atomics leave ~1e-17 there) must
    be 0 to 1e-12 of the slice's largest value."""
    from hipace_amd import decks
    from hipace_amd._lib import COMPS
    deck = decks.blowout_wake()
    deck.update(nx=n, ny=n, nz=6, n_steps=1)
    ge = api.SliceEngine(deck, tile_size=tile_size, sort_period=5)
    oe = oracle.Engine(deck)
    ge.begin_step()
    oe.begin_step()
    for isl in range(deck["nz"] - 1, -1, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
        gs, os_ = ge.slab(), oe.slab()
        for c in range(ge.ncomp):
            err = rel_err(gs[c], os_[c]) if np.any(os_[c]) else np.abs(gs[c]).max() / np.abs(os_).max()
            assert err < (1e-9 if np.any(os_[c]) else 1e-12), (isl, COMPS[c], err)
    assert ge.stats()["vcycles"] == oe.vcycles() > 0
    print(f"engine {n}^2 tile_size {tile_size}: V-cycles {oe.vcycles()}")
