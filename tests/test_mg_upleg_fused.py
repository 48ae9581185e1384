"""The up-leg of the mid levels 1 .. 3 of a V-cycle in one launch (k_up_fused, HPS_MG_UP_FUSED, default 1) against one launch
per level (=0).

A workgroup that owns a level-1 tile smooths the level-3 cells under it in LDS, then the level-2 cells, then its tile; the
per-cell update is the one expression (gs_cell) the level-by-level smoother uses, with its fused multiply-add spelled out.
The multigrid has no floating-point atomics (its norms are integer maxima), so a solve is reproducible bit for bit and every
operator-level comparison here is exact: solution planes, V-cycle count and final norm.

MultiGrid.upleg_fused_levels() says how many mid levels a handle fuses (0: none); the switch is read when the handle is
created.  Fused are levels 1 .. min(3, lowv_begin - 1) of cell-centred grids whose lower V is k_lower_v3 and starts at level 3
or deeper; level 1's tile shape is the level-by-level smoother's (64 x 32 above 300^2 cells, else 32 x 16).
"""
import os

import numpy as np
import pytest

from hipace_amd import decks

pytestmark = pytest.mark.gpu

G = 2
D = (0.1, 0.1)


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


class _switch:
    """HPS_MG_UP_FUSED in the environment while a solver or an engine is created"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("HPS_MG_UP_FUSED")
        os.environ["HPS_MG_UP_FUSED"] = self.value

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["HPS_MG_UP_FUSED"]
        else:
            os.environ["HPS_MG_UP_FUSED"] = self.old


def make_mg(api, nx, ny, switch):
    with _switch(switch):
        return api.MultiGrid(nx, ny, *D)


def make_slab(nx, ny, seed, chi_seed=None, guess=None):
    """(5, ny + 2g, nx + 2g): sol, rhs (fixed pseudo-random), a positive coefficient plane in [0.5, 1.5]"""
    rng = np.random.default_rng(seed)
    slab = np.zeros((5, ny + 2 * G, nx + 2 * G))
    slab[0:2] = rng.standard_normal((2, ny + 2 * G, nx + 2 * G))
    slab[0:2, G:-G, G:-G] = 0.0 if guess is None else guess
    slab[2:4] = rng.standard_normal((2, ny + 2 * G, nx + 2 * G))
    slab[4] = 0.5 + np.random.default_rng(seed + 1000 if chi_seed is None else chi_seed).random((ny + 2 * G, nx + 2 * G))
    return slab


def solve(api, mg, slab, tol_rel=1e-4):
    nx, ny = slab.shape[2] - 2 * G, slab.shape[1] - 2 * G
    f = api.Fields(nx, ny, G, 5, data=slab)
    it, rn = mg.solve1(f, 0, 2, 4, tol_rel=tol_rel)
    return f.numpy(), it, rn


def same(a, b):
    """two solves: planes, V-cycle count and final norm bit for bit"""
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.float64(a[2]).tobytes() == np.float64(b[2]).tobytes()


# (nx, ny, level-1 tile, lowv_begin, fused levels)
#  608^2: the smallest square grid with level 1 (304^2) on 64 x 32 tiles; partial last tiles in both directions
#  768 x 512: non-square, odd-sized levels in the lower V
#  1216^2: lowv_begin = 5 -- level 4 keeps its launch ahead of the fused one (and level 2, 304^2, is a 64 x 32 level of its own when not fused)
#  512^2, 576^2: level 1 on 32 x 16 tiles with two and three fused levels; 320^2: the smallest grid with two mid levels
FUSED = [(608, 608, "TileBig", 4, 3), (768, 512, "TileBig", 4, 3), (1024, 1024, "TileBig", 4, 3), (1216, 1216, "TileBig", 5, 3),
         (512, 512, "TileSmall", 3, 2), (576, 576, "TileSmall", 4, 3), (320, 320, "TileSmall", 3, 2)]


@pytest.mark.parametrize("nx,ny,tile,lb,nfused", FUSED)
def test_fused_against_one_launch_per_level(api, nx, ny, tile, lb, nfused):
    on, off = make_mg(api, nx, ny, "1"), make_mg(api, nx, ny, "0")
    assert on.info(schedule=True) == off.info(schedule=True)
    i = on.info()
    assert i["cc"] and i["lowv"] == "v3" and i["lowv_begin"] == lb and i["tiles"][1] == tile, i
    assert on.upleg_fused_levels() == nfused and off.upleg_fused_levels() == 0
    assert api.MultiGrid(nx, ny, *D).upleg_fused_levels() == nfused       # the default
    slab = make_slab(nx, ny, 3 * nx + ny)
    a, b = solve(api, on, slab), solve(api, off, slab)
    print(f"{nx}x{ny}: V-cycles {a[1]} / {b[1]}, norm {a[2]!r} / {b[2]!r}, max |diff| {np.abs(a[0] - b[0]).max():.3e}")
    assert a[1] >= 2, a[1]
    assert same(a, b)
    # a second solve on each handle (speculation depth > 1 now) with another coefficient plane
    slab2 = make_slab(nx, ny, 5 * nx + ny)
    a, b = solve(api, on, slab2), solve(api, off, slab2)
    print(f"{nx}x{ny} second solve: V-cycles {a[1]} / {b[1]}, max |diff| {np.abs(a[0] - b[0]).max():.3e}")
    assert a[1] >= 2, a[1]
    assert same(a, b)


# 256^2: k_lower_v3 from level 2 (one mid level); 132 x 66: k_lower_v<true>; 300^2: the generic bottom; 255^2: node-centred
@pytest.mark.parametrize("nx,ny,lowv", [(256, 256, "v3"), (132, 66, "v-cc"), (300, 300, "bottom"), (255, 255, "v-nodal")])
def test_grids_that_do_not_fuse(api, nx, ny, lowv):
    on, off = make_mg(api, nx, ny, "1"), make_mg(api, nx, ny, "0")
    for mg in (on, off):
        assert mg.info()["lowv"] == lowv
        assert mg.upleg_fused_levels() == 0
    slab = make_slab(nx, ny, 3 * nx + ny)
    a, b = solve(api, on, slab), solve(api, off, slab)
    print(f"{nx}x{ny} {lowv}: V-cycles {a[1]} / {b[1]}")
    assert a[1] >= 1
    assert same(a, b)


@pytest.mark.parametrize("n", [608, 512])
def test_five_vcycles_behind_one(api, n):
    """A solve that needs one V-cycle, then one that needs at least five on the same handle: the host adds gated V-cycles
    behind the speculated one, and the fused launch of each of them runs."""
    easy, hard = make_slab(n, n, 31), make_slab(n, n, 37)
    tol1 = None
    for tol in (0.5, 0.3, 0.2, 0.1, 0.05, 0.02):
        if solve(api, make_mg(api, n, n, "1"), easy, tol_rel=tol)[1] == 1:
            tol1 = tol
            break
    assert tol1 is not None, "no tolerance at which the first solve takes exactly one V-cycle"
    res = []
    for sw in ("1", "0"):
        mg = make_mg(api, n, n, sw)
        assert (mg.upleg_fused_levels() > 0) is (sw == "1")
        first = solve(api, mg, easy, tol_rel=tol1)
        assert first[1] == 1
        res.append((first, solve(api, mg, hard, tol_rel=1e-12)))
    print(f"{n}: tol {tol1}: V-cycles {res[0][0][1]} then {res[0][1][1]}")
    assert res[0][1][1] >= 5, res[0][1][1]
    assert same(res[0][0], res[1][0]) and same(res[0][1], res[1][1])


@pytest.mark.parametrize("n", [576, 608])
def test_nothing_stale_behind_an_inactive_vcycle(api, n):
    """A solve that converges on entry (its speculated V-cycle is gated off: the fused launch returns without storing) ahead
    of a normal one with another coefficient; and a handle's second solve is a fresh handle's."""
    s2 = make_slab(n, n, 11, chi_seed=22)
    s2[4] *= 3.0
    done = make_slab(n, n, 13, chi_seed=23)
    done[0:2] = solve(api, make_mg(api, n, n, "0"), done, tol_rel=1e-9)[0][0:2]
    fresh = solve(api, make_mg(api, n, n, "0"), s2)
    assert fresh[1] >= 2
    for sw in ("1", "0"):
        mg = make_mg(api, n, n, sw)
        r0 = solve(api, mg, done)
        assert r0[1] == 0, r0[1]
        assert same(solve(api, mg, s2), fresh)
        # five speculated V-cycles ahead of a solve that needs fewer: the later ones are inactive
        mg = make_mg(api, n, n, sw)
        deep = solve(api, mg, make_slab(n, n, 37), tol_rel=1e-12)
        assert deep[1] >= 5
        assert same(solve(api, mg, s2), fresh)


def _deck_608():
    """decks.blowout_wake() at 608^2 (level 1 on 64 x 32 tiles, three fused levels): 20 slices around the driver's centre, same
    cell length in zeta"""
    d = decks.blowout_wake()
    s = 608 / 64
    d.update(nx=608, ny=608, nz=20, n_steps=1, lo=(-8.0 * s, -8.0 * s, -1.2), hi=(8.0 * s, 8.0 * s, 1.2), beam_zmin=-1.19, beam_zmax=1.19)
    return d


def test_engine_slices(api):
    """20 slices of the blowout deck, fused against not: test_schedules_do_not_change_results' tolerance (two runs of one
    schedule differ by the order of the depositions' atomics), equal V-cycle totals."""
    deck = _deck_608()
    eng = []
    for sw in ("1", "0"):
        with _switch(sw):
            e = api.SliceEngine(deck, tile_size=16, sort_period=7)
        e.begin_step()
        for k in range(deck["nz"] - 1, -1, -1):
            e.solve_slice(k)
        e.sync()
        eng.append(e)
    a, b = eng
    assert a.stats()["slices"] == b.stats()["slices"] == 20
    print("V-cycles", a.stats()["vcycles"], b.stats()["vcycles"])
    assert a.stats()["vcycles"] == b.stats()["vcycles"] >= 20
    sa, sb = a.slab(), b.slab()
    for c, nm in enumerate(a.comp_names()):
        sc = max(np.abs(sb[c]).max(), 1e-300)
        print(nm, np.abs(sa[c] - sb[c]).max() / sc)
        assert np.abs(sa[c] - sb[c]).max() <= 1e-12 * sc, nm
    (ra, va), (rb, vb) = a.particles(), b.particles()
    assert ra.shape == rb.shape and np.array_equal(np.sort(va), np.sort(vb))
    assert np.abs(ra - rb).max() <= 1e-12 * np.abs(rb).max()
