"""k_lower_v3's coefficient image from a guest workgroup of the solve's initial level-0 pass (HPS_MG_COEF_GUEST, default 1)
against the image derived by the first lower V itself (=0).

The image -- the [acf | 1/diag] planes of the levels below the lower V's top level -- is a function of that level's coefficient
plane alone, and the guest evaluates cell for cell the expressions of the in-kernel derivation.  The multigrid has no
floating-point atomics (its norms are integer maxima), so a solve is reproducible bit for bit and every comparison here is
exact: solution planes, V-cycle count and final norm.

MultiGrid.info(schedule=True)["coef_guest"] says which of the two a handle does; the switch is read when the handle is
created.  The guest needs the initial pass on 64 x 32 tiles (level 0 of more than 300^2 cells) and k_lower_v3 as the lower V.
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
    """HPS_MG_COEF_GUEST in the environment while a solver or an engine is created"""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("HPS_MG_COEF_GUEST")
        os.environ["HPS_MG_COEF_GUEST"] = self.value

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["HPS_MG_COEF_GUEST"]
        else:
            os.environ["HPS_MG_COEF_GUEST"] = self.old


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


# 768 x 512 (levels 48 x 32, 24 x 16, 12 x 8, 6 x 4, 3 x 2) and 640 x 384 (40 x 24 ... 5 x 3) end on odd-sized levels: the masks of
# the 2 x 2 blocks that hang over a level's edge
@pytest.mark.parametrize("nx,ny", [(1024, 1024), (512, 512), (768, 512), (640, 384)])
def test_guest_against_in_kernel_derivation(api, nx, ny):
    on, off = make_mg(api, nx, ny, "1"), make_mg(api, nx, ny, "0")
    i_on, i_off = on.info(schedule=True), off.info(schedule=True)
    assert i_on["lowv"] == "v3" and i_on["tiles"][0] == "TileBig" and i_on["coef_guest"] is True
    assert i_off["lowv"] == "v3" and i_off["coef_guest"] is False
    assert {k: v for k, v in i_on.items() if k != "coef_guest"} == on.info() == off.info()
    assert api.MultiGrid(nx, ny, *D).info(schedule=True)["coef_guest"] is True       # the default
    slab = make_slab(nx, ny, 3 * nx + ny)
    a, b = solve(api, on, slab), solve(api, off, slab)
    print(f"{nx}x{ny}: V-cycles {a[1]} / {b[1]}, norm {a[2]!r} / {b[2]!r}, max |diff| {np.abs(a[0] - b[0]).max():.3e}")
    assert a[1] >= 2, a[1]      # (the image is used: copied in by more than one lower V)
    assert same(a, b)
    # a second solve on each handle (speculation depth > 1 now) with another coefficient
    slab2 = make_slab(nx, ny, 5 * nx + ny)
    a, b = solve(api, on, slab2), solve(api, off, slab2)
    assert same(a, b)


# 256^2: k_lower_v3 with the initial pass on 32 x 16 tiles; 132 x 66: k_lower_v<true>; 300^2: the generic bottom; 255^2: node-centred
@pytest.mark.parametrize("nx,ny,lowv", [(256, 256, "v3"), (132, 66, "v-cc"), (300, 300, "bottom"), (255, 255, "v-nodal")])
def test_grids_without_the_guest(api, nx, ny, lowv):
    on, off = make_mg(api, nx, ny, "1"), make_mg(api, nx, ny, "0")
    for mg in (on, off):
        i = mg.info(schedule=True)
        assert i["lowv"] == lowv and i["coef_guest"] is False
    slab = make_slab(nx, ny, 3 * nx + ny)
    a, b = solve(api, on, slab), solve(api, off, slab)
    print(f"{nx}x{ny} {lowv}: V-cycles {a[1]} / {b[1]}")
    assert a[1] >= 1
    assert same(a, b)


def test_no_stale_image(api):
    """One handle, two coefficient planes: the second solve is a fresh handle's.  And a solve that converges on entry (no lower V
    runs, the guest still does) ahead of a normal one."""
    nx = ny = 512
    s1, s2 = make_slab(nx, ny, 11, chi_seed=21), make_slab(nx, ny, 11, chi_seed=22)
    s2[4] *= 3.0
    mg = make_mg(api, nx, ny, "1")
    assert mg.info(schedule=True)["coef_guest"] is True
    solve(api, mg, s1)
    second = solve(api, mg, s2)
    fresh = solve(api, make_mg(api, nx, ny, "1"), s2)
    assert second[1] >= 2
    assert same(second, fresh)
    assert same(second, solve(api, make_mg(api, nx, ny, "0"), s2))
    # converged on entry, then a normal solve with another coefficient
    done = make_slab(nx, ny, 13, chi_seed=23)
    done[0:2] = solve(api, make_mg(api, nx, ny, "1"), done, tol_rel=1e-9)[0][0:2]
    mg = make_mg(api, nx, ny, "1")
    r0 = solve(api, mg, done)
    assert r0[1] == 0, r0[1]
    after = solve(api, mg, s2)
    # (speculation depth 1 on both handles: solve1_finish records max(1, V-cycles))
    fresh1 = make_mg(api, nx, ny, "1")
    assert same(after, solve(api, fresh1, s2))
    assert same(after, fresh)


def test_more_vcycles_than_speculated(api):
    """A solve that needs one V-cycle, then one that needs at least three: the host adds V-cycles one at a time behind the
    speculated one, and each of them copies the image in."""
    nx = ny = 512
    easy = make_slab(nx, ny, 31)
    hard = make_slab(nx, ny, 37)
    tol1 = None
    for tol in (0.5, 0.3, 0.2, 0.1, 0.05, 0.02):
        if solve(api, make_mg(api, nx, ny, "1"), easy, tol_rel=tol)[1] == 1:
            tol1 = tol
            break
    assert tol1 is not None, "no tolerance at which the first solve takes exactly one V-cycle"
    res = []
    for sw in ("1", "0"):
        mg = make_mg(api, nx, ny, sw)
        assert mg.info(schedule=True)["coef_guest"] is (sw == "1")
        first = solve(api, mg, easy, tol_rel=tol1)
        assert first[1] == 1
        res.append((first, solve(api, mg, hard, tol_rel=1e-8)))
    print(f"tol {tol1}: V-cycles {res[0][0][1]} then {res[0][1][1]}")
    assert res[0][1][1] >= 3, res[0][1][1]
    assert same(res[0][0], res[1][0]) and same(res[0][1], res[1][1])


def _guest_deck():
    """decks.blowout_wake() on the smallest grid whose solver takes the guest: 304^2 (level 0 above 300^2 cells: 64 x 32 tiles;
    304 -> 152 -> 76 -> 38 -> 19: k_lower_v3 from 38 x 38).  20 slices around the driver's centre, same cell length in zeta."""
    d = decks.blowout_wake()
    s = 304 / 64
    d.update(nx=304, ny=304, nz=20, n_steps=1, lo=(-8.0 * s, -8.0 * s, -1.2), hi=(8.0 * s, 8.0 * s, 1.2), beam_zmin=-1.19, beam_zmax=1.19)
    return d


def test_smallest_grid_with_the_guest(api):
    assert api.MultiGrid(304, 304, *D).info(schedule=True)["coef_guest"] is True
    for n in (128, 256, 300, 302):       # 302 -> 151: no level of at most 64 x 64 cells
        assert api.MultiGrid(n, n, *D).info(schedule=True)["coef_guest"] is False


def test_engine_slices(api):
    """20 slices of the blowout deck with the guest against without: test_schedules_do_not_change_results' tolerance (two runs of
    one schedule differ by the order of the depositions' atomics), equal V-cycle totals."""
    deck = _guest_deck()
    eng = []
    for sw in ("1", "0"):
        with _switch(sw):
            e = api.SliceEngine(deck, tile_size=16, sort_period=7)
        assert e.schedule()["mg_coef_guest"] is (sw == "1")
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
        assert np.abs(sa[c] - sb[c]).max() <= 1e-12 * sc, nm
    (ra, va), (rb, vb) = a.particles(), b.particles()
    assert ra.shape == rb.shape and np.array_equal(np.sort(va), np.sort(vb))
    assert np.abs(ra - rb).max() <= 1e-12 * np.abs(rb).max()
