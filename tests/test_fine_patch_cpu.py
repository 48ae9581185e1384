"""The plasma fine patch without a GPU: the numpy restatement of InitParticles (tests/plasma_init_reference.py), which is the
yardstick of tests/test_fine_patch_gpu.py, checked against what the reference's rules imply; and the Python surface (deck
keys, named deck, ctypes signatures, header)."""
import os
import re

import numpy as np
import pytest

from tests import plasma_init_reference as R
from hipace_amd import _lib, decks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(16, 16), (17, 13)]
LO, HI, NZ = (-8.0, -6.0, -3.0), (8.0, 6.0, 3.0), 10


def _uniform(nx, ny, ppc, density=1.0, normalized=True):
    """the uniform ppc lattice in the reference's order, and its weight"""
    dx, dy, dz = (HI[0] - LO[0]) / nx, (HI[1] - LO[1]) / ny, (HI[2] - LO[2]) / NZ
    n = ppc[0] * ppc[1]
    xs, ys = [], []
    for ip in range(n):
        jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
        xs.append((LO[0] + (ii + (0.5 + ip % ppc[0]) / ppc[0]) * dx).ravel())
        ys.append((LO[1] + (jj + (0.5 + ip // ppc[0]) / ppc[1]) * dy).ravel())
    return np.concatenate(xs), np.concatenate(ys), density * (1.0 / n if normalized else dx * dy * dz / n)


@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("T", [0, 1, 3, 7])
@pytest.mark.parametrize("normalized", [True, False])
def test_all_true_mask_is_the_uniform_fine_lattice(nx, ny, T, normalized):
    p = R.init_particles(nx, ny, LO, HI, NZ, (1, 2), (2, 4), np.ones((ny, nx), bool), T, density=3.0, normalized=normalized)
    x, y, w = _uniform(nx, ny, (2, 4), 3.0, normalized)
    assert np.array_equal(p["x"], x) and np.array_equal(p["y"], y)
    assert np.array_equal(p["w"], np.full(x.size, w))
    assert (p["L"] == T + 1).all()


@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("T", [0, 3])
def test_all_false_mask_is_the_uniform_coarse_lattice(nx, ny, T):
    p = R.init_particles(nx, ny, LO, HI, NZ, (2, 1), (4, 4), np.zeros((ny, nx), bool), T, density=3.0)
    x, y, w = _uniform(nx, ny, (2, 1), 3.0)
    assert np.array_equal(p["x"], x) and np.array_equal(p["y"], y)
    assert np.array_equal(p["w"], np.full(x.size, w))
    assert (p["L"] == 0).all()
    q = R.init_particles(nx, ny, LO, HI, NZ, (2, 1), density=3.0)          # no patch at all
    assert all(np.array_equal(p[k], q[k]) for k in ("x", "y", "w"))


@pytest.mark.parametrize("nx,ny", GRIDS)
@pytest.mark.parametrize("ppc,fine", [((1, 1), (4, 4)), ((2, 2), (4, 4)), ((1, 1), (2, 4))])
@pytest.mark.parametrize("normalized", [True, False])
def test_cell_weights_sum_to_the_density_and_particles_stay_in_their_cell(nx, ny, ppc, fine, normalized):
    T, dens = 3, 2.5
    mask = np.zeros((ny, nx), bool)
    mask[ny // 2 - 1:ny // 2 + 1, nx // 2 - 2:nx // 2 + 1] = True
    p = R.init_particles(nx, ny, LO, HI, NZ, ppc, fine, mask, T, density=dens, normalized=normalized)
    L = p["L"]
    assert set(np.unique(L)) == set(range(T + 2))                # coarse, every transition level, fine
    dx, dy, dz = (HI[0] - LO[0]) / nx, (HI[1] - LO[1]) / ny, (HI[2] - LO[2]) / NZ
    # every particle lies in its own cell
    assert (np.floor((p["x"] - LO[0]) / dx) == p["i"]).all() and (np.floor((p["y"] - LO[1]) / dy) == p["j"]).all()
    cell = p["j"] * nx + p["i"]
    count = np.bincount(cell, minlength=nx * ny).reshape(ny, nx)
    assert np.array_equal(count, np.where(L == 0, ppc[0] * ppc[1], fine[0] * fine[1]))
    wsum = np.bincount(cell, weights=p["w"], minlength=nx * ny)
    want = dens * (1.0 if normalized else dx * dy * dz)           # density * scale_fac * nppc
    assert np.abs(wsum / want - 1.0).max() <= 1e-14
    # the slot order: i_part outermost, cells x-fastest within one i_part
    key = p["i_part"] * (nx * ny) + cell
    assert (np.diff(key) > 0).all()


def test_single_cell_patch_gives_the_clipped_manhattan_distance():
    T = 3
    for nx, ny in GRIDS:
        for ci, cj in [(nx // 2, ny // 2), (0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)]:
            mask = np.zeros((ny, nx), bool)
            mask[cj, ci] = True
            L = R.level_map(mask, T, (0, nx - 1, 0, ny - 1))
            jj, ii = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
            want = np.maximum(0, T + 1 - (np.abs(ii - ci) + np.abs(jj - cj)))
            assert np.array_equal(L, want), (nx, ny, ci, cj)
            # a quarter of the diamond at a corner: clipped at the box edge
            assert (L > 0).sum() == ((np.abs(ii - ci) + np.abs(jj - cj)) <= T).sum()


@pytest.mark.parametrize("nx,ny", GRIDS)
def test_mask_outside_the_cropped_box_changes_nothing(nx, ny):
    radius, T = 2.0, 3
    dx, dy = (HI[0] - LO[0]) / nx, (HI[1] - LO[1]) / ny
    ilo, ihi, jlo, jhi = R.cell_box(nx, ny, LO, dx, dy, radius)
    assert 0 < ilo <= ihi < nx - 1 and 0 < jlo <= jhi < ny - 1     # really cropped
    mask = np.ones((ny, nx), bool)
    mask[jlo:jhi + 1, ilo:ihi + 1] = False                          # set only outside the box, right up to its edge
    a = R.init_particles(nx, ny, LO, HI, NZ, (1, 1), (4, 4), mask, T, radius=radius)
    b = R.init_particles(nx, ny, LO, HI, NZ, (1, 1), radius=radius)
    assert a["x"].size > 0 and (a["L"] == 0).all()
    assert all(np.array_equal(a[k], b[k]) for k in ("x", "y", "w"))
    # ... and a mask inside it does: the dilation stops at the box edge
    mask[jlo, ilo] = True
    c = R.init_particles(nx, ny, LO, HI, NZ, (1, 1), (4, 4), mask, T, radius=radius)
    assert (c["L"][jlo:jhi + 1, ilo:ihi + 1] > 0).sum() == sum(min(T - k, ihi - ilo) + 1 for k in range(min(T, jhi - jlo) + 1))
    assert (c["L"][:jlo] == 0).all() and (c["L"][:, :ilo] == 0).all()


def test_radius_hollow_core_and_density_leave_particles_out():
    nx, ny = GRIDS[1]
    mask = np.ones((ny, nx), bool)
    p = R.init_particles(nx, ny, LO, HI, NZ, (1, 1), (2, 2), mask, 2, radius=5.0, hollow_core_radius=1.5,
                         density_func=lambda x, y: np.where(x > 3.0, 0.0, 1.0 + 0.1 * x))
    r = np.hypot(p["x"], p["y"])
    assert p["x"].size > 0 and r.max() <= 5.0 and r.min() >= 1.5 and p["x"].max() <= 3.0
    assert np.array_equal(p["w"], (1.0 + 0.1 * p["x"]) * 0.25)


# ---- the Python surface ---------------------------------------------------------------------------------------------------

def test_defaults_are_off_and_kept_apart_from_the_default_deck():
    assert decks.PLASMA_INIT_DEFAULT == dict(plasma_fine_ppc=(0, 0), ion_fine_ppc=(0, 0), plasma_hollow_core_radius=0.0)
    assert not set(decks.PLASMA_INIT_DEFAULT) & set(decks._DEFAULT)
    assert not set(decks.PLASMA_INIT_DEFAULT) & set(decks.blowout_wake())
    # applied through a setter, like the collisions: the deck struct does not carry them
    assert not set(decks.PLASMA_INIT_DEFAULT) & {n for n, _ in _lib.Deck._fields_}


def test_named_deck_is_the_blowout_deck_with_a_disc_patch():
    d, base = decks.blowout_wake_fine_patch(), decks.blowout_wake()
    assert (d["nx"], d["ny"]) == (64, 64) and tuple(d["plasma_ppc"]) == (1, 1) and tuple(d["plasma_fine_ppc"]) == (4, 4)
    assert d["fine_transition_cells"] == 2 and d["plasma_hollow_core_radius"] == 0.0
    x = np.array([0.0, 1.9, 2.1])
    assert list(d["fine_patch"](x, 0.0 * x)) == [True, True, False]
    for k in ("plasma_fine_ppc", "ion_fine_ppc", "plasma_hollow_core_radius", "fine_patch", "fine_transition_cells"):
        d.pop(k)
    assert d == base
    import pickle
    assert pickle.loads(pickle.dumps(decks.blowout_wake_fine_patch())) == decks.blowout_wake_fine_patch()


def test_header_declares_the_entry_points_and_lib_carries_them():
    hdr = open(os.path.join(ROOT, "include", "hpslice.h")).read()
    for name, nargs in (("hps_engine_set_plasma_init", 4), ("hps_engine_set_fine_patch", 3)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert len(_lib._SIGS[name][1]) == nargs
    assert "PlasmaParticleContainerInit.cpp" in hdr and "fine_transition_cells" in hdr and "hollow_core_radius" in hdr
