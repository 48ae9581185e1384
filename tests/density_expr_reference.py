"""What a plasma sheet with a parsed density has to hold, from the numpy restatements of InitParticles
(tests/plasma_init_reference.py, tests/plasma_thermal_reference.py) and the host evaluation of the program (hps_expr_eval_host,
the routine the kernels run, compiled for the CPU).

The restatements give the lattice with the density taken as 1: positions, the engine's slot of every particle, and w =
scale_fac (the division by 4 of do_symmetrize and the coarse / fine factor included), behind the radius, hollow-core and
prevent_centered_particle tests.  A slot then holds a particle iff value > min_density, with the weight value * scale_fac --
one multiplication --, the value being the program's at the primary's (x, y, c t); the three mirror copies of do_symmetrize
carry their primary's weight."""
import numpy as np

from hipace_amd import api as A
from hipace_amd import expr as X
from tests import plasma_thermal_reference as TH


def program(text, constants=None, fold=True):
    return text if isinstance(text, X.Program) else X.compile_expr(text, ("x", "y", "z"), constants, fold=fold)


def host_value(prog, x, y, z):
    """the program on the CPU through the C routine, at arrays x, y and the number (or array) z"""
    x = np.asarray(x, dtype=np.float64)
    return A.Expression(program(prog)).evaluate_host(x, np.asarray(y, dtype=np.float64), np.broadcast_to(np.float64(z), x.shape))


def lattice(deck, species="plasma", mask=None, T=5, step=0):
    """The species' lattice with density 1, in the reference's order: x, y, scale (= w), slot, prim (index, in these arrays, of
    the particle whose value a particle carries: itself, or its primary under do_symmetrize), nslots."""
    ppc = tuple(deck[species + "_ppc"])
    fine = tuple(deck.get(species + "_fine_ppc", (0, 0)))
    use = mask is not None and any(fine)
    sym = bool(deck.get("plasmas_do_symmetrize", 0))
    radius = deck["plasma_radius"] if deck["plasma_radius"] > 0.0 else np.inf
    p = TH.init_particles_warm(deck["nx"], deck["ny"], deck["lo"], deck["hi"], deck["nz"], ppc, fine if use else None,
                               mask if use else None, T, density=1.0, radius=radius,
                               hollow_core_radius=deck.get("plasma_hollow_core_radius", 0.0), normalized=not deck.get("si_units", 0),
                               u_mean=deck.get(species + "_u_mean", (0.0, 0.0, 0.0)), u_std=deck.get(species + "_u_std") or (0.0, 0.0, 0.0),
                               seed=deck.get("plasma_seed", 0), species=0 if species == "plasma" else 1, step=step,
                               do_symmetrize=sym, prevent_centered_particle=bool(deck.get("plasmas_prevent_centered_particle", 0)))
    n = p["nprimary"]
    prim = np.tile(np.arange(n), 4) if sym else np.arange(n)
    return dict(x=p["x"], y=p["y"], scale=p["w"], slot=p["slot"], prim=prim, nslots=p["nslots"])


def expected(lat, prog, z, min_density=0.0):
    """the lattice's particles that the program keeps at c t = z: value > min_density at the primary (evaluated at the
    restatement's positions; the tests' programs have no threshold within rounding of a lattice point).  -> the same dict,
    filtered, prim re-indexed, plus "kept" (mask over the lattice)."""
    v = host_value(prog, lat["x"], lat["y"], z)
    kept = (v > min_density)[lat["prim"]]
    new = np.cumsum(kept) - 1
    out = {k: lat[k][kept] for k in ("x", "y", "scale", "slot")}
    out.update(prim=new[lat["prim"][kept]], nslots=lat["nslots"], kept=kept, w=(v[lat["prim"]] * lat["scale"])[kept])
    return out


def match(real, valid, ref):
    """e with: the engine's particle e[q] is the restatement's particle q, for a sheet in slot order (tile_size 0): the
    particle sits in its slot, and every other slot must be invalid"""
    live = valid != 0
    assert real.shape[1] == ref["nslots"] and int(live.sum()) == ref["x"].size
    want = np.zeros(ref["nslots"], dtype=bool)
    want[ref["slot"]] = True
    assert np.array_equal(live, want)
    return ref["slot"]


def assert_sheet(real, valid, ref, prog, z, width):
    """A sheet in slot order.  Positions to 1e-14 of the box width (tests/test_fine_patch_gpu.py: a handful of roundings and
    the GPU's fused multiply-adds in the lattice arithmetic); the weight bit for bit: the host's value at the position the
    engine holds for the primary, times scale_fac; invalid slots carry weight 0 and psi_half 0.  -> (kept, removed)"""
    e = match(real, valid, ref)
    assert np.abs(real[0][e] - ref["x"]).max() <= 1e-14 * width and np.abs(real[1][e] - ref["y"]).max() <= 1e-14 * width
    ep = e[ref["prim"]]
    want = host_value(prog, real[0][ep], real[1][ep], z) * ref["scale"]
    assert np.array_equal(real[2][e].view(np.uint64), want.view(np.uint64)), np.abs(real[2][e] - want).max()
    dead = valid == 0
    assert np.all(real[2][dead] == 0.0) and np.all(real[10][dead] == 0.0)
    return int(e.size), int(dead.sum())


def assert_same_particles(real, valid, real0, valid0):
    """A tile-sorted sheet holds the particles of the sheet in slot order, bit for bit: both sorted by (y, x) and then by every
    other component (mirror copies of do_symmetrize share lattice points), the invalid slots counted"""
    assert real.shape == real0.shape and int((valid == 0).sum()) == int((valid0 == 0).sum())
    a, b = real[:, valid != 0], real0[:, valid0 != 0]
    order = (1, 0, 2, 3, 4, 5, 6, 7, 8, 9, 10)
    a = a[:, np.lexsort([a[q] for q in reversed(order)])]
    b = b[:, np.lexsort([b[q] for q in reversed(order)])]
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
