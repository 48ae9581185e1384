"""The float64 numpy deposition of tests/util.py (deposit_current_ref) against the oracle's DepositCurrent, with the laser's
|a|^2 and ion levels 0 to 5 on, at every deposition order: the reference that tests/test_particle_dispatch_gpu.py holds the
tile kernels to is itself checked on a machine without a GPU."""
import numpy as np
import pytest

from tests.util import NCOMP, deposit_current_ref, rel_err, smooth_slab, thermal_sheet

LO, HI = (-8.0, -8.0), (8.0, 8.0)
COMP = [15, 16, 3, 18, 2, 17]          # jx jy jz rho chi rhomjz
AABS = 20


def _inputs(nx, ny, order, seed):
    g = (order + 1) // 2 + 1
    real, valid, _ = thermal_sheet(nx, ny, LO, HI, ppc=2, seed=seed, u_std=0.3)
    rng = np.random.default_rng(seed)
    n = real.shape[1]
    ion = rng.integers(0, 6, n).astype(np.int32)
    valid[rng.random(n) < 0.05] = 0
    real[5, :5] = -0.3                       # psi < 0: dropped
    real[5, 5:9] = 0.0                       # psi = 0 with ux, uy != 0: gamma/psi = inf, dropped
    real[3, 5:9], real[4, 5:9] = 0.2, -0.1
    real[5, 9:13] = 0.08                     # gamma/psi above 35 for the charged ones
    slab = smooth_slab(nx, ny, g, amp=0.2)
    slab[AABS] = np.abs(slab[AABS]) * 3.0    # |a|^2 >= 0, up to about 3
    return g, real, valid, ion, slab


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("laser,ionize", [(True, True), (True, False), (False, True)])
def test_numpy_deposition_matches_oracle(oracle, order, laser, ionize):
    nx, ny = 37, 29
    g, real, valid, ion, slab = _inputs(nx, ny, order, 11 + order)
    geom = oracle.make_geom(nx, ny, LO, HI, dz=0.3)
    aabs = AABS if laser else -1
    ref, rv, rw, rq = deposit_current_ref(slab, g, real, valid, ion, geom, COMP, -1.0, 1.0, order, can_ionize=ionize, aabs=aabs)
    o, r2, v2 = slab.copy(), real.copy(), valid.copy()
    nq = oracle.deposit_current(o, nx, ny, g, r2, v2, ion, geom, COMP, -1.0, 1.0, order, can_ionize=ionize, aabs=aabs)
    for c in COMP:
        assert rel_err(o[c] - slab[c], ref[c] - slab[c]) < 1e-12, c
    rest = [c for c in range(NCOMP) if c not in COMP]
    assert np.array_equal(o[rest], slab[rest])
    assert nq == rq and rq >= 9
    assert np.array_equal(v2, rv) and np.array_equal(r2[2], rw)


def test_numpy_deposition_sees_laser_and_levels(oracle):
    """The laser and the levels change the deposit: neither reference may ignore them."""
    nx, ny, order = 37, 29, 2
    g, real, valid, ion, slab = _inputs(nx, ny, order, 3)
    geom = oracle.make_geom(nx, ny, LO, HI, dz=0.3)
    base = deposit_current_ref(slab, g, real, valid, ion, geom, COMP, -1.0, 1.0, order)[0]
    las = deposit_current_ref(slab, g, real, valid, ion, geom, COMP, -1.0, 1.0, order, aabs=AABS)[0]
    lev = deposit_current_ref(slab, g, real, valid, ion, geom, COMP, -1.0, 1.0, order, can_ionize=True)[0]
    assert rel_err(las[18], base[18]) > 1e-3          # rho carries gamma/psi, which carries |a|^2
    assert rel_err(lev[17], base[17]) > 1e-1          # rhomjz carries the level
