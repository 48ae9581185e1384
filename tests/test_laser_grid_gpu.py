"""The laser envelope on a grid of its own (hps_engine_set_laser_grid) on the GPU: the two interpolation
kernels alone and inside the engine against the numpy restatement (tests/laser_grid_reference.py), and the engine
against the oracle where the oracle can stand in -- the same grid given explicitly, a vacuum run whose oracle lives on
the laser grid, a static pulse on an aligned sub-patch -- and the hand-off of laser-grid planes."""
import numpy as np
import pytest

from hipace_amd import decks
from tests import laser_grid_reference as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


# ---- 1. the operators alone ---------------------------------------------------------------------------------------------------

NX, NY, NG = 24, 20, 2                      # the engine's guard width at depos_order_xy = 2
FLO, FHI = (-3.0, -2.5), (3.0, 2.5)
NXL, NYL = 17, 13
PATCHES = {"partly outside": ((-1.3, -3.4), (4.1, 1.7)),          # off-centre, sticks out in +x and -y; 0.3176.. x 0.3923.. cells
           "inside": ((-2.1, -1.6), (1.4, 1.9)),                  # strictly inside the field box
           "containing": ((-4.2, -3.9), (4.6, 3.3))}              # strictly contains the field box


def field_geometry():
    dx, dy = (FHI[0] - FLO[0]) / NX, (FHI[1] - FLO[1]) / NY
    return dx, dy, R.pos_offset(FLO[0], FHI[0], dx, 0, NX - 1), R.pos_offset(FLO[1], FHI[1], dy, 0, NY - 1)


def laser_geometry(patch):
    lo, hi = PATCHES[patch]
    dxl, dyl = (hi[0] - lo[0]) / NXL, (hi[1] - lo[1]) / NYL
    return dxl, dyl, R.pos_offset(lo[0], hi[0], dxl, 0, NXL - 1), R.pos_offset(lo[1], hi[1], dyl, 0, NYL - 1)


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("patch", ["partly outside", "inside"])
def test_interp_aabs_operator(api, order, patch):
    """k_laser_interp_aabs: |a|^2 of a random complex plane on every field cell, guard cells included, to 1e-13 of the plane's
    maximum (at most 16 fp64 products per cell); a patch inside the box leaves exact zeros around it."""
    import torch
    rng = np.random.default_rng(17 + order)
    a = rng.standard_normal((NYL, NXL)) + 1j * rng.standard_normal((NYL, NXL))
    dx, dy, xoff, yoff = field_geometry()
    lg = laser_geometry(patch)
    want = R.interp_aabs(a, lg, NX, NY, NG, dx, dy, xoff, yoff, order)
    f = api.Fields(NX, NY, NG, 3, data=rng.standard_normal((3, NY + 2 * NG, NX + 2 * NG)))
    before = f.numpy().copy()
    op = api.LaserInterp((NXL, NYL), *PATCHES[patch], order=order)
    assert (op.dxl, op.dyl, op.xoffl, op.yoffl) == pytest.approx(lg, rel=1e-15)
    op.aabs(f, api.Geometry(NX, NY, FLO, FHI, 0.1), 1, torch.tensor(a, device="cuda"))
    got = f.numpy()
    err = np.abs(got[1] - want).max() / np.abs(want).max()
    print(f"aabs order {order} {patch}: {err:.3e}")
    assert err <= 1e-13
    assert np.array_equal(got[0], before[0]) and np.array_equal(got[2], before[2])
    assert np.abs(want[:NG]).max() > 0.0 or patch == "inside"          # guard cells inside the patch get a value
    if patch == "inside":
        away = want == 0.0
        assert away[:NG].all() and away[-NG:].all() and away[:, :NG].all() and away[:, -NG:].all() and away.sum() > 4 * NG * NG
        assert np.all(got[1][away] == 0.0)


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("patch", ["partly outside", "containing"])
def test_interp_chi_operator(api, order, patch):
    """k_laser_interp_chi: chi of the slab on the laser cells that lie on the field box shrunk by the guard width, the initial
    chi elsewhere -- on all four sides where the patch contains the box."""
    import torch
    rng = np.random.default_rng(29 + order)
    slab = rng.standard_normal((3, NY + 2 * NG, NX + 2 * NG))
    chi0 = rng.standard_normal((NYL, NXL))
    dx, dy, xoff, yoff = field_geometry()
    lg = laser_geometry(patch)
    want, inside = R.interp_chi(slab[2], chi0, lg, NX, NY, NG, dx, dy, xoff, yoff, NG, order)
    assert inside.any() and not inside.all()
    if patch == "containing":
        assert not inside[0].any() and not inside[-1].any() and not inside[:, 0].any() and not inside[:, -1].any()
    f = api.Fields(NX, NY, NG, 3, data=slab)
    op = api.LaserInterp((NXL, NYL), *PATCHES[patch], order=order)
    got = op.chi(f, api.Geometry(NX, NY, FLO, FHI, 0.1), 2, torch.tensor(chi0, device="cuda")).cpu().numpy()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"chi order {order} {patch}: {err:.3e}")
    assert err <= 1e-13
    assert np.array_equal(got[~inside], chi0[~inside])
    assert np.array_equal(f.numpy(), slab)


# ---- 2. the same grid, given explicitly ---------------------------------------------------------------------------------------

def plasma_deck(**kw):
    """the deck of tests/test_gpu_parity.py::test_evolving_laser_in_plasma_vs_oracle"""
    d = decks.laser_blowout_wake()
    d.update(nx=64, ny=64, nz=30, lo=(-16.0, -16.0, -4.0), hi=(16.0, 16.0, 4.0), laser_a0=1.5, laser_lambda0=0.4, dt=5.0, n_steps=3)
    d.update(kw)
    return d


@pytest.mark.parametrize("solver", [1, 2])
def test_same_grid_given_explicitly_vs_oracle(api, oracle, solver):
    """n_cell = (nx, ny), patch = box, interp_order 1: the grid path (interpolation kernels, chi plane, chi_initial) computes
    what the oracle computes on the field grid -- three steps, the envelope to 1e-9, every slab component of the last slice
    to 1e-8, the same V-cycle count."""
    deck = plasma_deck(laser_solver=solver)
    gd = dict(deck, laser_n_cell=(64, 64), laser_patch_lo=deck["lo"], laser_patch_hi=deck["hi"], laser_interp_order=1)
    ge = api.SliceEngine(gd, tile_size=16, sort_period=7)
    assert ge.laser_grid() == (64, 64, 0, 29)
    oe = oracle.Engine(deck)
    for step in range(3):
        ge.begin_step()
        oe.begin_step()
        for isl in range(deck["nz"] - 1, -1, -1):
            ge.solve_slice(isl)
            oe.solve_slice(isl)
        ga, oa = ge.laser_envelope(), oe.laser_envelope()
        err = np.abs(ga - oa).max() / np.abs(oa).max()
        print(f"solver {solver} step {step}: envelope {err:.3e}")
        assert err <= 1e-9, step
    assert ge.laser_vcycles() == oe.laser_vcycles() and (ge.laser_vcycles() > 0) == (solver == 2)
    gs, os_ = ge.slab(), oe.slab()
    names = ge.comp_names()
    for c in range(ge.ncomp):
        assert rel_err(gs[c], os_[c]) < 1e-8, (names[c], rel_err(gs[c], os_[c]))


# ---- 3. vacuum, a different grid, against the oracle on the laser grid -----------------------------------------------------------

@pytest.mark.parametrize("solver", [1, 2])
def test_vacuum_pulse_on_its_own_grid_vs_oracle(api, oracle, solver):
    """Field 32 x 32 x 12 on (-8, -8, -3) .. (8, 8, 3), laser 40 x 24 on (-6, -5, -2.1) .. (6, 5, 1.9): slices 1 .. 9, patch z
    -2.5 .. 2.  Without a plasma the envelope is what an engine whose field grid is the laser grid computes."""
    d = decks.laser_evolution()
    d.update(nx=32, ny=32, nz=12, lo=(-8.0, -8.0, -3.0), hi=(8.0, 8.0, 3.0), laser_solver=solver, n_steps=3)
    gd = dict(d, laser_n_cell=(40, 24), laser_patch_lo=(-6.0, -5.0, -2.1), laser_patch_hi=(6.0, 5.0, 1.9), laser_interp_order=1)
    od = dict(d, nx=40, ny=24, nz=9, lo=(-6.0, -5.0, -2.5), hi=(6.0, 5.0, 2.0))
    ge = api.SliceEngine(gd)
    assert ge.laser_grid() == (40, 24, 1, 9) and ge.laser_message_doubles() == 4 * 40 * 24
    oe = oracle.Engine(od)
    c_aabs = ge.comp_names().index("aabs")
    first = None
    for step in range(3):
        ge.begin_step()
        oe.begin_step()
        for isl in range(11, -1, -1):
            ge.solve_slice(isl)
            if isl in (0, 10, 11):
                assert np.all(ge.slab()[c_aabs] == 0.0), isl
            elif step == 0 and isl == 5:
                assert ge.slab()[c_aabs].max() > 0.1
        for isl in range(8, -1, -1):
            oe.solve_slice(isl)
        ga, oa = ge.laser_envelope(), oe.laser_envelope()
        assert ga.shape == oa.shape == (9, 24, 40)
        err = np.abs(ga - oa).max() / np.abs(oa).max()
        print(f"solver {solver} step {step}: envelope {err:.3e}")
        assert err <= 1e-9, step
        first = oa.copy() if first is None else first
    assert np.abs(oa - first).max() > 1e-3 * np.abs(first).max()          # the pulse did evolve
    assert ge.laser_vcycles() == oe.laser_vcycles() and (ge.laser_vcycles() > 0) == (solver == 2)


def test_laser_envelope_checksum_sums_over_the_laser_grid(api):
    """checksums()["laserEnvelope"]: sum |a_n| over the laser grid's cells and slices (field slices without a laser add nothing)"""
    d = decks.laser_evolution()
    d.update(nx=32, ny=32, nz=12, lo=(-8.0, -8.0, -3.0), hi=(8.0, 8.0, 3.0), laser_n_cell=(40, 24), laser_patch_lo=(-6.0, -5.0, -2.1),
             laser_patch_hi=(6.0, 5.0, 1.9), laser_interp_order=2)
    ge = api.SliceEngine(d)
    ge.set_diagnostics(True)
    for step in range(2):
        ge.run_step()
        want = np.abs(ge.laser_envelope()).sum()
        got = ge.checksums()["laserEnvelope"]
        assert want > 100.0 and abs(got - want) <= 1e-12 * want, (step, got, want)


# ---- 4. wiring in a plasma ------------------------------------------------------------------------------------------------------

WIRED = dict(laser_n_cell=(24, 20), laser_patch_lo=(-9.0, -10.0, -4.0), laser_patch_hi=(19.0, 10.5, 4.0))      # sticks out in +x


@pytest.mark.parametrize("order", [1, 2])
def test_engine_interpolates_between_the_grids(api, order):
    """After every slice the slab's aabs is the restatement's interpolation of that slice of the envelope, and the chi the
    envelope solver read is the restatement's interpolation of the slab's chi, the unperturbed plasma's outside the box."""
    d = plasma_deck(nx=32, ny=32, nz=12, laser_solver=1, n_steps=2, laser_interp_order=order, **WIRED)
    nxl, nyl, zlo, zhi, lo3, hi3, dxl, dyl, xoffl, yoffl = decks.laser_geometry(d)
    lg = (dxl, dyl, xoffl, yoffl)
    ge = api.SliceEngine(d, tile_size=16, sort_period=7)
    assert ge.laser_grid() == (nxl, nyl, zlo, zhi) == (24, 20, 0, 11)
    g, names = ge.ng, ge.comp_names()
    c_aabs, c_chi = names.index("aabs"), names.index("chi")
    dx = dy = 1.0
    xoff = yoff = -15.5
    chi0 = R.chi_initial(nxl, nyl, lg, [(d["plasma_density"], d["plasma_charge"], d["plasma_mass"], None)])
    assert np.all(chi0 == 1.0)
    worst_a = worst_c = 0.0
    envs = []
    for step in range(2):
        ge.begin_step()
        a = ge.laser_envelope()
        envs.append(a)
        for isl in range(11, -1, -1):
            ge.solve_slice(isl)
            slab = ge.slab()
            want = R.interp_aabs(a[isl - zlo], lg, 32, 32, g, dx, dy, xoff, yoff, order)
            worst_a = max(worst_a, np.abs(slab[c_aabs] - want).max() / max(np.abs(want).max(), 1e-300))
            want_chi, inside = R.interp_chi(slab[c_chi], chi0, lg, 32, 32, g, dx, dy, xoff, yoff, g, order)
            assert inside.any() and not inside.all()
            worst_c = max(worst_c, np.abs(ge.laser_chi() - want_chi).max() / np.abs(want_chi).max())
    print(f"order {order}: aabs {worst_a:.3e} chi {worst_c:.3e}")
    assert worst_a <= 1e-13 and worst_c <= 1e-13
    assert np.abs(envs[1] - envs[0]).max() > 1e-3 * np.abs(envs[0]).max()
    assert np.abs(slab[c_chi]).max() > 0.0 and np.ptp(want_chi[inside]) > 0.0          # chi of a perturbed plasma went through


# ---- 5. a static pulse on an aligned sub-patch ----------------------------------------------------------------------------------

def test_static_pulse_on_an_aligned_sub_patch_vs_full_grid_oracle(api, oracle):
    """Field 64 x 64 x 20 on +-16, w0 = 4, the envelope on 48 x 48 cells on +-12 (the field's nodes), interp_order 1: the wake is
    the full-grid oracle's but for the pulse's tail beyond the patch, |a|^2 <= a0^2 exp(-2 12^2 / 4^2) = a0^2 e^-18 relative.
    Bound: 100 x that, 1.5e-6 of every component's maximum (the factor is an allowance for the nonlinear response)."""
    d = decks.laser_blowout_wake()
    d.update(nx=64, ny=64, nz=20, lo=(-16.0, -16.0, -4.0), hi=(16.0, 16.0, 4.0), laser_a0=1.5, laser_w0=4.0, laser_solver=0)
    gd = dict(d, laser_n_cell=(48, 48), laser_patch_lo=(-12.0, -12.0, -4.0), laser_patch_hi=(12.0, 12.0, 4.0), laser_interp_order=1)
    ge = api.SliceEngine(gd, tile_size=16, sort_period=7)
    oe = oracle.Engine(d)
    ge.begin_step()
    oe.begin_step()
    for isl in range(19, -1, -1):
        ge.solve_slice(isl)
        oe.solve_slice(isl)
    gs, os_ = ge.slab(), oe.slab()
    names = ge.comp_names()
    worst = {}
    for c in range(ge.ncomp):
        worst[names[c]] = rel_err(gs[c], os_[c])
    print("static sub-patch:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 1.5e-6, (k, v)
    assert ge.laser_envelope().shape == (20, 48, 48)


# ---- 6. hand-off ----------------------------------------------------------------------------------------------------------------

def handoff_deck():
    return plasma_deck(nx=32, ny=32, nz=12, laser_solver=1, laser_interp_order=1, laser_n_cell=(24, 20),
                       laser_patch_lo=(-9.0, -10.0, -3.1), laser_patch_hi=(19.0, 10.5, 2.9))        # slices 1 .. 10 of 0 .. 11


def test_laser_grid_slice_messages_round_trip(api):
    """tests/test_gpu_parity.py::test_laser_slice_messages_round_trip with laser-grid planes: messages of 4 nxl nyl doubles;
    the slices without a laser (0 and 11) have no message and their export / import do nothing."""
    import torch
    d = handoff_deck()
    nz = d["nz"]
    a = api.SliceEngine(d)
    ref = api.SliceEngine(d)
    assert a.laser_grid() == (24, 20, 1, 10) and a.laser_message_doubles() == 4 * 24 * 20
    a.run_step()
    ref.run_step()
    ref.run_step()                       # the reference engine runs step 1 itself
    b = api.SliceEngine(d)
    b.set_laser_import(True, 1)
    b.begin_step()
    msg = torch.zeros(a.laser_message_doubles(), dtype=torch.float64, device="cuda")
    mark = torch.full_like(msg, 7.0)
    for isl in range(nz - 1, -1, -1):
        if isl in (0, 11):
            msg.copy_(mark)
        a.export_laser_slice(isl, msg)
        a.sync()
        if isl in (0, 11):
            assert torch.equal(msg, mark)
        b.import_laser_slice(isl, msg)
        b.sync()
    for isl in range(nz - 1, -1, -1):
        b.solve_slice(isl)
    assert np.abs(b.laser_envelope() - ref.laser_envelope()).max() <= 1e-12 * np.abs(ref.laser_envelope()).max()
    # and the step after that agrees too (a_{n-1} arrived as well)
    c = api.SliceEngine(d)
    c.set_laser_import(True, 2)
    c.begin_step()
    for isl in range(nz - 1, -1, -1):
        b.export_laser_slice(isl, msg)
        b.sync()
        c.import_laser_slice(isl, msg)
        c.sync()
    for isl in range(nz - 1, -1, -1):
        c.solve_slice(isl)
    ref.run_step()
    assert np.abs(c.laser_envelope() - ref.laser_envelope()).max() <= 1e-10 * np.abs(ref.laser_envelope()).max()


def test_laser_grid_through_steps_in_flight_on_one_gpu(api):
    """run_local_pipeline with two lanes over three steps hands laser-grid planes on and gives one engine's envelope"""
    import torch
    from hipace_amd.pipeline import run_local_pipeline
    d = handoff_deck()
    ref = api.SliceEngine(d, tile_size=16, sort_period=8)
    want = {}
    for s in range(3):
        ref.run_step()
        want[s] = ref.laser_envelope()
    engs = [api.SliceEngine(d, tile_size=16, sort_period=8) for _ in range(2)]
    got = {}

    def on_step_end(step, eng):
        got[step] = eng.laser_envelope()

    run_local_pipeline(engs, 3, torch.device("cuda", 0), on_step_end)
    for s in range(3):
        assert got[s].shape == (10, 20, 24)
        assert np.abs(got[s] - want[s]).max() <= 1e-10 * np.abs(want[s]).max(), s
    assert np.abs(want[2] - want[0]).max() > 1e-3 * np.abs(want[0]).max()


# ---- what the engine refuses ----------------------------------------------------------------------------------------------------

def test_engine_refuses_bad_laser_grids(api):
    from hipace_amd._lib import HpsError
    d = plasma_deck(nx=32, ny=32, nz=12, laser_solver=2)
    for extra, message in ((dict(laser_patch_lo=(-9.0, -9.0, 5.0), laser_patch_hi=(9.0, 9.0, 9.0)), "empty zeta range"),
                           (dict(laser_patch_lo=(3.0, -9.0, -2.0), laser_patch_hi=(3.0, 9.0, 2.0)), "positive volume"),
                           (dict(laser_interp_order=4), "interp_order"),
                           (dict(laser_n_cell=(25, 20)), "even")):
        with pytest.raises(HpsError, match=message):
            api.SliceEngine(dict(d, **extra))
    ge = api.SliceEngine(dict(d, laser_solver=1))
    ge.begin_step()
    with pytest.raises(HpsError, match="before the first"):
        ge.set_laser_grid((24, 20))
    with pytest.raises(HpsError, match="no laser"):
        api.SliceEngine(decks.blowout_wake()).set_laser_grid((24, 20))
