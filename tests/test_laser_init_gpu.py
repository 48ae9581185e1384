"""Several laser pulses, envelopes from samples and the in-situ laser reductions on the GPU: k_laser_init_pulses,
k_laser_add, k_laser_resample and k_insitu_laser against the numpy restatement of the reference's formulas
(tests/laser_init_reference.py), alone and inside runs, through steps in flight, and what the engine refuses."""
import math

import numpy as np
import pytest

from hipace_amd import decks
from tests import laser_init_reference as R

pytestmark = pytest.mark.gpu
EPS = R.EPS


@pytest.fixture(scope="module")
def api():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from hipace_amd import _lib, api as A
    _lib.lib()      # raises if libhpslice.so is missing: no fallback
    return A


GRIDS = {"24x20x16": dict(laser_n_cell=(24, 20), laser_patch_lo=(-6.0, -5.0, -3.0), laser_patch_hi=(6.0, 5.0, 3.0)),
         # two x-blocks of a 256-lane launch, nx no multiple of 64; slices 7 and 8 of 0 .. 15
         "300x3x2": dict(laser_n_cell=(300, 3), laser_patch_lo=(-6.0, -5.0, -0.3), laser_patch_hi=(6.0, 5.0, 0.1))}
SHAPES = {"24x20x16": (16, 20, 24), "300x3x2": (2, 3, 300)}


def static_deck(grid="24x20x16", **kw):
    """a static pulse in vacuum on a laser grid of its own: begin_step evaluates the initial envelope, nothing advances it"""
    d = decks.laser_evolution()
    d.update(nx=32, ny=32, nz=16, lo=(-8.0, -8.0, -3.0), hi=(8.0, 8.0, 3.0), laser_lambda0=0.4, laser_solver=0, dt=0.0, n_steps=1,
             laser_a0=1.2, laser_w0=2.0, laser_L0=1.5, laser_zfoc=3.0, laser_pos=(0.3, -0.2, 0.5))
    d.update(GRIDS[grid])
    d.update(kw)
    return d


P1 = dict(a0=1.2, w0=2.0, L0=1.5, position_mean=(0.3, -0.2, 0.5), focal_distance=3.0)
P2 = dict(a0=0.7, w0=1.4, L0=1.1, position_mean=(-0.8, 1.1, -0.6), focal_distance=-2.0, CEP=0.3, propagation_angle_yz=0.1,
          PFT_yz=math.pi / 2.0 + 0.05)


def initial_envelope(api, deck, pulses=None, samples=(), profiles=()):
    e = api.SliceEngine(deck)
    if pulses is not None:
        e.set_laser_pulses(pulses)
    for fn in profiles:
        e.add_laser_profile(fn)
    for s in samples:
        e.add_laser_samples(*s)
    e.begin_step()
    return e.laser_envelope()


def restated_pulses(deck, pulses):
    x, y, z = decks.laser_cell_centres(deck)
    return R.pulses([decks.laser_pulse(p) for p in pulses], deck["laser_lambda0"], x, y, z)


# ---- 1. pulses ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_two_pulses_vs_restatement(api, grid):
    """A driver and a tilted, angled, off-axis second pulse with a CEP: |delta| <= 16 eps (1 + Phi) max|a|, Phi the largest
    |Im(exponent)| (the rounding of the sincos and exp arguments; the restatement alone is 0.1 of eps (1 + Phi) max|a| from a
    40-digit evaluation)."""
    d = static_deck(grid)
    got = initial_envelope(api, d, [P1, P2])
    want, phi = restated_pulses(d, [P1, P2])
    assert got.shape == want.shape == SHAPES[grid]
    ratio = np.abs(got - want).max() / (EPS * (1.0 + phi) * np.abs(want).max())
    print(f"two pulses {grid}: Phi {phi:.2f}, worst |delta| = {ratio:.3f} eps (1 + Phi) max|a|")
    assert np.abs(want).max() > 0.5 and phi > 5.0
    one, _ = restated_pulses(d, [P1])
    assert np.abs(want - one).max() > 0.05                     # the second pulse is on this grid
    assert ratio <= 16.0


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_one_default_pulse_through_the_setter_is_the_decks_pulse(api, grid):
    d = static_deck(grid)
    plain = initial_envelope(api, d)
    got = initial_envelope(api, d, [P1])
    _, phi = restated_pulses(d, [P1])
    ratio = np.abs(got - plain).max() / (EPS * (1.0 + phi) * np.abs(plain).max())
    print(f"one pulse through the setter {grid}: {ratio:.3f} eps (1 + Phi) max|a|")
    assert np.abs(plain).max() > 0.5
    assert ratio <= 16.0


def test_three_equal_pulses_are_three_times_one(api):
    d = static_deck()
    one = initial_envelope(api, d, [P2])
    three = initial_envelope(api, d, [P2, P2, P2])
    _, phi = restated_pulses(d, [P2])
    assert np.abs(three - 3.0 * one).max() <= 16.0 * EPS * (1.0 + phi) * np.abs(three).max()
    assert np.abs(one).max() > 0.1


# ---- 2. samples -----------------------------------------------------------------------------------------------------------------------

def random_complex(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def test_samples_on_the_laser_grid_alone_are_the_envelope_bit_for_bit(api):
    d = static_deck()
    data = random_complex(SHAPES["24x20x16"], 11)
    got = initial_envelope(api, d, [], samples=[(0, data, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    assert np.array_equal(got, data)
    # two sets are added in the order given
    more = random_complex(SHAPES["24x20x16"], 12)
    got = initial_envelope(api, d, [], samples=[("grid", data, (0.0,) * 3, (1.0,) * 3), ("grid", more, (0.0,) * 3, (1.0,) * 3)])
    assert np.array_equal(got, data + more)


def test_a_profile_function_is_evaluated_on_the_cell_centres(api):
    d = static_deck()

    def fn(x, y, z):
        return (0.5 + 0.1 * x) * np.exp(-0.1 * y * y) + 1j * np.sin(z) * x

    x, y, z = decks.laser_cell_centres(d)
    got = initial_envelope(api, d, [], profiles=[fn])
    assert np.array_equal(got, fn(x[None, None, :], y[None, :, None], z[:, None, None]))
    # ... and through the deck key
    e = api.SliceEngine(dict(d, lasers=[], laser_profiles=[fn]))
    e.begin_step()
    assert np.array_equal(e.laser_envelope(), got)


def test_samples_on_top_of_a_pulse(api):
    """The pulse's own bound, 16 eps (1 + Phi) max|pulse|, plus the rounding of the one add: half an ulp of the sum in the kernel
    and half an ulp in numpy's want + data, together eps max|pulse + data|.  The samples (|data| about 4) do not widen the
    pulse's part of the bound."""
    d = static_deck()
    data = random_complex(SHAPES["24x20x16"], 13)
    for label, pulses, restated in (("the setter's pulse", [P2], [P2]), ("the deck's own pulse", None, [P1])):
        # (without the setter the deck's own pulse stays under the samples)
        got = initial_envelope(api, d, pulses, samples=[(0, data, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
        want, phi = restated_pulses(d, restated)
        bound = 16.0 * EPS * (1.0 + phi) * np.abs(want).max() + EPS * np.abs(want + data).max()
        worst = np.abs(got - (want + data)).max()
        print(f"samples on {label}: worst |delta| = {worst / bound:.3f} of 16 eps (1 + Phi) max|pulse| + eps max|sum|")
        assert np.abs(want).max() > 0.1 and np.abs(data).max() > 3.0
        assert worst <= bound


def si_deck():
    """the static deck's box in SI units, kp_inv = 10 um (decks.laser_blowout_wake_SI at test size)"""
    k = 10.0e-6
    d = decks.laser_blowout_wake_SI()
    d.update(nx=32, ny=32, nz=16, lo=(-8.0 * k, -8.0 * k, -3.0 * k), hi=(8.0 * k, 8.0 * k, 3.0 * k), laser_n_cell=(24, 20),
             laser_patch_lo=(-6.0 * k, -5.0 * k, -3.0 * k), laser_patch_hi=(6.0 * k, 5.0 * k, 3.0 * k))
    return d, k


# file grids coarser than the 24 x 20 x 16 laser grid (cells of 0.5 x 0.5 x 0.375) that do not cover it: zero and partial stencils
FILES = {"xyz": ((7, 9, 11), (-1.63, -2.93, -4.03), (0.7, 0.8, 0.9)),
         "xyt": ((6, 9, 11), (0.0, -2.93, -4.03), (0.61, 0.8, 0.9)),
         "rt": ((3, 9, 12), (0.0, 0.3), (0.53, 0.6))}               # r staggered by half a file cell; smallest laser r = 0.3536


@pytest.mark.parametrize("units", ["normalised", "SI"])
@pytest.mark.parametrize("geometry", sorted(FILES))
def test_resampled_file_vs_restatement(api, geometry, units):
    """|delta| <= 64 eps max|data| unit (eight products of three weights <= 1, or six terms per mode and stencil point), and an
    exact zero wherever the restatement has one"""
    shape, offset, spacing = FILES[geometry]
    data = random_complex(shape, 21 + len(geometry))
    if units == "SI":
        d, k = si_deck()
        c = decks.SI["c"]
        tlike = geometry != "xyz"
        offset = tuple(o * k / (c if (q == 0 and tlike) else 1.0) for q, o in enumerate(offset))
        spacing = tuple(s * k / (c if (q == 0 and tlike) else 1.0) for q, s in enumerate(spacing))
        unit = 2.5
    else:
        d, c, unit = static_deck(), 1.0, 1.0
    x, y, z = decks.laser_cell_centres(d)
    want = R.resample(geometry, data, offset, spacing, unit, x, y, z, c)
    got = initial_envelope(api, d, [], samples=[(geometry, data, offset, spacing, unit)])
    zero = want == 0.0
    ratio = np.abs(got - want).max() / (EPS * np.abs(data).max() * unit)
    print(f"{geometry} {units}: worst |delta| = {ratio:.3f} eps max|data| unit; {zero.sum()} of {zero.size} cells are zero")
    assert zero.sum() > 100 and (~zero).sum() > 1000 and np.abs(want).max() > 0.5 * unit
    assert ratio <= 64.0
    assert np.all(got[zero] == 0.0)


def test_bad_samples_and_pulses_are_refused(api):
    from hipace_amd._lib import HpsError
    d = static_deck()
    full = SHAPES["24x20x16"]
    one, three = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    e = api.SliceEngine(d)
    z = np.zeros(full, dtype=np.complex128)
    with pytest.raises(HpsError, match="extents of the laser grid"):
        e.add_laser_samples(0, np.zeros((16, 20, 23), dtype=np.complex128), three, one)
    with pytest.raises(HpsError, match="spacings must be positive"):
        e.add_laser_samples("xyz", np.zeros((3, 3, 3), dtype=np.complex128), three, (1.0, 0.0, 1.0))
    with pytest.raises(HpsError, match="spacings must be positive"):
        e.add_laser_samples("xyt", np.zeros((3, 3, 3), dtype=np.complex128), three, (-1.0, 1.0, 1.0))
    with pytest.raises(HpsError, match="extents must be positive"):
        e.add_laser_samples("xyz", np.zeros((3, 0, 3), dtype=np.complex128), three, one)
    with pytest.raises(HpsError, match="odd extent"):
        e.add_laser_samples("rt", np.zeros((2, 9, 12), dtype=np.complex128), (0.0, 0.3), (0.5, 0.6))
    with pytest.raises(HpsError, match="r < 0"):           # the smallest r of the grid is 0.3536: half a cell of 0.8 is beyond it
        e.add_laser_samples("rt", np.zeros((3, 9, 12), dtype=np.complex128), (0.0, 0.4), (0.5, 0.8))
    with pytest.raises(HpsError, match="geometry"):
        api._lib.check(api._lib.lib().hps_engine_add_laser_samples(e._h, 4, z.ctypes.data, (api.C.c_long * 3)(*full), (api.C.c_double * 3)(),
                                                                   (api.C.c_double * 3)(1.0, 1.0, 1.0), 1.0))
    with pytest.raises(ValueError, match="geometry"):
        e.add_laser_samples("tyx", z, three, one)
    with pytest.raises(ValueError, match="three axes"):
        e.add_laser_samples(0, z[0], three, one)
    with pytest.raises(ValueError, match="need 3 values"):
        e.add_laser_samples("xyz", z, (0.0, 0.0), one)
    with pytest.raises(HpsError, match="0 to 8 pulses"):
        e.set_laser_pulses([P1] * 9)
    with pytest.raises(ValueError, match="one of L0"):
        e.set_laser_pulses([dict(P1, tau=1.0)])
    for _ in range(4):
        e.add_laser_samples(0, z, three, one)
    with pytest.raises(HpsError, match="at most 4"):
        e.add_laser_samples(0, z, three, one)
    e.begin_step()
    with pytest.raises(HpsError, match="before the first"):
        e.add_laser_samples(0, z, three, one)
    with pytest.raises(HpsError, match="before the first"):
        e.set_laser_pulses([P1])
    # no Gaussian and no samples
    e = api.SliceEngine(d)
    e.set_laser_pulses([])
    with pytest.raises(HpsError, match="n = 0 needs"):
        e.begin_step()
    # no laser
    plain = api.SliceEngine(decks.blowout_wake())
    with pytest.raises(HpsError, match="no laser"):
        plain.set_laser_pulses([P1])
    with pytest.raises(HpsError, match="no laser"):
        plain.add_laser_samples("xyz", np.zeros((3, 3, 3), dtype=np.complex128), three, one)
    with pytest.raises(HpsError, match="no laser"):
        plain.set_insitu_laser(True)
    with pytest.raises(HpsError, match="not switched on"):
        api.SliceEngine(d).insitu_laser()


def test_add_laser_file_checks_the_wavelength(api, tmp_path):
    from hipace_amd import h5lite
    if not h5lite.available():
        pytest.skip("no HDF5 library")
    d, k = si_deck()
    shape, offset, spacing = FILES["xyz"]
    offset, spacing = [o * k for o in offset], [s * k for s in spacing]
    data = random_complex(shape, 31).astype(np.complex64)
    mesh = "/data/0/meshes/laserEnvelope"

    def write(name, lambda0):
        fn = str(tmp_path / name)
        with h5lite.File(fn, "w") as f:
            f.dataset(mesh, data)
            f.attr("/", "basePath", "/data/%T/")
            f.attr("/", "meshesPath", "meshes/")
            for key, v in dict(axisLabels=["z", "y", "x"], gridSpacing=spacing, gridGlobalOffset=offset, position=[0.0, 0.0, 0.0], unitSI=2.0,
                               angularFrequency=2.0 * math.pi * decks.SI["c"] / lambda0).items():
                f.attr(mesh, key, v)
        return fn

    e = api.SliceEngine(d)
    with pytest.raises(ValueError, match="is not the deck.s laser_lambda0"):
        e.add_laser_file(write("other.h5", 1.0e-6))
    e.set_laser_pulses([])
    e.add_laser_file(write("same.h5", d["laser_lambda0"]))
    e.begin_step()
    x, y, z = decks.laser_cell_centres(d)
    want = R.resample("xyz", data, offset, spacing, 2.0, x, y, z, decks.SI["c"])
    assert np.abs(e.laser_envelope() - want).max() <= 64.0 * EPS * np.abs(data).max() * 2.0 and np.abs(want).max() > 1.0


# ---- 3. in-situ values ------------------------------------------------------------------------------------------------------------------

def insitu_deck(n_cell, **kw):
    """the static deck on 12 slices, the laser on slices 1 .. 9 of them"""
    return static_deck(nz=12, laser_n_cell=n_cell, laser_patch_lo=(-6.0, -5.0, -2.1), laser_patch_hi=(6.0, 5.0, 1.9), **kw)


def check_rows(rows, a, deck, label):
    """rows of hps_engine_insitu_laser against numpy on the envelope a of the same step: row 0 to 4 eps relative (FMA contraction of
    re^2 + im^2), rows 1-5 to N eps of sum |term| (N cells), rows 6, 7 to 8 eps max|a|"""
    nxl, nyl, zlo, zhi, lo3, hi3, dxl, dyl, xoffl, yoffl = decks.laser_geometry(deck)
    x, y, z = decks.laser_cell_centres(deck)
    dz = (deck["hi"][2] - deck["lo"][2]) / deck["nz"]
    want, scale = R.insitu(a, x, y, dxl * dyl * dz)
    assert rows.shape == want.shape == (8, zhi - zlo + 1)
    n = nxl * nyl
    bound = np.concatenate([np.full((1, 1), 4.0), np.full((5, 1), float(n)), np.full((2, 1), 8.0)]) * EPS * scale
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0.0, np.abs(rows - want) / bound, np.where(rows == want, 0.0, np.inf))
    print(f"in-situ {label}: worst fractions of the bounds per row", " ".join(f"{v:.3f}" for v in ratio.max(axis=1)))
    assert ratio.max() <= 1.0
    return want


# k_insitu_laser: at most 32 workgroups of 256 lanes, and a lane takes four cells per trip of its stride loop
INSITU_LANES = 32 * 256
INSITU_TRIP = 4 * INSITU_LANES


@pytest.mark.parametrize("n_cell", [(23, 19), (24, 19), (24, 20), (5, 3), (130, 70), (260, 130), (301, 229)])
def test_insitu_rows_of_a_static_off_centre_pulse(api, n_cell):
    """mid factors 1, 1/2, 1/4; fewer cells than a wave; 130 x 70: more cells (9100) than the launch has lanes (8192), so some
    lanes take a second cell; 260 x 130 and 301 x 229: more cells (33800, 68929) than one trip of the stride loop covers (32768),
    so the loop repeats -- once for 1032 lanes, twice with a part-filled third trip and an odd nx -- and (i, j) is carried over
    several strides.  The laser on slices 1 .. 9 of 0 .. 11.  Two engines on one state and two steps with dt = 0 give the same
    bytes."""
    cells = n_cell[0] * n_cell[1]
    assert {(130, 70): INSITU_LANES < cells < INSITU_TRIP, (260, 130): INSITU_TRIP < cells < 2 * INSITU_TRIP,
            (301, 229): 2 * INSITU_TRIP < cells < 3 * INSITU_TRIP}.get(n_cell, cells < INSITU_LANES)
    d = insitu_deck(n_cell)
    e = api.SliceEngine(d)
    e.set_insitu_laser()
    assert e.laser_grid() == (n_cell[0], n_cell[1], 1, 9)
    e.run_step()
    a = e.laser_envelope()
    rows = e.insitu_laser_rows()
    want = check_rows(rows, a, d, f"{n_cell[0]} x {n_cell[1]}")
    assert want[0].max() > 0.5 and np.all(want[1] > 0.0) and np.abs(want[2]).max() > 0.0
    if n_cell != (5, 3):
        assert abs(want[2, 4] / want[1, 4] - 0.3) < 0.05 and abs(want[4, 4] / want[1, 4] + 0.2) < 0.05       # the centroid is the pulse's
    out = e.insitu_laser()
    assert np.array_equal(out["axis(a)"], rows[6] + 1j * rows[7]) and np.array_equal(out["[|a|^2*y]"], rows[4])
    for name, v in R.insitu_sum(rows).items():
        assert out["sum"][name] == v
    # a second engine on the same state, and the next step of this one (dt = 0: the same envelope)
    e2 = api.SliceEngine(dict(d, laser_insitu=1))
    e2.run_step()
    assert e2.insitu_laser_rows().tobytes() == rows.tobytes()
    e.run_step()
    assert e.insitu_laser_rows().tobytes() == rows.tobytes()
    # cleared by begin_step, filled slice by slice from the head
    e.begin_step()
    assert np.all(e.insitu_laser_rows() == 0.0)
    for isl in range(11, 5, -1):
        e.solve_slice(isl)
    part = e.insitu_laser_rows()
    assert np.array_equal(part[:, 5:], rows[:, 5:]) and np.all(part[:, :5] == 0.0)


def test_insitu_without_a_laser_grid_has_a_column_per_field_slice(api):
    d = {k: v for k, v in static_deck(nz=6).items() if not k.startswith("laser_n_cell") and not k.startswith("laser_patch")}
    assert not decks.has_laser_grid(d)
    e = api.SliceEngine(d)
    e.set_insitu_laser()
    e.run_step()
    rows = e.insitu_laser_rows()
    assert rows.shape == (8, 6)
    check_rows(rows, e.laser_envelope(), d, "field grid 32 x 32")


# ---- 4. in-situ in a run ----------------------------------------------------------------------------------------------------------------

def vacuum_deck(**kw):
    d = decks.laser_evolution()
    d.update(nx=32, ny=32, nz=12, lo=(-8.0, -8.0, -3.0), hi=(8.0, 8.0, 3.0), n_steps=3, laser_n_cell=(24, 20),
             laser_patch_lo=(-6.0, -5.0, -2.1), laser_patch_hi=(6.0, 5.0, 1.9), laser_interp_order=1)
    d.update(kw)
    return d


@pytest.mark.parametrize("solver", [1, 2])
def test_insitu_changes_nothing_in_a_vacuum_run(api, solver):
    """No plasma, so no atomics anywhere: with the switch on every slab component and the envelope are bit-identical to the run
    with it off; the rows of every step match numpy on that step's envelope"""
    d = vacuum_deck(laser_solver=solver)
    on, off = api.SliceEngine(d), api.SliceEngine(d)
    on.set_insitu_laser()
    first = None
    for step in range(3):
        on.begin_step()
        off.begin_step()
        a = on.laser_envelope()
        assert np.array_equal(a, off.laser_envelope())
        for isl in range(11, -1, -1):
            on.solve_slice(isl)
            off.solve_slice(isl)
            assert np.array_equal(on.slab(), off.slab()), (step, isl)
        rows = on.insitu_laser_rows()
        check_rows(rows, a, d, f"solver {solver} step {step}")
        out = on.insitu_laser()
        for name, v in R.insitu_sum(rows).items():
            assert out["sum"][name] == v and np.isfinite(v)
        first = rows if first is None else first
    assert np.abs(rows[0] - first[0]).max() > 1e-3 * first[0].max()          # the pulse did evolve


def test_insitu_rows_in_a_plasma_run(api):
    d = decks.laser_blowout_wake()
    d.update(nx=32, ny=32, nz=12, lo=(-16.0, -16.0, -4.0), hi=(16.0, 16.0, 4.0), laser_a0=1.5, laser_lambda0=0.4, dt=5.0, n_steps=2,
             laser_solver=1, laser_n_cell=(24, 20), laser_patch_lo=(-9.0, -10.0, -4.0), laser_patch_hi=(19.0, 10.5, 4.0), laser_insitu=1)
    e = api.SliceEngine(d, tile_size=16, sort_period=7)
    rows = []
    for step in range(2):
        e.begin_step()
        a = e.laser_envelope()
        for isl in range(11, -1, -1):
            e.solve_slice(isl)
        rows.append(e.insitu_laser_rows())
        check_rows(rows[-1], a, d, f"plasma step {step}")
    assert np.abs(rows[1] - rows[0]).max() > 0.0


# ---- 5. steps in flight -------------------------------------------------------------------------------------------------------------------

def test_insitu_through_steps_in_flight_on_one_gpu(api):
    """run_local_pipeline with two engines over four steps: each step's rows are one engine's, bit for bit (the imported planes
    are copies)"""
    import torch
    from hipace_amd.pipeline import run_local_pipeline
    d = vacuum_deck(laser_insitu=1, n_steps=4)
    ref = api.SliceEngine(d)
    want = {}
    for s in range(4):
        ref.run_step()
        want[s] = ref.insitu_laser_rows()
    engs = [api.SliceEngine(d) for _ in range(2)]
    got = {}

    def on_step_end(step, eng):
        got[step] = eng.insitu_laser_rows()

    run_local_pipeline(engs, 4, torch.device("cuda", 0), on_step_end)
    for s in range(4):
        assert got[s].shape == (8, 9) and got[s][0].max() > 0.1
        assert got[s].tobytes() == want[s].tobytes(), s
    assert np.abs(want[3] - want[0]).max() > 0.0


# ---- 6. the deck ----------------------------------------------------------------------------------------------------------------------

def test_laser_two_pulses_deck_runs(api):
    d = decks.laser_two_pulses(32, 20)
    e = api.SliceEngine(d, tile_size=16)
    x, y, z = decks.laser_cell_centres(d)
    want, phi = R.pulses([decks.laser_pulse(p) for p in d["lasers"]], d["laser_lambda0"], x, y, z)
    only_first, _ = R.pulses([decks.laser_pulse(d["lasers"][0])], d["laser_lambda0"], x, y, z)
    assert np.abs(want - only_first).max() > 0.2                      # the grid holds the second pulse too
    for step in range(2):
        e.run_step()
        assert np.all(np.isfinite(e.slab())) and np.all(np.isfinite(e.laser_envelope().view(np.float64)))
        out = e.insitu_laser()
        if step == 0:
            peak = (want.real ** 2 + want.imag ** 2).max()
            assert abs(out["sum"]["max(|a|^2)"] - peak) <= 1e-12 * peak and peak > 0.3      # a0^2 / (1 + q^2) = 0.44, 100 before the focus
        assert all(np.all(np.isfinite(v)) for k, v in out.items() if k != "sum")


# ---- 7. the order of the setters ----------------------------------------------------------------------------------------------------------

def test_a_grid_set_through_the_method_places_the_profile(api):
    """set_laser_grid records the grid in the engine's deck: a profile is evaluated where the engine's cells are"""
    g = GRIDS["24x20x16"]
    e = api.SliceEngine({k: v for k, v in static_deck().items() if k not in g})
    assert e.laser_grid() == (32, 32, 0, 15)
    e.set_laser_grid(g["laser_n_cell"], g["laser_patch_lo"], g["laser_patch_hi"])

    def fn(x, y, z):
        return (0.5 + 0.1 * x) * np.exp(-0.1 * y * y) + 1j * np.sin(z) * x

    x, y, z = decks.laser_cell_centres(static_deck())
    for a, b in zip(e.laser_cell_centres(), (x, y, z)):
        assert np.array_equal(a, b)
    e.set_laser_pulses([])
    e.add_laser_profile(fn)
    e.begin_step()
    assert np.array_equal(e.laser_envelope(), fn(x[None, None, :], y[None, :, None], z[:, None, None]))


def test_a_grid_set_after_the_samples_is_refused_before_the_step_begins(api):
    """geometry 0 is checked against the grid as the first begin_step finds it, and a refusal there leaves the engine as it was:
    the grid can still be put right"""
    from hipace_amd._lib import HpsError
    g = GRIDS["24x20x16"]
    data = random_complex(SHAPES["24x20x16"], 14)
    e = api.SliceEngine(static_deck())
    e.set_laser_pulses([])
    e.add_laser_samples(0, data, (0.0,) * 3, (1.0,) * 3)
    e.set_laser_grid((23, 20), g["laser_patch_lo"], g["laser_patch_hi"])
    with pytest.raises(HpsError, match="extents of the laser grid"):
        e.begin_step()
    e.set_laser_grid(g["laser_n_cell"], g["laser_patch_lo"], g["laser_patch_hi"])
    e.begin_step()
    assert np.array_equal(e.laser_envelope(), data)


def test_switching_the_insitu_rows_on_twice_keeps_them(api):
    d = insitu_deck((24, 20))
    e = api.SliceEngine(d)
    e.set_insitu_laser()
    e.run_step()
    rows = e.insitu_laser_rows()
    assert rows[0].max() > 0.5
    e.set_insitu_laser()
    assert e.insitu_laser_rows().tobytes() == rows.tobytes()
    e.set_insitu_laser(False)
    from hipace_amd._lib import HpsError
    with pytest.raises(HpsError, match="not switched on"):
        e.insitu_laser()
