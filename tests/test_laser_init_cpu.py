"""Several laser pulses, envelopes from samples and the in-situ laser reductions without a GPU: the numpy
restatement (tests/laser_init_reference.py) against the closed form of the single-pulse kernel, the oracle's shape factors and
the properties of trilinear resampling; reading a lasy-layout laser file; the exported symbols; what Python refuses.  The
kernels are compared with the restatement in tests/test_laser_init_gpu.py."""
import ctypes
import math
import os

import numpy as np
import pytest

from hipace_amd import decks
from tests import laser_init_reference as R


def grid_deck(**kw):
    d = decks.laser_evolution()
    d.update(nx=32, ny=32, nz=16, lo=(-8.0, -8.0, -3.0), hi=(8.0, 8.0, 3.0), laser_lambda0=0.4, laser_zfoc=3.0, laser_pos=(0.3, -0.2, 0.5),
             laser_n_cell=(24, 20), laser_patch_lo=(-6.0, -5.0, -3.0), laser_patch_hi=(6.0, 5.0, 3.0))
    d.update(kw)
    return d


def test_one_default_pulse_is_the_closed_form_of_the_single_pulse_kernel():
    """CEP 0, no angle, PFT_yz = pi/2: the literal complex formula and the real-arithmetic closed form of k_laser_init agree to
    16 eps (1 + Phi) max|a| (the bound of the GPU test; both are a few roundings from the exact value)."""
    d = grid_deck()
    x, y, z = decks.laser_cell_centres(d)
    assert (x.size, y.size, z.size) == (24, 20, 16)
    a, phi = R.pulses([R.deck_pulse(d)], d["laser_lambda0"], x, y, z)
    c = R.closed_form(d, x, y, z)
    ratio = np.abs(a - c).max() / (R.EPS * (1.0 + phi) * np.abs(c).max())
    print(f"one pulse: Phi {phi:.2f}, |restatement - closed form| = {ratio:.3f} eps (1 + Phi) max|a|")
    assert np.abs(c).max() > 0.5 * d["laser_a0"] and phi > 1.0
    assert ratio <= 16.0
    # ... and the pulse tuple that SliceEngine.set_laser_pulses sends for defaults is that pulse
    assert decks.laser_pulse(dict(a0=d["laser_a0"], w0=d["laser_w0"], L0=d["laser_L0"], position_mean=d["laser_pos"],
                                  focal_distance=d["laser_zfoc"])) == R.deck_pulse(d)


def test_cep_scales_the_pulse_and_the_angle_rotates_it():
    d = grid_deck()
    x, y, z = decks.laser_cell_centres(d)
    base = R.deck_pulse(d)
    a, _ = R.pulses([base], d["laser_lambda0"], x, y, z)
    b, _ = R.pulses([base[:5] + (0.3,) + base[6:]], d["laser_lambda0"], x, y, z)
    assert np.allclose(b, math.exp(0.3) * a, rtol=1e-14, atol=0.0)             # literal: e^CEP, no phase turn (MultiLaser.cpp:912)
    two, _ = R.pulses([base, base], d["laser_lambda0"], x, y, z)
    assert np.array_equal(two, a + a)
    t, phi = R.pulses([base[:6] + (0.1, math.pi / 2.0 + 0.05)], d["laser_lambda0"], x, y, z)
    assert phi > 5.0 and np.abs(t - a).max() > 0.1 * np.abs(a).max()


def test_restated_shape_factors_are_the_oracles(oracle):
    rng = np.random.default_rng(1)
    xs = np.concatenate([rng.uniform(-5.0, 30.0, 200), [-2.0, -0.5, 0.0, 0.5, 3.0, 7.5, 7.4999999999, 12.25]])
    cells, w = R.shape1(xs)
    for k, xv in enumerate(xs):
        cell, s = oracle.shape_factor(1, xv)
        assert cells[k] == cell
        assert np.allclose(w[k], s, rtol=0.0, atol=2e-16), (xv, w[k], s)


def trilinear(u, v, w):
    return (0.3 + 0.5 * u) * (1.1 - 0.25 * v) * (0.7 + 0.2 * w) + 1j * (0.2 - 0.4 * u) * (0.9 + 0.3 * v) * (1.0 - 0.1 * w)


@pytest.mark.parametrize("geometry", ["xyz", "xyt"])
def test_resampling_a_trilinear_function_returns_it(geometry):
    """A file grid finer than the laser grid that covers its middle: trilinear interpolation is exact on the interior, and a
    laser cell whose stencil lies wholly outside the file gets an exact zero."""
    c = 2.5
    x, y, z = np.linspace(-3.0, 3.0, 13), np.linspace(-2.0, 2.0, 9), np.linspace(-1.5, 1.5, 7)
    fx, fy = -2.05 + 0.1 * np.arange(42), -1.55 + 0.1 * np.arange(32)
    if geometry == "xyz":
        f0 = -1.02 + 0.08 * np.arange(27)
        zs = f0
        offset, spacing = (f0[0], fy[0], fx[0]), (0.08, 0.1, 0.1)
    else:
        f0 = 0.05 * np.arange(40)                            # t from the last slice backwards: z = zmax - c t
        zs = z[-1] - c * f0
        offset, spacing = (0.0, fy[0], fx[0]), (0.05, 0.1, 0.1)
    data = trilinear(fx[None, None, :], fy[None, :, None], zs[:, None, None])
    got = R.resample(geometry, data, offset, spacing, 2.0, x, y, z, c)
    X, Y, Z = np.broadcast_arrays(x[None, None, :], y[None, :, None], z[:, None, None])
    inside = (X >= fx[0]) & (X <= fx[-1]) & (Y >= fy[0]) & (Y <= fy[-1]) & (Z >= zs.min()) & (Z <= zs.max())
    away = (X < fx[0] - 0.1) | (X > fx[-1] + 0.1) | (Y < fy[0] - 0.1) | (Y > fy[-1] + 0.1) | (Z < zs.min() - 0.2) | (Z > zs.max() + 0.2)
    assert inside.sum() > 50 and away.sum() > 50
    want = 2.0 * trilinear(X, Y, Z)
    assert np.abs(got - want)[inside].max() <= 64 * R.EPS * np.abs(want).max()
    assert np.all(got[away] == 0.0)


def test_rt_with_mode_0_only_is_axisymmetric():
    rng = np.random.default_rng(5)
    data = rng.standard_normal((1, 9, 12)) + 1j * rng.standard_normal((1, 9, 12))
    x = y = (np.arange(16) - 7.5) * 0.25
    z = np.linspace(-1.0, 1.0, 5)
    offset, spacing = (0.0, 0.0), (0.3, 0.2)
    assert R.smallest_r_index(x, y, offset, spacing) == 0
    got = R.resample("rt", data, offset, spacing, 1.0, x, y, z)
    assert np.abs(got).max() > 0.1
    for sym in (got[:, ::-1, :], got[:, :, ::-1], got.transpose(0, 2, 1)):         # y -> -y, x -> -x, x <-> y
        assert np.abs(got - sym).max() <= 4 * R.EPS * np.abs(got).max()
    # three modes are not
    data3 = rng.standard_normal((3, 9, 12)) + 1j * rng.standard_normal((3, 9, 12))
    got3 = R.resample("rt", data3, offset, spacing, 1.0, x, y, z)
    assert np.abs(got3 - got3[:, ::-1, :]).max() > 1e-3 * np.abs(got3).max()


def test_insitu_restatement_on_a_known_plane():
    """a = 1 everywhere on 4 x 3 cells: max 1, energy 12 dV, centroid sums of the cell centres, axis(a) = mean of the two middle cells"""
    x, y = np.array([-1.5, -0.5, 0.5, 1.5]) + 0.25, np.array([-1.0, 0.0, 1.0])
    a = np.ones((2, 3, 4), dtype=np.complex128)
    a[1] *= 2.0j
    rows, scale = R.insitu(a, x, y, 0.5)
    assert rows[0].tolist() == [1.0, 4.0] and rows[1].tolist() == [6.0, 24.0]
    assert rows[2, 0] == pytest.approx(3 * x.sum() * 0.5) and rows[5, 0] == pytest.approx(4 * (y * y).sum() * 0.5)
    assert (rows[6, 0], rows[7, 0], rows[6, 1], rows[7, 1]) == (1.0, 0.0, 0.0, 2.0)
    assert R.mid_cells(23) == ((11, 11), 1.0) and R.mid_cells(24) == ((11, 12), 0.5)
    assert R.insitu_sum(rows)["max(|a|^2)"] == 4.0 and R.insitu_sum(rows)["[|a|^2]"] == 30.0


@pytest.mark.parametrize("kind", ["CDOUBLE", "CFLOAT"])
def test_read_laser_round_trip(tmp_path, kind):
    from hipace_amd import h5lite, openpmd_writer
    if not h5lite.available():
        pytest.skip("no HDF5 library")
    rng = np.random.default_rng(3)
    dtype = np.complex128 if kind == "CDOUBLE" else np.complex64
    omega = 2.0 * math.pi * decks.SI["c"] / 0.8e-6
    cases = {"xyt": (["t", "y", "x"], (4, 5, 6), [1.0e-15, 2.0e-6, 3.0e-6], [0.0, -5.0e-6, -9.0e-6], [0.0, 0.0, 0.0]),
             "xyz": (["z", "y", "x"], (4, 5, 6), [1.0e-6, 2.0e-6, 3.0e-6], [-2.0e-6, -5.0e-6, -9.0e-6], [0.5, 0.0, 0.5]),
             "rt": (["t", "r"], (3, 5, 6), [1.0e-15, 2.0e-6], [0.0, 0.0], [0.0, 0.0])}
    for geometry, (labels, shape, spacing, offset, position) in cases.items():
        data = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)
        fn = str(tmp_path / f"laser_{geometry}.h5")
        mesh = "/data/3/meshes/laserEnvelope"
        with h5lite.File(fn, "w") as f:
            f.dataset(mesh, data)
            f.attr("/", "basePath", "/data/%T/")
            f.attr("/", "meshesPath", "meshes/")
            f.attr("/", "openPMD", "1.1.0")
            f.attr(mesh, "axisLabels", labels)
            f.attr(mesh, "gridSpacing", spacing)
            f.attr(mesh, "gridGlobalOffset", offset)
            f.attr(mesh, "position", position)
            f.attr(mesh, "unitSI", 2.5)
            f.attr(mesh, "angularFrequency", omega)
        g, got, off, sp, unit, lambda0 = openpmd_writer.read_laser(fn, iteration=3)
        assert g == geometry and got.dtype == np.complex128 and np.array_equal(got, data.astype(np.complex128))
        assert sp == tuple(spacing) and unit == 2.5 and lambda0 == pytest.approx(0.8e-6, rel=1e-15)
        assert off == tuple(o + p * s for o, p, s in zip(offset, position, spacing))
        with pytest.raises(IOError, match="holds no mesh named"):
            openpmd_writer.read_laser(fn, iteration=3, name="other")
        with pytest.raises(IOError, match="holds no mesh named"):
            openpmd_writer.read_laser(fn, iteration=0)


def test_read_laser_refuses_other_files(tmp_path):
    from hipace_amd import h5lite, openpmd_writer
    if not h5lite.available():
        pytest.skip("no HDF5 library")
    mesh = "/data/0/meshes/laserEnvelope"

    def write(name, data, **attrs):
        fn = str(tmp_path / name)
        with h5lite.File(fn, "w") as f:
            f.dataset(mesh, data)
            for k, v in attrs.items():
                f.attr(mesh, k, v)
        return fn

    ok = dict(axisLabels=["t", "y", "x"], gridSpacing=[1.0, 1.0, 1.0], gridGlobalOffset=[0.0, 0.0, 0.0], position=[0.0, 0.0, 0.0],
              angularFrequency=1.0e15)
    z = np.zeros((2, 2, 2), dtype=np.complex128)
    with pytest.raises(IOError, match="CFLOAT, CDOUBLE"):
        openpmd_writer.read_laser(write("real.h5", z.real, **ok))
    with pytest.raises(IOError, match="axisLabels"):
        openpmd_writer.read_laser(write("labels.h5", z, **dict(ok, axisLabels=["x", "y", "z"])))
    with pytest.raises(IOError, match="angularFrequency"):
        openpmd_writer.read_laser(write("omega.h5", z, **{k: v for k, v in ok.items() if k != "angularFrequency"}))
    with pytest.raises(IOError, match="position 0"):
        openpmd_writer.read_laser(write("position.h5", z, **dict(ok, position=[0.5, 0.0, 0.0])))


def test_library_exports_the_laser_init_entry_points():
    from hipace_amd import _lib
    _lib.build()
    L = ctypes.CDLL(_lib.SO)
    C = ctypes
    want = {
        "hps_engine_set_laser_pulses": [C.c_void_p, C.c_int, C.POINTER(_lib.LaserPulse)],
        "hps_engine_add_laser_samples": [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.c_double],
        "hps_engine_set_insitu_laser": [C.c_void_p, C.c_int],
        "hps_engine_insitu_laser": [C.c_void_p, C.c_void_p],
    }
    for name, args in want.items():
        assert hasattr(L, name), name
        res, sig = _lib._SIGS[name]
        assert res is C.c_int and sig == args, name
    assert [n for n, _ in _lib.LaserPulse._fields_] == ["a0", "w0", "L0", "pos", "zfoc", "cep", "propagation_angle_yz", "pft_yz"]
    assert C.sizeof(_lib.LaserPulse) == 10 * 8
    hdr = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "hpslice.h")).read()
    flat = " ".join(hdr.split())
    assert "typedef struct { double a0, w0, L0, pos[3], zfoc, cep, propagation_angle_yz, pft_yz; } hps_laser_pulse;" in flat
    assert "int hps_engine_set_laser_pulses (void* handle, int n, const hps_laser_pulse* pulses);" in flat
    assert ("int hps_engine_add_laser_samples (void* handle, int geometry, const double* data_host, const long extent[3], "
            "const double offset[3], const double spacing[3], double unit);") in flat
    assert "int hps_engine_set_insitu_laser (void* handle, int on);" in flat
    assert "int hps_engine_insitu_laser (void* handle, double* out_host /* [8][nzl]" in flat


BAD_PULSES = {
    "both L0 and tau": (dict(a0=1.0, w0=1.0, L0=1.0, tau=1.0), "one of L0"),
    "neither L0 nor tau": (dict(a0=1.0, w0=1.0), "one of L0"),
    "unknown key": (dict(a0=1.0, w0=1.0, L0=1.0, cep=0.1), "unknown"),
    "no waist": (dict(a0=1.0, L0=1.0), "positive"),
    "negative length": (dict(a0=1.0, w0=1.0, tau=-1.0), "positive"),
    "two coordinates": (dict(a0=1.0, w0=1.0, L0=1.0, position_mean=(0.0, 0.0)), "three"),
}


@pytest.mark.parametrize("case", sorted(BAD_PULSES))
def test_bad_pulses_are_refused_with_a_message(case):
    pulse, message = BAD_PULSES[case]
    with pytest.raises(ValueError, match=message):
        decks.laser_pulse(pulse)


def test_pulse_defaults_and_tau():
    assert decks.LASER_PULSE_DEFAULT["PFT_yz"] == math.pi / 2.0 and decks.LASER_PULSE_DEFAULT["CEP"] == 0.0
    assert decks.laser_pulse(dict(a0=2.0, w0=3.0, tau=1.0e-14), c=decks.SI["c"]) == \
        (2.0, 3.0, 1.0e-14 * decks.SI["c"], (0.0, 0.0, 0.0), 0.0, 0.0, 0.0, math.pi / 2.0)


def test_laser_two_pulses_deck():
    d = decks.laser_two_pulses()
    base = decks.laser_evolution()
    assert (d["lo"], d["hi"], d["laser_solver"], d["dt"]) == (base["lo"], base["hi"], base["laser_solver"], base["dt"])
    assert decks.has_laser_grid(d) and d["laser_insitu"] == 1 and len(d["lasers"]) == 2
    first, second = (decks.laser_pulse(p) for p in d["lasers"])
    assert second[0] < first[0] and second[3][1] != 0.0 and second[6] != 0.0 and second[7] != math.pi / 2.0
    nxl, nyl, zlo, zhi, lo3, hi3, *_ = decks.laser_geometry(d)
    for p in (first, second):          # both pulses sit on the patch
        assert lo3[1] < p[3][1] - p[1] and p[3][1] + p[1] < hi3[1] and lo3[2] < p[3][2] - p[2] and p[3][2] + p[2] < hi3[2]
    x, y, z = decks.laser_cell_centres(d)
    assert (x.size, y.size, z.size) == (nxl, nyl, zhi - zlo + 1)
    dz = (d["hi"][2] - d["lo"][2]) / d["nz"]
    assert z[0] == pytest.approx(d["lo"][2] + (zlo + 0.5) * dz, abs=1e-14)
