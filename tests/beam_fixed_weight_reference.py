"""numpy restatement of the fixed_weight beam (injection_type = fixed_weight, profile = gaussian | can: BeamParticleContainer.cpp:
137-198, InitBeamFixedWeight3D / InitBeamFixedWeightSlice, BeamParticleContainerInit.cpp:348-475, GetInitialMomentum.H:36-48) as
hipace_amd generates it on the device (hps_engine_set_beam_fixed_weight), written from the reference's formulae and the
table of draws:

    key(tag, i) = hash(hash(seed, tag), i);  unit(k, c) = coll_unit(hash(k, c));  pair(k, c) = Box-Muller of unit(k, c), unit(k, c + 1)
    tag 1 (momentum)   m_x, m_y = pair(key, 0), m_z = cosine branch of pair(key, 2)       (tests/beam_init_reference.normal_deviates)
    tag 2 (z)          gaussian: n_z = cosine branch of pair(key, 0);  can: u = unit(key, 0)
    tag 3 (x, y)       n_x, n_y = pair(key, 0)

The means X(z), Y(z) are numbers or strings over z (hipace_amd/expr.py: Program.evaluate)."""
import numpy as np

from hipace_amd import decks, expr
from tests import beam_init_reference as B
from tests import plasma_thermal_reference as W

U64 = np.uint64
TAG_Z, TAG_XY = 2, 3
# roundings between the parameters and the weight (weight() below): density charge (1); sqrt(2 pi) (1); three times std sqrt(2 pi)
# and its product with the charge (6); the cell sizes (hi - lo)/n (6), their inverses (3), the product of the three and the
# product with the charge (3); N charge (1) and the division (1)
WEIGHT_ROUNDINGS = 22


def _key(seed, tag, i):
    return W.coll_hash(W.coll_hash(U64(seed), U64(tag)), np.asarray(i, dtype=U64))


def _pair(key, c):
    u1 = 1.0 - W.coll_unit(W.coll_hash(key, U64(c)))
    u2 = W.coll_unit(W.coll_hash(key, U64(c + 1)))
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def cell_size(deck):
    return tuple((deck["hi"][d] - deck["lo"][d]) / deck[n] for d, n in enumerate(("nx", "ny", "nz")))


def weight(deck, num_particles, position_std, density=None, total_charge=None):
    """|total_charge / (N charge)| (BeamParticleContainerInit.cpp:425) with the total charge of BeamParticleContainer.cpp:179-190"""
    q = deck["beam_charge"]
    if total_charge is None:
        total_charge = density * q
        for d in range(3):
            total_charge *= position_std[d] * np.sqrt(2.0 * np.pi)
    if not deck.get("si_units", 0):
        h = cell_size(deck)
        total_charge *= (1.0 / h[0]) * (1.0 / h[1]) * (1.0 / h[2])
    return abs(total_charge / (num_particles * q))


def mean_function(m, constants=None):
    """position_mean[0 | 1] as a function of arrays of z"""
    prog = m if isinstance(m, expr.Program) else expr.compile_expr(m, ("z",), constants)
    return prog.evaluate


def fixed_weight_beam(deck, num_particles, position_mean, position_std, u_mean=(0.0, 0.0, 0.0), u_std=(0.0, 0.0, 0.0), density=None,
                      total_charge=None, profile="gaussian", zmin=-np.inf, zmax=np.inf, radius=np.inf, do_symmetrize=False, z_foc=0.0,
                      duz_per_uz0_dzeta=0.0, seed=1, constants=None, first=0):
    """-> dict(soa (7, m nd) x y z ux uy uz w of EVERY draw in draw order, the m = 4 (do_symmetrize) or 1 copies of draw i at
    m i + q; valid (m nd) the validity of the particle's draw; i (m nd) its draw; z, x, y (nd) the draw's z and offsets before
    the shifts; X, Y (nd) the means at z; n_z (gaussian) or u (can), n_x, n_y, m (3, nd): the deviates).  The draws are
    first .. first + nd - 1 (first = 0: the beam)."""
    assert profile in ("gaussian", "can")
    m = 4 if do_symmetrize else 1
    assert num_particles % m == 0
    nd = num_particles // m
    c = decks.SI["c"] if deck.get("si_units", 0) else 1.0
    i = np.arange(first, first + nd, dtype=U64)
    out = dict(i=np.repeat(np.arange(first, first + nd), m))
    kz = _key(seed, TAG_Z, i)
    if profile == "can":
        out["u"] = W.coll_unit(W.coll_hash(kz, U64(0)))
        z = out["u"] * (zmax - zmin) + zmin
        z_mean = 0.5 * (zmin + zmax)
    else:
        out["n_z"], _ = _pair(kz, 0)
        z = position_mean[2] + position_std[2] * out["n_z"]
        z_mean = position_mean[2]
    out["n_x"], out["n_y"] = _pair(_key(seed, TAG_XY, i), 0)
    x, y = position_std[0] * out["n_x"], position_std[1] * out["n_y"]
    out.update(z=z, x=x, y=y)
    out["m"] = B.normal_deviates(seed, i)
    u = [u_mean[d] + u_std[d] * out["m"][d] if u_std[d] != 0.0 else np.full(nd, float(u_mean[d])) for d in range(3)]
    u[2] = u[2] + (z - z_mean) * duz_per_uz0_dzeta * u_mean[2]
    valid = (z >= zmin) & (z <= zmax) & (x * x + y * y <= radius * radius)
    if z_foc != 0.0:
        x = x - z_foc * u[0] / u[2]
        y = y - z_foc * u[1] / u[2]
    X, Y = mean_function(position_mean[0], constants)(z), mean_function(position_mean[1], constants)(z)
    out.update(X=X, Y=Y)
    w = weight(deck, num_particles, position_std, density, total_charge)
    soa = np.empty((7, m, nd))
    for q, (sx, sy) in enumerate(((1, 1), (-1, 1), (1, -1), (-1, -1))[:m]):
        soa[0, q] = X + x if sx > 0 else X - x
        soa[1, q] = Y + y if sy > 0 else Y - y
        soa[2, q] = z
        soa[3, q] = (u[0] if sx > 0 else -u[0]) * c
        soa[4, q] = (u[1] if sy > 0 else -u[1]) * c
        soa[5, q] = u[2] * c
        soa[6, q] = w
    out["soa"] = np.ascontiguousarray(soa.transpose(0, 2, 1).reshape(7, m * nd))
    out["valid"] = np.repeat(valid, m)
    out["weight"] = w
    return out


def slice_coordinate(deck, z):
    """t of Engine::set_beam_particles' rule: (z - lo_z) (1 / dz); the slice is int(t), truncated toward zero"""
    return (z - deck["lo"][2]) * (1.0 / cell_size(deck)[2])


def binned(deck, beam):
    """The beam as the engine holds it: dict(soa (7, n) head slice first, ascending draw inside a slice; off (nz + 1); i (n);
    order (n): positions in beam["soa"]; n_invalid, n_outside: particles left out)"""
    nz = deck["nz"]
    t = slice_coordinate(deck, beam["soa"][2])
    q = np.where((t > -1.0e9) & (t < 1.0e9), np.trunc(t), -1.0).astype(np.int64)
    inside = (q >= 0) & (q < nz)
    keep = beam["valid"] & inside
    p = nz - 1 - q[keep]
    order = np.flatnonzero(keep)[np.argsort(p, kind="stable")]
    off = np.concatenate([[0], np.cumsum(np.bincount(p, minlength=nz))]).astype(np.int64)
    return dict(soa=beam["soa"][:, order], off=off, i=beam["i"][order], order=order, n_invalid=int((~beam["valid"]).sum()),
                n_outside=int((beam["valid"] & ~inside).sum()))


def margins(deck, beam, position_std, zmin, zmax, radius):
    """the smallest distances of the draws from the cuts, in the units of the margin condition: (|t - integer|,
    |z - zmin|, |z - zmax| over pos_std_z, |x^2 + y^2 - radius^2| over radius^2); inf where a cut is infinite"""
    t = slice_coordinate(deck, beam["z"])
    dt = np.abs(t - np.rint(t)).min()
    dz = min(np.abs(beam["z"] - zmin).min(), np.abs(beam["z"] - zmax).min()) / position_std[2]
    r2 = beam["x"] ** 2 + beam["y"] ** 2
    dr = np.abs(r2 - radius * radius).min() / (radius * radius) if np.isfinite(radius) else np.inf
    return dt, dz, dr


# ---- the cases of tests/test_beam_fixed_weight_gpu.py (tests/test_beam_fixed_weight_cpu.py holds every one to the margin condition) ----

def small_deck(nx=16, ny=16, nz=8, si=False):
    """the blowout deck without its beam on nx x ny x nz cells of 0.2 (normalised) or 2 um (SI) about the origin"""
    d = decks.blowout_wake_SI() if si else decks.blowout_wake()
    h = 0.2 * (10.0e-6 if si else 1.0)
    lo = (-0.5 * nx * h, -0.5 * ny * h, -0.5 * nz * h)
    d.update(nx=nx, ny=ny, nz=nz, lo=lo, hi=tuple(-v for v in lo), n_steps=1, beam_profile=-1)
    return d


_GAUSSIAN = dict(num_particles=4096, position_mean=(0.11, -0.07, 0.1), position_std=(0.3, 0.25, 0.5), u_mean=(1.0, -2.0, 100.0),
                 u_std=(0.5, 0.4, 3.0), density=2.0, zmin=-0.65, zmax=0.95, radius=0.6, seed=1)      # the box ends at z = +-0.8


def cases():
    """{name: (deck, arguments of set_beam_fixed_weight)}"""
    um = 10.0e-6
    out = dict(
        gaussian=(small_deck(), dict(_GAUSSIAN)),
        can=(small_deck(), dict(_GAUSSIAN, num_particles=3000, profile="can", zmin=-0.55, zmax=0.7, duz_per_uz0_dzeta=0.3, seed=2)),
        programs=(small_deck(), dict(_GAUSSIAN, position_mean=("slope*(z-0.1)", "if(z>0, 0.1, -0.1) + 0.05*z^2", 0.1),
                                     constants=dict(slope=0.2), seed=3)),
        programs_alone=(small_deck(), dict(_GAUSSIAN, position_mean=("slope*(z-0.1)", "if(z>0, 0.1, -0.1) + 0.05*z^2", 0.1),
                                           constants=dict(slope=0.2), position_std=(1.0e-200, 1.0e-200, 0.5), radius=np.inf, seed=3)),
        symmetrized=(small_deck(), dict(_GAUSSIAN, do_symmetrize=True, seed=4)),
        focus=(small_deck(), dict(_GAUSSIAN, z_foc=0.3, duz_per_uz0_dzeta=0.25, seed=5)),
        launch_4099=(small_deck(), dict(_GAUSSIAN, num_particles=4099, seed=6)),
        launch_8198=(small_deck(), dict(_GAUSSIAN, num_particles=8198, seed=6)),
        si_charge=(small_deck(si=True), dict(num_particles=1000, position_mean=(0.1 * um, "0.1*z", 0.05 * um),
                                             position_std=(0.3 * um, 0.25 * um, 0.5 * um), u_mean=(0.0, 0.0, 1000.0), u_std=(1.0, 2.0, 10.0),
                                             total_charge=1.0e-12, radius=0.7 * um, seed=7)),
        normalized_density=(small_deck(), dict(_GAUSSIAN, num_particles=1000, seed=8)),
    )
    for n in (1, 63, 64, 65, 257):
        out[f"size_{n}"] = (small_deck(), dict(_GAUSSIAN, num_particles=n, zmin=-np.inf, seed=9))
    return out
