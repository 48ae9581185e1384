"""Numpy restatement of the reference's beam-plasma Coulomb collisions, the CPU side of tests/test_beam_collisions_*.py.

Written from doBeamPlasmaCoulombCollision (particles/collisions/CoulombCollision.cpp:238-348) and the is_beam_coll branches of
ElasticCollisionPerez.H and ComputeTemperature.H: species 1 is a beam slice, which carries uz where a plasma particle carries
psi -- gamma = sqrt(1 + u^2/c^2), u1z = uz, no 0.5 (g1/psi1 + g2/psi2) factor on dt, uz written back.  The pair update, the
generator, the shuffle and the plasma side's cell lists are those of tests/collision_reference.py.  A beam particle carries
no id: a cell's beam list is put in the lexicographic order of the 64-bit patterns of (x, y, z, ux, uy, uz, w), as
hipace_amd/csrc/collisions.hip does.

A beam slice is a dict of numpy arrays x, y, z, ux, uy, uz, w and nsub (< 0: absorbed).
"""
import math

import numpy as np

from tests.collision_reference import (C_SI, EP0, ME, NX, NY, PI, QE, cell_lists, chash, copy_sheet, make_sheet, shuffle,      # noqa: F401
                                       slice_key, temperature, thermal_cells, uniform, update)

ROWS = ("x", "y", "z", "ux", "uy", "uz", "w")


def make_beam(soa, nsub=None):
    soa = np.asarray(soa, dtype=np.float64)
    b = {k: soa[i].copy() for i, k in enumerate(ROWS)}
    b["nsub"] = np.zeros(soa.shape[1], dtype=np.int32) if nsub is None else np.array(nsub, dtype=np.int32)
    return b


def beam_soa(b):
    return np.stack([b[k] for k in ROWS])


def beam_key(b, ip):
    return tuple(int(np.float64(b[k][ip]).view(np.uint64)) for k in ROWS)


def beam_cell_lists(b, nx, ny, lo, dx, dy):
    """per cell the beam particles in the canonical order; absorbed, weightless and outside particles are in no cell"""
    dxi, dyi = 1.0 / dx, 1.0 / dy
    lists = {}
    for ip in range(len(b["x"])):
        if b["nsub"][ip] < 0 or b["w"][ip] == 0.0:
            continue
        i, j = int((b["x"][ip] - lo[0]) * dxi), int((b["y"][ip] - lo[1]) * dyi)
        if b["x"][ip] < lo[0] or b["y"][ip] < lo[1] or i >= nx or j >= ny:
            continue
        lists.setdefault(i + j * nx, []).append(ip)
    for c in lists:
        lists[c].sort(key=lambda ip: beam_key(b, ip))
    return lists


def beam_temperature(b, lst, m, inv_c2):
    n = len(lst)
    if n == 0:
        return 0.0
    vx = vy = vz = vs = 0.0
    for ip in lst:
        ux, uy, uz = float(b["ux"][ip]), float(b["uy"][ip]), float(b["uz"][ip])
        gm = math.sqrt(1.0 + (ux * ux + uy * uy + uz * uz) * inv_c2)
        us = ux * ux + uy * uy + uz * uz
        vx += ux / gm
        vy += uy / gm
        vz += uz / gm
        vs += us / gm / gm
    vx, vy, vz, vs = vx / n, vy / n, vz / n, vs / n
    return m / 3.0 * (vs - (vx * vx + vy * vy + vz * vz))


def elastic_beam(b, I1, s2, I2, q1, q2, m1, m2, ci2, dt, L, dens_fac, c, normalized, cell_key, log):
    """ElasticCollisionPerez with is_beam_coll = true, is_same_species = false, can_ionize1 = false"""
    inv_c, inv_c2 = 1.0 / c, 1.0 / (c * c)
    NI1, NI2 = len(I1), len(I2)
    T1t = T2t = -1.0
    if L <= 0.0:
        T1t = beam_temperature(b, I1, m1, inv_c2)
        T2t = temperature(s2, I2, m2, c, inv_c2)
    n1 = n2 = n12 = 0.0
    for ip in I1:
        n1 += float(b["w"][ip])
    for ip in I2:
        n2 += float(s2["w"][ip])
    if n1 == 0.0 or n2 == 0.0:
        return
    NK = max(NI1, NI2)
    for k in range(NK):
        n12 += min(float(b["w"][I1[k % NI1]]), float(s2["w"][I2[k % NI2]]))
    n1 *= dens_fac
    n2 *= dens_fac
    n12 *= dens_fac
    if T1t <= 0.0 or T2t <= 0.0:
        lmdD = 0.0
    else:
        lmdD = 1.0 / math.sqrt(n1 * q1 * q1 / (T1t * EP0) + n2 * q2 * q2 / (T2t * EP0))
    rmin = math.pow(4.0 * PI / 3.0 * max(n1, n2), -1.0 / 3.0)
    lmdD = max(lmdD, rmin)
    for k in range(NK):
        a1, a2 = I1[k % NI1], I2[k % NI2]
        if ci2:
            q2 *= float(s2["ion_lev"][a2])
        u1x, u1y, u1z = float(b["ux"][a1]), float(b["uy"][a1]), float(b["uz"][a1])
        u2x, u2y, psi2 = float(s2["ux"][a2]), float(s2["uy"][a2]), float(s2["psi"][a2])
        g1 = math.sqrt(1.0 + (u1x * u1x + u1y * u1y + u1z * u1z) * inv_c2)
        g2 = (1.0 + u2x * u2x * inv_c2 + u2y * u2y * inv_c2 + psi2 * psi2) / (2.0 * psi2)
        u1 = [u1x, u1y, u1z]
        u2 = [u2x, u2y, c * (g2 - psi2)]
        if update(u1, g1, u2, g2, n1, n2, n12, q1, m1, float(b["w"][a1]), q2, m2, float(s2["w"][a2]), dt * 1.0, L, lmdD,
                  normalized, cell_key, k, log):
            log["pairs"] += 1
        log["visited"].append((a1, a2))
        b["ux"][a1], b["uy"][a1], b["uz"][a1] = u1[0], u1[1], u1[2]
        g2 = math.sqrt(1.0 + (u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2]) * inv_c2)
        s2["ux"][a2], s2["uy"][a2], s2["psi"][a2] = u2[0], u2[1], g2 - u2[2] * inv_c


def collide_beam(b, s, nx, ny, lo, dx, dy, dz, q_beam, m_beam, q_pl, m_pl, dt, can_ionize_pl=False, coulomb_log=-1.0,
                 background_density_SI=0.0, normalized=True, seed=0, collision=0, step=0, islice=0):
    """doBeamPlasmaCoulombCollision on beam slice b and sheet s, in place.  dt: the run's time step in seconds.  Returns the log
    of tests/collision_reference.py::collide."""
    c = 1.0 if normalized else C_SI
    dens_fac = background_density_SI if normalized else (1.0 / dx) * (1.0 / dy) * (1.0 / dz)
    key = slice_key(seed, collision, step, islice)
    log = dict(pairs=0, branch=[0, 0, 0, 0], rejected=[0, 0], visited=[])
    la = beam_cell_lists(b, nx, ny, lo, dx, dy)
    lb = cell_lists(s, nx, ny, lo, dx, dy)
    for cell in sorted(la):
        if cell not in lb:
            continue
        cell_key = chash(key, cell)
        l1, l2 = la[cell], lb[cell]
        shuffle(l1, len(l1), cell_key, 0)
        shuffle(l2, len(l2), cell_key, 1)
        elastic_beam(b, l1, s, l2, q_beam, q_pl, m_beam, m_pl, can_ionize_pl, dt, coulomb_log, dens_fac, c, normalized, cell_key, log)
    return log


def omega_p(background_density_SI):
    return math.sqrt(background_density_SI * QE * QE / (EP0 * ME))


# ---- seeded beam slices shared by tests/test_beam_collisions_cpu.py and tests/test_beam_collisions_gpu.py -----------------
BEAM_OCCUPANCIES = (0, 1, 2, 3, 7, 40)


def beam_occupancy(cell):
    """the beam's count in a cell of the 8 x 8 box: against the sheet's (0, 1, 2, 3, 7, 64)[(cell + scale) % 6] every one of the
    36 combinations occurs among the first 36 cells"""
    return BEAM_OCCUPANCIES[(cell + cell // 6) % len(BEAM_OCCUPANCIES)]


def beam_cells(seed, lo, dx, si=False, uz_mean=2000.0, u_std=1.0, uz_std=None, equal_weights=False, weight=1.0):
    """A beam slice on the 8 x 8 grid of thermal_cells: beam_occupancy(cell) particles per cell, in an order unrelated to the
    cells; u = (N(0, u_std), N(0, u_std), N(uz_mean, uz_std)) (times c in SI units); weights 0.5 .. 1.5 times `weight`."""
    rng = np.random.default_rng(seed)
    c = C_SI if si else 1.0
    xs, ys = [], []
    for cell in range(NX * NY):
        n = beam_occupancy(cell)
        i, j = cell % NX, cell // NX
        xs.append(lo[0] + (i + 0.05 + 0.9 * rng.random(n)) * dx)
        ys.append(lo[1] + (j + 0.05 + 0.9 * rng.random(n)) * dx)
    x, y = np.concatenate(xs), np.concatenate(ys)
    n = x.size
    perm = rng.permutation(n)
    x, y = x[perm], y[perm]
    z = dx * rng.random(n)
    ux, uy = rng.normal(0.0, u_std, n), rng.normal(0.0, u_std, n)
    uz = rng.normal(uz_mean, u_std if uz_std is None else uz_std, n)
    w = (np.ones(n) if equal_weights else 0.5 + rng.random(n)) * weight
    return make_beam(np.stack([x, y, z, ux * c, uy * c, uz * c, w]))


def copy_beam(b):
    return {k: v.copy() for k, v in b.items()}


def pair_cell_sums(b, s, m_beam, m_pl, c, nx, ny, lo, dx):
    """per cell that holds both species: (sum m ux, sum m uy, sum m uz, sum m gamma, sum m |u|) over beam and plasma together,
    u in units of c"""
    la, lb = beam_cell_lists(b, nx, ny, lo, dx, dx), cell_lists(s, nx, ny, lo, dx, dx)
    out = {}
    for cell in la:
        if cell not in lb:
            continue
        l1, l2 = la[cell], lb[cell]
        bx, by, bz = b["ux"][l1] / c, b["uy"][l1] / c, b["uz"][l1] / c
        bg = np.sqrt(1.0 + bx * bx + by * by + bz * bz)
        ux, uy, psi = s["ux"][l2] / c, s["uy"][l2] / c, s["psi"][l2]
        g = (1.0 + ux * ux + uy * uy + psi * psi) / (2.0 * psi)
        uz = g - psi
        out[cell] = np.array([m_beam * bx.sum() + m_pl * ux.sum(), m_beam * by.sum() + m_pl * uy.sum(), m_beam * bz.sum() + m_pl * uz.sum(),
                              m_beam * bg.sum() + m_pl * g.sum(),
                              m_beam * np.sqrt(bx * bx + by * by + bz * bz).sum() + m_pl * np.sqrt(ux * ux + uy * uy + uz * uz).sum()])
    return out


# ---- the operator cases of tests/test_beam_collisions_gpu.py, computed once per session ------------------------------------
BIG_CELL = 27
# si: units; L: Coulomb logarithm (<= 0: automatic); bg: hipace.background_density_SI; wscale: SI weights (particles per macro-
# particle); dt: hipace.dt (normalised: in 1 / omega_p); heavy: a slow heavy beam (mass 1836, charge +1, uz about 1 c) in place
# of the electron beam at uz about 2000 c; spoil: absorbed, weightless and outside beam particles, invalid sheet particles;
# dup: two exactly duplicated beam particles in one cell; branches: branches of the angle sampler the case must reach
CASES = {
    "electron_norm_auto_dup": dict(si=False, L=-1.0, bg=1.0e24, dt=5.0, dup=True),
    "electron_norm_fixed": dict(si=False, L=10.0, bg=1.0e26, dt=5.0),
    "electron_norm_auto_spoiled": dict(si=False, L=-1.0, bg=1.0e24, dt=5.0, spoil=True),
    "electron_si_auto": dict(si=True, L=-1.0, wscale=1.0e8, dt=1.0e-13),
    "electron_si_fixed_spoiled": dict(si=True, L=10.0, wscale=1.0e8, dt=1.0e-13, spoil=True),
    "heavy_norm_auto_all_branches": dict(si=False, L=-1.0, bg=1.0e28, dt=1.0e6, heavy=True, branches=(0, 1, 2, 3)),
    "heavy_si_auto_all_branches": dict(si=True, L=-1.0, wscale=1.0e8, dt=1.0e-8, heavy=True, branches=(0, 1, 2, 3)),
    "heavy_si_fixed_all_branches": dict(si=True, L=10.0, wscale=1.0e8, dt=1.0e-8, heavy=True, branches=(0, 1, 2, 3), dup=True),
}
_reference = {}


def case_species(k):
    """(q_beam, m_beam, q_plasma, m_plasma) of a case"""
    q, m = (QE, ME) if k["si"] else (1.0, 1.0)
    return ((q, 1836.0 * m) if k.get("heavy") else (-q, m)) + (-q, m)


def case_dt(k):
    """the collision's dt in seconds"""
    return k["dt"] if k["si"] else k["dt"] / omega_p(k["bg"])


def reference_case(name):
    """(beam before, sheet before, beam after, sheet after, log, lo, dx, duplicated pair or None)"""
    if name in _reference:
        return _reference[name]
    k = CASES[name]
    si = k["si"]
    s, lo, dx = thermal_cells(21, si=si, big_cell=BIG_CELL)
    s["w"] *= k.get("wscale", 1.0)
    if k.get("heavy"):
        b = beam_cells(31, lo, dx, si=si, uz_mean=1.0, u_std=0.02, uz_std=0.3, weight=k.get("wscale", 1.0))
    else:
        b = beam_cells(31, lo, dx, si=si, uz_mean=2000.0, u_std=1.0, weight=k.get("wscale", 1.0))
    dup = None
    if k.get("dup"):
        lst = [l for c, l in sorted(beam_cell_lists(b, NX, NY, lo, dx, dx).items()) if len(l) == 7][0]
        dup = (lst[2], lst[5])
        for r in ROWS:
            b[r][dup[1]] = b[r][dup[0]]
    if k.get("spoil"):
        b["nsub"][::7] = -1
        b["w"][3::11] = 0.0
        b["x"][5::13] = lo[0] + (NX + 0.5) * dx
        b["y"][6::17] = lo[1] - 0.5 * dx
        s["valid"][::7] = 0
        s["w"][3::11] = 0.0
    b0, s0 = copy_beam(b), copy_sheet(s)
    qb, mb, qp, mp = case_species(k)
    log = collide_beam(b, s, NX, NY, lo, dx, dx, dx, qb, mb, qp, mp, case_dt(k), coulomb_log=k["L"], background_density_SI=k.get("bg", 0.0),
                       normalized=not si, seed=77, collision=1, step=3, islice=5)
    _reference[name] = (b0, s0, b, s, log, lo, dx, dup)
    return _reference[name]
