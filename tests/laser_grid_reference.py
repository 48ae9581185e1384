"""The laser envelope on a grid of its own, restated in numpy from the reference's formulas (laser/MultiLaser.cpp:
MakeLaserGeometry :58-115, UpdateLaserAabs :253-284, SetInitialChi :293-332, InterpolateChi :334-407, the B-spline shape
factors of particles/particles_utils/ShapeFactors.H:122-195 and GetPosOffset, fields/Fields.H:71-77).  Plain loops over
the (order + 1)^2 stencil, vectorised over the cells; nothing here is taken from the kernels."""
import math

import numpy as np


def pos_offset(lo, hi, h, small, big):
    """GetPosOffset: position of cell 0 of a box small .. big whose centre is the centre of lo .. hi"""
    return 0.5 * (lo + hi - h * (small + big))


def round_half_away(v):
    """std::round"""
    return math.floor(v + 0.5) if v >= 0.0 else -math.floor(-v + 0.5)


def geometry(nx, ny, nz, lo, hi, n_cell=None, patch_lo=None, patch_hi=None):
    """MakeLaserGeometry -> (nxl, nyl, zeta_lo, zeta_hi, lo3, hi3, dxl, dyl, xoffl, yoffl)"""
    n = [nx, ny] if n_cell is None else [int(n_cell[0]), int(n_cell[1])]
    plo = [float(v) for v in (lo if patch_lo is None else patch_lo)]
    phi = [float(v) for v in (hi if patch_hi is None else patch_hi)]
    dz = (hi[2] - lo[2]) / nz
    poff_z = pos_offset(lo[2], hi[2], dz, 0, nz - 1)
    inv = 1.0 / dz
    zeta_lo = max(0, int(round_half_away((plo[2] - poff_z) * inv)))
    zeta_hi = min(nz - 1, int(round_half_away((phi[2] - poff_z) * inv)))
    plo[2] = (zeta_lo - 0.5) * dz + poff_z
    phi[2] = (zeta_hi + 0.5) * dz + poff_z
    assert zeta_lo <= zeta_hi and all(phi[q] > plo[q] for q in range(3)), "Laser box must have positive volume"
    dxl, dyl = (phi[0] - plo[0]) / n[0], (phi[1] - plo[1]) / n[1]
    return (n[0], n[1], zeta_lo, zeta_hi, tuple(plo), tuple(phi), dxl, dyl,
            pos_offset(plo[0], phi[0], dxl, 0, n[0] - 1), pos_offset(plo[1], phi[1], dyl, 0, n[1] - 1))


def slice_z(k, lo_z, hi_z, small, big):
    """z of slice k of a geometry lo_z .. hi_z whose slices are small .. big (InitLaserSlice :818, 865)"""
    dz = (hi_z - lo_z) / (big - small + 1)
    return k * dz + pos_offset(lo_z, hi_z, dz, small, big)


def shape(order, xmid):
    """compute_single_shape_factor<false, order>(xmid, ix) for ix = 0 .. order: -> (cells (..., order + 1) int, factors)"""
    xmid = np.asarray(xmid, dtype=np.float64)
    if order == 0:
        c = np.floor(xmid + 0.5)
        s = [np.ones_like(xmid)]
        first = c
    elif order == 1:
        f = np.floor(xmid)
        t = xmid - f
        s = [1.0 - t, t]
        first = f
    elif order == 2:
        f = np.floor(xmid + 0.5)
        t = xmid - f
        s = [0.5 * (0.5 - t) * (0.5 - t), 0.75 - t * t, 0.5 * (0.5 + t) * (0.5 + t)]
        first = f - 1
    else:
        f = np.floor(xmid)
        t = xmid - f
        s = [1.0 / 6.0 * (1.0 - t) * (1.0 - t) * (1.0 - t), 2.0 / 3.0 - t * t * (1.0 - t / 2.0),
             2.0 / 3.0 - (1.0 - t) * (1.0 - t) * (1.0 - 0.5 * (1.0 - t)), 1.0 / 6.0 * t * t * t]
        first = f - 1
    cells = np.stack([first.astype(np.int64) + k for k in range(order + 1)], axis=-1)
    return cells, np.stack(s, axis=-1)


def interp_aabs(a, lg, nx, ny, ng, dx, dy, xoff, yoff, order):
    """UpdateLaserAabs: a (nyl, nxl) complex on the laser grid lg = (dxl, dyl, xoffl, yoffl) -> |a|^2 on the field cells
    -ng .. n - 1 + ng (the grown box), array (ny + 2 ng, nx + 2 ng); laser cells outside the plane are skipped"""
    dxl, dyl, xoffl, yoffl = lg
    nyl, nxl = a.shape
    abssq = a.real * a.real + a.imag * a.imag
    x = np.arange(-ng, nx + ng) * dx + xoff
    y = np.arange(-ng, ny + ng) * dy + yoff
    cx, sx = shape(order, (x - xoffl) * (1.0 / dxl))
    cy, sy = shape(order, (y - yoffl) * (1.0 / dyl))
    out = np.zeros((ny + 2 * ng, nx + 2 * ng))
    for iy in range(order + 1):
        for ix in range(order + 1):
            ok = ((cy[:, iy] >= 0) & (cy[:, iy] <= nyl - 1))[:, None] & ((cx[:, ix] >= 0) & (cx[:, ix] <= nxl - 1))[None, :]
            v = abssq[np.clip(cy[:, iy], 0, nyl - 1)[:, None], np.clip(cx[:, ix], 0, nxl - 1)[None, :]]
            out += np.where(ok, sx[None, :, ix] * sy[:, None, iy] * v, 0.0)
    return out


def chi_limits(n, ng_shrink, h, off, hl, offl):
    """:358-372 in one direction: the laser cells where the field box, shrunk by the guard width, ends"""
    pos_lo = ng_shrink * h + off
    pos_hi = (n - 1 - ng_shrink) * h + off
    inv = 1.0 / hl
    return math.ceil((pos_lo - offl) * inv), math.floor((pos_hi - offl) * inv)


def interp_chi(chi_slab, chi_initial, lg, nx, ny, ng, dx, dy, xoff, yoff, shrink, order):
    """InterpolateChi: chi_slab (ny + 2 ng, nx + 2 ng) incl. guard cells -> (nyl, nxl); -> (chi, inside mask)"""
    dxl, dyl, xoffl, yoffl = lg
    nyl, nxl = chi_initial.shape
    x_lo, x_hi = chi_limits(nx, shrink, dx, xoff, dxl, xoffl)
    y_lo, y_hi = chi_limits(ny, shrink, dy, yoff, dyl, yoffl)
    i, j = np.arange(nxl), np.arange(nyl)
    inside = ((y_lo <= j) & (j <= y_hi))[:, None] & ((x_lo <= i) & (i <= x_hi))[None, :]
    cx, sx = shape(order, (i * dxl + xoffl - xoff) * (1.0 / dx))
    cy, sy = shape(order, (j * dyl + yoffl - yoff) * (1.0 / dy))
    acc = np.zeros((nyl, nxl))
    for iy in range(order + 1):
        for ix in range(order + 1):
            jj = np.clip(cy[:, iy] + ng, 0, ny + 2 * ng - 1)
            ii = np.clip(cx[:, ix] + ng, 0, nx + 2 * ng - 1)
            acc += sx[None, :, ix] * sy[:, None, iy] * chi_slab[jj[:, None], ii[None, :]]
    return np.where(inside, acc, chi_initial), inside


def chi_initial(nxl, nyl, lg, species, mu0=1.0, radius=0.0, hollow_core_radius=0.0):
    """SetInitialChi with a uniform density inside radius (0: infinite) and outside the hollow core: species = [(density, charge,
    mass, initial level or None)], summed: density q^2 mu0 / m, times level^2 for an ionisable species"""
    dxl, dyl, xoffl, yoffl = lg
    x = (np.arange(nxl) * dxl + xoffl)[None, :]
    y = (np.arange(nyl) * dyl + yoffl)[:, None]
    rsq = x * x + y * y
    there = np.ones_like(rsq, dtype=bool)
    if radius > 0.0:
        there &= ~(rsq > radius * radius)
    there &= ~(rsq < hollow_core_radius * hollow_core_radius)
    out = np.zeros((nyl, nxl))
    for density, q, m, level in species:
        f = q * q * mu0 / m
        if level is not None:
            f *= level * level
        out += np.where(there, density, 0.0) * f
    return out
