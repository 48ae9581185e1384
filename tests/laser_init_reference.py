"""numpy restatement of the reference's initial laser envelope and in-situ laser reductions, written from its formulas:

  * MultiLaser::InitLaserSlice, laser/MultiLaser.cpp:876-915 -- the Gaussian pulse with carrier-envelope phase, propagation
    angle and pulse-front tilt, in complex128, literal: CEP is added to the exponent as a real number (:912);
  * Laser::GetEnvelopeFromFile, laser/Laser.cpp:177-336 -- the three file geometries xyt, xyz and rt through order-1 shape
    factors (compute_shape_factor<1>, particles/particles_utils/ShapeFactors.H), samples outside the file counting as zero;
  * MultiLaser::InSituComputeDiags, laser/MultiLaser.cpp:923-1003 -- the eight rows per slice.

The yardstick of tests/test_laser_init_cpu.py and tests/test_laser_init_gpu.py (the oracle knows none of this)."""
import math

import numpy as np

EPS = 2.2e-16


# ---- pulses ----------------------------------------------------------------------------------------------------------------------

def pulse(p, k0, X, Y, Z):
    """One Gaussian pulse p = (a0, w0, L0, position_mean, focal_distance, CEP, propagation_angle_yz, PFT_yz) at the positions X, Y,
    Z (broadcastable) -> (envelope, largest |Im(exponent)|).  :876-915, line by line."""
    a0, w0, L0, (x0, y0, z0), zfoc, cep, propagation_angle_yz, PFT_yz = p
    PFT_yz = PFT_yz - math.pi / 2.0
    x, y, z = X - x0, Y - y0, Z - z0
    yp = math.cos(propagation_angle_yz + PFT_yz) * y - math.sin(propagation_angle_yz + PFT_yz) * z
    zp = math.sin(propagation_angle_yz + PFT_yz) * y + math.cos(propagation_angle_yz + PFT_yz) * z
    diffract_factor = 1.0 + 1j * (zp - zfoc + z0 * math.cos(propagation_angle_yz)) * 2.0 / (k0 * w0 * w0)
    inv_complex_waist_2 = 1.0 / (w0 * w0 * diffract_factor)
    prefactor = a0 / diffract_factor
    time_exponent = zp * zp / (L0 * L0)
    stcfactor = prefactor * np.exp(-time_exponent)
    exp_argument = -(x * x + yp * yp) * inv_complex_waist_2
    last = 1j * yp * k0 * propagation_angle_yz + cep
    envelope = stcfactor * np.exp(exp_argument) * np.exp(last)
    return envelope, float(np.abs((exp_argument + last).imag).max())


def pulses(plist, lambda0, x, y, z):
    """The sum over the pulses, in order, on the cells x (nx), y (ny), z (nz) -> (a [nz][ny][nx], Phi = largest |Im(exponent)|)"""
    k0 = 2.0 * math.pi / lambda0
    X, Y, Z = x[None, None, :], y[None, :, None], z[:, None, None]
    a, phi = np.zeros((z.size, y.size, x.size), dtype=np.complex128), 0.0
    for p in plist:
        e, f = pulse(p, k0, X, Y, Z)
        a, phi = a + e, max(phi, f)
    return a, phi


def deck_pulse(deck):
    """the deck's own pulse as a tuple for `pulse` (CEP 0, no angle, PFT_yz = pi/2)"""
    return (deck["laser_a0"], deck["laser_w0"], deck["laser_L0"], tuple(deck["laser_pos"]), deck.get("laser_zfoc", 0.0), 0.0, 0.0,
            math.pi / 2.0)


def closed_form(deck, x, y, z):
    """What the single-pulse kernel has always computed (real arithmetic, one exp and one sincos per cell): with q = (z - zfoc) 2 /
    (k0 w0^2), a = a0/(1 + i q) exp(-(r^2/w0^2)/(1 + q^2) - z^2/L0^2) (cos + i sin)(q (r^2/w0^2)/(1 + q^2))."""
    a0, w0, L0, (x0, y0, z0), zfoc = deck["laser_a0"], deck["laser_w0"], deck["laser_L0"], deck["laser_pos"], deck.get("laser_zfoc", 0.0)
    k0 = 2.0 * math.pi / deck["laser_lambda0"]
    X, Y, Z = x[None, None, :] - x0, y[None, :, None] - y0, z[:, None, None] - z0
    q = (Z - zfoc + z0) * 2.0 / (k0 * w0 * w0)
    den = 1.0 + q * q
    dr, di = 1.0 / den, -q / den
    r2 = X * X + Y * Y
    er, ei = -r2 * dr / (w0 * w0) - Z * Z / (L0 * L0), -r2 * di / (w0 * w0)
    m = np.exp(er)
    ar, ai = a0 * dr, a0 * di
    return m * (ar * np.cos(ei) - ai * np.sin(ei)) + 1j * (m * (ar * np.sin(ei) + ai * np.cos(ei)))


# ---- samples ---------------------------------------------------------------------------------------------------------------------

def shape1(mid):
    """compute_shape_factor<1>: -> (left cell [..], weights [.., 2])"""
    mid = np.asarray(mid, dtype=np.float64)
    cell = np.floor(mid)
    t = mid - cell
    return cell.astype(np.int64), np.stack([1.0 - t, t], axis=-1)


def _take(data, idx, valid):
    """data[idx] where valid, 0 elsewhere (idx: tuple of broadcastable index arrays)"""
    shape = np.broadcast(*idx, valid).shape
    clipped = tuple(np.clip(np.broadcast_to(i, shape), 0, n - 1) for i, n in zip(idx, data.shape))
    return np.where(np.broadcast_to(valid, shape), data[clipped], 0.0)


def resample(geometry, data, offset, spacing, unit, x, y, z, c=1.0):
    """Laser.cpp:177-336 on the laser cells x (nx), y (ny), z (nz; z[-1] is the last laser slice): -> [nz][ny][nx] complex.
    geometry "xyt": data [nt][ny][nx]; "xyz": [nz][ny][nx]; "rt": [modes][nt][nr].  offset = gridGlobalOffset + position *
    gridSpacing and spacing per axis in the file's order.  The sums run in the reference's order."""
    data = np.asarray(data, dtype=np.complex128)
    X, Y, Z = x[None, None, :], y[None, :, None], z[:, None, None]
    zmax = z[-1]
    out = np.zeros((z.size, y.size, x.size), dtype=np.complex128)
    if geometry in ("xyt", "xyz"):
        e0, e1, e2 = data.shape
        ic, sx = shape1((X - offset[2]) / spacing[2])
        jc, sy = shape1((Y - offset[1]) / spacing[1])
        kc, sz = shape1((zmax - Z) / c / spacing[0] if geometry == "xyt" else (Z - offset[0]) / spacing[0])
        for iz in range(2):
            for iy in range(2):
                for ix in range(2):
                    cx, cy, cz = ic + ix, jc + iy, kc + iz
                    valid = (cx >= 0) & (cx < e2) & (cy >= 0) & (cy < e1) & (cz >= 0) & (cz < e0)
                    w = sx[..., ix] * sy[..., iy] * sz[..., iz]
                    out = out + np.where(valid, w * (_take(data, (cz, cy, cx), valid) * unit), 0.0)
        return out
    assert geometry == "rt"
    nm, e1, e2 = data.shape
    r, theta = np.sqrt(X * X + Y * Y), np.arctan2(Y, X)
    ic, sr = shape1((r - offset[1]) / spacing[1])
    kc, st = shape1((zmax - Z) / c / spacing[0])
    assert ic.min() >= 0, "a laser cell reaches a sample index < 0 in r (the reference asserts there)"
    for it in range(2):
        for ir in range(2):
            cr, ct = ic + ir, kc + it
            valid = (cr < e2) & (ct >= 0) & (ct < e1)
            w = sr[..., ir] * st[..., it]
            out = out + np.where(valid, w * (_take(data[0], (ct, cr), valid) * unit), 0.0)
            for im in range(1, nm // 2 + 1):
                out = out + np.where(valid, w * np.cos(im * theta) * (_take(data[2 * im - 1], (ct, cr), valid) * unit), 0.0)
                out = out + np.where(valid, w * np.sin(im * theta) * (_take(data[2 * im], (ct, cr), valid) * unit), 0.0)
    return out


def smallest_r_index(x, y, offset, spacing):
    """floor of the smallest (r - rmin)/dr over the laser cells: < 0 is what the reference asserts against (Laser.cpp:303)"""
    r = math.sqrt(np.abs(x).min() ** 2 + np.abs(y).min() ** 2)
    return math.floor((r - offset[1]) / spacing[1])


# ---- in-situ ---------------------------------------------------------------------------------------------------------------------

ROWS = ("max(|a|^2)", "[|a|^2]", "[|a|^2*x]", "[|a|^2*x*x]", "[|a|^2*y]", "[|a|^2*y*y]")


def mid_cells(n):
    """the one or two middle cells of n and their factor (:944-949)"""
    lo, hi = (n - 1) // 2, n // 2
    return (lo, hi), (1.0 if lo == hi else 0.5)


def insitu(a, x, y, dxdydz):
    """InSituComputeDiags on every plane of a [nz][ny][nx] -> (rows [8][nz], scale [8][nz]): rows 0-5 as ROWS (1-5 times dx dy dz),
    6 and 7 Re and Im of axis(a); scale: what the rounding of a row is relative to -- the row itself for 0, dx dy dz sum |term| for
    1-5, max |a| of the plane for 6 and 7."""
    nz, ny, nx = a.shape
    s = a.real * a.real + a.imag * a.imag
    X, Y = x[None, None, :], y[None, :, None]
    terms = [s, s * X, s * X * X, s * Y, s * Y * Y]
    rows, scale = np.zeros((8, nz)), np.zeros((8, nz))
    rows[0] = s.max(axis=(1, 2))
    scale[0] = rows[0]
    for q, t in enumerate(terms, start=1):
        rows[q] = t.sum(axis=(1, 2)) * dxdydz
        scale[q] = np.abs(t).sum(axis=(1, 2)) * dxdydz
    (xl, xh), fx = mid_cells(nx)
    (yl, yh), fy = mid_cells(ny)
    axis = np.zeros(nz, dtype=np.complex128)
    for j in sorted({yl, yh}):
        for i in sorted({xl, xh}):
            axis = axis + a[:, j, i]
    axis = axis * (fx * fy)
    rows[6], rows[7] = axis.real, axis.imag
    scale[6] = scale[7] = np.abs(a).max(axis=(1, 2))
    return rows, scale


def insitu_sum(rows):
    """the per-step totals the reference writes as "integrated" (:988-996): the maximum of row 0, the sums of rows 1-5"""
    return {name: (rows[q].max() if q == 0 else rows[q].sum()) for q, name in enumerate(ROWS)}
