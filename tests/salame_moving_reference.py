"""numpy restatements for the tests of SALAME on a witness species of a moving-beam engine: the moving beam's deposit
of chosen species (k_beam_deposit_dyn<ORDER, 1, 1>, beam.hip), SalameMultiplyBeamWeight on one slice of the container
(k_salame_scale_moving, salame.hip), and the jz-weighted mean of Ez that SALAME holds to its target."""
import numpy as np


def shape(order, xmid):
    """compute_shape_factor of the reference (ShapeFactors.H:27-108): (left-most cell, weights[order + 1])"""
    xmid = np.asarray(xmid, dtype=np.float64)
    if order == 0:
        return np.floor(xmid + 0.5).astype(int), [np.ones_like(xmid)]
    if order == 1:
        xf = np.floor(xmid); t = xmid - xf
        return xf.astype(int), [1.0 - t, t]
    if order == 2:
        xr = np.floor(xmid + 0.5); t = xmid - xr
        return xr.astype(int) - 1, [0.5 * (0.5 - t) ** 2, 0.75 - t * t, 0.5 * (0.5 + t) ** 2]
    xf = np.floor(xmid); t = xmid - xf; u = 1.0 - t
    return xf.astype(int) - 1, [u ** 3 / 6.0, 2.0 / 3.0 - t * t * (1.0 - 0.5 * t), 2.0 / 3.0 - u * u * (1.0 - 0.5 * u), t ** 3 / 6.0]


def geometry(deck):
    """-> (dx, dy, dz, xoff, yoff, guard cells, c) as the engine derives them from the deck (Engine::create)"""
    nx, ny, nz = deck["nx"], deck["ny"], deck["nz"]
    lo, hi = deck["lo"], deck["hi"]
    dx, dy, dz = (hi[0] - lo[0]) / nx, (hi[1] - lo[1]) / ny, (hi[2] - lo[2]) / nz
    xoff = 0.5 * (lo[0] + hi[0] - dx * (nx - 1))
    yoff = 0.5 * (lo[1] + hi[1] - dy * (ny - 1))
    g = (deck["order"] + 1) // 2 + 1
    return dx, dy, dz, xoff, yoff, g, (299792458.0 if deck.get("si_units", 0) else 1.0)


def deposit(deck, soa, charges, live=None, absolute=False):
    """BeamDepositCurrent on the particles soa (7, n) with per-particle charge `charges` (n,): -> (jx, jy, jz), each a padded
    plane (ny + 2g, nx + 2g).  live: mask of the particles that deposit (default: all).  absolute: every term's magnitude is
    deposited instead -- the size of what a cell's sum is rounded against."""
    dx, dy, dz, xoff, yoff, g, c = geometry(deck)
    nx, ny, order = deck["nx"], deck["ny"], deck["order"]
    out = np.zeros((3, ny + 2 * g, nx + 2 * g))
    soa = np.asarray(soa, dtype=np.float64)
    if live is not None:
        soa, charges = soa[:, live], np.asarray(charges)[live]
    if soa.shape[1] == 0:
        return out
    x, y, _, ux, uy, uz, w = soa
    invvol = 1.0 / (dx * dy * dz) if deck.get("si_units", 0) else 1.0
    csq_inv = 1.0 / (c * c)
    gaminv = 1.0 / np.sqrt(1.0 + ux * ux * csq_inv + uy * uy * csq_inv + uz * uz * csq_inv)
    wq = np.asarray(charges, dtype=np.float64) * invvol * w
    i0, sx = shape(order, (x - xoff) * (1.0 / dx))
    j0, sy = shape(order, (y - yoff) * (1.0 / dy))
    for iy in range(order + 1):
        for ix in range(order + 1):
            s = sx[ix] * sy[iy]
            for q, u in enumerate((ux, uy, uz)):
                t = s * (wq * (u * gaminv))
                np.add.at(out[q], (j0 + iy + g, i0 + ix + g), np.abs(t) if absolute else t)
    return out


def slice_range(bnd, nz, islice):
    """the container's index range of slice islice (block nz - 1 - islice from the head)"""
    p = nz - 1 - islice
    return int(bnd[p]), int(bnd[p + 1])


def scale(soa, tags, bnd, nz, islice, species, W):
    """SalameMultiplyBeamWeight (Salame.cpp:407-435) on slice islice of a container nobody has slipped into: -> the weight row
    afterwards; the selected particles' w * W in one rounding (an exact 0 for W = 0), every other weight as it was"""
    w = np.array(soa[6], dtype=np.float64)
    a, b = slice_range(bnd, nz, islice)
    sel = np.zeros(w.size, dtype=bool)
    sel[a:b] = np.isin(tags[a:b], list(species))
    w[sel] = 0.0 if W == 0.0 else w[sel] * W
    return w, sel


def weighted_mean_ez(ez_next, jz):
    """sum(jz Ez) / sum(jz) over the valid cells: what SalameGetW forms of the slice behind the beam slice"""
    return float((jz * ez_next).sum() / jz.sum())


def flatness(ez, jz_of, slices, dz, lo_z, slope=0.0):
    """ez [nz, ny, nx]; jz_of[k]: the SALAME beam's own jz on its slice k (valid cells).  -> (largest deviation of the jz-weighted
    mean of Ez on slice k - 1 from the target Ez_initial + slope (zeta - zeta_initial) over `slices`, Ez_initial): the measure of
    tests/test_salame_gpu.py::_flatness with the beam's current given instead of taken from the jz_beam diagnostic, which in a
    driver + witness engine holds the driver's current too"""
    head = max(slices)
    ez0 = weighted_mean_ez(ez[head], jz_of[head])
    zeta = lambda k: (k - 1) * dz + lo_z + 0.5 * dz
    z0 = head * dz + lo_z + 0.5 * dz
    dev = max(abs(weighted_mean_ez(ez[k - 1], jz_of[k]) - (ez0 + slope * (zeta(k) - z0))) for k in slices)
    return dev, ez0
