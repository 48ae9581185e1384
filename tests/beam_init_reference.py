"""numpy restatement of the general fixed_ppc beam (InitBeamFixedPPC3D / InitBeamFixedPPCSlice, particles/beam/
BeamParticleContainerInit.cpp:119-346; get_position_unit_cell, particles/particles_utils/ParticleUtil.H:30-64) as hipace_amd
restates it for the whole box (hipace_amd/csrc/beam_init.hip): lattice, selection, weights, the counter-based draws of
random_ppc and u_std, and the order -- slices head first, then j, i, i_part.  The density is any callable of numpy arrays
(x, y, z): Program.evaluate of hipace_amd/expr.py for a program.  The draws use the restatement of coll_hash in
tests/plasma_thermal_reference.py."""
import numpy as np

from hipace_amd import decks
from tests import plasma_thermal_reference as W

U64 = np.uint64
TAG_POSITION, TAG_MOMENTUM = 0, 1      # second link of the draws' key


def geometry(deck):
    lo, hi = deck["lo"], deck["hi"]
    h = tuple((hi[d] - lo[d]) / deck[n] for d, n in enumerate(("nx", "ny", "nz")))
    c = decks.SI["c"] if deck.get("si_units", 0) else 1.0
    nppc = int(np.prod(deck["beam_ppc"]))
    scale_fac = h[0] * h[1] * h[2] / nppc if deck.get("si_units", 0) else 1.0 / nppc
    return h, c, nppc, scale_fac


def unit_cell(ppc, i_part):
    """get_position_unit_cell: the sub-indices of i_part (arrays), x slowest, then z, y fastest"""
    nyz = ppc[1] * ppc[2]
    return i_part // nyz, (i_part % nyz) % ppc[1], (i_part % nyz) // ppc[1]


def uniform_draws(seed, tag, slots, comp):
    """unit(hash(hash(hash(seed, tag), slot), comp)) in [0, 1)"""
    zk = W.coll_hash(W.coll_hash(U64(seed), U64(tag)), np.asarray(slots, dtype=U64))
    return W.coll_unit(W.coll_hash(zk, U64(comp)))


def normal_deviates(seed, slots):
    """(3, n) standard normal deviates of the slots: Box-Muller as tests/plasma_thermal_reference.normal_deviates -- (n_x, n_y)
    from draws (0, 1), n_z the cosine branch of draws (2, 3) -- on the key hash(hash(seed, TAG_MOMENTUM), slot)"""
    zk = W.coll_hash(W.coll_hash(U64(seed), U64(TAG_MOMENTUM)), np.asarray(slots, dtype=U64))

    def pair(a):
        u1 = 1.0 - W.coll_unit(W.coll_hash(zk, U64(a)))
        u2 = W.coll_unit(W.coll_hash(zk, U64(a + 1)))
        r = np.sqrt(-2.0 * np.log(u1))
        return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)

    n0, n1 = pair(0)
    n2, _ = pair(2)
    return np.stack([n0, n1, n2])


def slice_points(deck, k, random_ppc=(0, 0, 0), seed=1):
    """every lattice point of slice k in the order j, i, i_part: x, y, z, the global slot and the selection by the window"""
    nx, ny, ppc, lo = deck["nx"], deck["ny"], deck["beam_ppc"], deck["lo"]
    h, _, nppc, _ = geometry(deck)
    j, i, ip = np.meshgrid(np.arange(ny), np.arange(nx), np.arange(nppc), indexing="ij")
    j, i, ip = j.ravel(), i.ravel(), ip.ravel()
    slot = ((k * ny + j) * nx + i) * nppc + ip
    sub = unit_cell(ppc, ip)
    r = [(0.5 + sub[d]) / ppc[d] for d in range(3)]
    for d in range(3):
        if random_ppc[d]:
            r[d] = uniform_draws(seed, TAG_POSITION, slot, d)
    x = lo[0] + (i + r[0]) * h[0]
    y = lo[1] + (j + r[1]) * h[1]
    z = lo[2] + (k + r[2]) * h[2]
    if any(random_ppc):      # the cell's lower corner is tested
        tx, ty, tz = lo[0] + i * h[0], lo[1] + j * h[1], np.full(x.shape, lo[2] + k * h[2])
    else:
        tx, ty, tz = x, y, z
    rx, ry = tx - deck["beam_pos_mean"][0], ty - deck["beam_pos_mean"][1]
    rad = deck["beam_radius"]
    inside = ~((tz >= deck["beam_zmax"]) | (tz < deck["beam_zmin"]) | ((rx * rx + ry * ry) > rad * rad))
    return x, y, z, slot, inside


def fixed_ppc_beam(deck, density, min_density=0.0, u_std=(0.0, 0.0, 0.0), random_ppc=(0, 0, 0), seed=1, slices=None):
    """-> dict(soa (7, n) x y z ux uy uz w, off (nz + 1), slot (n), density (n), normal (3, n) the deviates behind the momenta).
    slices: the slice indices to visit (default nz - 1 down to 0: head first); off then counts the visited ones only."""
    _, c, _, scale_fac = geometry(deck)
    nz = deck["nz"]
    ks = list(range(nz - 1, -1, -1)) if slices is None else list(slices)
    parts, off = [], [0]
    for k in ks:
        x, y, z, slot, inside = slice_points(deck, k, random_ppc, seed)
        dens = np.asarray(density(x, y, z), dtype=np.float64)
        keep = inside & ~(dens <= min_density)
        parts.append((x[keep], y[keep], z[keep], slot[keep], dens[keep]))
        off.append(off[-1] + int(keep.sum()))
    x, y, z, slot, dens = (np.concatenate([p[q] for p in parts]) for q in range(5))
    nrm = normal_deviates(seed, slot) if any(u_std) else np.zeros((3, x.size))
    um = deck["beam_umean"]
    u = [(um[d] + u_std[d] * nrm[d]) * c if u_std[d] != 0.0 else np.full(x.size, um[d] * c) for d in range(3)]
    soa = np.stack([x, y, z, u[0], u[1], u[2], np.abs(dens * scale_fac)])
    return dict(soa=soa, off=np.array(off, dtype=np.int64), slot=slot.astype(np.int64), density=dens, normal=nrm)


def flattop_count(deck):
    """closed form of the flat-top beam's particle count for a window that cuts no lattice point in x, y (radius beyond the box):
    nx ny ppc_x ppc_y times the lattice planes z_m = lo_z + (m + 0.5) dz / ppc_z with zmin <= z_m < zmax"""
    h, _, _, _ = geometry(deck)
    ppc = deck["beam_ppc"]
    m = np.arange(deck["nz"] * ppc[2])
    zm = deck["lo"][2] + (m // ppc[2] + (0.5 + m % ppc[2]) / ppc[2]) * h[2]
    planes = int(((zm >= deck["beam_zmin"]) & (zm < deck["beam_zmax"])).sum())
    return deck["nx"] * deck["ny"] * ppc[0] * ppc[1] * planes
