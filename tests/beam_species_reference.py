"""numpy restatement of what an engine with several beam species does to its container, and the beams the species
tests share.  merge(): the binning of hps_engine_set_beam_particles (slice = int((z - lo_z)/dz), head slice first, input order
kept) per species, then inside every slice the species in the order they were filled."""
import numpy as np

from tests import external_field_reference as R


def bin_species(soa, lo_z, dz, nz):
    """-> (slice p counted from the head, per particle; -1: outside the box), as the engine's cast does"""
    t = (np.asarray(soa[2], dtype=np.float64) - lo_z) * (1.0 / dz)
    q = np.where((t > -1.0e9) & (t < 1.0e9), np.trunc(t), -1).astype(np.int64)      # (the cast truncates towards zero)
    return np.where((q < 0) | (q >= nz), -1, nz - 1 - q)


def merge(species, lo_z, dz, nz):
    """species: list of (7, n_k) arrays in fill order -> (B int64 [nz + 1], soa (7, n), tags uint8 [n], counts [k]) of the
    merged container"""
    where = [bin_species(s, lo_z, dz, nz) for s in species]
    cols, tags, B = [], [], [0]
    for p in range(nz):
        for k, (s, w) in enumerate(zip(species, where)):
            sel = np.flatnonzero(w == p)
            cols.append(np.asarray(s)[:, sel])
            tags.append(np.full(sel.size, k, dtype=np.uint8))
        B.append(B[-1] + sum(int((w == p).sum()) for w in where))
    soa = np.concatenate(cols, axis=1) if cols else np.zeros((7, 0))
    return np.array(B, dtype=np.int64), soa, np.concatenate(tags) if tags else np.zeros(0, np.uint8), [int((w >= 0).sum()) for w in where]


def moments(soa, nsub_ok=None, c=1.0):
    """{sum w, sum w uz/c, sum w (uz/c)^2, min uz/c} over the particles of soa (absorbed ones carry w = 0 and are left out by
    the caller)"""
    w, u = soa[6], soa[5] / c
    if w.size == 0:
        return np.array([0.0, 0.0, 0.0, np.inf])
    return np.array([w.sum(), (w * u).sum(), (w * u * u).sum(), u.min()])


# ---- the beams of tests/test_beam_species_gpu.py: the 32 x 32 x 12 vacuum box of external_field_reference (dz = 0.4) ----------
def fingerprint(soa, base, k):
    """weights base*(1 + 1e-6 (k 10^5 + i)): far below one ulp of any external field once deposited, and every particle of every
    species carries its own"""
    out = np.array(soa, dtype=np.float64)
    out[6] = base * (1.0 + 1.0e-6 * (k * 100000 + np.arange(out.shape[1])))
    return out


def three_species(base=1.0e-200):
    """[(record, (7, n) particles)] x 3 on the vacuum box: A the 333 particles of vacuum_beam (slow ones that slip in mid-step,
    one that leaves through the wall, slices 4 and 11 empty); B 2600 positrons of twice the mass on slices 2 and 3 (more than
    2048 in slice 2: the partition's 1024-lane stride wraps twice there), not pushed in z; C 150 heavy particles on slices
    5 .. 10, twelve of them with u_z = 0.1 (0.81 backwards per step of 0.9: through two slices of 0.4).  Slices 0 and 1 hold A
    alone, slices 4 and 11 nobody."""
    rng = np.random.default_rng(7)
    a = R.vacuum_beam(333)
    nb = 2600
    b = np.zeros((7, nb))
    b[0], b[1] = rng.uniform(-1.0, 1.0, nb), rng.uniform(-1.0, 1.0, nb)
    b[2] = -2.4 + 2 * 0.4 + rng.uniform(0.01, 0.79, nb)
    b[2, :2200] = -2.4 + 2 * 0.4 + rng.uniform(0.01, 0.39, 2200)      # slice 2: 2200 and what the line above left there
    b[3], b[4], b[5] = rng.normal(0.0, 0.4, nb), rng.normal(0.0, 0.4, nb), 20.0 + rng.normal(0.0, 1.0, nb)
    nc = 150
    c = np.zeros((7, nc))
    c[0], c[1] = rng.uniform(-1.0, 1.0, nc), rng.uniform(-1.0, 1.0, nc)
    c[2] = -2.4 + 5 * 0.4 + rng.uniform(0.02, 6 * 0.4 - 0.02, nc)     # slices 5 .. 10
    c[3], c[4], c[5] = rng.normal(0.0, 0.3, nc), rng.normal(0.0, 0.3, nc), 40.0 + rng.normal(0.0, 2.0, nc)
    c[5, :12] = 0.1
    c[3, :12] = c[4, :12] = 0.0
    c[2, :12] = -2.4 + 10 * 0.4 + rng.uniform(0.2, 0.38, 12)         # (five such steps end above the box's lower end)
    recs = [dict(charge=-1.0, mass=1.0, n_subcycles=4, do_z_push=True),
            dict(charge=1.0, mass=2.0, n_subcycles=7, do_z_push=False),
            dict(charge=-1.0, mass=5.0, n_subcycles=2, do_z_push=True)]
    return [(r, fingerprint(s, base, k)) for k, (r, s) in enumerate(zip(recs, (a, b, c)))]


def one_species_deck(deck, rec, rr=None):
    """the deck of a one-species engine with this species' constants"""
    return dict(deck, beam_charge=rec["charge"], beam_mass=rec["mass"], beam_n_subcycles=rec["n_subcycles"],
                beam_no_z_push=int(not rec["do_z_push"]),
                beam_radiation_reaction=int(rec.get("radiation_reaction", 0) if rr is None else rr))


def by_weight(soa):
    """the particles that still carry their fingerprint (w != 0: not absorbed), sorted by it -> (7, m)"""
    live = soa[:, soa[6] != 0.0]
    return live[:, np.argsort(live[6], kind="stable")]


def ulps(a, b):
    s = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.finfo(float).tiny)
    return float((np.abs(a - b) / np.spacing(s)).max()) if a.size else 0.0
