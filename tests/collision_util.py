"""Helpers shared by the GPU tests of both kinds of Coulomb collision (tests/test_collisions_gpu.py and
tests/test_beam_collisions_gpu.py): sheets of the numpy restatement to and from the device, the 8 x 8 box of the operator
cases, the deviation measure, and access to an engine's own sheet."""
import ctypes as C

import numpy as np

from tests import collision_reference as R


def to_gpu(api, s):
    n = len(s["x"])
    real = np.zeros((11, n))
    real[0], real[1], real[2] = s["x"], s["y"], s["w"]
    real[3], real[4], real[5] = s["ux"], s["uy"], s["psi"]
    real[6], real[7] = s["x"], s["y"]
    real[8], real[9], real[10] = s["ux"], s["uy"], s["psi"]
    return api.PlasmaSheet(real, valid=s["valid"], ion_lev=s["ion_lev"], key=s["key"])


def from_gpu(sheet):
    real, _ = sheet.numpy()
    return real[8], real[9], real[10]


def geometry(api, lo, dx, si):
    hi = (lo[0] + R.NX * dx, lo[1] + R.NY * dx)
    consts = (R.C_SI, R.EP0, 4.0e-7 * np.pi, R.QE, R.ME) if si else (1.0,) * 5
    return api.Geometry(R.NX, R.NY, lo, hi, dx, bc=1, normalized=not si, consts=consts)


def deviation(s_ref, gpu, c, lo, dx):
    """max over particles of |du| / rms(u of the cell), u = (ux, uy, c psi) as the collisions leave them"""
    worst = 0.0
    for cell, lst in R.cell_lists(s_ref, R.NX, R.NY, lo, dx, dx).items():
        ref = np.stack([s_ref["ux"][lst], s_ref["uy"][lst], c * s_ref["psi"][lst]])
        got = np.stack([gpu[0][lst], gpu[1][lst], c * gpu[2][lst]])
        rms = np.sqrt((ref[:2] ** 2).sum() / len(lst))      # (psi is about 1: the thermal u sets the scale, c psi rounds finer)
        worst = max(worst, np.abs(got - ref).max() / rms)
    return worst


def sheet_arrays(api, p):
    from hipace_amd import _lib
    n = p.n
    real = np.empty((11, n))
    idc = np.empty(n, dtype=np.uint64)
    lev = np.empty(n, dtype=np.int32)
    for k, nm in enumerate(_lib.PL_REAL):
        _lib.check(_lib.lib().hps_memcpy_d2h(real[k].ctypes.data_as(C.c_void_p), C.c_void_p(getattr(p, nm)), real[k].nbytes))
    _lib.check(_lib.lib().hps_memcpy_d2h(idc.ctypes.data_as(C.c_void_p), C.c_void_p(p.idcpu), idc.nbytes))
    _lib.check(_lib.lib().hps_memcpy_d2h(lev.ctypes.data_as(C.c_void_p), C.c_void_p(p.ion_lev), lev.nbytes))
    return real, idc, lev


def write_thermal(p, seed, u_std):
    from hipace_amd import _lib
    rng = np.random.default_rng(seed)
    for nm in ("ux_half", "uy_half"):
        u = rng.normal(0.0, u_std, p.n)
        _lib.check(_lib.lib().hps_memcpy_h2d(C.c_void_p(getattr(p, nm)), u.ctypes.data_as(C.c_void_p), u.nbytes))


def small_deck(deck, **kw):
    d = dict(deck, nx=32, ny=32, nz=8, n_steps=1, plasma_ppc=(2, 2))
    d["lo"] = tuple(d["lo"][:2]) + (d["lo"][2] * 0.08,)
    d["hi"] = tuple(d["hi"][:2]) + (d["hi"][2] * 0.08,)
    d.update(kw)
    return d


def sheet_from(api, real, idc, lev):
    key = ((idc >> np.uint64(24)) & np.uint64((1 << 39) - 1)).astype(np.int64) - 1
    return api.PlasmaSheet(real, valid=((idc >> np.uint64(63)) & np.uint64(1)).astype(np.int32), ion_lev=lev, key=key)
