"""beams.external_E / external_B as expression programs, the parts that need no GPU: the compiler
(hipace_amd/expr.py) against plain numpy and against the C routine on the host (hps_expr_eval_host), the check's refusals,
the Python refusals, the ABI, the decks, and the pin of the numpy restatement of the beam push
(tests/external_field_reference.py) against the oracle.

libm: hps_expr_eval_host calls the C library's functions, Program.evaluate numpy's (its own SIMD kernels for some).  Measured
here over the table below (worst element per row, in ulps of the result): 0 for + - * / sqrt, comparisons, selects, abs,
floor, ceil, fmod, min, max, heaviside and the integer powers (asserted bit-equal), and for log, log10, sin, cos, erf; 1 ulp
for pow, exp, tan, asin, acos, atan, atan2, sinh, cosh; 2 ulps for tanh; 0.5 and 1 ulp of the largest term for the two rows
that add several functions up.  Both libraries document errors of at most a few ulps; the assertion is 4 ulps."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from hipace_amd import _lib, decks, expr
from tests import external_field_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RNG = np.random.default_rng(7)
N = 257
X, Y, Z, T = [RNG.uniform(-2.0, 2.0, N) for _ in range(4)]
X[:4] = [0.0, -0.0, 1.0, -1.0]      # heaviside(0, .), fmod and comparisons at equality
Y[:4] = [0.0, 1.0, 1.0, -1.0]
KP, E0 = 0.75, 3.0
CONSTS = dict(kp=KP, E0=E0)
H = lambda a, b: np.where(a < 0, 0.0, np.where(a == 0, b, 1.0))      # noqa: E731
B2F = lambda m: m.astype(np.float64)                                  # noqa: E731

# (expression, the same formula in plain numpy, exact = only + - * / sqrt, comparisons, selects and their kin)
TABLE = [
    ("x + y", lambda x, y, z, t: x + y, True),
    ("x - y", lambda x, y, z, t: x - y, True),
    ("x * y", lambda x, y, z, t: x * y, True),
    ("x / y", lambda x, y, z, t: x / y, True),
    ("-x", lambda x, y, z, t: -x, True),
    ("+x", lambda x, y, z, t: x, True),
    ("-x^2", lambda x, y, z, t: -(x * x), True),
    ("2^3^2", lambda x, y, z, t: np.full_like(x, 512.0), True),
    ("x**3", lambda x, y, z, t: x * x * x, True),
    ("x^-2", lambda x, y, z, t: 1.0 / (x * x), True),
    ("y^8", lambda x, y, z, t: ((((((y * y) * y) * y) * y) * y) * y) * y, True),
    ("x^0", lambda x, y, z, t: np.ones_like(x), True),
    ("abs(x)^y", lambda x, y, z, t: np.power(np.abs(x), y), False),
    ("pow(abs(x), 2.5)", lambda x, y, z, t: np.power(np.abs(x), 2.5), False),
    ("pow(x, 2)", lambda x, y, z, t: x * x, True),
    ("(x + y) * (z - t) / (1 + x*x)", lambda x, y, z, t: (x + y) * (z - t) / (1 + x * x), True),
    ("1/2*kp*E0*x", lambda x, y, z, t: 1 / 2 * KP * E0 * x, True),
    ("x < y", lambda x, y, z, t: B2F(x < y), True),
    ("x <= y", lambda x, y, z, t: B2F(x <= y), True),
    ("x > y", lambda x, y, z, t: B2F(x > y), True),
    ("x >= y", lambda x, y, z, t: B2F(x >= y), True),
    ("x == y", lambda x, y, z, t: B2F(x == y), True),
    ("x != y", lambda x, y, z, t: B2F(x != y), True),
    ("x > 0 and y > 0", lambda x, y, z, t: B2F((x > 0) & (y > 0)), True),
    ("x > 0 or y > 0", lambda x, y, z, t: B2F((x > 0) | (y > 0)), True),
    ("not x > 0", lambda x, y, z, t: B2F(~(x > 0)), True),
    ("x > 0 and y > 0 or not z > 0 and t < 1", lambda x, y, z, t: B2F(((x > 0) & (y > 0)) | (~(z > 0) & (t < 1))), True),
    ("if(x > y, x, y)", lambda x, y, z, t: np.where(x > y, x, y), True),
    ("if(z > -0.2, 0.2*y, -0.1*y)", lambda x, y, z, t: np.where(z > -0.2, 0.2 * y, -0.1 * y), True),
    ("if(x > 0, if(y > 0, 1, 2), if(z > 0, 3, 4*t))", lambda x, y, z, t: np.where(x > 0, np.where(y > 0, 1.0, 2.0), np.where(z > 0, 3.0, 4 * t)), True),
    ("sqrt(abs(x))", lambda x, y, z, t: np.sqrt(np.abs(x)), True),
    ("abs(x)", lambda x, y, z, t: np.abs(x), True),
    ("floor(3*x)", lambda x, y, z, t: np.floor(3 * x), True),
    ("ceil(3*x)", lambda x, y, z, t: np.ceil(3 * x), True),
    ("fmod(x, y)", lambda x, y, z, t: np.fmod(x, y), True),
    ("fmod(5*x, 0.7)", lambda x, y, z, t: np.fmod(5 * x, 0.7), True),
    ("min(x, y)", lambda x, y, z, t: np.where(x < y, x, y), True),
    ("max(x, y)", lambda x, y, z, t: np.where(x > y, x, y), True),
    ("heaviside(x, 0.5)", lambda x, y, z, t: H(x, 0.5), True),
    ("heaviside(x, y)", lambda x, y, z, t: H(x, y), True),
    ("exp(x)", lambda x, y, z, t: np.exp(x), False),
    ("log(abs(x) + 0.1)", lambda x, y, z, t: np.log(np.abs(x) + 0.1), False),
    ("log10(abs(x) + 0.1)", lambda x, y, z, t: np.log10(np.abs(x) + 0.1), False),
    ("sin(3*x)", lambda x, y, z, t: np.sin(3 * x), False),
    ("cos(3*x)", lambda x, y, z, t: np.cos(3 * x), False),
    ("tan(x/2)", lambda x, y, z, t: np.tan(x / 2), False),
    ("asin(x/2)", lambda x, y, z, t: np.arcsin(x / 2), False),
    ("acos(x/2)", lambda x, y, z, t: np.arccos(x / 2), False),
    ("atan(x)", lambda x, y, z, t: np.arctan(x), False),
    ("atan2(y, x)", lambda x, y, z, t: np.arctan2(y, x), False),
    ("sinh(x)", lambda x, y, z, t: np.sinh(x), False),
    ("cosh(x)", lambda x, y, z, t: np.cosh(x), False),
    ("tanh(x)", lambda x, y, z, t: np.tanh(x), False),
    ("erf(x)", None, False),
    ("E0*cos(kp*t)*exp(-x^2/2) + pi", lambda x, y, z, t: E0 * np.cos(KP * t) * np.exp(-(x * x) / 2) + np.pi, False),
    ("sin(x) + cos(y)*tan(z/2) + exp(t) + atan2(x, y) + log(abs(x) + 1) + sinh(x) + tanh(y)",
     lambda x, y, z, t: np.sin(x) + np.cos(y) * np.tan(z / 2) + np.exp(t) + np.arctan2(x, y) + np.log(np.abs(x) + 1) + np.sinh(x) + np.tanh(y), False),
    ("clight*mu0*epsilon0*clight + q_e/m_e*1e-11 + m_p/m_e + hbar/r_e*1e19 + true - false",
     lambda x, y, z, t: np.full_like(x, 299792458.0 * 1.25663706212e-06 * 8.8541878128e-12 * 299792458.0 + 1.602176634e-19 / 9.1093837015e-31 * 1e-11
                                     + 1.67262192369e-27 / 9.1093837015e-31 + 1.054571817e-34 / 2.817940326204929e-15 * 1e19 + 1.0 - 0.0), True),
]


SUMS = {len(TABLE) - 3, len(TABLE) - 2}      # "E0*cos(...)... + pi" (terms up to 3 + pi) and the sum of seven functions (exp(t) up to 7.4)


def _deep(n):
    """a right-nested sum whose stack reaches exactly n values: x + (x + ( ... + x))"""
    return "x + (" * (n - 1) + "x" + ")" * (n - 1)


def _long(n_ins):
    """a left-nested sum of n_ins instructions (odd): x + y + x + y ..."""
    terms = (n_ins + 1) // 2
    return " + ".join("xy"[k % 2] for k in range(terms))


TABLE += [
    (_deep(16), lambda x, y, z, t: _sum_right(x, 16), True),
    (_long(255), lambda x, y, z, t: _sum_left(x, y, 128), True),
]


def _sum_right(x, n):
    r = x
    for _ in range(n - 1):
        r = x + r
    return r


def _sum_left(x, y, terms):
    r = x
    for k in range(1, terms):
        r = r + (x, y)[k % 2]
    return r


def _host(prog, *arrays):
    e, keep = prog.c_struct()
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in arrays]
    out = np.empty(a[0].shape)
    ptrs = (C.c_void_p * max(len(a), 1))(*[v.ctypes.data for v in a])
    _lib.check(_lib.lib().hps_expr_eval_host(C.byref(e), len(a), out.size, ptrs, out.ctypes.data_as(C.c_void_p)))
    return out


def _ulps(a, b, scale=None):
    """largest |a - b| in units of the spacing of doubles at `scale` (default: at the values themselves)"""
    ok = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~ok & ~np.isnan(a)], b[~ok & ~np.isnan(b)])
    if not ok.any():
        return 0.0
    s = np.maximum(np.abs(a[ok]), np.abs(b[ok])) if scale is None else scale[ok]
    return float((np.abs(a[ok] - b[ok]) / np.spacing(np.maximum(s, np.finfo(float).tiny))).max())


def test_the_table_is_as_large_as_asked_and_covers_every_opcode():
    assert len(TABLE) >= 40
    used = set()
    for text, _, _ in TABLE:
        used |= {op for op, _ in expr.compile_expr(text, constants=CONSTS, fold=False).ins}
    assert used == set(expr.OPS), set(expr.OPS) - used
    assert expr.compile_expr(_deep(16)).depth == 16 and len(expr.compile_expr(_long(255)).ins) == 255


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_three_evaluators_agree(row):
    text, formula, exact = TABLE[row]
    prog = expr.compile_expr(text, constants=CONSTS)
    with np.errstate(all="ignore"):
        mine = prog.evaluate(X, Y, Z, T)
        host = _host(prog, X, Y, Z, T)
        if formula is not None:
            plain = np.broadcast_to(formula(X, Y, Z, T), X.shape)
            if exact:
                assert np.array_equal(mine, plain, equal_nan=True), text
            else:
                assert _ulps(mine, plain) == 0.0, text      # the same numpy calls in the same order
    if exact:
        assert np.array_equal(host, mine, equal_nan=True), text
    else:
        # a sum of terms is compared in ulps of its largest term: cancellation amplifies a term's last bit
        scale = np.abs(mine) + 8.0 if row in SUMS else None
        u = _ulps(host, mine, scale)
        print(f"{text}: host against numpy {u:.2f} ulp")
        assert u <= 4.0, (text, u)


def test_the_256_instruction_program_runs_and_one_more_is_refused():
    text = _long(255) + " + 0.5"      # 257 instructions
    with pytest.raises(ValueError, match="too many instructions"):
        expr.compile_expr(text)
    p = expr.compile_expr(_long(255))
    p256 = expr.Program(p.ins + [("neg", 0)], p.consts, p.variables)
    assert len(p256.ins) == 256
    assert np.array_equal(_host(p256, X, Y, Z, T), -_sum_left(X, Y, 128))


def test_folding_changes_no_value_and_finds_the_constant_zero():
    for text, _, _ in TABLE:
        a = expr.compile_expr(text, constants=CONSTS)
        b = expr.compile_expr(text, constants=CONSTS, fold=False)
        assert len(a.ins) <= len(b.ins)
        with np.errstate(all="ignore"):
            assert np.array_equal(a.evaluate(X, Y, Z, T), b.evaluate(X, Y, Z, T), equal_nan=True), text
    p = expr.compile_expr("2*kp*E0 + sqrt(2)/3", constants=CONSTS)
    assert p.is_constant and p.consts == [2 * KP * E0 + np.sqrt(2.0) / 3]
    for zero in ("0", "0.", 0, 0.0, "kp - kp", "0*pi", "if(1 > 2, 5, 0)", "-0.0"):
        assert expr.compile_expr(zero, constants=CONSTS).is_zero, zero
    for not_zero in ("x - x", "0*x", "1e-300", "kp"):
        assert not expr.compile_expr(not_zero, constants=CONSTS).is_zero, not_zero
    # constants as expression strings, resolved recursively
    p = expr.compile_expr("kp_inv*x", constants=dict(ne=1.25e24, kp_inv="clight / sqrt(ne * q_e^2  / (epsilon0 * m_e))"))
    kp_inv = 299792458.0 / np.sqrt(1.25e24 * (1.602176634e-19 * 1.602176634e-19) / (8.8541878128e-12 * 9.1093837015e-31))
    assert p.consts == [kp_inv] and np.array_equal(p.evaluate(X, Y, Z, T), kp_inv * X)


def _raw(ins, consts, n_vars=4):
    ia = (_lib.ExprIns * max(len(ins), 1))(*[_lib.ExprIns(o, a) for o, a in ins])
    ca = (C.c_double * max(len(consts), 1))(*consts)
    e = _lib.Expr(len(ins), len(consts), C.cast(ia, C.POINTER(_lib.ExprIns)), C.cast(ca, C.POINTER(C.c_double)))
    depth = C.c_int(-1)
    st = _lib.lib().hps_expr_check(C.byref(e), n_vars, C.byref(depth))
    return st, depth.value, _lib.lib().hps_last_error().decode(), (e, ia, ca)


def test_check_refuses_broken_programs_each_with_its_message():
    O = expr.OP
    var = lambda k: (O["var"], k)      # noqa: E731
    add = (O["add"], 0)
    assert _raw([var(0), var(1), add], [])[:2] == (0, 2)
    cases = [
        ([var(0), (99, 0)], [], "bad opcode"),
        ([var(0), (-1, 0)], [], "bad opcode"),
        ([var(4)], [], "variable index beyond n_vars"),
        ([(O["const"], 1)], [1.0], "constant index outside the pool"),
        ([(O["const"], 0)], [], "constant index outside the pool"),
        ([var(0), (O["powi"], 9)], [], "integer power beyond HPS_EXPR_MAX_POWI"),
        ([var(0), add], [], "stack underflow"),
        ([(O["select"], 0)], [], "stack underflow"),
        ([var(0), var(1)], [], "does not end with exactly one value"),
        ([var(0)] * 17 + [add] * 16, [], "stack overflow"),
        ([var(0)] + [var(1), add] * 128, [], "more than HPS_EXPR_MAX_INS instructions"),
        ([var(0)], [0.0] * 65, "more than HPS_EXPR_MAX_CONST constants"),
        ([], [], "empty program"),
    ]
    for ins, consts, msg in cases:
        st, _, err, _ = _raw(ins, consts)
        assert st == 1 and msg in err and err.startswith("hps_expr_check: "), (msg, st, err)
    assert len([var(0)] + [var(1), add] * 128) == 257
    assert _raw([var(0)] * 16 + [add] * 15, [])[:2] == (0, 16)
    assert "more than HPS_EXPR_MAX_VARS" in _raw([var(0)], [], n_vars=9)[2]
    # the evaluators check first: nothing runs from a broken program
    e = _raw([var(0), add], [])[3][0]
    out = np.full(3, 7.0)
    ptrs = (C.c_void_p * 4)(*[X.ctypes.data] * 4)
    assert _lib.lib().hps_expr_eval_host(C.byref(e), 4, 3, ptrs, out.ctypes.data_as(C.c_void_p)) == 1
    assert "hps_expr_eval_host: stack underflow" in _lib.lib().hps_last_error().decode() and np.all(out == 7.0)
    assert _lib.lib().hps_expr_eval(C.byref(e), 4, 3, ptrs, out.ctypes.data_as(C.c_void_p), None) == 1      # refused ahead of any device call
    assert "hps_expr_eval: stack underflow" in _lib.lib().hps_last_error().decode()


@pytest.mark.parametrize("text,what,token", [
    ("x + foo", "unknown name", "foo"), ("bar(x)", "unknown name", "bar"), ("sin(x, y)", "wrong arity", "sin"),
    ("atan2(x)", "wrong arity", "atan2"), ("if(x, 1)", "wrong arity", "if"), ("heaviside(x)", "wrong arity", "heaviside"),
    ("x $ y", "unsupported syntax", "$"), ("x +", "unsupported syntax", ""), ("x < y < z", "unsupported syntax", "x < y < z"),
    ("x[0]", "unsupported syntax", "x[0]"), ("'a'", "unsupported syntax", "'a'"), ("x % y", "unsupported syntax", "x % y"),
    ("a1*x", "cyclic constants", "a1 -> a2 -> a1"), (_deep(17), "too deep", ""), (_long(257), "too many instructions", ""),
])
def test_python_refusals_name_the_token(text, what, token):
    with pytest.raises(ValueError) as e:
        expr.compile_expr(text, constants=dict(a1="a2 + 1", a2="2*a1"))
    assert what in str(e.value) and token in str(e.value), str(e.value)


def test_two_or_four_components_are_refused():
    for comps in (("x", "y"), ("x", "y", "z", "t"), "x", ()):
        with pytest.raises(ValueError, match="three components"):
            expr.compile_components(comps, "beams.external_E")
    assert expr.compile_components(None, "beams.external_B") is None
    three = expr.compile_components((".5*x", 0.5, "0."), "beams.external_E")
    assert [p.is_zero for p in three] == [False, False, True] and three[1].consts == [0.5]


def test_header_and_sigs_carry_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "hpslice.h")).read()
    for name, nargs in (("hps_expr_check", 3), ("hps_expr_eval_host", 5), ("hps_expr_eval", 6), ("hps_engine_set_beam_external_fields", 3)):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert len(_lib._SIGS[name][1]) == nargs
    for name, value in (("HPS_EXPR_MAX_INS", expr.MAX_INS), ("HPS_EXPR_MAX_DEPTH", expr.MAX_DEPTH), ("HPS_EXPR_MAX_CONST", expr.MAX_CONST),
                        ("HPS_EXPR_MAX_POWI", expr.MAX_POWI), ("HPS_EXPR_MAX_VARS", expr.MAX_VARS)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1)) == value
    enum = re.search(r"enum \{ (HPS_EX_CONST = 0.*?) \};", hdr, re.S).group(1)
    names = [n.strip().split(" ")[0] for n in enum.split(",")]
    assert names == ["HPS_EX_" + n.upper() for n in expr.OPS] + ["HPS_EX_NOPS"]
    assert (expr.MAX_INS, expr.MAX_DEPTH, expr.MAX_CONST) == (256, 16, 64)


# the keys beam_evolution() and blowout_wake_SI() returned before this feature
_DEFAULT_KEYS = set("""nx ny nz lo hi order deriv_type plasma_ppc plasma_density plasma_radius plasma_charge plasma_mass max_qsa n_subcycles
beam_profile beam_zmin beam_zmax beam_radius beam_density beam_umean beam_pos_mean beam_pos_std beam_ppc beam_charge bc mg_tol_rel
mg_tol_abs deposit_rho n_steps dt beam_n_subcycles beam_mass ext_E_slope bxby_solver predcorr_tol predcorr_max_iter predcorr_mix
field_bc laser_on laser_a0 laser_w0 laser_L0 laser_lambda0 laser_pos laser_zfoc laser_solver beam_radiation_reaction
background_density_SI beam_no_z_push laser_mg_tol_rel laser_mg_tol_abs laser_use_phase grid_current_on grid_current_peak
grid_current_mean grid_current_std si_units plasma_no_neutralize ion_on ion_ppc ion_density ion_mass ion_charge ion_init_level ion_Z
ion_energies ion_seed beam_spin_tracking beam_initial_spin beam_spin_anom""".split())


def test_existing_decks_keep_their_keys_and_the_parsed_deck_differs_in_the_slopes_and_the_entry():
    assert set(decks.beam_evolution()) == _DEFAULT_KEYS
    assert set(decks.blowout_wake_SI()) == _DEFAULT_KEYS
    assert "beam_external_fields" not in decks._DEFAULT and "beam_external_fields" not in decks.ADAPTIVE_DEFAULT
    a, b = decks.beam_evolution(), decks.beam_evolution_parsed()
    assert set(b) - set(a) == {"beam_external_fields"} and set(a) <= set(b)
    assert {k for k in a if a[k] != b[k]} == {"ext_E_slope"}
    assert a["ext_E_slope"] == (0.5, 0.5) and b["ext_E_slope"] == (0.0, 0.0)
    assert b["beam_external_fields"] == dict(E=(".5*x", ".5*y", "0."))
    E = expr.compile_components(b["beam_external_fields"]["E"], "E")
    assert [p.is_zero for p in E] == [False, False, True]
    assert np.array_equal(E[0].evaluate(X, Y, Z, T), 0.5 * X) and np.array_equal(E[1].evaluate(X, Y, Z, T), 0.5 * Y)


@pytest.mark.parametrize("bc,spin", [(2, False), (0, True), (1, False)])
def test_restatement_reproduces_the_oracle_in_a_linear_field(oracle, bc, spin):
    """The pin of tests/external_field_reference.py: E = (s0 x, s1 y, 0) from Program.evaluate, B = 0, against the oracle run
    with the deck's ext_E_slope = (s0, s1) on the zero-weight beam of the GPU tests in a deck without plasma -- every grid
    field is exactly zero, so the oracle's gather adds nothing.  (The oracle has no z slope: s2 = 0 here; the z term of the
    restatement is pinned on the GPU against the engine's ext_Ez_slope path.)  Every surviving particle, every quantity, to
    1e-13 of the quantity's maximum; the oracle drops the absorbed particle, the restatement marks it."""
    s0, s1 = R.LINEAR_SLOPES[:2]
    deck = R.vacuum_deck(order=2, spin=spin, bc=bc)
    soa = R.vacuum_beam()
    ref = R.BeamRestatement(deck, soa, R.compile_fields((f"{s0}*x", f"{s1}*y", "0")))
    for _ in range(deck["n_steps"]):
        ref.run_step()
    assert ref.n_absorbed == (1 if bc == 2 else 0) and ref.n_slipped_mid_step >= 3 and not (ref.islice < 0).any()
    odeck = dict(deck, ext_E_slope=(s0, s1))
    orc = oracle.Engine(odeck)
    assert orc.set_beam_particles(soa) == 0
    orc.run()
    scale = np.abs(ref.state()[:, ref.alive]).max(axis=1)
    seen = 0
    for isl in range(deck["nz"]):
        want = orc.beam_slice(isl)
        idx = np.flatnonzero(ref.alive & (ref.islice == isl))
        assert want.shape[1] == idx.size, (isl, want.shape, idx.size)
        if idx.size == 0:
            continue
        ko, kr = np.lexsort((want[1], want[0])), np.lexsort((ref.y[idx], ref.x[idx]))
        got = ref.state()[:, idx[kr]]
        for q in range(6):
            assert np.abs(got[q] - want[q, ko]).max() <= 1e-13 * scale[q], (isl, q)
        if spin:
            ws = orc.beam_spin(isl)[:, ko]
            assert np.abs(ref.s[:, idx[kr]] - ws).max() <= 1e-13
        seen += idx.size
    assert seen == ref.alive.sum() == soa.shape[1] - ref.n_absorbed
