"""Compiler of the input file's parsed functions (beams.external_E(x,y,z,t), ...) to the expression programs of the C ABI
(include/hpslice.h: hps_expr).  Standard `ast` module only; the library has no text parser.

Grammar: numbers, names, parentheses, + - * /, unary + -, ^ and ** (power: right-associative, tighter than a unary minus on
its left, so -x^2 = -(x^2) and 2^3^2 = 512), < <= > >= == !=, and / or / not, the functions of FUNCTIONS, pow(a,b),
if(c,a,b).  A literal integer exponent with |n| <= 8 is a repeated multiplication.  Comparisons do not chain.

Predefined names (utils/Parser.H:34-51, values of docs/source/run/parameters.rst): pi true false clight epsilon0 mu0 q_e m_e
m_p hbar r_e; `constants` plays the role of my_constants and may hold numbers or expression strings over other constants
(resolved recursively; a cycle is an error).

Constant sub-trees are folded with the interpreter below, whose every operation rounds once as the C routine's does: folding
changes no value.  Program.evaluate is that interpreter over numpy arrays -- the restatement the tests compare against."""
import ast
import ctypes as C
import re

import numpy as np

from ._lib import Expr, ExprIns as Ins

OPS = ["const", "var", "add", "sub", "mul", "div", "neg", "pow", "powi", "lt", "le", "gt", "ge", "eq", "ne", "and", "or", "not",
       "select", "sqrt", "exp", "log", "log10", "sin", "cos", "tan", "asin", "acos", "atan", "atan2", "sinh", "cosh", "tanh",
       "abs", "floor", "ceil", "fmod", "min", "max", "heaviside", "erf"]      # index = value of the HPS_EX_* enum
OP = {n: i for i, n in enumerate(OPS)}
MAX_INS, MAX_DEPTH, MAX_CONST, MAX_POWI, MAX_VARS = 256, 16, 64, 8, 8      # HPS_EXPR_MAX_*
# name -> number of arguments
FUNCTIONS = dict(sqrt=1, exp=1, log=1, log10=1, sin=1, cos=1, tan=1, asin=1, acos=1, atan=1, atan2=2, sinh=1, cosh=1, tanh=1,
                 abs=1, floor=1, ceil=1, fmod=2, min=2, max=2, heaviside=2, erf=1, pow=2)
NPOP = {n: 1 for n in OPS}
NPOP.update({n: 2 for n in ("add", "sub", "mul", "div", "pow", "lt", "le", "gt", "ge", "eq", "ne", "and", "or", "atan2", "fmod",
                            "min", "max", "heaviside")})
NPOP.update(const=0, var=0, select=3)
PREDEFINED = dict(pi=3.14159265358979323846, true=1.0, false=0.0, clight=299792458.0, epsilon0=8.8541878128e-12,
                  mu0=1.25663706212e-06, q_e=1.602176634e-19, m_e=9.1093837015e-31, m_p=1.67262192369e-27, hbar=1.054571817e-34,
                  r_e=2.817940326204929e-15)


def _erf(a):
    import math
    return np.vectorize(math.erf, otypes=[np.float64])(a)


def _apply(op, arg, a, b, c):
    """one instruction on float64 arrays: one rounding per operation"""
    with np.errstate(all="ignore"):
        if op == "add": return a + b
        if op == "sub": return a - b
        if op == "mul": return a * b
        if op == "div": return a / b
        if op == "neg": return -a
        if op == "pow": return np.power(a, b)
        if op == "powi":
            n = abs(arg)
            r = np.ones_like(a) if n == 0 else a
            for _ in range(1, n):
                r = r * a
            return 1.0 / r if arg < 0 else r
        if op == "lt": return (a < b).astype(np.float64)
        if op == "le": return (a <= b).astype(np.float64)
        if op == "gt": return (a > b).astype(np.float64)
        if op == "ge": return (a >= b).astype(np.float64)
        if op == "eq": return (a == b).astype(np.float64)
        if op == "ne": return (a != b).astype(np.float64)
        if op == "and": return ((a != 0.0) & (b != 0.0)).astype(np.float64)
        if op == "or": return ((a != 0.0) | (b != 0.0)).astype(np.float64)
        if op == "not": return (a == 0.0).astype(np.float64)
        if op == "select": return np.where(c != 0.0, a, b)
        if op == "abs": return np.abs(a)
        if op == "min": return np.where(a < b, a, b)
        if op == "max": return np.where(a > b, a, b)
        if op == "heaviside": return np.where(a < 0.0, 0.0, np.where(a == 0.0, b, 1.0))
        if op == "erf": return _erf(a)
        if op == "asin": return np.arcsin(a)
        if op == "acos": return np.arccos(a)
        if op == "atan": return np.arctan(a)
        if op == "atan2": return np.arctan2(a, b)
        if op == "fmod": return np.fmod(a, b)
        return getattr(np, op)(a)      # sqrt exp log log10 sin cos tan sinh cosh tanh floor ceil


class Program:
    """ins: [(opcode name, operand)], consts: the pool, variables: the names of the inputs"""

    def __init__(self, ins, consts, variables, text=""):
        self.ins, self.consts, self.variables, self.text = list(ins), [float(v) for v in consts], tuple(variables), text
        self.depth = _depth(self.ins)

    @property
    def is_constant(self):
        return len(self.ins) == 1 and self.ins[0][0] == "const"

    @property
    def is_zero(self):
        """folds to the constant 0: the engine skips it"""
        return self.is_constant and self.consts[self.ins[0][1]] == 0.0

    def evaluate(self, *arrays):
        """pure-numpy interpreter of the instruction set; arrays: one per variable (broadcast against each other)"""
        if len(arrays) != len(self.variables):
            raise ValueError(f"evaluate: {len(self.variables)} arrays expected ({', '.join(self.variables)}), got {len(arrays)}")
        arrs = np.broadcast_arrays(*[np.asarray(a, dtype=np.float64) for a in arrays]) if arrays else []
        shape = arrs[0].shape if arrs else ()
        st = []
        for op, arg in self.ins:
            if op == "const":
                st.append(np.full(shape, self.consts[arg], dtype=np.float64))
            elif op == "var":
                st.append(arrs[arg])
            else:
                n = NPOP[op]
                b = st.pop() if n >= 2 else None
                a = st.pop()
                c = st.pop() if n == 3 else None
                st.append(np.asarray(_apply(op, arg, a, b, c), dtype=np.float64))
        assert len(st) == 1
        return st[0]

    def c_struct(self):
        """-> (hps_expr, keep-alive): the ctypes image of the program"""
        ins = (Ins * max(len(self.ins), 1))(*[Ins(OP[o], int(a)) for o, a in self.ins])
        consts = (C.c_double * max(len(self.consts), 1))(*self.consts)
        e = Expr(len(self.ins), len(self.consts), C.cast(ins, C.POINTER(Ins)), C.cast(consts, C.POINTER(C.c_double)))
        return e, (ins, consts)

    def __repr__(self):
        return f"Program({self.text!r}: {len(self.ins)} instructions, depth {self.depth}, {len(self.consts)} constants)"


def _depth(ins):
    sp = deepest = 0
    for op, _ in ins:
        sp += 1 - NPOP[op]
        deepest = max(deepest, sp)
    return deepest


_BIN = {ast.Add: "add", ast.Sub: "sub", ast.Mult: "mul", ast.Div: "div"}
_CMP = {ast.Lt: "lt", ast.LtE: "le", ast.Gt: "gt", ast.GtE: "ge", ast.Eq: "eq", ast.NotEq: "ne"}


def _to_python(text):
    """the reference's syntax as a Python expression: ^ is **, if( and if ( are a call, a line break inside a quoted
    multi-line value of the input file is white space"""
    return re.sub(r"\bif\s*\(", "_if_(", re.sub(r"\s+", " ", text).replace("^", "**")).strip()


def _token(text, node):
    seg = ast.get_source_segment(text, node)
    return seg if seg else type(node).__name__


class _Compiler:
    def __init__(self, text, variables, constants, fold, resolving):
        self.text, self.src = text, _to_python(text)
        self.variables, self.user, self.fold, self.resolving = tuple(variables), dict(constants or {}), fold, resolving
        self.ins, self.consts = [], []

    def fail(self, what, tok):
        raise ValueError(f"expression {self.text!r}: {what}: {tok!r}")

    def const_value(self, name, node):
        """my_constants entry: a number, or an expression string over other constants"""
        v = self.user[name]
        if isinstance(v, str):
            if name in self.resolving:
                self.fail("cyclic constants", " -> ".join(self.resolving + (name,)))
            sub = _Compiler(v, (), self.user, True, self.resolving + (name,)).compile()
            if not sub.is_constant:      # (cannot happen: no variables)
                self.fail("constant does not reduce to a number", name)
            return sub.consts[sub.ins[0][1]]
        return float(v)

    def push_const(self, v):
        v = float(v)
        for i, c in enumerate(self.consts):
            if c == v and np.signbit(c) == np.signbit(v):
                break
        else:
            i = len(self.consts)
            self.consts.append(v)
        self.ins.append(("const", i))

    def emit(self, op, arg, nargs):
        """append the instruction; fold it when its nargs arguments are the last nargs instructions and all constants"""
        tail = self.ins[len(self.ins) - nargs:] if nargs else []
        if self.fold and nargs and len(tail) == nargs and all(o == "const" for o, _ in tail):
            vals = [np.array([self.consts[a]], dtype=np.float64) for _, a in tail]
            a, b, c = (vals + [None, None])[:3] if nargs < 3 else (vals[1], vals[2], vals[0])
            r = float(np.asarray(_apply(op, arg, a, b, c), dtype=np.float64)[0])
            del self.ins[len(self.ins) - nargs:]
            self.push_const(r)
        else:
            self.ins.append((op, arg))

    def visit(self, n):
        if isinstance(n, ast.Constant):
            if isinstance(n.value, bool) or not isinstance(n.value, (int, float)):
                self.fail("unsupported syntax", _token(self.src, n))
            self.push_const(n.value)
        elif isinstance(n, ast.Name):
            if n.id in self.variables:
                self.ins.append(("var", self.variables.index(n.id)))
            elif n.id in self.user:
                self.push_const(self.const_value(n.id, n))
            elif n.id in PREDEFINED:
                self.push_const(PREDEFINED[n.id])
            else:
                self.fail("unknown name", n.id)
        elif isinstance(n, ast.UnaryOp):
            if isinstance(n.op, ast.UAdd):
                self.visit(n.operand)
            elif isinstance(n.op, ast.USub):
                self.visit(n.operand)
                self.emit("neg", 0, 1)
            elif isinstance(n.op, ast.Not):
                self.visit(n.operand)
                self.emit("not", 0, 1)
            else:
                self.fail("unsupported syntax", _token(self.src, n))
        elif isinstance(n, ast.BinOp):
            if isinstance(n.op, ast.Pow):
                self.power(n.left, n.right)
            elif type(n.op) in _BIN:
                self.visit(n.left)
                self.visit(n.right)
                self.emit(_BIN[type(n.op)], 0, 2)
            else:
                self.fail("unsupported syntax", _token(self.src, n))
        elif isinstance(n, ast.Compare):
            if len(n.ops) != 1 or type(n.ops[0]) not in _CMP:
                self.fail("unsupported syntax", _token(self.src, n))
            self.visit(n.left)
            self.visit(n.comparators[0])
            self.emit(_CMP[type(n.ops[0])], 0, 2)
        elif isinstance(n, ast.BoolOp):
            op = "and" if isinstance(n.op, ast.And) else "or"
            self.visit(n.values[0])
            for v in n.values[1:]:
                self.visit(v)
                self.emit(op, 0, 2)
        elif isinstance(n, ast.Call):
            if not isinstance(n.func, ast.Name) or n.keywords:
                self.fail("unsupported syntax", _token(self.src, n))
            name = "if" if n.func.id == "_if_" else n.func.id
            if name == "if":
                if len(n.args) != 3:
                    self.fail("wrong arity (3 arguments expected)", "if")
                for a in n.args:
                    self.visit(a)
                self.emit("select", 0, 3)
            elif name in FUNCTIONS:
                if len(n.args) != FUNCTIONS[name]:
                    self.fail(f"wrong arity ({FUNCTIONS[name]} argument{'s' * (FUNCTIONS[name] > 1)} expected)", name)
                if name == "pow":
                    self.power(n.args[0], n.args[1])
                else:
                    for a in n.args:
                        self.visit(a)
                    self.emit(name, 0, len(n.args))
            else:
                self.fail("unknown name", name)
        else:
            self.fail("unsupported syntax", _token(self.src, n))

    def power(self, base, expo):
        """a literal integer exponent (-3, 2, 2.0) with |n| <= 8: repeated multiplication; otherwise pow"""
        lit, sign = expo, 1
        while isinstance(lit, ast.UnaryOp) and isinstance(lit.op, (ast.USub, ast.UAdd)):
            sign = -sign if isinstance(lit.op, ast.USub) else sign
            lit = lit.operand
        if isinstance(lit, ast.Constant) and isinstance(lit.value, (int, float)) and not isinstance(lit.value, bool) \
                and float(lit.value) == int(lit.value) and abs(int(lit.value)) <= MAX_POWI:
            self.visit(base)
            self.emit("powi", sign * int(lit.value), 1)
        else:
            self.visit(base)
            self.visit(expo)
            self.emit("pow", 0, 2)

    def compile(self):
        try:
            tree = ast.parse(self.src, mode="eval")
        except SyntaxError as e:
            line = (e.text or self.src)
            col = max((e.offset or 1) - 1, 0)
            m = re.match(r"\s*(\w+|\S)", line[col:])
            self.fail("unsupported syntax", m.group(1) if m else line.strip())
        self.visit(tree.body)
        if len(self.ins) > MAX_INS:
            self.fail(f"too many instructions ({len(self.ins)} > {MAX_INS})", self.text.strip()[:40])
        if len(self.consts) > MAX_CONST:
            self.fail(f"too many constants ({len(self.consts)} > {MAX_CONST})", self.text.strip()[:40])
        # constants that folding left without a user
        used = sorted({a for o, a in self.ins if o == "const"})
        remap = {old: new for new, old in enumerate(used)}
        ins = [(o, remap[a]) if o == "const" else (o, a) for o, a in self.ins]
        p = Program(ins, [self.consts[i] for i in used], self.variables, self.text)
        if p.depth > MAX_DEPTH:
            self.fail(f"too deep (stack depth {p.depth} > {MAX_DEPTH})", self.text.strip()[:40])
        return p


def compile_expr(text, variables=("x", "y", "z", "t"), constants=None, fold=True):
    """text (or a number) -> Program over `variables`.  ValueError naming the offending token: unknown name, wrong arity,
    unsupported syntax, too many instructions, too deep, cyclic constants.  fold=False keeps constant sub-trees unfolded."""
    if isinstance(text, (int, float)) and not isinstance(text, bool):
        text = repr(float(text))
    if not isinstance(text, str):
        raise ValueError(f"expression {text!r}: a string or a number is expected")
    if len(variables) > MAX_VARS:
        raise ValueError(f"expression {text!r}: more than {MAX_VARS} variables")
    return _Compiler(text, variables, constants, fold, ()).compile()


def compile_density(text_or_table, constants=None):
    """<plasma>.density(x,y,z) -- a string, a number or a Program -- or a density table -- a list of (position, string) pairs
    in the order given -- over ("x", "y", "z").  -> (Programs, positions or None)"""
    def one(v):
        if isinstance(v, Program):
            return v
        return compile_expr(v, ("x", "y", "z"), constants)
    if isinstance(text_or_table, (str, int, float, Program)):
        return [one(text_or_table)], None
    pairs = list(text_or_table)
    if not pairs or any(not hasattr(p, "__len__") or isinstance(p, (str, bytes)) or len(p) != 2 for p in pairs):
        raise ValueError("density table: a non-empty list of (position, expression) pairs is expected")
    return [one(e) for _, e in pairs], [float(z) for z, _ in pairs]


def c_programs(programs):
    """-> (ctypes array of hps_expr, keep-alive)"""
    arr, keep = (Expr * len(programs))(), []
    for q, p in enumerate(programs):
        arr[q], k = p.c_struct()
        keep.append(k)
    return arr, keep


def compile_components(comps, what, constants=None, variables=("x", "y", "z", "t")):
    """three expressions (strings or numbers) -> three Programs; None -> None"""
    if comps is None:
        return None
    if isinstance(comps, (str, bytes)) or not hasattr(comps, "__len__") or len(comps) != 3:
        n = len(comps) if hasattr(comps, "__len__") and not isinstance(comps, (str, bytes)) else 1
        raise ValueError(f"{what}: three components are expected, got {n}")
    return [compile_expr(c, variables, constants) for c in comps]
