"""ctypes binding of the C-ABI boundary declared in ``include/ceed.h``.

The binding is library-agnostic: it is handed the path of a shared object that
exports the ``Ceed*`` entry points.  The package itself only ever passes the
product library (``csrc/libceed_mi355x.so``, resource ``/gpu/hip/mi355x``);
tests, ``smoke()`` and the ``cpu_baseline`` leg of ``bench.py`` may additionally
bind the CPU oracle (``oracle/liboracle_ceed.so``) through the same class so the
parity tests drive both backends with identical call sequences -- the sequences
of the reference's ``src/setuplibceed.c`` / ``src/matops.c``.

Raw pointers only cross the boundary: numpy arrays on the host side, integer
device addresses (e.g. ``torch.Tensor.data_ptr()``) on the device side.

The prototypes are read out of ``include/ceed.h`` (and ``include/ceed_contact.h``, ``include/ceed_support.h`` and ``include/ceed_surface_field.h``: the contact, the support and the surface-field entry points) at import (``header_prototypes``) and declared on every library loaded, so a call
with an argument missing or of the wrong kind is a Python exception before anything reaches C.  ``L.lib.CeedName(...)`` is the raw call:
it returns the library's code and raises nothing (a code that is inspected, the destroy paths).  ``L.CeedName(...)`` is its checked
twin: same prototype, ``CeedError`` with the library's message on a non-zero code; an optional entry point the library lacks has no
twin (ask ``L.has`` first).
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import os
import re
from typing import Optional, Sequence

import numpy as np

from . import portable as pt
from .portable import (BLOCK_HOST_CHUNK, _np_f64, block_combine_host, block_gram_host, chebyshev_step_pointblock_host,  # noqa: F401
                       leapfrog_step_host, pointblock_invert_host, pointblock_mult_host)          # (the array forms, under their names here too)

c_int = C.c_int32
c_scalar_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int32)

MEM_HOST, MEM_DEVICE = 0, 1
COPY_VALUES, USE_POINTER, OWN_POINTER = 0, 1, 2
NOTRANSPOSE, TRANSPOSE = 0, 1
EVAL_NONE, EVAL_INTERP, EVAL_GRAD, EVAL_WEIGHT = 0, 1, 2, 16
GAUSS, GAUSS_LOBATTO = 0, 1

QFUNCTION_USER = C.CFUNCTYPE(C.c_int, C.c_void_p, c_int, C.POINTER(c_scalar_p), C.POINTER(c_scalar_p))

PRODUCT_LIB = os.environ.get(  # override only for A/B-ing kernel builds (tools/); must still be a *mi355x* build
    "CEEDPETSCSOLID_MI355X_LIB", os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libceed_mi355x.so"))


class CeedError(RuntimeError):
    pass


# ---- the prototypes of a header of the ABI as ctypes types -----------------------------------------------------------------------
class _Handle:
    """Parameter type of an opaque handle (``typedef struct X_private *X``) and of a pointer to one: whatever ``c_void_p`` takes (a
    ``c_void_p``, ``byref`` of one, an address held as an integer such as the CEED_* sentinels, None for NULL) except text, which
    ``c_void_p`` would pass on as the address of the string."""

    @staticmethod
    def from_param(v, _vp=C.c_void_p):
        if type(v) is _vp or v is None:
            return v
        if isinstance(v, (str, bytes, bytearray)):
            raise TypeError("a handle is expected, not text")
        return _vp.from_param(v)


_BASE_TYPES = {"int": C.c_int, "double": C.c_double, "size_t": C.c_size_t, "int32_t": C.c_int32, "int64_t": C.c_int64,
               "unsigned char": C.c_ubyte, "CeedQFunctionUser": C.c_void_p}      # (a callback is passed as the address it was cast to)
Prototype = collections.namedtuple("Prototype", "restype argtypes optional")
Prototypes = collections.namedtuple("Prototypes", "types functions data")


def _ctype(types: dict, decl: str, named: bool, where: str):
    """The ctypes type of a C parameter declaration (``named``: it may end in the parameter's name) or return type.  The pointer depth
    is the number of ``*`` and ``[]``; a base type outside ``types`` is an error, never a ``void *``."""
    depth = decl.count("*") + decl.count("[")
    words = re.sub(r"\[[^\]]*\]|\*|\bconst\b", " ", decl).split()
    if named and len(words) > 1 and " ".join(words) not in types:
        words.pop()
    base = " ".join(words)
    if base in ("char", "void") and depth:
        t, depth = (C.c_char_p if base == "char" else C.c_void_p), depth - 1
    elif base in types:
        t = types[base]
    else:
        raise CeedError(f"{where}: unknown type '{base}' in '{decl.strip()}'")
    for _ in range(0 if t is _Handle else depth):
        t = C.POINTER(t)
    return t


def header_prototypes(path: str, types: Optional[dict] = None) -> Prototypes:
    """Of a header written like include/ceed.h: its typedefs as ctypes types (on top of ``types``, those of a header it includes),
    ``{name: Prototype}`` of every ``CEED_EXTERN[_OPTIONAL] <ret> Name(args);`` in the order of declaration, its data symbols."""
    if not os.path.exists(path):
        raise CeedError(f"header not found: {path} -- the binding takes its prototypes from it")
    with open(path) as f:
        txt = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    txt = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", " ", txt, flags=re.M)          # preprocessor lines and their continuations
    types = dict(_BASE_TYPES if types is None else types)
    types.update({n: _Handle for n in re.findall(r"\btypedef\s+struct\s+\w+\s*\*\s*(\w+)\s*;", txt)})
    types.update({n: C.c_int for n in re.findall(r"\btypedef\s+enum\s*\{[^}]*\}\s*(\w+)\s*;", txt)})
    types.update({n: types[b] for b, n in re.findall(r"\btypedef\s+(\w+)\s+(\w+)\s*;", txt) if b in types})
    functions = {}
    for optional, ret, name, args in re.findall(r"\bCEED_EXTERN(_OPTIONAL)?\s+([^;()]+?)\b(\w+)\s*\(([^()]*)\)\s*;", txt):
        where, args = f"{path}: {name}", [] if args.strip() in ("", "void") else args.split(",")
        functions[name] = Prototype(_ctype(types, ret, False, where), tuple(_ctype(types, a, True, where) for a in args), bool(optional))
    return Prototypes(types, functions, re.findall(r"\bCEED_EXTERN\s+[^;()]+?\b(\w+)\s*(?:\[\d*\])?\s*;", txt))


def declare(cdll, functions: dict, chk) -> dict:
    """Put ``argtypes`` and ``restype`` on every function of ``functions`` that ``cdll`` exports and return ``{name: checked twin}``:
    ``cdll[name]`` is a function object of its own, given the same prototype and ``chk(code, function, arguments)`` as its ``errcheck``."""
    twins = {}
    for name, p in functions.items():
        if hasattr(cdll, name):
            for f in (getattr(cdll, name), cdll[name]):
                f.restype, f.argtypes = p.restype, p.argtypes
            if p.restype is C.c_int:
                f.errcheck = chk
            twins[name] = f
    return twins


HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ceed.h")
PROTOTYPES = header_prototypes(HEADER)
# include/ceed_contact.h (CeedXContact*, all optional) on top of the typedefs of include/ceed.h, which it includes
CONTACT_HEADER = os.path.join(os.path.dirname(HEADER), "ceed_contact.h")
CONTACT_PROTOTYPES = header_prototypes(CONTACT_HEADER, PROTOTYPES.types)
# include/ceed_support.h (CeedXSupport*, all optional), read the same way
SUPPORT_HEADER = os.path.join(os.path.dirname(HEADER), "ceed_support.h")
SUPPORT_PROTOTYPES = header_prototypes(SUPPORT_HEADER, PROTOTYPES.types)
# include/ceed_surface_field.h (the CeedXSurfaceLoadApply* of loads that vary over the faces, all optional), read the same way
SURFACE_FIELD_HEADER = os.path.join(os.path.dirname(HEADER), "ceed_surface_field.h")
SURFACE_FIELD_PROTOTYPES = header_prototypes(SURFACE_FIELD_HEADER, PROTOTYPES.types)


class CeedLib:
    """One loaded shared object exporting the ``include/ceed.h`` ABI: ``lib`` the raw functions, ``CeedName`` their checked twins."""

    # what include/ceed.h declares: CEED_EXTERN functions, CEED_EXTERN_OPTIONAL functions (the product library exports them, another
    # backend of the ABI -- the CPU oracle -- may not: the callers ask ``has`` and otherwise take the portable form), data symbols
    FUNCTIONS = [n for n, p in PROTOTYPES.functions.items() if not p.optional]
    OPTIONAL = [n for n, p in PROTOTYPES.functions.items() if p.optional]
    DATA = list(PROTOTYPES.data)
    CONTACT = list(CONTACT_PROTOTYPES.functions)       # include/ceed_contact.h: optional like OPTIONAL, declared and checked the same way
    SUPPORT = list(SUPPORT_PROTOTYPES.functions)       # include/ceed_support.h: likewise
    SURFACE_FIELD = list(SURFACE_FIELD_PROTOTYPES.functions)       # include/ceed_surface_field.h: likewise

    def __init__(self, path: str = PRODUCT_LIB):
        if not os.path.exists(path):
            raise CeedError(f"Ceed backend library not found: {path} -- build it first "
                            "(python -c 'import __graft_entry__ as g; g.build()'); there is no fallback path")
        self.path = path
        if "mi355x" in os.path.basename(path):
            # One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64 /
            # libhsa-runtime64 (soname libamdhip64.so.7, same as /opt/rocm's); two copies in
            # one process cannot both open the device.  Importing torch first makes the
            # loader satisfy this library's NEEDED entry with torch's already-loaded copy
            # (measured on the GPU box: tools/diag_hip_runtime.py).  A plain C host without
            # torch gets /opt/rocm's runtime through the usual search path.
            import torch  # noqa: F401
        # RTLD_LOCAL: the oracle and the product export the same Ceed* names
        self.lib = C.CDLL(path, mode=getattr(os, "RTLD_LOCAL", 0) | getattr(os, "RTLD_NOW", 2))
        L = self.lib
        def errcheck(rc, _func, _args, chk=self.chk):          # a plain function: a checked call that succeeds pays for no more than this
            if rc:
                chk(rc)
        self.errcheck = errcheck
        vars(self).update(declare(L, PROTOTYPES.functions, errcheck))      # instance attributes: nothing between a call and its function
        vars(self).update(declare(L, CONTACT_PROTOTYPES.functions, errcheck))
        vars(self).update(declare(L, SUPPORT_PROTOTYPES.functions, errcheck))
        vars(self).update(declare(L, SURFACE_FIELD_PROTOTYPES.functions, errcheck))
        L.CeedXSetErrorReturn(1)
        for s in ("VECTOR_ACTIVE", "VECTOR_NONE", "ELEMRESTRICTION_NONE", "BASIS_COLLOCATED", "QFUNCTION_NONE", "REQUEST_IMMEDIATE"):
            setattr(self, s, C.c_void_p.in_dll(L, "CEED_" + s).value)          # the sentinels: addresses, as integers
        self.STRIDES_BACKEND = (c_int * 3).in_dll(L, "CEED_STRIDES_BACKEND")

    def chk(self, rc: int):
        if rc:
            msg = self.lib.CeedXLastError()
            raise CeedError(msg.decode() if msg else f"Ceed error {rc}")

    def has(self, symbol: str) -> bool:
        return hasattr(self.lib, symbol)

    def missing_symbols(self, optional: bool = True):
        """Declared symbols this library lacks.  ``optional=False`` leaves the CEED_EXTERN_OPTIONAL ones out: what another backend of
        the ABI must export; the product library exports all of them (build() checks with the default)."""
        want = self.FUNCTIONS + self.DATA + (self.OPTIONAL + self.CONTACT + self.SUPPORT + self.SURFACE_FIELD if optional else [])
        return [s for s in want if not hasattr(self.lib, s)]


def out_value(fn, ctype, *args):
    """The value ``fn(*args, &value)`` writes into its last parameter, a ``ctype``."""
    v = ctype()
    fn(*args, C.byref(v))
    return v.value


# ---- point-block Jacobi: the CEED_EXTERN_OPTIONAL vector operations; where the library lacks one, its portable form (portable.py) ------
def _pb_check(who: str, blocks: "Vector", n: int):
    if n % 3:
        raise CeedError(f"{who}: vector length {n} is not a multiple of 3")
    if blocks.n < 3 * n:
        raise CeedError(f"{who}: block vector of {blocks.n} entries is shorter than 3 x {n}")


def pointblock_invert(blocks: "Vector", want_n_bad: bool = True) -> Optional[int]:
    """CeedXVectorPointBlockInvert, in place; returns the number of blocks with a bad pivot (one sync) or, with
    ``want_n_bad=False``, None without involving the host.  The portable NumPy form where the library lacks the entry point."""
    L = blocks.L
    if L.has("CeedXVectorPointBlockInvert"):
        return out_value(L.CeedXVectorPointBlockInvert, C.c_int, blocks.h) if want_n_bad else L.CeedXVectorPointBlockInvert(blocks.h, None)
    if blocks.n % 9:
        raise CeedError(f"pointblock_invert: vector length {blocks.n} is not a multiple of 9")
    inv, nb = pointblock_invert_host(blocks.to_numpy())
    pt.assign(blocks, inv)
    return nb if want_n_bad else None


def pointblock_mult(w: "Vector", blocks: "Vector", x: "Vector"):
    """CeedXVectorPointBlockMult: w_n = B_n x_n."""
    L = w.L
    if L.has("CeedXVectorPointBlockMult"):
        L.CeedXVectorPointBlockMult(w.h, blocks.h, x.h)
        return
    if w.n != x.n:
        raise CeedError("pointblock_mult: vector lengths differ")
    _pb_check("pointblock_mult", blocks, x.n)
    pt.assign(w, pointblock_mult_host(blocks.to_numpy(), x.to_numpy()))


def chebyshev_step_pointblock(x: "Vector", d: "Vector", r: Optional["Vector"], b: "Vector", t: Optional["Vector"], blocks: "Vector",
                              c1: float, c2: float, assign_x: bool):
    """CeedXVectorChebyshevStepPointBlock: ri = b - t; d = c1 B ri + c2 d; x = d or x + d (ri stored if r is given)."""
    L = x.L
    if L.has("CeedXVectorChebyshevStepPointBlock"):
        L.CeedXVectorChebyshevStepPointBlock(x.h, d.h, _h(r), b.h, _h(t), blocks.h, c1, c2, int(bool(assign_x)))
        return
    if any(v is not None and v.n != x.n for v in (d, r, b, t)):
        raise CeedError("chebyshev_step_pointblock: vector lengths differ")
    _pb_check("chebyshev_step_pointblock", blocks, x.n)
    xn, dn, ri = chebyshev_step_pointblock_host(None if assign_x else x.to_numpy(), d.to_numpy() if c2 != 0.0 else None, b.to_numpy(),
                                                t.to_numpy() if t is not None else None, blocks.to_numpy(), c1, c2, assign_x)
    for v, a in ((r, ri), (d, dn), (x, xn)):
        if v is not None:
            pt.assign(v, a)


class Csr:
    """Assembled sparse operator on L-vectors (CeedXCsr*): the coarse multigrid level."""

    def __init__(self, ceed: "Ceed", rowptr, cols, coo_slot, unit_rows=()):
        self.L, self._ceed = ceed.L, ceed
        self.h = C.c_void_p()
        rp = np.ascontiguousarray(rowptr, dtype=np.int32); cl = np.ascontiguousarray(cols, dtype=np.int32)
        sl = np.ascontiguousarray(coo_slot, dtype=np.int32); ur = np.ascontiguousarray(unit_rows, dtype=np.int32)
        self.nrows, self.nnz, self.ncoo = rp.size - 1, int(rp[-1]), sl.size
        self.L.CeedXCsrCreate(ceed.h, self.nrows, rp.ctypes.data_as(c_int_p), cl.ctypes.data_as(c_int_p), sl.size,
                              sl.ctypes.data_as(c_int_p), ur.size, ur.ctypes.data_as(c_int_p), C.byref(self.h))

    def assemble(self, coo_values: "Vector"):
        self.L.CeedXCsrAssemble(self.h, coo_values.h)

    def apply(self, x: "Vector", y: "Vector"):
        self.L.CeedXCsrApply(self.h, x.h, y.h)

    def diagonal(self, d: "Vector"):
        self.L.CeedXCsrGetDiagonal(self.h, d.h)

    # ---- pieces of the aggregation hierarchy (amg.py) ------------------------------------------------------
    @classmethod
    def rect(cls, ceed: "Ceed", nrows: int, ncols: int, rowptr, cols, vals=None) -> "Csr":
        """nrows x ncols matrix with fixed values (``vals``) or values computed by ``update()`` (``vals=None``)."""
        self = cls.__new__(cls)
        self.L, self.h, self._ceed = ceed.L, C.c_void_p(), ceed
        rp = np.ascontiguousarray(rowptr, dtype=np.int32); cl = np.ascontiguousarray(cols, dtype=np.int32)
        if rp.size != nrows + 1 or cl.size != int(rp[-1]):
            raise ValueError("rowptr / cols do not describe an nrows-row pattern")
        self.nrows, self.ncols, self.nnz, self.ncoo = nrows, ncols, int(rp[-1]), 0
        vp = None
        if vals is not None:
            va = np.ascontiguousarray(vals, dtype=np.float64)
            if va.size != self.nnz:
                raise ValueError("one value per pattern entry expected")
            vp = va.ctypes.data_as(C.POINTER(C.c_double))
        self.L.CeedXCsrCreateRect(ceed.h, nrows, ncols, rp.ctypes.data_as(c_int_p), cl.ctypes.data_as(c_int_p), vp, C.byref(self.h))
        return self

    @classmethod
    def product(cls, left: "Csr", right: "Csr", variable: int, dense: bool = False) -> "Csr":
        """left * right with one operand of fixed values and the other (``variable``: 0 left, 1 right) read at every
        ``update()``; pattern and term lists are worked out by the library (CeedXCsrCreateProduct)."""
        self = cls.__new__(cls)
        self.L, self.h, self._ceed = left.L, C.c_void_p(), left._ceed
        self.L.CeedXCsrCreateProduct(left.h, right.h, variable, 1 if dense else 0, C.byref(self.h))
        self.nrows, self.ncols, self.nnz = self.pattern()[:3]
        self.ncoo = 0
        return self

    def pattern(self):
        """(nrows, ncols, nnz, rowptr, cols): copies of the library's host pattern."""
        nr, nc, nz = c_int(), c_int(), c_int()
        rp, cl = c_int_p(), c_int_p()
        self.L.CeedXCsrGetPattern(self.h, C.byref(nr), C.byref(nc), C.byref(nz), C.byref(rp), C.byref(cl))
        rowptr = np.ctypeslib.as_array(rp, shape=(nr.value + 1,)).copy()
        cols = np.ctypeslib.as_array(cl, shape=(max(nz.value, 1),))[:nz.value].copy() if nz.value else np.zeros(0, np.int32)
        return nr.value, nc.value, nz.value, rowptr, cols

    def update(self):
        self.L.CeedXCsrUpdate(self.h)

    def get_values(self, v: "Vector"):
        self.L.CeedXCsrGetValues(self.h, v.h)

    def values(self, ceed: "Ceed" = None) -> np.ndarray:
        v = (ceed or self._ceed).vector(max(self.nnz, 1))
        self.get_values(v)
        out = v.to_numpy()[:self.nnz].copy()
        v.destroy()
        return out

    def invert_dense_spd(self):
        self.L.CeedXCsrInvertDenseSPD(self.h)

    def destroy(self):
        if self.h:
            self.L.lib.CeedXCsrDestroy(C.byref(self.h))
            self.h = None


class _FaceHandle:
    """A term on a list of element faces, on the device: what is common to the entry points ``PREFIX``Create, SetDirichletMask,
    GetKernelName and Destroy, which every such term has with the same arguments.  Optional in a library: without ``PREFIX``Create the
    caller (``PORTABLE``) takes its portable NumPy form.  A term spells out its four calls (``_create`` ... ``_destroy``), so that the
    static check of every call site's argument count still sees them."""
    PREFIX = PORTABLE = ""

    def __init__(self, ceed: "Ceed", P: int, Q: int, offsets, lsize: int):
        self.L, self._ceed = ceed.L, ceed
        if not self.L.has(self.PREFIX + "Create"):
            raise CeedError(f"{self.L.path} has no {self.PREFIX}Create: use the portable form ({self.PORTABLE})")
        self.h = C.c_void_p()
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1, P * P)
        self.nface = off.shape[0]
        self._create(ceed.h, P, Q, off.ctypes.data_as(c_int_p), lsize)

    def set_dirichlet_mask(self, mask: Optional[np.ndarray]):
        _, p, n = Operator._bytes(mask)
        self._set_mask(p, n)

    @property
    def kernel_name(self) -> str:
        return (self._kernel_name() or b"").decode()

    def destroy(self):
        if self.h:
            self._destroy()
            self.h = None


SURFACE_TRACTION, SURFACE_PRESSURE = 0, 1


class SurfaceLoadHandle(_FaceHandle):
    """CeedXSurfaceLoad*: traction, follower pressure and its tangent on a list of element faces."""
    PREFIX, PORTABLE = "CeedXSurfaceLoad", "surface.SurfaceLoad"

    def _create(self, ceed_h, P, Q, off, lsize): self.L.CeedXSurfaceLoadCreate(ceed_h, self.nface, P, Q, off, lsize, C.byref(self.h))
    def _set_mask(self, p, n): self.L.CeedXSurfaceLoadSetDirichletMask(self.h, MEM_HOST, p, n)
    def _kernel_name(self): return out_value(self.L.CeedXSurfaceLoadGetKernelName, C.c_char_p, self.h)
    def _destroy(self): self.L.lib.CeedXSurfaceLoadDestroy(C.byref(self.h))

    def apply_add(self, kind: int, coef, scale: float, X: "Vector", u: Optional["Vector"], y: "Vector"):   # y += scale g
        cf = (C.c_double * 3)(*[float(v) for v in coef])
        self.L.CeedXSurfaceLoadApplyAdd(self.h, int(kind), cf, scale, X.h, _h(u), y.h)

    def apply_tangent_add(self, p: float, scale: float, X: "Vector", u: Optional["Vector"], du: "Vector", y: "Vector"):   # y += scale p T(u) du
        self.L.CeedXSurfaceLoadApplyTangentAdd(self.h, p, scale, X.h, _h(u), du.h, y.h)

    # include/ceed_surface_field.h: loads that vary over the faces.  ``field``: a Vector of lsize (traction) or lsize / 3 (pressure) values
    def apply_field_add(self, kind: int, field: "Vector", scale: float, X: "Vector", u: Optional["Vector"], y: "Vector"):
        self.L.CeedXSurfaceLoadApplyFieldAdd(self.h, int(kind), _h(field), scale, X.h, _h(u), y.h)

    def apply_field_tangent_add(self, field: "Vector", scale: float, X: "Vector", u: Optional["Vector"], du: "Vector", y: "Vector"):
        self.L.CeedXSurfaceLoadApplyFieldTangentAdd(self.h, _h(field), scale, X.h, _h(u), du.h, y.h)

    def apply_hydrostatic_add(self, gamma: float, level: float, up, scale: float, X: "Vector", u: Optional["Vector"], y: "Vector"):
        e = (C.c_double * 3)(*[float(v) for v in up])
        self.L.CeedXSurfaceLoadApplyHydrostaticAdd(self.h, gamma, level, e, scale, X.h, _h(u), y.h)

    def apply_hydrostatic_tangent_add(self, gamma: float, level: float, up, scale: float, X: "Vector", u: Optional["Vector"], du: "Vector",
                                      y: "Vector"):
        e = (C.c_double * 3)(*[float(v) for v in up])
        self.L.CeedXSurfaceLoadApplyHydrostaticTangentAdd(self.h, gamma, level, e, scale, X.h, _h(u), du.h, y.h)


CONTACT_PLANE, CONTACT_SPHERE = 0, 1
CONTACT_NSTATE = 7                  # per point: K (xx, yy, zz, yz, xz, xy), then the gap


class ContactHandle(_FaceHandle):
    """CeedXContact* (include/ceed_contact.h): penalty contact of a list of element faces with a rigid plane or sphere."""
    PREFIX, PORTABLE = "CeedXContact", "contact.ContactSurface"

    def _create(self, ceed_h, P, Q, off, lsize): self.L.CeedXContactCreate(ceed_h, self.nface, P, Q, off, lsize, C.byref(self.h))
    def _set_mask(self, p, n): self.L.CeedXContactSetDirichletMask(self.h, MEM_HOST, p, n)
    def _kernel_name(self): return out_value(self.L.CeedXContactGetKernelName, C.c_char_p, self.h)
    def _destroy(self): self.L.lib.CeedXContactDestroy(C.byref(self.h))

    def set_obstacle(self, kind: int, params, penalty: float):
        par = [float(v) for v in params]
        self.L.CeedXContactSetObstacle(self.h, int(kind), (C.c_double * 8)(*(par + [0.0] * (8 - len(par)))), penalty)

    def apply_residual_add(self, scale: float, X: "Vector", u: "Vector", y: "Vector", state: "Vector"):   # y += scale r(u); state := state(u)
        self.L.CeedXContactApplyResidualAdd(self.h, scale, X.h, u.h, y.h, state.h)

    def apply_tangent_add(self, scale: float, state: "Vector", du: "Vector", y: "Vector"):                 # y += scale C du
        self.L.CeedXContactApplyTangentAdd(self.h, scale, state.h, du.h, y.h)

    def diagonal_add(self, scale: float, state: "Vector", d: "Vector"):                                    # d += scale diag C
        self.L.CeedXContactDiagonalAdd(self.h, scale, state.h, d.h)


class SupportHandle(_FaceHandle):
    """CeedXSupport* (include/ceed_support.h): linear spring and dashpot supports on a list of element faces.  The state has the layout
    of the contact state (CONTACT_NSTATE per point: K, then w J)."""
    PREFIX, PORTABLE = "CeedXSupport", "support.SupportSurface"

    def _create(self, ceed_h, P, Q, off, lsize): self.L.CeedXSupportCreate(ceed_h, self.nface, P, Q, off, lsize, C.byref(self.h))
    def _set_mask(self, p, n): self.L.CeedXSupportSetDirichletMask(self.h, MEM_HOST, p, n)
    def _kernel_name(self): return out_value(self.L.CeedXSupportGetKernelName, C.c_char_p, self.h)
    def _destroy(self): self.L.lib.CeedXSupportDestroy(C.byref(self.h))

    def form_state(self, kn: float, kt: float, X: "Vector", state: "Vector"):                              # state := the state of (kn, kt)
        self.L.CeedXSupportFormState(self.h, kn, kt, X.h, state.h)

    def apply_force_add(self, scale: float, state: "Vector", x: "Vector", y: "Vector"):                    # y += scale K x, x as it is
        self.L.CeedXSupportApplyForceAdd(self.h, scale, state.h, x.h, y.h)

    def apply_tangent_add(self, scale: float, state: "Vector", dx: "Vector", y: "Vector"):                 # y += scale K dx
        self.L.CeedXSupportApplyTangentAdd(self.h, scale, state.h, dx.h, y.h)

    def diagonal_add(self, scale: float, state: "Vector", d: "Vector"):                                    # d += scale diag K
        self.L.CeedXSupportDiagonalAdd(self.h, scale, state.h, d.h)


class Graph:
    def __init__(self, L, h):
        self.L, self.h = L, h

    def launch(self):
        self.L.CeedXGraphLaunch(self.h)

    def stale(self) -> int:
        """What CeedXGraphLaunch would refuse for (0: nothing) -- local to this rank."""
        return out_value(self.L.CeedXGraphIsStale, C.c_int, self.h)

    def destroy(self):
        if self.h:
            self.L.lib.CeedXGraphDestroy(C.byref(self.h))
            self.h = None


class Ceed:
    def __init__(self, lib: CeedLib, resource: str):
        self.L = lib
        self.h = C.c_void_p()
        self._scalars = None
        lib.CeedInit(resource.encode(), C.byref(self.h))

    @property
    def resource(self) -> str:
        return out_value(self.L.CeedGetResource, C.c_char_p, self.h).decode()

    @property
    def preferred_memtype(self) -> int:
        return out_value(self.L.CeedGetPreferredMemType, C.c_int, self.h)

    def has_qfunction(self, name: str) -> bool:
        """Does the library have a device functor for the QFunction ``name`` (CeedXHasQFunction)?  False where it lacks the entry point."""
        return self.L.has("CeedXHasQFunction") and bool(out_value(self.L.CeedXHasQFunction, C.c_int, self.h, name.encode()))

    def set_stream(self, hip_stream: int):
        self.L.CeedXSetStream(self.h, hip_stream)

    def synchronize(self):
        self.L.CeedXSynchronize(self.h)

    def clock_probe(self, spin_us: int = 2000) -> float:
        """Shader clock (GHz) while the work queued on this Ceed's stream runs (CeedXClockProbe)."""
        return out_value(self.L.CeedXClockProbe, C.c_double, self.h, spin_us)

    def comm_size(self):
        """(ranks, this rank) of the Ceed's RCCL communicator as RCCL reports them (CeedXCommGetSize); (0, -1) without one."""
        n, r = C.c_int(), C.c_int()
        self.L.CeedXCommGetSize(self.h, C.byref(n), C.byref(r))
        return n.value, r.value

    @property
    def scalars(self) -> "Vector":
        """The Ceed's one register file of device scalars, made at first use: 8 working slots, two coefficients for each of 32 steps."""
        if self._scalars is None:
            self._scalars = self.vector(8 + 2 * 32)
        return self._scalars

    def scalar_divide(self, scalars: "Vector", dst: int, num: int, den: int, scale: float = 1.0):
        """scalars[dst] = scale * scalars[num] / scalars[den] (den < 0: no division; a non-positive denominator gives 0)"""
        self.L.CeedXScalarDivide(scalars.h, dst, num, den, scale)

    def all_reduce(self, v: "Vector", first: int = 0, n: Optional[int] = None):
        """Entries [first, first + n) of v (default: all) summed over the ranks of the Ceed's communicator, in place, on its stream."""
        self.L.CeedXCommAllReduce(self.h, v.h, first, v.n if n is None else n)

    def capture(self, fn) -> "Graph":
        """Record the device work `fn()` queues on this Ceed into a hipGraph (CeedXGraph*)."""
        self.L.CeedXGraphBeginCapture(self.h)
        g, ok = C.c_void_p(), False
        try:
            fn()
            ok = True
        finally:
            rc = self.L.lib.CeedXGraphEndCapture(self.h, C.byref(g))
            if not ok and rc == 0 and g:           # fn() raised: the recording is ended and dropped, the error propagates
                self.L.lib.CeedXGraphDestroy(C.byref(g))
        self.L.chk(rc)
        return Graph(self.L, g)

    def destroy(self):
        if self._scalars is not None:
            self._scalars.destroy()
        if self.h:
            self.L.lib.CeedDestroy(C.byref(self.h))

    # -- factories ---------------------------------------------------------
    def vector(self, n: int) -> "Vector":
        return Vector(self, n)

    def tensor_vector(self, n: int, device) -> "Vector":
        """A vector over a zeroed torch tensor ``.t`` on ``device`` (several ranks: interface sums and torch.distributed reductions act
        on the tensor in place), borrowed as a host array or a device pointer; whoever changes ``.t`` behind the Ceed calls ``touched()``."""
        import torch
        v = self.vector(n)
        v.t = torch.zeros(max(n, 1), dtype=torch.float64, device=device)[:n]
        if v.t.device.type != "cuda":
            v.set_array(v.t.numpy(), copy=False)
        v.touched()                  # (a device tensor: handed over as a device pointer)
        return v

    def block(self, n: int, k: int, ld: Optional[int] = None) -> "BlockVector":
        """k columns of length n in one allocation of k * ld doubles (ld = n unless given) in the Ceed's own memory: a BlockVector."""
        return BlockVector(self, n, k, ld)

    def elem_restriction(self, nelem, elemsize, ncomp, compstride, lsize, offsets) -> "ElemRestriction":
        return ElemRestriction(self, nelem, elemsize, ncomp, compstride, lsize, offsets=offsets)

    def strided_restriction(self, nelem, elemsize, ncomp, lsize, strides=None) -> "ElemRestriction":
        return ElemRestriction(self, nelem, elemsize, ncomp, 0, lsize, strides=strides, strided=True)

    def basis_lagrange(self, dim, ncomp, P, Q, qmode) -> "Basis":
        return Basis(self, dim, ncomp, P, Q, qmode)

    def qfunction(self, name: str, f=None, source: Optional[str] = None) -> "QFunction":
        return QFunction(self, name, f, source)

    def qfunction_identity(self, size, inmode, outmode) -> "QFunction":
        return QFunction(self, "Identity", identity=(size, inmode, outmode))

    def operator(self, qf: "QFunction") -> "Operator":
        return Operator(self, qf)


def _h(vec: Optional["Vector"]):
    """The handle of a vector, None (NULL) for an absent one."""
    return vec.h if vec is not None else None


class Vector:
    t = None            # the torch tensor behind the vector (Ceed.tensor_vector only)

    def __init__(self, ceed: Ceed, n: int):
        self.ceed, self.L, self.n = ceed, ceed.L, int(n)
        self.h = C.c_void_p()
        self._keep = None
        self.L.CeedVectorCreate(ceed.h, n, C.byref(self.h))

    def set_array(self, arr: np.ndarray, copy=True):
        """self := arr.  ``copy=False`` borrows ``arr`` itself (CEED_USE_POINTER: the vector's results appear in it), so it must be
        the memory the library can use as it is -- a C-contiguous, writable float64 ndarray of the vector's size; anything else
        would be converted into a private copy that the caller never sees, and is refused."""
        if not copy:
            if not (isinstance(arr, np.ndarray) and arr.dtype == np.float64 and arr.flags.c_contiguous and arr.flags.writeable
                    and arr.size == self.n):
                raise ValueError(f"set_array(copy=False) borrows the array itself: a C-contiguous, writable float64 ndarray of {self.n} "
                                 f"entries is needed, not {type(arr).__name__}"
                                 + (f" {arr.dtype}{list(arr.shape)}, contiguous={arr.flags.c_contiguous}, writeable={arr.flags.writeable}"
                                    if isinstance(arr, np.ndarray) else ""))
            a = arr
            self._keep = a
        else:
            a = _np_f64(arr)
        assert a.size == self.n, (a.size, self.n)
        self.L.CeedVectorSetArray(self.h, MEM_HOST, COPY_VALUES if copy else USE_POINTER, a.ctypes.data_as(c_scalar_p))
        return self

    def set_device_pointer(self, ptr: int):
        """Borrow a device buffer (CEED_MEM_DEVICE, CEED_USE_POINTER), matops.c:40-41."""
        self.L.CeedVectorSetArray(self.h, MEM_DEVICE, USE_POINTER, C.cast(C.c_void_p(ptr), c_scalar_p))
        return self

    def take_array(self, mtype=MEM_HOST):
        self.L.CeedVectorTakeArray(self.h, mtype, None)
        self._keep = None

    def set_value(self, v: float):
        self.L.CeedVectorSetValue(self.h, v)
        return self

    def to_numpy(self) -> np.ndarray:
        p = c_scalar_p()
        self.L.CeedVectorGetArrayRead(self.h, MEM_HOST, C.byref(p))
        out = np.ctypeslib.as_array(p, shape=(self.n,)).copy() if self.n else np.zeros(0)
        self.L.CeedVectorRestoreArrayRead(self.h, C.byref(p))
        return out

    def device_pointer(self) -> int:
        """Device address of the vector's storage (valid until the next Set/Take)."""
        p = c_scalar_p()
        self.L.CeedVectorGetArray(self.h, MEM_DEVICE, C.byref(p))
        addr = C.cast(p, C.c_void_p).value
        self.L.CeedVectorRestoreArray(self.h, C.byref(p))
        return addr

    def reciprocal(self):
        self.L.CeedVectorReciprocal(self.h)

    # ---- vectors over a torch tensor (Ceed.tensor_vector) -----------------------------------------------------------------
    def fill(self, arr):
        """self := arr (host array), keeping the alias of a tensor-backed vector intact."""
        if self.t is None:
            return self.set_array(arr)
        import torch
        self.t.copy_(torch.from_numpy(_np_f64(arr)))
        self.touched()

    def touched(self):
        """The tensor behind the vector was modified outside the Ceed: a device tensor is handed over again, which drops the host mirror."""
        if self.t is not None and self.t.device.type == "cuda":
            self.set_device_pointer(self.t.data_ptr())

    # ---- CeedXVector* (formulas: include/ceed.h): self is the vector written (the left operand of a dot), None an absent operand ----
    def axpby(self, a: float, x: "Vector", b: float):                      # self = a x + b self
        self.L.CeedXVectorAXPBY(self.h, a, x.h, b)

    def waxpby(self, a: float, x: "Vector", b: float, y: "Vector"):        # self = a x + b y
        self.L.CeedXVectorWAXPBY(self.h, a, x.h, b, y.h)

    def pointwise_mult(self, x: "Vector", y: "Vector"):                    # self = x .* y
        self.L.CeedXVectorPointwiseMult(self.h, x.h, y.h)

    def dot(self, y: "Vector", weight: Optional["Vector"] = None) -> float:   # sum weight .* self .* y, read on the host
        return out_value(self.L.CeedXVectorDot, C.c_double, self.h, y.h, _h(weight))

    def dot_to(self, y: "Vector", scalars: "Vector", slot: int, weight: Optional["Vector"] = None):   # the same into scalars[slot]
        self.L.CeedXVectorDotTo(self.h, y.h, _h(weight), scalars.h, slot)

    def axpby_scalars(self, scalars, ia: int, sa: float, x, ib: int, sb: float):   # axpby, a = sa scalars[ia], b = sb scalars[ib]; index < 0: 1
        self.L.CeedXVectorAXPBYScalars(self.h, scalars.h, ia, sa, x.h, ib, sb)

    def chebyshev_start(self, d, r, b, t, dinv, c1: float, assign_x: bool):   # r = b - t;  d = c1 dinv .* r;  self = d or self + d
        self.L.CeedXVectorChebyshevStart(self.h, d.h, r.h, b.h, _h(t), dinv.h, c1, int(bool(assign_x)))

    def chebyshev_update(self, d, r, t, dinv, c1: float, c2: float, assign_x: bool = False):   # r -= t;  d = c1 dinv .* r + c2 d;  self (+)= d
        self.L.CeedXVectorChebyshevUpdate(self.h, d.h, r.h, _h(t), dinv.h, c1, c2, int(bool(assign_x)))

    def chebyshev_step(self, d, r, b, t, dinv, c1: float, c2: float, assign_x: bool):   # ri = b - t (stored if r);  d = c1 dinv .* ri + c2 d;  self (+)= d
        self.L.CeedXVectorChebyshevStep(self.h, d.h, _h(r), b.h, _h(t), dinv.h, c1, c2, int(bool(assign_x)))

    def leapfrog_step(self, vh: "Vector", r: "Vector", f: Optional["Vector"], m: "Vector", load: float, c1: float, c2: float, dt: float,
                      n: Optional[int] = None, scalars: Optional["Vector"] = None, slot: int = 0):
        """CeedXVectorLeapfrogStep on the first n rows (default: all of self), self the displacement x: on the rows with m > 0
        vh = c1 vh + c2 (load f - r) / m, self += dt vh; scalars[slot] = the kinetic energy at the step r belongs to (None: no sum).
        Where the library lacks the entry point (the CPU oracle) the portable form works in place on the vectors' host arrays."""
        n = self.n if n is None else int(n)
        if self.L.has("CeedXVectorLeapfrogStep"):
            self.L.CeedXVectorLeapfrogStep(self.h, vh.h, r.h, _h(f), m.h, load, c1, c2, dt, n, _h(scalars), slot)
            return
        who, ops = "leapfrog_step", [("x", self), ("vh", vh), ("r", r), ("m", m)] + ([("f", f)] if f is not None else [])
        if any(v is None for _, v in ops):
            raise CeedError(f"{who}: x, vh, r and m must be vectors")
        if n < 1:
            raise CeedError(f"{who}: the number of rows n must be at least 1 (n = {n})")
        for i, (name, v) in enumerate(ops):
            if v.n < n:
                raise CeedError(f"{who}: {name} holds {v.n} entries, n = {n} are read")
            for other, w in ops[:i]:
                if w is v:
                    raise CeedError(f"{who}: {other} and {name} are the same vector: the operands must be pairwise distinct")
            if scalars is v:
                raise CeedError(f"{who}: scalars must not be one of the operands ({name})")
        if scalars is not None and not 0 <= slot < scalars.n:
            raise CeedError(f"{who}: scalar {slot} of {scalars.n}")
        with self.host_view(True) as xa, vh.host_view(True) as va, r.host_view(False) as ra, m.host_view(False) as ma, \
                (f.host_view(False) if f is not None else contextlib.nullcontext()) as fa:
            ke = leapfrog_step_host(xa[:n], va[:n], ra[:n], None if f is None else fa[:n], ma[:n], load, c1, c2, dt, scalars is not None)
        if scalars is not None:
            with scalars.host_view(True) as sa:
                sa[slot] = ke

    @contextlib.contextmanager
    def host_view(self, write: bool):
        """The vector's host storage as a NumPy array WITHOUT a copy (CeedVectorGetArray / GetArrayRead ... Restore), valid inside the
        ``with`` block only; ``write``: the array may be written."""
        p = c_scalar_p()
        (self.L.CeedVectorGetArray if write else self.L.CeedVectorGetArrayRead)(self.h, MEM_HOST, C.byref(p))
        try:
            yield np.ctypeslib.as_array(p, shape=(self.n,)) if self.n else np.zeros(0)
        finally:
            (self.L.CeedVectorRestoreArray if write else self.L.CeedVectorRestoreArrayRead)(self.h, C.byref(p))

    def destroy(self):
        if self.h:
            self.L.lib.CeedVectorDestroy(C.byref(self.h))


# ---- block vectors: CeedXVectorBlockGram / CeedXVectorBlockCombine; their portable forms are in portable.py ------------------------
BLOCK_MAX_COLS = 48


def block_limits(lib: CeedLib):
    """(largest column count, rows of a chunk of the library's Gram reduction, its largest number of partial matrices, rows of a chunk
    of its combination, the combination's largest grid) as CeedXVectorBlockGetLimits reports them; (48, None, None, None, None) where
    the library lacks the block entry points."""
    if not lib.has("CeedXVectorBlockGetLimits"):
        return BLOCK_MAX_COLS, None, None, None, None
    v = [c_int() for _ in range(5)]
    lib.CeedXVectorBlockGetLimits(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def _block_check(who: str, n: int, ld: int, ranges):
    """The checks of csrc/block_args.hpp for the portable form: ranges = (name, first column, count, vector length)."""
    if n < 1:
        raise CeedError(f"{who}: the number of rows n must be at least 1 (n = {n}, ld = {ld})")
    if ld < n:
        raise CeedError(f"{who}: the leading dimension ld must be at least n (n = {n}, ld = {ld})")
    for name, x0, kx, length in ranges:
        if not 1 <= kx <= BLOCK_MAX_COLS:
            raise CeedError(f"{who}: {name}: a column count must lie in 1 .. 48")
        if x0 < 0:
            raise CeedError(f"{who}: {name}: a first column must not be negative")
        if (x0 + kx) * ld - (ld - n) > length:
            raise CeedError(f"{who}: {name}: the column range reaches past the end of its vector")


class BlockVector:
    """k columns of length n in ONE allocation of k * ld doubles in the Ceed's own memory (device memory for the product library, host
    memory for the CPU oracle), column j at element j * ld.  ``owner`` is the CeedVector over the whole allocation, which the block
    operations (``gram``, ``combine``) take; ``cols[j]`` is an ordinary CeedVector that borrows column j, which operators, the mass apply
    and the V-cycle take one at a time.

    A column and the owner are two CeedVectors over the same memory, and each carries the validity flags of its mirrors.
    The rule that keeps them coherent: the memory itself is the only copy that counts.  A block-level write (``combine``, ``fill``,
    ``zero``) hands every column written over again, which drops a host mirror it may have; a column-level write is not seen here, so
    every block-level call hands the owner over again first.  Neither ever keeps a host mirror across a write of the other; whoever
    writes the tensor ``t`` directly calls ``touched()``.  (On the CPU oracle all of them are the same host array and there is nothing to
    keep coherent.)"""

    def __init__(self, ceed: Ceed, n: int, k: int, ld: Optional[int] = None):
        import torch
        self.ceed, self.L, self.n, self.k = ceed, ceed.L, int(n), int(k)
        self.ld = self.n if ld is None else int(ld)
        if self.n < 1 or self.k < 1 or self.ld < self.n:
            raise ValueError(f"a block needs n >= 1, k >= 1 and ld >= n (n = {n}, k = {k}, ld = {ld})")
        self.on_device = ceed.preferred_memtype == MEM_DEVICE
        dev = torch.device("cuda", torch.cuda.current_device()) if self.on_device else torch.device("cpu")
        self.t = torch.zeros(self.k * self.ld, dtype=torch.float64, device=dev)
        self.owner = self._view(self.t)
        self.cols = [self._view(self.t[j * self.ld:j * self.ld + self.n]) for j in range(self.k)]
        self._cvec = {}

    def _view(self, t) -> "Vector":
        v = self.ceed.vector(t.numel())
        v.t = t
        if not self.on_device:
            v.set_array(t.numpy(), copy=False)
        v.touched()
        return v

    def __getitem__(self, j: int) -> "Vector":
        return self.cols[j]

    def touched(self, first: int = 0, count: Optional[int] = None):
        """The memory was written behind the vectors: the owner and the columns [first, first + count) are handed over again."""
        self.owner.touched()
        for v in self.cols[first:self.k if count is None else first + count]:
            v.touched()

    # ---- host access (tests, the solver's start vectors and results): through the tensor, never through a vector's mirror ------
    def to_numpy(self) -> np.ndarray:
        """A copy [k][n] of the columns (the padding left out)."""
        if self.on_device:
            self.ceed.synchronize()
        return self.t.cpu().numpy().reshape(self.k, self.ld)[:, :self.n].copy()

    def fill(self, arr, first: int = 0):
        """Columns first .. := the rows of ``arr`` ([count][n], host); the padding is left as it is."""
        import torch
        a = _np_f64(arr).reshape(-1, self.n)
        if self.on_device:
            self.ceed.synchronize()
        self.t.view(self.k, self.ld)[first:first + a.shape[0], :self.n].copy_(torch.from_numpy(a))
        if self.on_device:
            torch.cuda.current_stream().synchronize()
        self.touched(first, a.shape[0])

    # ---- the block operations ---------------------------------------------------------------------------------------------------
    def _portable(self, who: str, symbol: str) -> bool:
        if self.L.has(symbol):
            return False
        if self.on_device:
            raise CeedError(f"{who}: {self.L.path} has no {symbol} and the block is in device memory: the portable form works on host arrays only")
        return True

    def _host(self, first: int, count: int) -> np.ndarray:
        return self.t.numpy().reshape(self.k, self.ld)[first:first + count, :self.n]

    def gram(self, other: "BlockVector", G: "Vector", a0: int = 0, ka: Optional[int] = None, b0: int = 0, kb: Optional[int] = None,
             weight: Optional["Vector"] = None):
        """G[i][j] = sum_r weight[r] self_{a0+i}[r] other_{b0+j}[r] (CeedXVectorBlockGram) into the first ka * kb entries of the vector G,
        row-major; nothing is read on the host."""
        ka = self.k - a0 if ka is None else ka
        kb = other.k - b0 if kb is None else kb
        if other.n != self.n or other.ld != self.ld:
            raise CeedError("BlockVector.gram: the blocks differ in n or ld")
        self.owner.touched(); other.owner.touched()
        if not self._portable("BlockVector.gram", "CeedXVectorBlockGram"):
            self.L.CeedXVectorBlockGram(self.owner.h, a0, ka, other.owner.h, b0, kb, self.n, self.ld, _h(weight), G.h)
            return
        _block_check("BlockVector.gram", self.n, self.ld, [("A", a0, ka, self.owner.n), ("B", b0, kb, other.owner.n)])
        if G.n < ka * kb:
            raise CeedError(f"BlockVector.gram: G holds {G.n} entries, {ka} x {kb} are written")
        if weight is not None and weight.n < self.n:
            raise CeedError(f"BlockVector.gram: the weight holds {weight.n} entries, n = {self.n} are read")
        pt.assign(G, block_gram_host(self._host(a0, ka), other._host(b0, kb), None if weight is None else weight.to_numpy()[:self.n]))

    def combine(self, A: "BlockVector", Cm, y0: int = 0, ky: Optional[int] = None, a0: int = 0, ka: Optional[int] = None, beta: float = 0.0):
        """self_{y0+j} = sum_i A_{a0+i} Cm[i][j] + beta self_{y0+j} (CeedXVectorBlockCombine); ``Cm`` is a host array [ka][ky] (written to
        a device vector kept with the block) or a Vector that already holds it row-major."""
        ka = A.k - a0 if ka is None else ka
        ky = self.k - y0 if ky is None else ky
        if A.n != self.n or A.ld != self.ld:
            raise CeedError("BlockVector.combine: the blocks differ in n or ld")
        if not isinstance(Cm, Vector):
            cm = _np_f64(Cm)
            if cm.shape != (ka, ky):
                raise CeedError(f"BlockVector.combine: C is {cm.shape}, {ka} x {ky} expected")
            if cm.size not in self._cvec:
                self._cvec[cm.size] = self.ceed.vector(cm.size)
            Cm = self._cvec[cm.size].set_array(cm.reshape(-1))
        self.owner.touched(); A.owner.touched()
        if not self._portable("BlockVector.combine", "CeedXVectorBlockCombine"):
            self.L.CeedXVectorBlockCombine(self.owner.h, y0, ky, A.owner.h, a0, ka, Cm.h, beta, self.n, self.ld)
        else:
            _block_check("BlockVector.combine", self.n, self.ld, [("Y", y0, ky, self.owner.n), ("A", a0, ka, A.owner.n)])
            if Cm.n < ka * ky:
                raise CeedError(f"BlockVector.combine: C holds {Cm.n} entries, {ka} x {ky} are read")
            if A.t.data_ptr() == self.t.data_ptr() and y0 < a0 + ka and a0 < y0 + ky:
                raise CeedError(f"BlockVector.combine: the columns {y0} .. {y0 + ky} of Y overlap the columns {a0} .. {a0 + ka} of A: "
                                "the kernel does not work in place")
            block_combine_host(self._host(y0, ky), A._host(a0, ka), Cm.to_numpy()[:ka * ky].reshape(ka, ky), beta)
        for v in self.cols[y0:y0 + ky]:           # a block-level write: the columns written are handed over again
            v.touched()

    def destroy(self):
        for v in self.cols + [self.owner] + list(self._cvec.values()):
            v.destroy()
        self.cols, self._cvec = [], {}


class ElemRestriction:
    def __init__(self, ceed, nelem, elemsize, ncomp, compstride, lsize, offsets=None, strides=None, strided=False):
        self.ceed, self.L = ceed, ceed.L
        self.nelem, self.elemsize, self.ncomp, self.lsize = int(nelem), int(elemsize), int(ncomp), int(lsize)
        self.h = C.c_void_p()
        if strided:
            st = self.L.STRIDES_BACKEND if strides is None else (c_int * 3)(*strides)
            self.L.CeedElemRestrictionCreateStrided(ceed.h, nelem, elemsize, ncomp, lsize, st, C.byref(self.h))
        else:
            off = np.ascontiguousarray(offsets, dtype=np.int32)
            assert off.size == nelem * elemsize
            self.L.CeedElemRestrictionCreate(ceed.h, nelem, elemsize, ncomp, compstride, lsize, MEM_HOST, COPY_VALUES,
                                             off.ctypes.data_as(c_int_p), C.byref(self.h))

    def _create_vector(self, n: int, evector: bool) -> Vector:
        v = Vector.__new__(Vector)
        v.ceed, v.L, v.n, v._keep, v.h = self.ceed, self.L, n, None, C.c_void_p()
        self.L.CeedElemRestrictionCreateVector(self.h, None if evector else C.byref(v.h), C.byref(v.h) if evector else None)
        return v

    def create_lvector(self) -> Vector:
        return self._create_vector(self.lsize, False)

    def create_evector(self) -> Vector:
        return self._create_vector(self.nelem * self.elemsize * self.ncomp, True)

    def apply(self, tmode, u: Vector, v: Vector):
        self.L.CeedElemRestrictionApply(self.h, tmode, u.h, v.h, self.L.REQUEST_IMMEDIATE)

    def multiplicity(self, mult: Vector):
        self.L.CeedElemRestrictionGetMultiplicity(self.h, mult.h)

    def destroy(self):
        if self.h:
            self.L.lib.CeedElemRestrictionDestroy(C.byref(self.h))


class Basis:
    def __init__(self, ceed, dim, ncomp, P, Q, qmode):
        self.ceed, self.L = ceed, ceed.L
        self.dim, self.ncomp, self.P, self.Q, self.qmode = dim, ncomp, P, Q, qmode
        self.h = C.c_void_p()
        self.L.CeedBasisCreateTensorH1Lagrange(ceed.h, dim, ncomp, P, Q, qmode, C.byref(self.h))

    @property
    def num_qpts(self) -> int:
        return out_value(self.L.CeedBasisGetNumQuadraturePoints, c_int, self.h)

    def _table(self, fn, shape):
        p = c_scalar_p()
        fn(self.h, C.byref(p))
        return np.ctypeslib.as_array(p, shape=shape).copy()

    @property
    def interp1d(self):
        return self._table(self.L.CeedBasisGetInterp1D, (self.Q, self.P))

    @property
    def grad1d(self):
        return self._table(self.L.CeedBasisGetGrad1D, (self.Q, self.P))

    @property
    def qweight1d(self):
        return self._table(self.L.CeedBasisGetQWeights1D, (self.Q,))

    def apply(self, nelem, tmode, emode, u: Vector, v: Vector):
        self.L.CeedBasisApply(self.h, nelem, tmode, emode, u.h, v.h)

    def destroy(self):
        if self.h:
            self.L.lib.CeedBasisDestroy(C.byref(self.h))


class QFunction:
    """``name`` is the reference QFunction name (e.g. ``HyperFSdF``); ``source`` the
    "file:name" locator the reference passes (setuplibceed.c:49-53)."""

    def __init__(self, ceed, name, f=None, source=None, identity=None):
        self.ceed, self.L, self.name = ceed, ceed.L, name
        self.h = C.c_void_p()
        self._ctx = None
        if identity is not None:
            size, inmode, outmode = identity
            self.L.CeedQFunctionCreateIdentity(ceed.h, size, inmode, outmode, C.byref(self.h))
        else:
            src = (source or f"qfunctions/{name}.h:{name}").encode()
            self.L.CeedQFunctionCreateInterior(ceed.h, 1, None if f is None else C.cast(f, C.c_void_p), src, C.byref(self.h))

    def add_input(self, name, size, emode):
        self.L.CeedQFunctionAddInput(self.h, name.encode(), size, emode)
        return self

    def add_output(self, name, size, emode):
        self.L.CeedQFunctionAddOutput(self.h, name.encode(), size, emode)
        return self

    def set_context(self, values: Sequence[float], reported_size: Optional[int] = None):
        """Borrowed context of doubles (Physics {nu, E}: elasticity.h:33-36).
        ``reported_size`` lets tests reproduce the reference's sizeof(pointer) quirk."""
        self._ctx = _np_f64(values).copy()
        size = self._ctx.nbytes if reported_size is None else reported_size
        self.L.CeedQFunctionSetContext(self.h, self._ctx.ctypes.data_as(C.c_void_p), size)
        return self

    def destroy(self):
        if self.h:
            self.L.lib.CeedQFunctionDestroy(C.byref(self.h))


class Operator:
    def __init__(self, ceed, qf: QFunction):
        self.ceed, self.L, self.qf = ceed, ceed.L, qf
        self.h = C.c_void_p()
        self.L.CeedOperatorCreate(ceed.h, qf.h, self.L.QFUNCTION_NONE, self.L.QFUNCTION_NONE, C.byref(self.h))
        self._keep = []

    def set_field(self, name, rstr, basis, vec):
        """rstr/basis/vec: wrapper objects, or None for the NONE/COLLOCATED sentinels,
        or the string "active" for CEED_VECTOR_ACTIVE."""
        L = self.L
        r = L.ELEMRESTRICTION_NONE if rstr is None else rstr.h
        b = L.BASIS_COLLOCATED if basis is None else basis.h
        assert not isinstance(vec, str) or vec == "active"
        v = L.VECTOR_ACTIVE if isinstance(vec, str) else L.VECTOR_NONE if vec is None else vec.h
        L.CeedOperatorSetField(self.h, name.encode(), r, b, v)
        self._keep.append((rstr, basis, vec))
        return self

    def apply(self, vin: Optional[Vector], vout: Optional[Vector]):
        L = self.L
        L.CeedOperatorApply(self.h, L.VECTOR_NONE if vin is None else vin.h, L.VECTOR_NONE if vout is None else vout.h, L.REQUEST_IMMEDIATE)

    def apply_add(self, vin: Vector, vout: Vector):                         # vout += A vin
        self.L.CeedOperatorApplyAdd(self.h, vin.h, vout.h, self.L.REQUEST_IMMEDIATE)

    def apply_residual(self, vin: Vector, t: Vector, b: Vector, w: Vector):   # w = b - A vin in the apply's epilogue (t: scratch)
        self.L.CeedXOperatorApplyResidual(self.h, vin.h, t.h, b.h, w.h)

    def apply_chebyshev(self, vin, t, x, d, r, b, dinv, c1: float, c2: float, assign_x: bool = False):
        """t = A vin consumed where it is formed by the smoother's step on x (with b: Vector.chebyshev_step, without: chebyshev_update)"""
        self.L.CeedXOperatorApplyChebyshev(self.h, vin.h, t.h, x.h, d.h, _h(r), _h(b), dinv.h, c1, c2, int(bool(assign_x)))

    def assemble_diagonal(self, vec: Vector):
        self.L.CeedOperatorLinearAssembleDiagonal(self.h, vec.h, self.L.REQUEST_IMMEDIATE)

    def assemble_pointblock_diagonal(self, vec: Vector):
        """CeedOperatorLinearAssemblePointBlockDiagonal (CEED_EXTERN_OPTIONAL: check ``CeedLib.has`` first): the 3 x 3 nodal blocks,
        [node][comp out][comp in], the block of the node at component-0 L-offset o at 3 * o."""
        self.L.CeedOperatorLinearAssemblePointBlockDiagonal(self.h, vec.h, self.L.REQUEST_IMMEDIATE)

    @property
    def kernel_name(self) -> str:
        return (out_value(self.L.CeedXOperatorGetKernelName, C.c_char_p, self.h) or b"").decode()

    @staticmethod
    def _bytes(mask):
        """(the byte array to keep alive over the call, its pointer, its length) of a mask; (None, None, 0) of an absent one"""
        if mask is None:
            return None, None, 0
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        return m, m.ctypes.data_as(C.POINTER(C.c_ubyte)), m.size

    def set_dirichlet_mask(self, mask: Optional[np.ndarray]):
        _, p, n = self._bytes(mask)
        self.L.CeedXOperatorSetDirichletMask(self.h, MEM_HOST, p, n)

    def set_dirichlet_mask_mode(self, mask_in, mask_out=None, mode: int = 3):
        """1 = masked entries read as zero on input, 2 = masked rows dropped on output, 3 = both; transfer operators have different
        L-vectors on their two sides and take both masks."""
        mi, mo = self._bytes(mask_in), self._bytes(mask_out)
        self.L.CeedXOperatorSetDirichletMaskMode(self.h, MEM_HOST, mi[1], mi[2], mo[1], mo[2], mode)

    def set_fine_scale(self, scale: Optional[Vector]):      # the fine-side 1 / multiplicity of a transfer operator (None clears)
        self.L.CeedXOperatorSetFineScale(self.h, _h(scale))

    def set_overlap_split(self, n_leading_elems: int, priority: Optional[np.ndarray]):
        """CeedXOperatorSetOverlapSplit: leading elements / priority L-vector entries of the split-phase apply."""
        _, p, n = self._bytes(priority)
        self.L.CeedXOperatorSetOverlapSplit(self.h, n_leading_elems if priority is not None else 0, p, n)

    def apply_state(self, u: "Vector"):
        """CeedXOperatorApplyState: write only the stored state (passive gradu output) of a residual-shaped operator."""
        self.L.CeedXOperatorApplyState(self.h, u.h)

    def mass_term_available(self) -> bool:
        """CeedXOperatorMassTermAvailable: is a fused kernel with the mass term (K + c M in the launches of K) instantiated for this
        Jacobian operator's (P, Q, QFunction)?  False where the library lacks the entry point (CEED_EXTERN_OPTIONAL: the CPU oracle); an
        operator that is no Jacobian is refused by the library."""
        return self.L.has("CeedXOperatorMassTermAvailable") and bool(out_value(self.L.CeedXOperatorMassTermAvailable, C.c_int, self.h))

    def set_mass_term(self, c: float):
        """CeedXOperatorSetMassTerm: every apply form of this Jacobian operator then gives (K + c M) x; 0 clears the term.  A recorded
        graph keeps the coefficient it was recorded with.  The diagonals ignore the term."""
        if not self.L.has("CeedXOperatorSetMassTerm"):
            raise CeedError("this library has no CeedXOperatorSetMassTerm (CEED_EXTERN_OPTIONAL): apply the mass operator on its own")
        self.L.CeedXOperatorSetMassTerm(self.h, c)

    def apply_phase(self, vin: "Vector", vout: "Vector", phase: int):
        self.L.CeedXOperatorApplyPhase(self.h, vin.h, vout.h, phase)

    def set_timing(self, enable: bool):
        self.L.CeedXOperatorSetTiming(self.h, int(enable))

    def get_timing(self):
        ms, n = C.c_double(), C.c_int64()
        self.L.CeedXOperatorGetTiming(self.h, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def launch_info(self) -> dict:
        """CeedXOperatorGetLaunchInfo: how the last apply was launched (segments of the pipelined restriction transpose)."""
        out = (C.c_int * 4)()
        self.L.CeedXOperatorGetLaunchInfo(self.h, out)
        return dict(segments=out[0], streams=out[1], assemble_launches=out[2], last_segment_elements=out[3])

    def apply_with_halo(self, vin: "Vector", vout: "Vector", halo):
        """CeedXOperatorApplyWithHalo: the (split-phase) apply and the interface sum of its output in one call; `halo` is a
        halo.RcclHalo or a raw CeedXHalo handle."""
        self.L.CeedXOperatorApplyWithHalo(self.h, vin.h, vout.h, getattr(halo, "h", halo))

    def destroy(self):
        if self.h:
            self.L.lib.CeedOperatorDestroy(C.byref(self.h))
