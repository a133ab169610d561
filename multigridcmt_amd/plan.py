"""Python handle on a device hierarchy (``mgcmt_plan`` of include/mgcmt_hip.h).

One plan = one operator (plus optional mass operator) on one grid size with a fixed coarsest level:
the Galerkin factors of every level (MGCMTSolver.py:318) and the level vectors live on the GPU.
"""
import ctypes
from collections import OrderedDict
from ctypes import c_double, c_int, c_int64, c_void_p

import numpy as np

from . import _lib, hostmem
from ._lib import OP_A, OP_M, SLOT_F, SLOT_T, SLOT_V, SLOT_W, PlanDesc, as_dp, check


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# the creator of a plan whose operator has a per-point part, by (axes, StructuredOperator.point_part kind); it takes the
# arrays of point_part in their order, and how messages name the kind
_POINT_CREATORS = {(2, "diag"): "mgcmt_plan_create_pot", (2, "bonds"): "mgcmt_plan_create_bonds", (2, "planes"): "mgcmt_plan_create_nine",
                   (3, "diag"): "mgcmt_plan_create3d_pot", (3, "bonds"): "mgcmt_plan_create3d_bonds", (3, "planes"): "mgcmt_plan_create3d_stencil"}
_POINT_NAMES = {"diag": "a point diagonal", "bonds": "a point diagonal and point bonds", "planes": "a point stencil (a point diagonal and more)"}


class Plan:
    def __init__(self, op, lowest, nvec=1, mass=None, device=0, row_begin=0, row_end=0, strip_levels=0):
        self._h = c_void_p()
        self.op = op
        self.mass = mass
        self.dim = {"1d": 1, "2d": 2, "3d": 3}[op.dimension]
        self.g = op.g
        self.lowest = int(lowest)
        self.nvec = int(nvec)
        self.device = device
        sharded = bool(row_begin or row_end or strip_levels)
        kind, arrays = op.point_part()
        if kind is not None and (mass is not None or sharded):
            raise self._point_refusal(kind, mass is not None)
        if self.dim == 3:
            desc, keep = self._desc3d(op, mass, sharded)
        else:
            nterms, xfac, yfac = op.factor_blocks()
            desc = PlanDesc()
            desc.dim, desc.nterms, desc.g, desc.lowest = self.dim, nterms, self.g, self.lowest
            desc.xfac = as_dp(xfac) if xfac is not None else None
            desc.yfac = as_dp(yfac)
            keep = [xfac, yfac]
            if mass is not None:
                mt, mx, my = mass.factor_blocks()
                desc.m_nterms = mt
                desc.m_xfac = as_dp(mx) if mx is not None else None
                desc.m_yfac = as_dp(my)
                keep += [mx, my]
            desc.nvec, desc.device = self.nvec, device
            desc.row_begin, desc.row_end, desc.strip_levels = row_begin, row_end, strip_levels
        if kind is not None:
            # the per-point hierarchy (level 0: the operator's planes, below it R (.) P) is built at creation
            arrays = [_f64(a) for a in arrays]
            create = getattr(_lib.lib(), _POINT_CREATORS[self.dim, kind])
            check(create(ctypes.byref(desc), *[as_dp(a) for a in arrays], ctypes.byref(self._h)))
        elif self.dim == 3 and mass is not None:
            mt, mz, my, mx = mass.factor_blocks()
            check(_lib.lib().mgcmt_plan_create3d_mass(ctypes.byref(desc), mt, as_dp(mz), as_dp(my), as_dp(mx), ctypes.byref(self._h)))
        elif self.dim == 3:
            check(_lib.lib().mgcmt_plan_create3d(ctypes.byref(desc), ctypes.byref(self._h)))
        else:
            check(_lib.lib().mgcmt_plan_create(ctypes.byref(desc), ctypes.byref(self._h)))
        del keep
        n = c_int(0)
        check(_lib.lib().mgcmt_plan_num_levels(self._h, ctypes.byref(n)))
        self.num_levels = n.value
        self.shapes = [self.level_shape(l) for l in range(self.num_levels)]
        self._shifts = None
        self.op_stale = False        # set_point_diagonal has replaced the diagonal: the plan no longer describes self.op

    def _point_refusal(self, kind, mass):
        """The error of a plan whose operator has a per-point part and that is given a mass operator (`mass`) or a row strip:
        such plans are whole grids without a mass operator."""
        subject = "%s operator with %s" % ("a 3-D" if self.dim == 3 else "an", _POINT_NAMES[kind])
        if not mass:
            return ValueError(subject + " is not sharded")
        return ValueError("%s takes no mass operator: the Rayleigh-quotient routines (rqmin, vcycle_rqmg, ...) do not run on it; vcycle / "
                          "vcycle_matrix%s, the smoothers wjacobi and gseidel_rb, apply and drivers.block_eigensolve do"
                          % (subject, "" if self.dim == 3 else " / fmg"))

    def _desc3d(self, op, mass, sharded):
        """the description of a 3-D plan and the arrays it points at"""
        if mass is not None and (mass.dimension != "3d" or mass.g != op.g):
            raise ValueError("the mass operator of a 3-D plan must be a 3-D operator on the same %d^3 grid" % op.g)
        if mass is not None and not 1 <= len(mass.terms) <= _lib.MAX_TERMS:
            raise ValueError("a 3-D mass operator has 1 .. %d Kronecker terms, not %d" % (_lib.MAX_TERMS, len(mass.terms)))
        if sharded:
            raise ValueError("3-D plans are not sharded")
        if self.lowest > 16:
            raise ValueError("lowest_level=%d: the coarsest 3-D level is solved directly and may be at most 16^3" % self.lowest)
        nterms, zfac, yfac, xfac = op.factor_blocks()
        desc = _lib.Plan3dDesc()
        desc.nterms, desc.nvec, desc.g, desc.lowest = nterms, self.nvec, self.g, self.lowest
        desc.zfac, desc.yfac, desc.xfac = as_dp(zfac), as_dp(yfac), as_dp(xfac)
        desc.device = self.device
        return desc, [zfac, yfac, xfac]

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if self._h:
            _lib.lib().mgcmt_plan_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- geometry ---------------------------------------------------------------------------------
    def level_shape(self, level):
        r, c, b = c_int64(0), c_int64(0), c_int64(0)
        check(_lib.lib().mgcmt_plan_level_shape(self._h, level, ctypes.byref(r), ctypes.byref(c), ctypes.byref(b)))
        return r.value, c.value, b.value

    def size(self, level=0):
        r, c, _ = self.shapes[level]
        return r * c

    def factors(self, level, which, op=OP_A):
        """Host copy of a level's Kronecker factors: array [nterms, 3, n]."""
        src = self.op if op == OP_A else self.mass
        nterms = len(src.terms)
        n = (self.g >> level) if (which == 1 or self.dim >= 2) else 1
        out = np.zeros((nterms, 3, n))
        check(_lib.lib().mgcmt_plan_get_factors(self._h, op, level, which, as_dp(out), out.size))
        return out

    def point_stencil(self, level):
        """Host copy of the per-point part of `level` of a plan whose operator has a point diagonal: level 0 the diagonal,
        array [rows, cols]; below it the 9-point stencil R D P, array [3, 3, rows, cols] — entry [a, b, i, j] is the
        coefficient of point (i + a - 1, j + b - 1) in row (i, j).  Level 0 of an operator with ``point_bonds``: the three
        planes D, E, S, array [3, rows, cols]; of an operator with ``point_stencil``: [3, 3, rows, cols] like the levels below.  3-D: [g, g, g] on level 0 ([4, g, g, g] = D, Bx, By, Bz with bonds) and the 27-point stencil
        [3, 3, 3, g_l, g_l, g_l] below — entry [a, b, c, z, y, x] is the coefficient of point (z + a - 1, y + b - 1, x + c - 1); level 0 of
        a 3-D operator with ``point_stencil`` has that shape too."""
        kind = self.op.point_part()[0] if level == 0 else "planes"      # (below level 0: the Galerkin product's 3^dim planes)
        lead = {"bonds": (self.dim + 1,), "planes": (3,) * self.dim}.get(kind, ())
        out = np.zeros(lead + (self.g >> level,) * self.dim)
        check(_lib.lib().mgcmt_plan_get_point_stencil(self._h, level, as_dp(out), out.size))
        return out

    def level_path_3d(self, level):
        """(kind, marching) of a 3-D plan's level: one of _lib.PATH3D_* and whether the marching kernels run it."""
        kind, marching = c_int(0), c_int(0)
        check(_lib.lib().mgcmt_plan3d_level_path(self._h, level, ctypes.byref(kind), ctypes.byref(marching)))
        return kind.value, bool(marching.value)

    def level_tiled(self, level):
        """Whether `level` runs the tile kernels of a nine-plane level (mgcmt_plan_level_tiled; decided at creation from the
        level's kind and size and the environment variable MGCMT_NINE_TILE)."""
        t = c_int(0)
        check(_lib.lib().mgcmt_plan_level_tiled(self._h, level, ctypes.byref(t)))
        return bool(t.value)

    def level_halo(self, level):
        """(halo rows kept around every vector of `level`, how many of them a sharded cycle exchanges and reads)"""
        h, x = c_int(0), c_int(0)
        check(_lib.lib().mgcmt_plan_level_halo(self._h, level, ctypes.byref(h), ctypes.byref(x)))
        return h.value, x.value

    def vec_ptr(self, level, slot, vec=0):
        p = c_void_p()
        check(_lib.lib().mgcmt_vec_ptr(self._h, level, slot, vec, ctypes.byref(p)))
        return p.value

    # -- data -------------------------------------------------------------------------------------
    def set_shifts(self, shifts, stream=None):
        s = _f64(np.atleast_1d(shifts)).reshape(-1)
        check(_lib.lib().mgcmt_set_shifts(self._h, as_dp(s), len(s), stream))
        self._shifts = s.copy()

    def upload(self, level, slot, vec, host, stream=None):
        a = _f64(host).reshape(-1)
        check(_lib.lib().mgcmt_upload(self._h, level, slot, vec, as_dp(a), a.size, stream))

    def download(self, level, slot, vec, stream=None):
        out = hostmem.empty(self.size(level))  # (large results: recycled page-locked memory, one DMA)
        check(_lib.lib().mgcmt_download(self._h, level, slot, vec, as_dp(out), out.size, stream))
        return out

    def download_into(self, level, slot, vec, out, stream=None):
        """Like download, into a caller-provided contiguous float64 array of the level's size."""
        if not (out.flags.c_contiguous and out.dtype == np.float64 and out.size == self.size(level)):
            raise ValueError("download_into needs a contiguous float64 array of the level's size")
        check(_lib.lib().mgcmt_download(self._h, level, slot, vec, as_dp(out), out.size, stream))

    def fill(self, level, slot, vec, value, stream=None):
        check(_lib.lib().mgcmt_fill(self._h, level, slot, vec, c_double(value), stream))

    def zero(self, level, slot, vec, stream=None):
        check(_lib.lib().mgcmt_zero(self._h, level, slot, vec, stream))

    def copy(self, level, src_slot, src_vec, dst_slot, dst_vec, stream=None):
        check(_lib.lib().mgcmt_copy(self._h, level, src_slot, src_vec, dst_slot, dst_vec, stream))

    def sync(self, stream=None):
        check(_lib.lib().mgcmt_sync(stream))

    # -- the path ---------------------------------------------------------------------------------
    def smooth(self, level, kind, nu, omega=1.0, k=1, stream=None):
        check(_lib.lib().mgcmt_smooth(self._h, level, kind, nu, c_double(omega), k, stream))

    def residual_restrict(self, level, k=1, stream=None):
        check(_lib.lib().mgcmt_residual_restrict(self._h, level, k, stream))

    def prolong_correct(self, level, k=1, stream=None):
        check(_lib.lib().mgcmt_prolong_correct(self._h, level, k, stream))

    def coarse_solve(self, level, k=1, stream=None):
        check(_lib.lib().mgcmt_coarse_solve(self._h, level, k, stream))

    def vcycle(self, nu1, nu2, kind, omega=1.0, k=1, nu_coarse=4, gram_schmidt=False, level=0, stream=None, zero_start=False):
        """zero_start: the iterate on `level` is to be taken as zero, whatever V holds (the reference's eigen-drivers
        start every cycle this way, 1DPotMatrixVcycle.py:70).  The library's first pass then neither reads V nor
        needs it cleared (MGCMT_CYCLE_ZERO_START)."""
        flags = (_lib.CYCLE_GRAM_SCHMIDT if gram_schmidt else 0) | (_lib.CYCLE_ZERO_START if zero_start else 0)
        check(_lib.lib().mgcmt_vcycle(self._h, level, nu1, nu2, nu_coarse, kind, c_double(omega), k, flags, stream))

    def twogrid(self, nu1, nu2, kind, omega=1.0, k=1, level=0, stream=None):
        check(_lib.lib().mgcmt_twogrid(self._h, level, nu1, nu2, kind, c_double(omega), k, stream))

    def apply(self, level, src, dst, op=OP_A, with_shift=False, stream=None):
        check(_lib.lib().mgcmt_apply(self._h, op, level, src[0], src[1], dst[0], dst[1], 1 if with_shift else 0, stream))

    def restrict(self, level, src, dst, stream=None):
        check(_lib.lib().mgcmt_restrict(self._h, level, src[0], src[1], dst[0], dst[1], stream))

    def prolong(self, level, src, dst, accumulate=False, stream=None):
        check(_lib.lib().mgcmt_prolong(self._h, level, src[0], src[1], dst[0], dst[1], 1 if accumulate else 0, stream))

    def dot(self, level, a, b, stream=None):
        out = c_double(0.0)
        check(_lib.lib().mgcmt_dot(self._h, level, a[0], a[1], b[0], b[1], ctypes.byref(out), stream))
        return out.value

    def gram(self, level, vectors, stream=None):
        """Gram matrix (len(vectors) <= 6) of the (slot, vec) pairs in one pass; synchronises."""
        nv = len(vectors)
        slots = (ctypes.c_int * nv)(*[v[0] for v in vectors])
        vecs = (ctypes.c_int * nv)(*[v[1] for v in vectors])
        out = np.zeros((nv, nv))
        check(_lib.lib().mgcmt_gram(self._h, level, nv, slots, vecs, _lib.as_dp(out), stream))
        return out

    def ritz_pair(self, level, x, w, scratch, stream=None):
        """(<x,x>, <x,w>, <w,w>, <x,A w>, <w,A w>) with the unshifted operator of `level`: the 2 x 2 Rayleigh-Ritz problem
        on span{x, w} when <x, A x> is known.  One pass over x and w on 2-D 5-point levels (nothing stored); `scratch`
        ((slot, vec), distinct from x and w) receives A w elsewhere.  Synchronises."""
        out = np.zeros(5)
        check(_lib.lib().mgcmt_ritz_pair(self._h, level, x[0], x[1], w[0], w[1], scratch[0], scratch[1], as_dp(out), stream))
        return out

    def rayleigh_residual(self, level, slot, k, stream=None):
        """(rq, res): Rayleigh quotients <v, A v>/<v, v> and residual norms ||(A - mu I) v|| of columns 0..k-1 of `slot`
        (mu = the plan's shifts); one synchronisation for all columns.  Slot W is the scratch."""
        rq, res = np.zeros(k), np.zeros(k)
        check(_lib.lib().mgcmt_rayleigh_residual(self._h, level, slot, k, as_dp(rq), as_dp(res), stream))
        return rq, res

    def rqmin(self, level, slot, vecs, nu, robust=False, want_rho=True, stream=None):
        """nu steps of the reference's rqmin (MGCMTSolver.py:17-57) on `level`, resident on the device (mgcmt_rqmin): vecs[0]
        of `slot` is the iterate, vecs[1..5] work space.  Returns rho (one synchronisation) or None (want_rho=False: none)."""
        v = (ctypes.c_int * 6)(*[int(i) for i in vecs])
        rho = c_double(0.0)
        check(_lib.lib().mgcmt_rqmin(self._h, level, slot, v, int(nu), 1 if robust else 0, ctypes.byref(rho) if want_rho else None, stream))
        return rho.value if want_rho else None

    def vcycle_rqmg(self, slot, vecs, nu1, nu2, robust=False, want_rho=True, stream=None):
        """One cycle of the reference's Rayleigh-quotient multigrid (MGCMTSolver.py:99-122) over all levels of the plan,
        resident on the device (mgcmt_vcycle_rqmg); vecs as for rqmin, on every level."""
        v = (ctypes.c_int * 6)(*[int(i) for i in vecs])
        rho = c_double(0.0)
        check(_lib.lib().mgcmt_vcycle_rqmg(self._h, slot, v, int(nu1), int(nu2), 1 if robust else 0, ctypes.byref(rho) if want_rho else None, stream))
        return rho.value if want_rho else None

    def rq_line_step(self, level, x, w, x_out, g, work=None, robust=False, record=-1, stream=None):
        """x_out = x + delta w minimising the Rayleigh quotient over span{x, w} (the 2 x 2 problem of rqmin,
        MGCMTSolver.py:33-50) and g = 2 (A x_out - rho M x_out), on the device without a host round trip
        (mgcmt_rq_line_step); vectors are (slot, vec) pairs.  w=None: rho and g of x alone.  record >= 0: rho is kept as
        that entry of the device-side history (rq_history)."""
        def pair(v):
            return None if v is None else (ctypes.c_int * 2)(int(v[0]), int(v[1]))
        check(_lib.lib().mgcmt_rq_line_step(self._h, level, pair(x), pair(w), pair(x_out), pair(g), pair(work), 1 if robust else 0, int(record),
                                            stream))

    def rq_history(self, first, count, stream=None):
        """entries [first, first + count) of the Rayleigh quotients recorded by rq_line_step (one synchronisation)"""
        out = np.empty(int(count))
        check(_lib.lib().mgcmt_rq_history(self._h, int(first), int(count), _lib.as_dp(out), stream))
        return out

    @staticmethod
    def _pcg_begin_args(vecs, rtol, zero_start, flexible):
        """the vector list, the tolerance and the flags as both begins take them"""
        flags = (_lib.PCG_ZERO_START if zero_start else 0) | (_lib.PCG_FLEXIBLE if flexible else 0)
        return (ctypes.c_int * 4)(*[int(i) for i in vecs]), c_double(rtol), flags

    def pcg_begin(self, vecs, rtol, zero_start=False, flexible=False, stream=None):
        """Start a V-cycle-preconditioned conjugate-gradient solve of (A - mu I) x = f on level 0 (mgcmt_pcg_begin): f is in
        F[0] column 0 and, unless zero_start, x_0 in column vecs[0] of slot W; vecs = four distinct columns of W (x, p, q, p2).
        mu is the plan's shift 0.  Nothing synchronises."""
        check(_lib.lib().mgcmt_pcg_begin(self._h, *self._pcg_begin_args(vecs, rtol, zero_start, flexible), stream))

    def pcg_iterate(self, iterations, nu1, nu2, kind, omega=1.0, nu_coarse=4, stream=None):
        """Queue `iterations` iterations (one cycle, one operator application and four fused passes each) without
        synchronising; the ones behind the iteration that meets the tolerance change nothing (mgcmt_pcg_iterate)."""
        check(_lib.lib().mgcmt_pcg_iterate(self._h, int(iterations), int(nu1), int(nu2), int(nu_coarse), kind, c_double(omega), stream))

    def pcg_status(self, history=0, stream=None):
        """(iterations done, status, indefinite, ||f||, the first `history` recorded ||r_k||) — the one synchronisation of a
        solve (mgcmt_pcg_status); status is _lib.PCG_RUNNING, PCG_CONVERGED or PCG_BREAKDOWN."""
        it, st, fnorm = c_int(0), c_int(0), c_double(0.0)
        hist = np.zeros(int(history))
        check(_lib.lib().mgcmt_pcg_status(self._h, ctypes.byref(it), ctypes.byref(st), ctypes.byref(fnorm), as_dp(hist) if hist.size else None,
                                          hist.size, stream))
        return it.value, st.value & 0xff, bool(st.value & _lib.PCG_INDEFINITE), fnorm.value, hist

    def pcg_begin_k(self, k, vecs, rtol, zero_start=False, flexible=False, stream=None):
        """Start k conjugate-gradient solves at once, (A - mu_c I) x_c = f_c with mu_c the plan's shift c (mgcmt_pcg_begin_k): f_c is
        in F[0] column c and, unless zero_start, x_0 of column c in column vecs[0] + c of slot W; vecs = the first columns of four
        ranges of k consecutive columns of W (x, p, q, p2) that do not overlap, so the plan stores at least 4 k vectors.  Nothing
        synchronises."""
        check(_lib.lib().mgcmt_pcg_begin_k(self._h, int(k), *self._pcg_begin_args(vecs, rtol, zero_start, flexible), stream))
        self._pcg_k = int(k)

    def pcg_iterate_k(self, iterations, nu1, nu2, kind, omega=1.0, nu_coarse=4, stream=None):
        """Queue `iterations` iterations of the batched solve without synchronising: one k-column cycle and the passes on all
        columns per iteration; a column that has stopped is frozen while the others go on (mgcmt_pcg_iterate_k)."""
        check(_lib.lib().mgcmt_pcg_iterate_k(self._h, int(iterations), int(nu1), int(nu2), int(nu_coarse), kind, c_double(omega), stream))

    def pcg_status_k(self, history=0, stream=None):
        """(columns still running, iterations done[k], status[k], indefinite[k], ||f||[k], the first `history` recorded ||r_k|| of
        every column as a (k, history) array) — the one synchronisation of a batched solve (mgcmt_pcg_status_k)."""
        k = getattr(self, "_pcg_k", 1)           # (without a begin the library refuses the call)
        running = c_int(0)
        it, st = (ctypes.c_int * k)(), (ctypes.c_int * k)()
        fnorm, hist = np.zeros(k), np.zeros((k, int(history)))
        check(_lib.lib().mgcmt_pcg_status_k(self._h, ctypes.byref(running), it, st, as_dp(fnorm), as_dp(hist) if hist.size else None,
                                            int(history), stream))
        st = np.array(st[:], dtype=np.int64)
        return running.value, np.array(it[:], dtype=np.int64), st & 0xff, (st & _lib.PCG_INDEFINITE) != 0, fnorm, hist

    def pcg_time_pass(self, which, reps, stream=None):
        """average milliseconds of one pass of a conjugate-gradient iteration (_lib.PCG_PASS_*) with its scalar kernel, on the
        vectors of the solve in progress, which are scratch afterwards (mgcmt_pcg_time_pass)"""
        ms = c_double(0.0)
        check(_lib.lib().mgcmt_pcg_time_pass(self._h, int(which), int(reps), ctypes.byref(ms), stream))
        return ms.value

    def lincomb(self, level, terms, dst, stream=None):
        """dst <- sum of coeff * (slot, vec) over `terms` = [(coeff, (slot, vec)), ...] (at most four)."""
        nt = len(terms)
        coeffs = np.array([float(c) for c, _ in terms])
        slots = (ctypes.c_int * nt)(*[v[0] for _, v in terms])
        vecs = (ctypes.c_int * nt)(*[v[1] for _, v in terms])
        check(_lib.lib().mgcmt_lincomb(self._h, level, nt, _lib.as_dp(coeffs), slots, vecs, dst[0], dst[1], stream))

    def block_gram(self, level, a, b, stream=None):
        """A^T B for lists of (slot, vec) pairs, len(a) <= 12, len(b) <= 4, in one pass; synchronises."""
        na, nb = len(a), len(b)
        out = np.zeros((na, nb))
        check(_lib.lib().mgcmt_block_gram(self._h, level, na, (ctypes.c_int * na)(*[v[0] for v in a]), (ctypes.c_int * na)(*[v[1] for v in a]),
                                          nb, (ctypes.c_int * nb)(*[v[0] for v in b]), (ctypes.c_int * nb)(*[v[1] for v in b]),
                                          _lib.as_dp(out), stream))
        return out

    def block_combine(self, level, inputs, outputs, coeffs, stream=None):
        """outputs[j] <- sum_i coeffs[i, j] * inputs[i] ((slot, vec) pairs; <= 12 inputs, <= 4 distinct outputs; an output
        may be one of the inputs)."""
        nin, nout = len(inputs), len(outputs)
        c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float64).reshape(nin, nout))
        check(_lib.lib().mgcmt_block_combine(self._h, level, nin, (ctypes.c_int * nin)(*[v[0] for v in inputs]),
                                             (ctypes.c_int * nin)(*[v[1] for v in inputs]), nout,
                                             (ctypes.c_int * nout)(*[v[0] for v in outputs]), (ctypes.c_int * nout)(*[v[1] for v in outputs]),
                                             _lib.as_dp(c), stream))

    def block_pencil(self, level, s, a_s, m_s=None, stream=None):
        """(H, G) = (S^T AS, S^T MS) for lists of (slot, vec) pairs of equal length m <= 48 (m_s=None: M = I, G = S^T S): every
        vector read once in one pass on the matrix cores (mgcmt_block_pencil); full m x m matrices; synchronises."""
        m = len(s)
        if len(a_s) != m or (m_s is not None and len(m_s) != m):
            raise ValueError("block_pencil: S, AS and MS name the same number of vectors")

        def ints(vs, which):
            return (ctypes.c_int * m)(*[v[which] for v in vs])
        H, G = np.zeros((m, m)), np.zeros((m, m))
        check(_lib.lib().mgcmt_block_pencil(self._h, level, m, ints(s, 0), ints(s, 1), ints(a_s, 0), ints(a_s, 1),
                                            None if m_s is None else ints(m_s, 0), None if m_s is None else ints(m_s, 1),
                                            _lib.as_dp(H), _lib.as_dp(G), stream))
        return H, G

    def block_combine_wide(self, level, inputs, outputs, coeffs, stream=None):
        """outputs[j] <- sum_i coeffs[i, j] * inputs[i] ((slot, vec) pairs; <= 48 inputs, <= 16 distinct outputs; an output
        may be one of the inputs)."""
        nin, nout = len(inputs), len(outputs)
        c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float64).reshape(nin, nout))
        check(_lib.lib().mgcmt_block_combine_wide(self._h, level, nin, (ctypes.c_int * nin)(*[v[0] for v in inputs]),
                                                  (ctypes.c_int * nin)(*[v[1] for v in inputs]), nout,
                                                  (ctypes.c_int * nout)(*[v[0] for v in outputs]),
                                                  (ctypes.c_int * nout)(*[v[1] for v in outputs]), _lib.as_dp(c), stream))

    def block_deflate(self, level, q, w, want_coeffs=False, stream=None):
        """w[j] <- w[j] - sum_i <q[i], w[j]> q[i] ((slot, vec) pairs; <= 64 vectors q, <= 16 distinct vectors w, none of them a
        q): two stream-ordered passes, the coefficients staying on the device (mgcmt_block_deflate).  want_coeffs: returns the
        len(q) x len(w) coefficients <q[i], w[j]> and synchronises."""
        nq, k = len(q), len(w)
        c = np.zeros((nq, k)) if want_coeffs else None
        check(_lib.lib().mgcmt_block_deflate(self._h, level, nq, (ctypes.c_int * nq)(*[v[0] for v in q]), (ctypes.c_int * nq)(*[v[1] for v in q]),
                                             k, (ctypes.c_int * k)(*[v[0] for v in w]), (ctypes.c_int * k)(*[v[1] for v in w]),
                                             None if c is None else _lib.as_dp(c), stream))
        return c

    def block_density(self, level, xs, weights, dst, stream=None):
        """dst <- sum_t weights[t] * xs[t]^2 point by point ((slot, vec) pairs; <= 64 vectors xs, dst none of them): one
        stream-ordered pass that reads every vector once (mgcmt_block_density) — the charge density of states with their
        occupations.  Bit-reproducible."""
        nq = len(xs)
        w = np.array([float(f) for f in weights])
        if w.size != nq:
            raise ValueError("block_density: one weight per vector")
        check(_lib.lib().mgcmt_block_density(self._h, level, nq, (ctypes.c_int * nq)(*[v[0] for v in xs]), (ctypes.c_int * nq)(*[v[1] for v in xs]),
                                             _lib.as_dp(w), dst[0], dst[1], stream))

    def mix_residual(self, level, out, inp, r, prev=(), stream=None):
        """r <- out - inp point by point ((slot, vec) pairs; r none of the vectors read) and, from the same pass over out, inp
        and the <= 8 earlier residuals ``prev``, the inner products (<r, prev[j]> in the order given, <r, r>, <out, out>) as
        len(prev) + 2 numbers (mgcmt_mix_residual): the residual of an Anderson-mixing step, its row of the Gram matrix and
        the relative change sqrt(<r, r> / <out, out>).  Synchronises.  Bit-reproducible, whatever the launch's grid."""
        nprev = len(prev)
        res = np.zeros(nprev + 2)
        check(_lib.lib().mgcmt_mix_residual(self._h, level, out[0], out[1], inp[0], inp[1], r[0], r[1], nprev,
                                            (ctypes.c_int * nprev)(*[v[0] for v in prev]) if nprev else None,
                                            (ctypes.c_int * nprev)(*[v[1] for v in prev]) if nprev else None, _lib.as_dp(res), stream))
        return res

    def mix_combine(self, level, xs, rs, alpha, beta, dst, stream=None):
        """dst <- sum_i alpha[i] * (xs[i] + beta * rs[i]) point by point ((slot, vec) pairs; <= 9 pairs; dst may be xs[0] and no
        other input): one stream-ordered pass over the 2 len(xs) vectors (mgcmt_mix_combine) — the new iterate of an
        Anderson-mixing step.  Bit-reproducible."""
        p = len(xs)
        a = np.array([float(c) for c in alpha])
        if len(rs) != p or a.size != p:
            raise ValueError("mix_combine: one residual and one coefficient per vector x")
        ints = lambda vs, i: (ctypes.c_int * p)(*[v[i] for v in vs])
        check(_lib.lib().mgcmt_mix_combine(self._h, level, p, ints(xs, 0), ints(xs, 1), ints(rs, 0), ints(rs, 1), _lib.as_dp(a), float(beta),
                                           dst[0], dst[1], stream))

    def set_point_diagonal(self, terms, stream=None):
        """The per-point diagonal of the plan's operator <- sum of coeff * (slot, vec) over `terms` = [(coeff, (slot, vec)), ...]
        (at most four level-0 vectors of this plan, the arithmetic of lincomb), and the per-point planes of every level below
        formed again on the device (mgcmt_plan_set_point_diagonal): the plan then holds the bits of a plan created from that
        diagonal; bonds and the off-centre planes of a stencil stay.  Stream-ordered, no allocation, no synchronisation.
        From here on the plan no longer describes ``self.op`` (``op_stale`` is set; ``point_stencil(level)`` stays the truth),
        so it leaves get_plan's cache if it is in it: no later caller is handed a plan with this diagonal.  A plan that left the
        cache this way belongs to whoever holds it: release_plans() no longer closes it, its holder's close() (or the last
        reference going away) does."""
        nt = len(terms)
        coeffs = np.array([float(c) for c, _ in terms])
        slots = (ctypes.c_int * nt)(*[v[0] for _, v in terms])
        vecs = (ctypes.c_int * nt)(*[v[1] for _, v in terms])
        check(_lib.lib().mgcmt_plan_set_point_diagonal(self._h, nt, _lib.as_dp(coeffs), slots, vecs, stream))
        self.op_stale = True
        for key, cached in list(_PLANS.items()):
            if cached is self:
                del _PLANS[key]

    def copy_across(self, level, src, other, dst, stream=None):
        """(slot, vec) `dst` of the plan `other` <- (slot, vec) `src` of this plan on `level`: a device-to-device copy between two
        plans of the same dimension and level shape on one device (mgcmt_copy_across)."""
        check(_lib.lib().mgcmt_copy_across(self._h, level, src[0], src[1], other._h, dst[0], dst[1], stream))

    def block_project(self, level, b, w, ab=None, aw=None, want_coeffs=False, stream=None):
        """block_deflate with companions: w[j] <- w[j] - sum_i <b[i], w[j]> b[i] and, with ab and aw, aw[j] <- aw[j] -
        sum_i <b[i], w[j]> ab[i] ((slot, vec) pairs; <= 64 vectors b, <= 16 distinct vectors w; mgcmt_block_project).
        want_coeffs: returns the len(b) x len(w) coefficients and synchronises."""
        nb, k = len(b), len(w)
        if (ab is None) != (aw is None) or (ab is not None and (len(ab) != nb or len(aw) != k)):
            raise ValueError("block_project: ab and aw come together, as long as b and w")

        def ints(vs, which):
            return None if vs is None else (ctypes.c_int * len(vs))(*[v[which] for v in vs])
        c = np.zeros((nb, k)) if want_coeffs else None
        check(_lib.lib().mgcmt_block_project(self._h, level, nb, ints(b, 0), ints(b, 1), ints(ab, 0), ints(ab, 1), k, ints(w, 0), ints(w, 1),
                                             ints(aw, 0), ints(aw, 1), None if c is None else _lib.as_dp(c), stream))
        return c

    def block_orthonormalize(self, level, w, aw=None, drop_tol=1e-12, want_t=False, want_dropped=False, stream=None):
        """One Cholesky-QR step w <- w T and, with aw, aw <- aw T on <= 16 distinct vectors ((slot, vec) pairs;
        mgcmt_block_orthonormalize): T upper triangular with T^T (w^T w) T = I; a column whose pivot of the scaled Gram
        matrix is <= drop_tol comes back as exact zeros.  Returns None, T (want_t), the mask of dropped columns
        (want_dropped) or the pair; either one synchronises."""
        k = len(w)
        if aw is not None and len(aw) != k:
            raise ValueError("block_orthonormalize: aw as long as w")

        def ints(vs, which):
            return None if vs is None else (ctypes.c_int * len(vs))(*[v[which] for v in vs])
        t = np.zeros((k, k)) if want_t else None
        mask = ctypes.c_uint(0)
        check(_lib.lib().mgcmt_block_orthonormalize(self._h, level, k, ints(w, 0), ints(w, 1), ints(aw, 0), ints(aw, 1), c_double(drop_tol),
                                                    None if t is None else _lib.as_dp(t), ctypes.byref(mask) if want_dropped else None, stream))
        if want_t and want_dropped:
            return t, int(mask.value)
        return t if want_t else int(mask.value) if want_dropped else None

    def axpy(self, level, alpha, x, y, stream=None):
        check(_lib.lib().mgcmt_axpy(self._h, level, c_double(alpha), x[0], x[1], y[0], y[1], stream))

    def scale(self, level, alpha, v, stream=None):
        check(_lib.lib().mgcmt_scale(self._h, level, c_double(alpha), v[0], v[1], stream))

    def gramschmidt(self, level, slot, k, modified=1, stream=None):
        check(_lib.lib().mgcmt_gramschmidt(self._h, level, slot, k, 1 if modified else 0, stream))

    def normalize(self, level, slot, k, stream=None):
        check(_lib.lib().mgcmt_normalize(self._h, level, slot, k, stream))

    def fused_pass(self, level, kind, nsweep, omega=1.0, mode=0, k=1, stream=None):
        check(_lib.lib().mgcmt_fused_pass(self._h, level, kind, nsweep, c_double(omega), mode, k, stream))

    def fused_max_sweeps(self, level, kind):
        n = c_int(0)
        check(_lib.lib().mgcmt_fused_max_sweeps(self._h, level, kind, ctypes.byref(n)))
        return n.value

    def operator_kind(self, level):
        """One of _lib.OPK_*: how the library recognised the operator of `level` (decides the kernels it runs on)."""
        n = ctypes.c_int(0)
        check(_lib.lib().mgcmt_level_operator_kind(self._h, level, ctypes.byref(n)))
        return n.value

    def fused_max_recompute(self, level, kind, nsweep):
        n = c_int(0)
        check(_lib.lib().mgcmt_fused_max_recompute(self._h, level, kind, nsweep, ctypes.byref(n)))
        return n.value

    def set_option(self, option, value):
        check(_lib.lib().mgcmt_plan_set_option(self._h, option, int(value)))

    def carry_pending(self):
        """True while the last vcycle's carried right-hand side (OPT_CARRY) is waiting for an identical next cycle."""
        n = c_int(0)
        check(_lib.lib().mgcmt_carry_pending(self._h, ctypes.byref(n)))
        return bool(n.value)

    def bandwidth_probe(self, level, kind, blocks, reps, stream=None):
        ms = c_double(0.0)
        check(_lib.lib().mgcmt_bandwidth_probe(self._h, level, kind, blocks, reps, ctypes.byref(ms), stream))
        return ms.value

    def time_smoother(self, level, kind, nu, omega, reps, stream=None):
        ms = c_double(0.0)
        check(_lib.lib().mgcmt_time_smoother(self._h, level, kind, nu, c_double(omega), reps, ctypes.byref(ms), stream))
        return ms.value

    def time_fused_pass(self, level, kind, nsweep, omega, mode, reps, stream=None):
        """average milliseconds of one fused pass (mode as fused_pass) over `reps` launches, HIP events on the stream"""
        ms = c_double(0.0)
        check(_lib.lib().mgcmt_time_fused_pass(self._h, level, kind, nsweep, c_double(omega), mode, reps, ctypes.byref(ms), stream))
        return ms.value


# --------------------------------------------------------------------------------------------------
# plan cache: callers of the reference API pass the operator on every call
# --------------------------------------------------------------------------------------------------

_PLANS = OrderedDict()
_MAX_PLANS = 6


def _log2(x):
    return int(x).bit_length() - 1


def get_plan(op, lowest, nvec=1, mass=None):
    """A cached plan for (operator, coarsest size, mass operator) with room for at least nvec vectors."""
    key = (op.fingerprint(), int(lowest), None if mass is None else mass.fingerprint())
    plan = _PLANS.get(key)
    if plan is not None and plan.nvec >= nvec:
        _PLANS.move_to_end(key)
        return plan
    if plan is not None:
        plan.close()
        del _PLANS[key]
    plan = Plan(op, lowest, nvec=nvec, mass=mass)
    _PLANS[key] = plan
    while len(_PLANS) > _MAX_PLANS:
        _, old = _PLANS.popitem(last=False)
        old.close()
    return plan


def release_plans():
    """Free every cached device hierarchy."""
    while _PLANS:
        _, p = _PLANS.popitem()
        p.close()


def apply_operator(op, x):
    """A @ x on the GPU for a StructuredOperator (x: (n,), (n,1) or (n,k))."""
    x = np.asarray(x, dtype=np.float64)
    n = op.shape[0]
    cols = x.reshape(n, -1)
    # a single level is enough (3-D: the coarsest level may be at most 16^3; the levels below hold no vectors until used)
    plan = get_plan(op, op.g if op.dimension != "3d" else min(op.g, 16), nvec=1)
    out = np.empty_like(cols)
    for c in range(cols.shape[1]):
        plan.upload(0, SLOT_V, 0, cols[:, c])
        plan.apply(0, (SLOT_V, 0), (SLOT_T, 0))
        out[:, c] = plan.download(0, SLOT_T, 0)
    return out.reshape(x.shape)
