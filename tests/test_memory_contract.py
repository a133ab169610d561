"""Memory contract of the device code: where a kernel reads and writes, beyond "the interior it returns is right".

Three gaps of the rest of the suite (which creates a plan, runs one sequence, downloads interiors and closes the plan):
  * a store past a chunk end into a halo row, the next column, another slot or a scratch buffer that lands after the
    sequence's last read changes no downloaded number — it shows in a LATER call on the same plan (the plan cache of
    MGCMTSolver, drivers.block_eigensolve);
  * the emulator's hipMalloc is malloc: fresh large blocks are zero pages, so reliance on uninitialised device memory is
    invisible on the CPU half of every parity test;
  * "halo rows of a whole-grid plan are exact zeros" is stated in comments and checked nowhere.

The emulated runtime's guard mode (tests/hip_cpu_mock/hipmock_runtime.cpp: red zones round every hipMalloc block, payloads
that start as NaN, range checks of the host-initiated copies) closes them on the CPU; the two both-backend tests are their
GPU-visible form.  One case matrix (CASES) serves every test.

What MGCMT_OPT_RECOMPUTE means at these sizes: 1 (the default) lets a down leg skip its store on levels of at least 2^22
points only, so on every grid of this module it runs exactly the passes of 0; the no-store down pass (mode 2 | 8) and the
recomputing up pass (mode 1 | npre << 4) run with 2, which forces them on every fused level.  The policy cases therefore
run all three values with MGCMT_OPT_TAIL = 0 (every level above the coarsest runs its own row-streaming passes, the 9-point
Galerkin levels included) and with both fused smoothers: weighted Jacobi recomputes on every policy, the multicolour
sweeps on 5-point levels only (four-colour sweeps on a 9-point level have no recompute path: mgcmt_fused_max_recompute is
0 there).  test_policy_cases_reach_the_recompute_passes checks that reach; the no-store / recompute pair is also called
directly on an Op9c, an Op9cv and a 1-D level.

Exclusions from the matrix, with reasons (nothing is left out because it fails):
  * MGCMT_OPT_TAIL = 1 (the dense tail) on the emulator: forming its matrix takes 1024 workgroups of 1024 threads, minutes
    per plan (tests/conftest.py); the GPU backend runs it.
  * unsupported combinations.  Point-potential plans: no lexicographic smoothers, twogrid, Rayleigh-quotient entries or
    mass operator (MGCMT_ERR_UNSUPPORTED).  3-D plans: no lexicographic smoothers, twogrid, ritz_pair, rayleigh_residual,
    fused_pass (MGCMT_ERR_UNSUPPORTED), Rayleigh-quotient entries only with a mass operator.  Multicolour sweeps on 9-point
    levels: no recompute (above).  MGCMT_OPT_TWO_LEVEL applies to constant 5-point levels under weighted Jacobi only, and
    its passes are a no-store down pass and a recomputing up pass: with MGCMT_OPT_RECOMPUTE = 0 the cycle runs the
    single-level passes whatever MGCMT_OPT_TWO_LEVEL says (the policy cases with rec0 are that); with 1 and 2 the
    two-level passes run (one case with 1, two with 2).
  * the general-CSR plan is left out of test_halo_and_padding_stay_zero: it has its own five entries, one column, and every
    vector is a hipMalloc block of its own, n complex numbers with no halo rows, padding or unused columns, and there is
    no accessor to its storage — nothing lies beside a vector for that test to look at.  Its device arrays (vectors,
    indptr / indices / values of every level, none of them cleared after hipMalloc) are covered by the red zones and the
    NaN payload of test_guarded_csr_plan_and_solver_fmg alone, and by the reuse test.
  * row-strip (sharded) plans: their halos hold the neighbours' rows.
  * the emulated runtime checks a copy of kind hipMemcpyDefault on the sides that point into a live block; the library
    issues none today.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from multigridcmt_amd import _lib
from multigridcmt_amd.operators import (StructuredOperator, laplacian_operator, mehrstellen_mass, mehrstellen_operator,
                                        identity_operator, potential_operator, potential_well_operator, tri_identity, tri_laplacian)
from multigridcmt_amd.plan import Plan

V, F, T, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_T, _lib.SLOT_W
WJ, LEX, SOR, MC = _lib.WJACOBI, _lib.GS_LEX, _lib.SOR_LEX, _lib.GS_MC
SCALE = -1 / np.pi ** 2
DEFAULT_OPTIONS = {_lib.OPT_FUSED: 1, _lib.OPT_FUSED_ROWS: 0, _lib.OPT_RECOMPUTE: 1, _lib.OPT_TWO_LEVEL: 1, _lib.OPT_TAIL: 1,
                   _lib.OPT_LEX_WAVE: 1, _lib.OPT_LEX_CHAIN: 1, _lib.OPT_MGS_BLOCK: 1, _lib.OPT_GRAPH: 1}


# ---- the emulated runtime's guard mode -------------------------------------------------------------------------------

class Violation(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("side", ctypes.c_int), ("bytes", ctypes.c_ulonglong), ("offset", ctypes.c_longlong),
                ("seq", ctypes.c_ulonglong), ("length", ctypes.c_ulonglong)]

    def __repr__(self):
        return "Violation(kind=%d, side=%d, bytes=%d, offset=%d, seq=%d, length=%d)" % (self.kind, self.side, self.bytes, self.offset, self.seq, self.length)


RED_ZONE, RANGE, BAD_FREE = 1, 2, 3


class Guard:
    """ctypes handle on the guard functions of libmgcmt_emu.so (the library the `backend` fixture has bound)."""

    def __init__(self):
        self.lib = ctypes.CDLL(_lib.library_path())
        self.lib.hipmock_guard_take.argtypes = [ctypes.POINTER(Violation), ctypes.c_int]
        self.lib.hipmock_malloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.lib.hipmock_free.argtypes = [ctypes.c_void_p]
        self.lib.hipmock_memset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
        self.lib.hipmock_memcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def enable(self, on):
        self.lib.hipmock_guard_enable(1 if on else 0)

    def take(self):
        """check every live block, then return and clear all records"""
        self.lib.hipmock_guard_check_all()
        buf = (Violation * 64)()
        n = self.lib.hipmock_guard_take(buf, 64)
        return [buf[i] for i in range(min(n, 64))]

    def live(self):
        return self.lib.hipmock_guard_live_blocks()


@pytest.fixture
def guard(backend):
    if backend != "emu":
        pytest.skip("the guard mode lives in the emulated runtime (host memory); the GPU runs the two both-backend tests")
    from multigridcmt_amd import general, plan
    plan.release_plans()
    general.release_plans()
    g = Guard()
    g.enable(False)
    g.take()
    yield g
    g.enable(False)
    g.take()


# ---- steps: one entry-point call each, with the vectors it may write ----------------------------------------------------
# writes(plan) -> set of (level, slot, column): derived from include/mgcmt_hip.h (the comment of each entry; slot T is the
# scratch of the smoothers, cycles and residual_restrict — they exchange the roles of V and T —, slot W of rayleigh_residual)

class Step:
    def __init__(self, label, run, writes, cycle=False):
        self.label, self.run, self.writes = label, run, writes
        self.cycle = cycle      # a mgcmt_vcycle call: the GPU runs it three times (graph capture and replay)


def _cols(level_slots, k):
    return lambda p: {(l, s, q) for l, s in level_slots for q in range(k)}


def smooth(l, kind, nu, omega, k):
    return Step("smooth(l=%d,kind=%d,nu=%d,k=%d)" % (l, kind, nu, k), lambda p: p.smooth(l, kind, nu, omega, k=k), _cols([(l, V), (l, T)], k))


def vcycle(nu1, nu2, kind, omega, k, nuc=2, gs=False, level=0, zero_start=False):
    def run(p):
        p.vcycle(nu1, nu2, kind, omega=omega, k=k, nu_coarse=nuc, gram_schmidt=gs, level=level, zero_start=zero_start)

    def writes(p):
        return {(l, s, q) for l in range(level, p.num_levels) for s in ((V, T) if l == level else (V, F, T)) for q in range(k)}
    return Step("vcycle(%d,%d,kind=%d,k=%d,nuc=%d,gs=%d,level=%d,zero=%d)" % (nu1, nu2, kind, k, nuc, gs, level, zero_start), run, writes, cycle=True)


def twogrid(nu1, nu2, kind, omega, k, level=0):
    return Step("twogrid(kind=%d,level=%d)" % (kind, level), lambda p: p.twogrid(nu1, nu2, kind, omega=omega, k=k, level=level),
                _cols([(level, V), (level, T), (level + 1, V), (level + 1, F), (level + 1, T)], k))


def apply(l, src, dst, op=_lib.OP_A, with_shift=False):
    return Step("apply(l=%d,op=%d)" % (l, op), lambda p: p.apply(l, src, dst, op=op, with_shift=with_shift), lambda p: {(l,) + tuple(dst)})


def restrict(l, src, dst):
    return Step("restrict(l=%d)" % l, lambda p: p.restrict(l, src, dst), lambda p: {(l + 1,) + tuple(dst)})


def prolong(l, src, dst, accumulate):
    return Step("prolong(l=%d,acc=%d)" % (l, accumulate), lambda p: p.prolong(l, src, dst, accumulate=accumulate), lambda p: {(l,) + tuple(dst)})


def residual_restrict(l, k):
    return Step("residual_restrict(l=%d)" % l, lambda p: p.residual_restrict(l, k=k), _cols([(l, T), (l + 1, F), (l + 1, V)], k))


def prolong_correct(l, k):
    return Step("prolong_correct(l=%d)" % l, lambda p: p.prolong_correct(l, k=k), _cols([(l, V)], k))


def coarse_solve(k):
    return Step("coarse_solve", lambda p: p.coarse_solve(p.num_levels - 1, k=k), lambda p: {(p.num_levels - 1, V, q) for q in range(k)})


def fused_pass(l, kind, nsweep, omega, mode, k):
    ls = [(l, V), (l, T)] + ([(l + 1, F)] if (mode & 3) == 2 else [])
    return Step("fused_pass(l=%d,kind=%d,n=%d,mode=%d)" % (l, kind, nsweep, mode), lambda p: p.fused_pass(l, kind, nsweep, omega, mode=mode, k=k), _cols(ls, k))


def set_shifts(shifts):
    return Step("set_shifts", lambda p: p.set_shifts(shifts), lambda p: set())


def set_option(option, value):
    return Step("set_option(%d,%d)" % (option, value), lambda p: p.set_option(option, value), lambda p: set())


def rayleigh_residual(l, slot, k):
    return Step("rayleigh_residual", lambda p: np.concatenate(p.rayleigh_residual(l, slot, k)), _cols([(l, W)], k))


def ritz_pair(l, x, w, scratch):
    return Step("ritz_pair", lambda p: p.ritz_pair(l, x, w, scratch), lambda p: {(l,) + tuple(scratch)})


RQ_VECS = (0, 1, 2, 3, 4, 5)


def rqmin(l, slot, nu):
    return Step("rqmin(l=%d,nu=%d)" % (l, nu), lambda p: np.array([p.rqmin(l, slot, RQ_VECS, nu)]), lambda p: {(l, slot, q) for q in RQ_VECS})


def vcycle_rqmg(slot, nu1, nu2):
    return Step("vcycle_rqmg", lambda p: np.array([p.vcycle_rqmg(slot, RQ_VECS, nu1, nu2)]),
                lambda p: {(l, slot, q) for l in range(p.num_levels) for q in RQ_VECS})


def rq_line_step(l, x, w, x_out, g, work=None):
    out = [v for v in (x_out if w is not None else None, g, work) if v is not None]
    return Step("rq_line_step(w=%s)" % (w is not None), lambda p: p.rq_line_step(l, x, w, x_out, g, work=work), lambda p: {(l,) + tuple(v) for v in out})


def gram(l, vectors):
    return Step("gram", lambda p: p.gram(l, vectors), lambda p: set())


def block_gram(l, a, b):
    return Step("block_gram", lambda p: p.block_gram(l, a, b), lambda p: set())


def block_combine(l, inputs, outputs, coeffs):
    return Step("block_combine", lambda p: p.block_combine(l, inputs, outputs, coeffs), lambda p: {(l,) + tuple(v) for v in outputs})


def lincomb(l, terms, dst):
    return Step("lincomb", lambda p: p.lincomb(l, terms, dst), lambda p: {(l,) + tuple(dst)})


def gramschmidt(l, slot, k, modified=1):
    return Step("gramschmidt(k=%d,mod=%d)" % (k, modified), lambda p: p.gramschmidt(l, slot, k, modified=modified), _cols([(l, slot)], k))


def normalize(l, slot, k):
    return Step("normalize", lambda p: p.normalize(l, slot, k), _cols([(l, slot)], k))


# ---- operators ------------------------------------------------------------------------------------------------------------

def _lap1d(g):
    return laplacian_operator(g, "1d") * SCALE


def _var1d(g):
    t = tri_laplacian(g) * SCALE
    t[1] += 3.0 * np.random.RandomState(3).rand(g)
    return StructuredOperator("1d", g, [(None, t)])


def _lap2d(g):
    return laplacian_operator(g, "2d") * SCALE


def _well(g):
    return potential_well_operator(g, 20.0, (g // 4, 3 * g // 4))


def _separable(g, three_terms):
    rng = np.random.RandomState(11)
    Lx, Ly = tri_laplacian(g) * SCALE, tri_laplacian(g) * SCALE
    Lx[1] += 3.0 * rng.rand(g)
    Ly[1] += 3.0 * rng.rand(g)
    terms = [(tri_identity(g), Ly), (Lx, tri_identity(g))]
    if three_terms:
        dp, dq = np.zeros((3, g)), np.zeros((3, g))
        dp[1], dq[1] = 1.0 + 4.0 * rng.rand(g), 0.5 + 6.0 * rng.rand(g)
        terms.append((dp, dq))
    return StructuredOperator("2d", g, terms)


def _point(g):
    return potential_operator(g, 5.0 * np.random.RandomState(17).rand(g, g))


def _lap3d(g):
    return laplacian_operator(g, "3d") * SCALE


# ---- the case matrix ------------------------------------------------------------------------------------------------------
# A case: operator (and mass operator), plan arguments, options, the number of active columns k (< nvec: columns k.. are
# unused), the levels whose V and F start as random numbers, a call sequence and the vectors downloaded at its end (only
# what the header documents as results: the iterates of the coarser levels are scratch).

class Case:
    def __init__(self, name, op, g, lowest, nvec, k, steps, downloads, mass=None, options=None, init_levels=(0,), shifts=None):
        self.name, self.make_op, self.g, self.lowest, self.nvec, self.k = name, op, g, lowest, nvec, k
        self.steps, self.downloads, self.make_mass = steps, downloads, mass
        self.options = dict(options or {})
        self.init_levels = init_levels
        self.shifts = 0.2 + 0.5 * np.arange(k) if shifts is None else np.asarray(shifts, dtype=float)

    def plan(self):
        return Plan(self.make_op(self.g), self.lowest, nvec=self.nvec, mass=self.make_mass(self.g) if self.make_mass else None)

    def options_on(self, backend):
        o = dict(DEFAULT_OPTIONS)
        o[_lib.OPT_TAIL] = 2 if backend == "emu" else 1     # the emulator keeps the dense tail off (conftest); the GPU's default is the dense tail
        o.update(self.options)
        return o

    def start(self, p, backend):
        """options, shifts and the start vectors: everything a run of the steps depends on"""
        for o, val in self.options_on(backend).items():
            p.set_option(o, val)
        p.set_shifts(self.shifts)
        rng = np.random.RandomState(1000 + len(self.name))
        for l in self.init_levels:
            for s in (V, F):
                for q in range(self.k):
                    p.upload(l, s, q, rng.rand(p.size(l)))

    def run(self, p, after_step=None, cycle_repeats=1):
        outs = []
        for st in self.steps:
            r = st.run(p)
            for _ in range(cycle_repeats - 1 if st.cycle else 0):
                st.run(p)
            if r is not None:
                outs.append((st.label, np.array(r, dtype=float)))
            if after_step:
                after_step(st)
        for l, s, q in self.downloads:
            outs.append(("download(%d,%d,%d)" % (l, s, q), np.array(p.download(l, s, q))))
        return outs


def _vk(k, level=0, slots=(V,)):
    return [(level, s, q) for s in slots for q in range(k)]


def _cycle_case(name, op, g, lowest, kind, omega, k, options, nvec=None, zero_start=False, mass=None, nu=(2, 2, 2), gs=False, extra=()):
    steps = [vcycle(nu[0], nu[1], kind, omega, k, nuc=nu[2], gs=gs, zero_start=zero_start)] + list(extra)
    return Case(name, op, g, lowest, nvec or k + 1, k, steps, _vk(k) + _vk(k, 1, (F,)), mass=mass, options=options)


CASES = []
# every fused policy x MGCMT_OPT_RECOMPUTE 0 / 1 / 2 with a short chunk (MGCMT_OPT_FUSED_ROWS = 6) and without the tail, so
# that every level above the coarsest runs its own passes: Op5 / Op9c (Laplacian), Op5-diag / Op9cv (well), Op9<2>, Op9<3>,
# Op9m3 (Mehrstellen), Op5P / the pointwise levels (point potential).  Both fused smoothers, one cycle each: weighted
# Jacobi (with rec2: no-store and recompute passes on every level) and multicolour (with rec2: on the 5-point levels).
_POLICIES = [("op5", _lap2d, None), ("well", _well, None), ("sep2", lambda g: _separable(g, False), None),
             ("sep3", lambda g: _separable(g, True), None), ("mehr", mehrstellen_operator, mehrstellen_mass), ("point", _point, None)]
for pname, pop, pmass in _POLICIES:
    for rec in (0, 1, 2):
        k = 3 if rec == 2 else 1
        CASES.append(Case("%s_rec%d_rows6" % (pname, rec), pop, 64, 8 if rec else 2, k + 1, k,
                          [vcycle(2, 2, WJ, 2. / 3., k, nuc=2, zero_start=rec == 2), vcycle(2, 2, MC, 1.15, k, nuc=2)],
                          _vk(k) + _vk(k, 1, (F,)), mass=pmass, options={_lib.OPT_RECOMPUTE: rec, _lib.OPT_FUSED_ROWS: 6, _lib.OPT_TAIL: 0}))


def _no_store_pieces(name, op):
    """the no-store down pass and the recomputing up pass of level 1 (32 x 32, a 9-point Galerkin level) called directly, with
    6-row chunks, from a stored and from a "zero, uncleared" iterate"""
    w = 2. / 3.
    return Case(name, op, 64, 8, 4, 3,
                [fused_pass(1, WJ, 2, w, 2 | 8, 3), smooth(2, WJ, 2, w, 3), fused_pass(1, WJ, 2, w, 1 | (2 << 4), 3),
                 fused_pass(1, WJ, 1, w, 2 | 8 | 4, 3), smooth(2, MC, 1, 1.0, 3), fused_pass(1, WJ, 2, w, 1 | 4 | (1 << 4), 3)],
                _vk(3, 1) + _vk(3, 2, (F,)), options={_lib.OPT_FUSED_ROWS: 6}, init_levels=(1, 2))


CASES += [
    # 1-D: Laplacian and variable tridiagonal; all four smoother kinds, the pieces of a cycle one by one, twogrid
    Case("lap1d_pieces", _lap1d, 256, 8, 4, 3,
         [smooth(0, WJ, 2, 2. / 3., 3), smooth(0, MC, 2, 1.0, 3), smooth(0, LEX, 2, 1.0, 3), smooth(0, SOR, 2, 1.2, 3),
          residual_restrict(0, 3), vcycle(1, 1, WJ, 2. / 3., 3, level=1), prolong_correct(0, 3), twogrid(1, 2, MC, 1.0, 3),
          fused_pass(0, WJ, 2, 2. / 3., 0, 3), fused_pass(0, MC, 1, 1.0, 2, 3), set_shifts([0.1, 0.3, 0.6]), vcycle(2, 2, MC, 1.0, 3, nuc=2)],
         _vk(3) + _vk(3, 1, (F,))),
    Case("var1d_cycle_unfused", _var1d, 64, 2, 2, 1,
         [smooth(0, SOR, 1, 1.3, 1), vcycle(2, 1, LEX, 1.0, 1, nuc=1), vcycle(1, 2, WJ, 0.8, 1, nuc=3, zero_start=True)], _vk(1),
         options={_lib.OPT_FUSED: 0}),
    Case("lap1d_16_fused", _lap1d, 16, 2, 4, 3, [vcycle(2, 2, WJ, 2. / 3., 3, gs=True), gramschmidt(0, V, 3, 0)], _vk(3)),
    # 1-D no-store and recompute passes (kernels_fused1d.hip): in the cycle (MGCMT_OPT_RECOMPUTE = 2) and called directly
    Case("lap1d_rec2_256", _lap1d, 256, 8, 4, 3,
         [vcycle(2, 2, WJ, 2. / 3., 3, zero_start=True), vcycle(2, 2, MC, 1.0, 3), fused_pass(0, WJ, 2, 2. / 3., 2 | 8, 3),
          fused_pass(0, WJ, 2, 2. / 3., 1 | (2 << 4), 3), fused_pass(0, MC, 1, 1.0, 2 | 8, 3), fused_pass(0, MC, 1, 1.0, 1 | (1 << 4), 3)],
         _vk(3) + _vk(3, 1, (F,)), options={_lib.OPT_RECOMPUTE: 2}),
    Case("var1d_rec2_64", _var1d, 64, 2, 2, 1, [vcycle(2, 2, MC, 1.0, 1), vcycle(3, 2, WJ, 0.8, 1, zero_start=True)], _vk(1),
         options={_lib.OPT_RECOMPUTE: 2}),
    # the same pair on a constant (Op9c) and a variable (Op9cv) 9-point Galerkin level
    _no_store_pieces("op9c_no_store_rows6", _lap2d),
    _no_store_pieces("op9cv_no_store_rows6", _well),
    # 2-D constant Laplacian: the entry points one by one, transfers between named vectors, apply with and without shift
    Case("op5_pieces", _lap2d, 64, 8, 4, 3,
         [apply(0, (V, 0), (T, 1), with_shift=True), apply(0, (V, 1), (W, 0)), restrict(0, (F, 1), (T, 0)), prolong(0, (T, 0), (W, 1), False),
          prolong(0, (T, 0), (W, 1), True), residual_restrict(0, 3), smooth(1, MC, 2, 1.1, 3), residual_restrict(1, 3),
          residual_restrict(2, 3), coarse_solve(3), prolong_correct(2, 3), prolong_correct(1, 3), prolong_correct(0, 3),
          fused_pass(0, WJ, 2, 2. / 3., 2 | 8, 3), fused_pass(0, WJ, 2, 2. / 3., 1 | (2 << 4), 3), fused_pass(0, MC, 1, 1.0, 4, 3),
          fused_pass(1, MC, 1, 1.0, 2 | 4, 3), fused_pass(1, WJ, 1, 0.8, 1, 3), twogrid(2, 2, WJ, 2. / 3., 3, level=1),
          lincomb(0, [(0.5, (V, 0)), (-2.0, (F, 1))], (W, 2)), block_combine(0, [(V, 0), (V, 1), (F, 2)], [(W, 0), (V, 1)], np.arange(6.0) - 2),
          gram(0, [(V, 0), (W, 2), (F, 1)]), block_gram(0, [(V, 0), (V, 1), (V, 2)], [(F, 0), (W, 1)]), normalize(0, W, 3)],
         _vk(3, 0, (V, W)) + _vk(3, 1, (V, F)), init_levels=(0, 1)),
    # lexicographic sweeps: wave pipeline (chained and not), band wavefront, one workgroup; one wave wide and several blocks wide
    Case("op5_lex_64", _lap2d, 64, 8, 2, 1,
         [smooth(0, LEX, 2, 1.0, 1), set_option(_lib.OPT_LEX_CHAIN, 0), smooth(0, SOR, 2, 1.2, 1), set_option(_lib.OPT_LEX_WAVE, 2),
          smooth(0, LEX, 1, 1.0, 1), smooth(0, SOR, 1, 1.1, 1), set_option(_lib.OPT_LEX_WAVE, 0), smooth(0, LEX, 1, 1.0, 1),
          set_option(_lib.OPT_LEX_WAVE, 1), vcycle(1, 1, LEX, 1.0, 1, nuc=1)], _vk(1)),
    Case("op5_lex_256_k3", _lap2d, 256, 8, 4, 3, [smooth(0, LEX, 1, 1.0, 3), set_option(_lib.OPT_LEX_WAVE, 2), smooth(0, SOR, 1, 1.2, 3)], _vk(3)),
    # two-level passes (MGCMT_OPT_TWO_LEVEL = 2) with chunks of 6, 22 and automatic rows; several column blocks wide
    _cycle_case("op5_two_level_256_rows22", _lap2d, 256, 8, WJ, 2. / 3., 1, {_lib.OPT_TWO_LEVEL: 2, _lib.OPT_RECOMPUTE: 2, _lib.OPT_FUSED_ROWS: 22}, nvec=2),
    _cycle_case("op5_two_level_128_rows6_k3", _lap2d, 128, 2, WJ, 2. / 3., 3, {_lib.OPT_TWO_LEVEL: 2, _lib.OPT_RECOMPUTE: 2, _lib.OPT_FUSED_ROWS: 6},
                zero_start=True, nu=(3, 2, 2), extra=[set_shifts([0.9, 0.1, 0.4]), vcycle(3, 2, WJ, 2. / 3., 3, nuc=2)]),
    _cycle_case("op5_two_level_rec1_128", _lap2d, 128, 8, WJ, 2. / 3., 1, {_lib.OPT_TWO_LEVEL: 2, _lib.OPT_RECOMPUTE: 1}, nvec=2),
    _cycle_case("op5_two_level_off_128", _lap2d, 128, 8, WJ, 2. / 3., 1, {_lib.OPT_TWO_LEVEL: 0, _lib.OPT_RECOMPUTE: 2}, nvec=2),
    # narrower than a wave; Gram-Schmidt inside the cycle, blocked and column by column; the tail off
    _cycle_case("op5_16_gs", _lap2d, 16, 2, MC, 1.0, 3, {_lib.OPT_TAIL: 0}, gs=True),
    Case("op5_128_mgs_forms", _lap2d, 128, 8, 4, 3,
         [gramschmidt(0, V, 3), set_option(_lib.OPT_MGS_BLOCK, 0), gramschmidt(0, F, 3), gramschmidt(0, V, 2, 0),
          vcycle(1, 1, WJ, 2. / 3., 3, nuc=1, gs=True), vcycle(1, 1, WJ, 2. / 3., 3, nuc=1, level=1)], _vk(3, 0, (V, F))),
    _cycle_case("well_unfused_k3", _well, 64, 8, MC, 1.0, 3, {_lib.OPT_FUSED: 0}, zero_start=True),
    # Rayleigh-quotient entries: 1-D, square well, Mehrstellen with its mass operator
    Case("well_rq", _well, 32, 2, 7, 2,
         [rayleigh_residual(0, V, 2), ritz_pair(0, (V, 0), (F, 1), (T, 3)), rqmin(0, V, 3), vcycle_rqmg(V, 2, 2),
          rq_line_step(0, (V, 0), None, None, (T, 0)), rq_line_step(0, (V, 0), (F, 0), (T, 1), (T, 0))], _vk(1) + [(0, T, 0), (0, T, 1)]),
    Case("lap1d_rq", _lap1d, 64, 2, 7, 2, [rqmin(0, V, 2), vcycle_rqmg(V, 1, 2), rayleigh_residual(0, V, 2)], _vk(1)),
    Case("mehr_rq_mass", mehrstellen_operator, 32, 4, 7, 2,
         [apply(0, (V, 0), (T, 6), op=_lib.OP_M), vcycle_rqmg(V, 2, 1), rqmin(1, V, 2), ritz_pair(0, (V, 0), (F, 0), (W, 0)),
          rq_line_step(0, (V, 0), (F, 0), (T, 1), (T, 0), work=(T, 2))], _vk(1) + [(0, T, 6), (0, T, 1)], mass=mehrstellen_mass, init_levels=(0, 1)),
    # point potential: the kernels_pointwise levels one by one
    Case("point_pieces", _point, 32, 4, 4, 3,
         [apply(0, (V, 0), (T, 1), with_shift=True), apply(1, (V, 1), (T, 0)), smooth(1, WJ, 2, 2. / 3., 3), smooth(1, MC, 1, 1.0, 3),
          residual_restrict(1, 3), prolong_correct(1, 3), fused_pass(0, WJ, 2, 2. / 3., 2, 3), vcycle(2, 2, MC, 1.0, 3, nuc=2, level=1),
          vcycle(2, 2, WJ, 2. / 3., 3, nuc=2, gs=True)], _vk(3) + [(0, T, 1), (1, T, 0)] + _vk(3, 1), init_levels=(0, 1)),
    # 3-D, without and with a mass operator
    Case("lap3d_16", _lap3d, 16, 4, 3, 2,
         [smooth(0, WJ, 2, 2. / 3., 2), smooth(0, MC, 1, 1.0, 2), apply(0, (V, 0), (T, 1)), restrict(0, (F, 0), (T, 0)), prolong(0, (T, 0), (W, 0), True),
          vcycle(2, 2, WJ, 2. / 3., 2, nuc=2), vcycle(1, 1, MC, 1.0, 2, nuc=1, gs=True, zero_start=True)], _vk(2) + _vk(2, 1, (F,))),
    Case("well3d_mass_rq", lambda g: potential_well_operator(g, 20.0, (g // 4, 3 * g // 4), dimension="3d"), 8, 2, 7, 1,
         [apply(0, (V, 0), (T, 6), op=_lib.OP_M), rqmin(0, V, 2), vcycle_rqmg(V, 1, 1), vcycle(1, 1, MC, 1.0, 1, nuc=1)],
         _vk(1) + [(0, T, 6)], mass=lambda g: identity_operator(g, "3d")),
]
CASE_IDS = [c.name for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


# ---- the general-CSR plan (csrc/csr.hip): its own small interface -----------------------------------------------------------

def _csr_matrix(n=128):
    rng = np.random.RandomState(5)
    bands = [rng.rand(n - abs(o)) + 1j * rng.rand(n - abs(o)) for o in (-2, -1, 1, 2)]
    A = sp.diags(bands, [-2, -1, 1, 2]) + sp.diags(6.0 + rng.rand(n) + 0.3j * rng.rand(n))
    return sp.csr_matrix(A)


def _csr_run(plan, after_step=None):
    rng = np.random.RandomState(6)
    n = plan.n
    outs = []
    for label, call in (("smooth_wj", lambda: plan.smooth(0, WJ, 2, 2. / 3., shift=0.3)), ("smooth_gs", lambda: plan.smooth(0, LEX, 2, 1.0, shift=0.3)),
                        ("smooth_sor", lambda: plan.smooth(0, SOR, 1, 1.2)), ("apply", lambda: plan.apply(0, V, T, shift=0.1)),
                        ("vcycle_gs", lambda: plan.vcycle(2, 2, LEX, shift=0.3)), ("vcycle_wj", lambda: plan.vcycle(1, 2, WJ, omega=0.7, nu_coarse=2))):
        if label in ("smooth_wj", "vcycle_gs"):
            plan.upload(0, V, rng.rand(n) + 1j * rng.rand(n))
            plan.upload(0, F, rng.rand(n) - 1j * rng.rand(n))
        call()
        if after_step:
            after_step(label)
        outs.append((label, plan.download(0, T if label == "apply" else V).view(np.float64).copy()))
    return outs


# ---- tests ----------------------------------------------------------------------------------------------------------------

def _same(a, b, what):
    assert len(a) == len(b)
    for (la, xa), (lb, xb) in zip(a, b):
        assert la == lb
        assert np.array_equal(xa, xb), "%s: %s differs (max |diff| %r)" % (what, la, np.abs(xa - xb).max())


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_guarded_run_is_clean_and_bit_identical(guard, case):
    """Every case with the guard off and on (the plan created after the switch: all of its memory is guarded).  No red
    zone is touched, no host-initiated copy leaves its block — checked after every entry-point call and after close() —,
    every result is finite and equal, bit for bit, to the unguarded run's: a kernel that reads what nothing wrote reads
    NaN under the guard and zero pages without it (a NaN that reaches a result through a product with zero counts)."""
    runs = []
    for on in (False, True):
        guard.enable(on)
        p = case.plan()
        try:
            case.start(p, "emu")
            assert guard.take() == []

            def after(st):
                bad = guard.take()
                assert bad == [], "%s after %s: %r" % (case.name, st.label, bad)
            runs.append(case.run(p, after))
        finally:
            p.close()
        assert guard.take() == [], "violations found when the plan was destroyed"
        assert guard.live() == 0, "the destroyed plan left device blocks behind"
    for label, x in runs[1]:
        assert np.all(np.isfinite(x)), "%s: %s is not finite under the guard" % (case.name, label)
    _same(runs[0], runs[1], case.name + " guard off / on")


def test_guarded_csr_plan_and_solver_fmg(guard):
    """The same for the general-CSR plan and for fmg through the drop-in solver class (whose plan comes from the cache)."""
    from multigridcmt_amd import MGCMTSolver, MGCMTStencilMaker, general, plan
    from multigridcmt_amd.general import CsrPlan
    A = _csr_matrix()
    g = 32
    H = _lap2d(g)
    f = np.random.RandomState(9).rand(g * g)
    runs = []
    for on in (False, True):
        guard.enable(on)
        p = CsrPlan(A, 32)
        try:
            def after(label):
                bad = guard.take()
                assert bad == [], "csr after %s: %r" % (label, bad)
            outs = _csr_run(p, after)
        finally:
            p.close()
        solver, sm = MGCMTSolver(), MGCMTStencilMaker()
        x = solver.fmg(f.copy(), H, sm, nu1=2, nu2=2, shift=0.4, lowest_level=4, dimension="2d")
        outs.append(("fmg", np.array(x, dtype=float)))
        assert guard.take() == [], "fmg"
        plan.release_plans()
        general.release_plans()
        assert guard.take() == [] and guard.live() == 0
        runs.append(outs)
    for label, x in runs[1]:
        assert np.all(np.isfinite(x)), label
    _same(runs[0], runs[1], "csr / fmg guard off / on")


class _Raw:
    """The raw storage of every slot, level and column of a plan through mgcmt_vec_ptr / mgcmt_plan_level_halo /
    mgcmt_plan_level_shape (emulator: the pointers are host memory).  The smoothers and cycles exchange the roles of V and T
    of a level, so the two are followed as BUFFERS: buffer V (T) is the allocation that was slot V (T) when the plan was
    new, and mgcmt_vec_ptr tells which slot it is now."""

    def __init__(self, p):
        self.p = p
        self.geom, self.first = [], []
        for l in range(p.num_levels):
            nr, gc, _ = p.level_shape(l)
            halo = p.level_halo(l)[0]
            # the column pitch: vec_ptr(.., 1) - vec_ptr(.., 0) in doubles
            stride = (p.vec_ptr(l, V, 1) - p.vec_ptr(l, V, 0)) // 8
            assert stride >= (nr + 2 * halo) * gc
            self.geom.append((nr, gc, halo, stride))
            self.first.append({V: p.vec_ptr(l, V, 0), T: p.vec_ptr(l, T, 0)})

    def swapped(self):
        """per level: slot V is buffer T now"""
        out = []
        for l, first in enumerate(self.first):
            now = {V: self.p.vec_ptr(l, V, 0), T: self.p.vec_ptr(l, T, 0)}
            assert now == first or now == {V: first[T], T: first[V]}, "level %d: V / T point at neither of their two buffers" % l
            out.append(now != first)
        return out

    def view(self, l, slot):
        """[nvec, stride] array over the whole allocation of (l, slot): halo rows, interior, halo rows, padding per column"""
        nr, gc, halo, stride = self.geom[l]
        base = self.p.vec_ptr(l, slot, 0) - 8 * halo * gc
        return np.ctypeslib.as_array((ctypes.c_double * (stride * self.p.nvec)).from_address(base)).reshape(self.p.nvec, stride)

    def interiors(self):
        """{(level, buffer): copy of the interiors of all columns}; buffer = slot for F and W"""
        out, swapped = {}, self.swapped()
        for l, (nr, gc, halo, stride) in enumerate(self.geom):
            for s in (V, F, T, W):
                b = V + T - s if s in (V, T) and swapped[l] else s
                out[(l, b)] = self.view(l, s)[:, halo * gc:(halo + nr) * gc].copy()
        return out

    def outside_interior_is_zero(self, what):
        for l, (nr, gc, halo, stride) in enumerate(self.geom):
            for s in (V, F, T, W):
                a = self.view(l, s).view(np.uint64)
                for name, part in (("halo rows above", a[:, :halo * gc]), ("halo rows below / padding", a[:, (halo + nr) * gc:])):
                    if part.any():
                        q, i = np.argwhere(part)[0]
                        raise AssertionError("%s: %s of level %d slot %d column %d are not zero (element %d of %d)" % (what, name, l, s, q, i, part.shape[1]))


def _marker(p, l, s, q):
    return np.random.RandomState(7000 + 97 * l + 13 * s + q).rand(p.size(l)) + 1.0


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_halo_and_padding_stay_zero(guard, case):
    """After every entry-point call: the halo rows (3-D: planes) above and below every vector and the padding up to the next
    column are exact zeros in every slot of every level; the columns q >= k still hold the markers uploaded before (a marker
    of its own per level, slot and column; V and T followed through their exchange as buffers); the vectors the entry does
    not write (include/mgcmt_hip.h) are bitwise unchanged."""
    guard.enable(True)
    p = case.plan()
    try:
        raw = _Raw(p)       # (mgcmt_vec_ptr allocates: every slot of every level exists from here on)
        for l in range(p.num_levels):
            for s in (V, F, T, W):
                for q in range(p.nvec):
                    p.upload(l, s, q, _marker(p, l, s, q))
        assert not any(raw.swapped())
        case.start(p, "emu")
        raw.outside_interior_is_zero(case.name + " after the uploads")
        state = {"before": raw.interiors(), "swapped": raw.swapped(), "named": set()}

        def after(st):
            what = "%s after %s" % (case.name, st.label)
            raw.outside_interior_is_zero(what)
            now, before, swapped = raw.interiors(), state["before"], raw.swapped()
            # the buffers behind the vectors the entry may write: a V or T it names is the buffer that held the slot
            # before the call or the one that holds it now
            written = set()
            for l, s, q in st.writes(p):
                for sw in (state["swapped"][l], swapped[l]):
                    written.add((l, V + T - s if s in (V, T) and sw else s, q))
            state["named"] |= written
            for l in range(p.num_levels):
                for b in (V, F, T, W):
                    for q in range(p.nvec):
                        if (l, b, q) not in written:
                            assert np.array_equal(now[(l, b)][q], before[(l, b)][q]), "%s: level %d buffer %d column %d changed" % (what, l, b, q)
                        if q >= case.k and (l, b, q) not in state["named"]:
                            assert np.array_equal(now[(l, b)][q], _marker(p, l, b, q)), "%s: marker of level %d buffer %d column %d lost" % (what, l, b, q)
            assert guard.take() == [], what
            state["before"], state["swapped"] = now, swapped
        case.run(p, after)
    finally:
        p.close()
    assert guard.take() == []


@pytest.mark.parametrize("pname", [n for n, _, _ in _POLICIES])
def test_policy_cases_reach_the_recompute_passes(backend, pname):
    """The rec2 policy cases do run what they are there for: with the options of the case, every level the cycle smooths
    with a fused pass can recompute the two pre-smoothing sweeps of the weighted-Jacobi cycle (so MGCMT_OPT_RECOMPUTE = 2
    makes its down pass a no-store pass and its up pass a recomputing one), no tail takes the coarse levels away, and the
    multicolour cycle recomputes exactly where the operator is a 5-point one."""
    case = CASES[CASE_IDS.index(pname + "_rec2_rows6")]
    assert case.options[_lib.OPT_RECOMPUTE] == 2 and case.options[_lib.OPT_TAIL] == 0 and case.options[_lib.OPT_FUSED_ROWS] == 6
    five = (_lib.OPK_FIVE_POINT, _lib.OPK_FIVE_DIAG, _lib.OPK_POINT_DIAG)
    p = case.plan()
    try:
        case.start(p, backend)
        fused = [l for l in range(p.num_levels - 1) if p.fused_max_sweeps(l, WJ) > 0]
        # (the coarse levels of a point potential run the kernels of kernels_pointwise.hip, one launch per operation: only
        # its level 0 has fused passes)
        assert fused[:2] == ([0] if pname == "point" else [0, 1]), "level 0 and its Galerkin level run fused passes"
        for l in fused:
            assert p.fused_max_sweeps(l, WJ) >= 2 and p.fused_max_recompute(l, WJ, 2) >= 2, "level %d" % l
            assert (p.fused_max_recompute(l, MC, 2) >= 2) == (p.operator_kind(l) in five), "level %d" % l
        assert pname == "point" or p.operator_kind(1) not in five, "the Galerkin level is a 9-point level"
    finally:
        p.close()


def test_policy_cases_cover_every_operator_kind(backend):
    kinds = set()
    for pname, _, _ in _POLICIES:
        p = CASES[CASE_IDS.index(pname + "_rec2_rows6")].plan()
        try:
            kinds |= {p.operator_kind(l) for l in range(p.num_levels - 1)}
        finally:
            p.close()
    assert kinds >= {_lib.OPK_GENERAL, _lib.OPK_FIVE_POINT, _lib.OPK_FIVE_DIAG, _lib.OPK_NINE_CONST, _lib.OPK_NINE_VAR,
                     _lib.OPK_POINT_DIAG, _lib.OPK_NINE_POINT}, kinds
    for name, kind in (("op9c_no_store_rows6", _lib.OPK_NINE_CONST), ("op9cv_no_store_rows6", _lib.OPK_NINE_VAR)):
        p = CASES[CASE_IDS.index(name)].plan()
        try:
            assert p.operator_kind(1) == kind
        finally:
            p.close()


# the mixed sequence that uses a plan before a case runs on it: other smoothers, other k, other options, a lexicographic
# sweep, a Rayleigh-quotient call and a Gram-Schmidt where the plan supports them
def _pollute(p, case):
    rng = np.random.RandomState(77)
    point = getattr(p.op, "point_diagonal", None) is not None
    nv = p.nvec
    for l in range(min(2, p.num_levels)):
        for s in (V, F, T, W):
            for q in range(nv):
                p.upload(l, s, q, rng.rand(p.size(l)) - 0.5)
    p.set_shifts(0.05 + 0.3 * np.arange(nv))
    for o, val in ((_lib.OPT_FUSED_ROWS, 6), (_lib.OPT_RECOMPUTE, 2), (_lib.OPT_TWO_LEVEL, 2), (_lib.OPT_TAIL, 0), (_lib.OPT_MGS_BLOCK, 0)):
        p.set_option(o, val)
    p.smooth(0, WJ, 3, 0.7, k=nv)
    p.smooth(0, MC, 2, 1.05, k=nv)
    p.vcycle(2, 2, WJ, omega=2. / 3., k=nv, nu_coarse=2)
    p.vcycle(1, 3, MC, omega=1.0, k=nv, nu_coarse=1, gram_schmidt=True)
    if p.num_levels > 2:
        p.vcycle(2, 1, WJ, omega=0.8, k=1, nu_coarse=2, level=1)
    p.set_option(_lib.OPT_FUSED, 0)
    p.vcycle(1, 1, MC, omega=1.0, k=nv, nu_coarse=3, zero_start=True)
    p.set_option(_lib.OPT_FUSED, 1)
    p.set_option(_lib.OPT_TAIL, 2)
    p.vcycle(2, 2, MC, omega=1.0, k=1, nu_coarse=2)
    if p.dim != 3 and not point:
        p.smooth(0, LEX, 1, 1.0, k=nv)
        p.set_option(_lib.OPT_LEX_WAVE, 2)
        p.smooth(0, SOR, 1, 1.2, k=1)
        p.rayleigh_residual(0, V, nv)
        if p.num_levels > 1:
            p.twogrid(1, 1, WJ, omega=2. / 3., k=nv)
    if nv >= 6 and not point and (p.dim != 3 or p.mass is not None):
        p.rqmin(0, V, RQ_VECS, 2)
        p.vcycle_rqmg(V, RQ_VECS, 1, 1)
    p.gramschmidt(0, V, nv)
    p.gramschmidt(0, F, nv, modified=0)
    p.normalize(0, T, nv)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_reused_plan_equals_fresh_plan(backend, case):
    """A case on a plan that has run a long mixed sequence first (then: options restored, V and F uploaded again) gives the
    bits of the same case on a fresh plan — a polluted halo, stale scratch, a stale tail matrix, a stale coarse
    factorisation or a stale captured graph changes them.  On the GPU every cycle of a case is called three times (graph
    replay from the second call on, as test_fuzz does)."""
    outs = []
    for reuse in (False, True):
        p = case.plan()
        try:
            if reuse:
                _pollute(p, case)
            case.start(p, backend)
            outs.append(case.run(p, cycle_repeats=3 if backend == "hip" else 1))
        finally:
            p.close()
    _same(outs[0], outs[1], case.name + " fresh / reused plan")


def test_reused_csr_plan_equals_fresh_plan(backend):
    from multigridcmt_amd.general import CsrPlan
    A = _csr_matrix()
    outs = []
    for reuse in (False, True):
        p = CsrPlan(A, 32)
        try:
            if reuse:
                rng = np.random.RandomState(8)
                p.upload(0, V, rng.rand(p.n))
                p.upload(0, F, rng.rand(p.n) * 1j)
                p.vcycle(3, 1, SOR, omega=1.1, shift=0.9, nu_coarse=1)
                p.smooth(0, WJ, 3, 0.5, shift=-0.2)
                p.apply(0, V, T, shift=2.0)
            outs.append(_csr_run(p))
        finally:
            p.close()
    _same(outs[0], outs[1], "csr fresh / reused plan")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_apply_of_zero_interior_is_zero(backend, case):
    """After the mixed sequence the interior of V is set to zero by upload (mgcmt_zero would clear the halos too): A v, M v
    and one Jacobi sweep with F = 0 are then exactly zero on every level — a non-zero halo row shows in the first or last
    row."""
    p = case.plan()
    try:
        _pollute(p, case)
        case.start(p, backend)
        k = case.k
        for l in range(p.num_levels):
            z = np.zeros(p.size(l))
            for q in range(k):
                p.upload(l, V, q, z)
                p.upload(l, F, q, z)
            ops = [_lib.OP_A] + ([_lib.OP_M] if p.mass is not None else [])
            for op in ops:
                for q in range(k):
                    for with_shift in (False, True):
                        p.apply(l, (V, q), (W, q), op=op, with_shift=with_shift)
                        out = p.download(l, W, q)
                        assert not out.any(), "%s: apply(op=%d, shift=%d) of a zero vector on level %d, column %d: rows %r" % (
                            case.name, op, with_shift, l, q, np.unique(np.nonzero(out)[0] // p.level_shape(l)[1])[:8])
            p.smooth(l, WJ, 1, 2. / 3., k=k)
            for q in range(k):
                out = p.download(l, V, q)
                assert not out.any(), "%s: a Jacobi sweep from zero with F = 0 on level %d, column %d" % (case.name, l, q)
    finally:
        p.close()


def test_guard_mode_detects_planted_errors(guard):
    """The guard itself: planted on a block of the mock allocator from Python (host memory of this process; nothing runs on
    a device, no product code is changed) — one byte before and one after the payload, a memset that straddles its end, a
    free of a bogus pointer — each is recorded with its kind, side and offset; a clean block records nothing; with the mode
    off nothing is recorded and hipMalloc / hipFree behave as malloc / free."""
    lib, n = guard.lib, 1000
    assert lib.hipmock_guard_red_zone_bytes() >= 2 * 256 * 8       # two rows of the widest 2-D level of this module
    guard.enable(True)
    ptr = ctypes.c_void_p()
    assert lib.hipmock_malloc(ctypes.byref(ptr), n) == 0
    payload = (ctypes.c_ubyte * n).from_address(ptr.value)
    assert all(b == 0xFF for b in payload) and np.isnan(np.frombuffer(payload, dtype=np.float64, count=n // 8)).all()
    assert guard.take() == [] and guard.live() == 1
    clean = ctypes.c_void_p()
    assert lib.hipmock_malloc(ctypes.byref(clean), 64) == 0

    (ctypes.c_ubyte * 1).from_address(ptr.value - 1)[0] = 0
    bad = guard.take()
    assert [(v.kind, v.side, v.offset, v.bytes) for v in bad] == [(RED_ZONE, 0, -1, n)], bad
    seq = bad[0].seq
    assert guard.take() == []                                          # recorded once, the zone repaired

    (ctypes.c_ubyte * 1).from_address(ptr.value + n)[0] = 7
    (ctypes.c_ubyte * 1).from_address(ptr.value + n + 100)[0] = 7
    bad = guard.take()
    assert [(v.kind, v.side, v.offset, v.bytes, v.seq) for v in bad] == [(RED_ZONE, 1, n, n, seq)], bad

    assert lib.hipmock_memset(ptr, 0, n) == 0 and guard.take() == []        # the whole payload: fine
    assert lib.hipmock_memset(ptr.value + n - 8, 0, 16) != 0                # straddles the end: refused and recorded
    bad = guard.take()
    assert [(v.kind, v.side, v.offset, v.bytes, v.length, v.seq) for v in bad] == [(RANGE, 1, n - 8, n, 16, seq)], bad
    assert lib.hipmock_memset(ptr.value - 8, 0, 16) != 0                    # starts below the payload
    bad = guard.take()
    assert [(v.kind, v.side, v.offset) for v in bad] == [(RANGE, 0, -8)], bad

    host = (ctypes.c_ubyte * 32)()                                          # hipMemcpyDefault (4): the sides are looked up
    assert lib.hipmock_memcpy(ptr.value + n - 32, host, 32, 4) == 0 and lib.hipmock_memcpy(host, ptr, 32, 4) == 0 and guard.take() == []
    assert lib.hipmock_memcpy(ptr.value + n - 16, host, 32, 4) != 0
    bad = guard.take()
    assert [(v.kind, v.side, v.offset, v.length, v.seq) for v in bad] == [(RANGE, 1, n - 16, 32, seq)], bad
    assert lib.hipmock_memcpy(host, ptr.value + n, 8, 2) != 0               # device to host, from the red zone
    assert [(v.kind, v.side, v.offset) for v in guard.take()] == [(RANGE, 1, n)]

    assert lib.hipmock_free(ptr.value + 16) != 0                            # not the start of a live block: nothing is freed
    bad = guard.take()
    assert [(v.kind, v.side) for v in bad] == [(BAD_FREE, -1)] and guard.live() == 2

    (ctypes.c_ubyte * 1).from_address(ptr.value + n + 5)[0] = 1        # damage that only hipFree sees
    assert lib.hipmock_free(ptr) == 0
    bad = guard.take()
    assert [(v.kind, v.side, v.offset, v.seq) for v in bad] == [(RED_ZONE, 1, n + 5, seq)], bad
    assert lib.hipmock_free(ptr) != 0                                       # a second free of the same block
    assert [(v.kind,) for v in guard.take()] == [(BAD_FREE,)]

    # a guarded block outlives the switch and is still freed as a guarded block; a block of the plain mode likewise
    guard.enable(False)
    plain = ctypes.c_void_p()
    assert lib.hipmock_malloc(ctypes.byref(plain), n) == 0 and guard.live() == 1
    assert lib.hipmock_memset(plain.value + n - 8, 0, 8) == 0
    assert lib.hipmock_free(clean) == 0 and guard.live() == 0
    guard.enable(True)
    assert lib.hipmock_free(plain) == 0
    assert guard.take() == []
    guard.enable(False)
    assert lib.hipmock_malloc(ctypes.byref(plain), 0) == 0 and plain.value    # (malloc(1), as before)
    assert lib.hipmock_free(plain) == 0 and guard.take() == []
