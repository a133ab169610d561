"""The vector algebra of csrc/kernels_blas.hip against extended precision: the two-pass reductions (dot, gram, block_gram,
normalize), the elementwise kernels (lincomb, block_combine, axpy, scale, fill, copy) and the four Gram-Schmidt paths
(k_mgs_small; the blocked Cholesky-QR k_mgs_gram / k_mgs_factor / k_mgs_apply with its device-side gate; k_mgs_step; the
classical form), on workspaces built the way processor._vector_plan builds them — from below one wave up to the sizes
where the block counts are capped and the grid-stride loops make a second trip.

Every tolerance here is one of three kinds:
  * a chain-length bound: (number of roundings on the longest path of the kernel's fixed summation tree or of the
    elementwise formula) * 2^-53 * (sum of the absolute values of the terms) — derived next to where it is used;
  * a stated multiple of the error of the fp64 restatement of the reference (oracle.sparse_ref.RefProcessor) on the same
    input, both measured against the exact thin-QR factor in extended precision;
  * the project's parity bar of 1e-10 (NORTH_STAR of tests/test_parity_reference.py).

The Gram-Schmidt tests print one line "GSACC ..." per case with the measured distances (pytest -s); the table of
profiles/r14_vector_algebra_accuracy.md was made from those lines."""
import ctypes
import functools
import math

import numpy as np
import pytest

from conftest import rel_err
from multigridcmt_amd import MGCMTProcessor, _lib
from multigridcmt_amd.operators import StructuredOperator, laplacian_operator, tri_identity
from multigridcmt_amd.plan import Plan, release_plans
from oracle.sparse_ref import RefProcessor

V, F, T, W = _lib.SLOT_V, _lib.SLOT_F, _lib.SLOT_T, _lib.SLOT_W
U = 2.0 ** -53                      # unit roundoff of fp64
NORTH_STAR = 1e-10

# ---- extended precision ------------------------------------------------------------------------------------------------
# The references are computed in np.longdouble where that is the x87 80-bit format (eps = 2^-63 = 1.08e-19) or better; where
# it is not (longdouble == double on some platforms) in mpmath numbers of 113 bits held in object arrays, which NumPy
# combines with the same operators.
LD_NATIVE = bool(np.finfo(np.longdouble).eps < 2e-19)
if LD_NATIVE:
    assert np.finfo(np.longdouble).eps < 2e-19

    def xp(a):
        return np.asarray(a, dtype=np.longdouble)

    def xsqrt(s):
        return np.sqrt(s)
else:
    import mpmath
    mpmath.mp.prec = 113
    assert mpmath.mp.eps < 2e-19

    def xp(a):
        a = np.asarray(a)
        if a.dtype == object:
            return a
        out = np.empty(a.shape, dtype=object)
        out.ravel()[:] = [mpmath.mpf(float(v)) for v in a.ravel()]
        return out if out.shape else out[()]

    def xsqrt(s):
        return mpmath.sqrt(s)


def f64(a):
    return np.asarray(a).astype(np.float64)


def xdot(a, b):
    """<a, b> of two extended-precision vectors, pairwise summation"""
    return (a * b).sum()


def exact_dot(x, y):
    """(sum of x_i y_i, sum of |x_i y_i|) of two fp64 vectors.  A product of two doubles has 106 bits: in the 64-bit
    significand of the extended format it is rounded (relative 2^-64), its leading double hi and the rest lo are then summed
    without error by math.fsum — the result is exact up to 2^-64 of the sum of |x_i y_i|, 1/2048 of one unit of the bounds
    below.  (From 2^17 terms on only the leading parts go through fsum; the rests, 2^-53 of them, are summed pairwise.)"""
    p = xp(x) * xp(y)
    hi = f64(p)
    lo = p - xp(hi)
    low = math.fsum(f64(lo).tolist()) if len(hi) < (1 << 17) else lo.sum()
    return xp(math.fsum(hi.tolist())) + xp(low), float(np.abs(hi).sum())      # (the scale of the bound: pairwise in fp64 will do)


# ---- the launch geometry of the reductions (kernels_blas.hip) ------------------------------------------------------------
RED_THREADS = 256                   # kRedThreads
RED_PER_THREAD = 8                  # reduce_blocks: one block per kRedThreads * 8 elements ...
RED_MAX_BLOCKS = 1024               # ... up to kRedMaxBlocks
MGS_GRAM_BLOCKS = 768               # kMgsGramBlocks
MGS_SMALL_MAX_N = 4096              # kMgsSmallMaxN
MGS_BLOCK_COND = 100.0              # kMgsBlockCond


def reduce_blocks(n):
    return max(1, min(RED_MAX_BLOCKS, -(-n // (RED_THREADS * RED_PER_THREAD))))


def chain_length(n):
    """D: the roundings on the longest path from an element to the result of a two-pass reduction over n elements.
    First pass (k_dot_partial, k_gram_partial, k_block_gram): the product (1; none where it is fused into an fma), the
    thread's own chain of ceil(n / (blocks * 256)) additions, the 6 steps of the 64-lane shuffle tree, the 4 wave sums of
    the workgroup added in turn.  Second pass (k_dot_final): ceil(blocks / 256) additions per thread, the shuffle tree (6),
    the wave sums (4).  n = 2^22: 1 + 16 + 6 + 4 + 4 + 6 + 4 = 41; n = 16384 (8 blocks): 1 + 8 + 6 + 4 + 1 + 6 + 4 = 30."""
    nb = reduce_blocks(n)
    return 1 + -(-n // (nb * RED_THREADS)) + 6 + 4 + -(-nb // RED_THREADS) + 6 + 4


assert chain_length(1 << 22) == 41 and max(chain_length(1 << e) for e in range(1, 23)) <= 48

# below a wave; one wave; a partial workgroup; one workgroup; one block's 8 elements per thread; two blocks; the first sizes
# past kMgsSmallMaxN
SIZES = [2, 4, 32, 64, 128, 256, 2048, 4096, 8192, 16384]
N_GRAM_SECOND_TRIP = 1 << 19        # k_mgs_gram: 2^18 double2 / 256 = 1024 blocks wanted, 768 launched
N_REDUCE_SECOND_TRIP = 1 << 22      # reduce_blocks capped at 1024: 16 elements per thread, two trips of 8


def vector_plan(n, nvec):
    """a single-level 1 x n workspace as processor._vector_plan builds it (not cached: the test closes it)"""
    return Plan(StructuredOperator("1d", n, [(None, tri_identity(n))]), n, nvec=max(nvec, 2))


LAYOUTS = [("1d", n) for n in SIZES] + [("2d", 0), ("2d", 1), ("3d", 0)]
LAYOUT_IDS = ["n%d" % n for n in SIZES] + ["2d-g128-level0", "2d-g128-level1", "3d-g16"]


def open_layout(layout, nvec):
    """(plan, level): the 1-D workspaces, and the 16 halo rows of a 2-D level / the halo planes of a 3-D one"""
    kind, arg = layout
    if kind == "1d":
        return vector_plan(arg, nvec), 0
    if kind == "2d":
        return Plan(laplacian_operator(128, "2d"), 64, nvec=nvec), arg
    return Plan(laplacian_operator(16, "3d"), 8, nvec=nvec), 0


def sample_vectors(rng, n, count):
    """fp64 vectors, alternately with random signs and with mixed magnitudes (entries scaled by 10^randint(-8, 9)), so that
    cancellation and the summation order show"""
    out = []
    for i in range(count):
        x = rng.uniform(-1.0, 1.0, n)
        if i % 2:
            x = x * 10.0 ** rng.randint(-8, 9, n)
        out.append(x)
    return out


# ---- raw storage: halo rows and padding --------------------------------------------------------------------------------
def _memcpy():
    """the device-to-host copy behind the bound library — hipmock_memcpy of the emulated runtime, hipMemcpy of the HIP
    runtime libmgcmt_hip.so is linked against (a symbol lookup in a library searches what it depends on) — or None"""
    fn = None
    for name in ("hipmock_memcpy", "hipMemcpy"):
        try:
            fn = getattr(_lib.lib(), name)
            break
        except AttributeError:
            pass
    if fn is None:
        return None
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return fn


class Raw:
    """Bit patterns of whole slots of one level: per column the halo rows above, the interior, the halo rows below and the
    padding up to the next column (mgcmt_vec_ptr, mgcmt_plan_level_halo), copied with hipMemcpy.  Where the library does not
    let hipMemcpy through, the interiors alone (mgcmt_download)."""

    def __init__(self, p, level, slots=(V, F, T, W)):
        self.p, self.level, self.slots = p, level, slots
        nr, gc, _ = p.level_shape(level)
        self.n = nr * gc
        self.lead = p.level_halo(level)[0] * gc
        self.stride = (p.vec_ptr(level, V, 1) - p.vec_ptr(level, V, 0)) // 8
        assert self.stride >= self.n + 2 * self.lead
        self.copy = _memcpy()

    def take(self):
        out = {}
        for s in self.slots:
            if self.copy is None:
                out[s] = np.stack([self.p.download(self.level, s, q) for q in range(self.p.nvec)]).view(np.uint64)
                continue
            self.p.sync()
            buf = np.empty(self.p.nvec * self.stride, dtype=np.uint64)
            rc = self.copy(buf.ctypes.data, self.p.vec_ptr(self.level, s, 0) - 8 * self.lead, buf.nbytes, 2)
            assert rc == 0
            out[s] = buf.reshape(self.p.nvec, self.stride)
        return out

    def interior(self, snap, slot, vec):
        a = snap[slot][vec]
        return (a if self.copy is None else a[self.lead:self.lead + self.n]).view(np.float64)

    def assert_only_written(self, before, after, outputs, what):
        """every vector not in `outputs` has the bits it had, halo and padding included; of an output the halo and padding"""
        for s in self.slots:
            for q in range(self.p.nvec):
                b, a = before[s][q], after[s][q]
                if (s, q) in outputs:
                    if self.copy is None:
                        continue
                    same = np.array_equal(b[:self.lead], a[:self.lead]) and np.array_equal(b[self.lead + self.n:], a[self.lead + self.n:])
                    assert same, "%s: the halo or padding of output (%d, %d) changed" % (what, s, q)
                else:
                    assert np.array_equal(b, a), "%s: vector (%d, %d), not an output, changed" % (what, s, q)


@pytest.mark.parametrize("layout", [LAYOUTS[0], LAYOUTS[3], LAYOUTS[11], LAYOUTS[12]], ids=[LAYOUT_IDS[i] for i in (0, 3, 11, 12)])
def test_raw_storage_is_what_the_halo_checks_read(backend, layout):
    """The halo checks below are not skipped on this backend, and look where they think they look: of a fresh plan (cleared
    when allocated) one uploaded vector shows in its interior and nowhere else."""
    p, level = open_layout(layout, 3)
    try:
        raw = Raw(p, level)
        assert raw.copy is not None, "hipMemcpy cannot be reached through the bound library: halo rows would go unchecked"
        x = np.random.RandomState(9).rand(p.size(level)) + 1.0
        p.upload(level, F, 1, x)
        snap = raw.take()
        assert np.array_equal(raw.interior(snap, F, 1), x)
        snap[F][1][raw.lead:raw.lead + raw.n] = 0
        assert not any(snap[s].any() for s in (V, F, T, W))
    finally:
        p.close()


# =========================================================================================================================
# 1. reductions
# =========================================================================================================================
WHERE6 = [(V, 0), (F, 1), (T, 2), (W, 3), (V, 4), (W, 5)]       # vectors in different slots


def check_entry(got, x, y, n, what):
    exact, mag = exact_dot(x, y)
    err = abs(float(xp(got) - exact))
    assert err <= chain_length(n) * U * mag, "%s: |got - exact| = %.3g = %.2f units of 2^-53 sum|x y| (D = %d)" % (
        what, err, err / (U * mag) if mag else float("inf"), chain_length(n))
    return err / (U * mag) if mag else 0.0


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_dot_and_gram(backend, layout):
    """mgcmt_dot and mgcmt_gram (nv = 1..6) against the exact sums: |got - exact| <= D 2^-53 sum |x_i y_i| per entry, D =
    chain_length(n); the Gram matrix exactly symmetric; the same bits on a second call and after unrelated vectors of the
    plan have been overwritten."""
    p, level = open_layout(layout, 6)
    try:
        n = p.size(level)
        rng = np.random.RandomState(100 + n)
        vs = sample_vectors(rng, n, 6)
        for v, (s, q) in zip(vs, WHERE6):
            p.upload(level, s, q, v)
        worst = 0.0
        dots = {}
        for a, b in ((0, 1), (2, 3), (1, 3), (0, 0), (1, 1), (5, 2)):
            dots[(a, b)] = p.dot(level, WHERE6[a], WHERE6[b])
            worst = max(worst, check_entry(dots[(a, b)], vs[a], vs[b], n, "dot(%d, %d) of %d" % (a, b, n)))
        grams = {}
        for nv in range(1, 7):
            G = p.gram(level, WHERE6[:nv])
            grams[nv] = G
            assert np.array_equal(G, G.T), nv
            for a in range(nv):
                for b in range(a, nv):
                    if nv == 6 or (a, b) == (nv - 1, nv - 1) or (a, b) == (0, nv - 1):
                        worst = max(worst, check_entry(G[a, b], vs[a], vs[b], n, "gram of %d, entry (%d, %d), n = %d" % (nv, a, b, n)))
        for nv in range(1, 6):        # (a pair's sum does not depend on how many vectors ride along: one fixed order per pair)
            assert np.array_equal(grams[nv], grams[6][:nv, :nv]), nv
        # determinism: again, and again after the other vectors of the plan have changed
        for round_ in range(2):
            for (a, b), want in dots.items():
                assert p.dot(level, WHERE6[a], WHERE6[b]) == want, (round_, a, b)
            for nv in (1, 3, 6):
                assert np.array_equal(p.gram(level, WHERE6[:nv]), grams[nv]), (round_, nv)
            for s, q in ((V, 1), (F, 0), (T, 5), (W, 0)):
                p.upload(level, s, q, rng.rand(n))
        print("REDACC %s dot/gram n=%d worst=%.2f units (D=%d)" % (backend, n, worst, chain_length(n)))
    finally:
        p.close()


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_block_gram(backend, layout):
    """mgcmt_block_gram, na in {1, 5, 12} by nb in {1, 3, 4}, vectors in all four slots with indices up to 39 of a plan
    that stores 40 per slot: every entry within D 2^-53 sum |a_i b_i| of the exact sum; deterministic."""
    p, level = open_layout(layout, 40)
    try:
        n = p.size(level)
        rng = np.random.RandomState(200 + n)
        A = [(W, 39), (W, 32), (F, 35), (V, 0), (T, 38), (W, 1), (F, 0), (V, 33), (T, 2), (W, 36), (F, 39), (V, 37)]
        B = [(V, 34), (F, 35), (T, 39), (W, 0)]                  # (F, 35) is on both sides
        host = {}
        for w, v in zip(A + [B[0], B[2], B[3]], sample_vectors(rng, n, 15)):
            host[w] = v
            p.upload(level, w[0], w[1], v)
        exact = {(a, b): exact_dot(host[a], host[b]) for a in A for b in B}
        worst = 0.0
        first = {}
        for na in (1, 5, 12):
            for nb in (1, 3, 4):
                G = p.block_gram(level, A[:na], B[:nb])
                first[(na, nb)] = G
                for i, a in enumerate(A[:na]):
                    for j, b in enumerate(B[:nb]):
                        ex, mag = exact[(a, b)]
                        err = abs(float(xp(G[i, j]) - ex))
                        assert err <= chain_length(n) * U * mag, (n, na, nb, i, j, err / (U * mag))
                        worst = max(worst, err / (U * mag))
        p.upload(level, V, 1, rng.rand(n))
        p.upload(level, W, 38, rng.rand(n))
        for (na, nb), G in first.items():
            assert np.array_equal(p.block_gram(level, A[:na], B[:nb]), G), (na, nb)
        print("REDACC %s block_gram n=%d worst=%.2f units (D=%d)" % (backend, n, worst, chain_length(n)))
    finally:
        p.close()


def normalize_columns(rng, n):
    """random signs; mixed magnitudes; norms 1e-150 and 1e+150 (their squares stay finite; a square scaled afterwards would not)"""
    a, b, c, d = sample_vectors(rng, n, 4)
    c = c * (1e-150 / np.linalg.norm(c))
    d = sample_vectors(rng, n, 1)[0]
    d = d * (1e+150 / np.linalg.norm(d))
    return [a, b, c, d]


def check_normalized(got, x, n, what):
    """x / |x| elementwise.  The sum of squares has no cancellation: its relative error is at most D 2^-53, the square root
    halves that and rounds once, the division rounds once — within (4 + D) 2^-53 |x_i| / |x| with room to spare."""
    lx = xp(x)
    ref = lx / xsqrt(xdot(lx, lx))
    err = np.abs(f64(xp(got) - ref))
    tol = (4 + chain_length(n)) * U * np.abs(f64(ref))
    bad = np.flatnonzero(~(err <= tol))
    assert bad.size == 0, "%s: element %d off by %.3g, allowed %.3g" % (what, bad[0], err[bad[0]], tol[bad[0]])


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_normalize(backend, layout):
    """mgcmt_normalize (k_dot_partial, k_scale_by_norm) on four columns — random signs, mixed magnitudes, norms 1e-150 and
    1e+150 — elementwise against x / |x| in extended precision; a fifth column, the halo rows and the padding keep their
    bits; the same bits from the same input twice."""
    p, level = open_layout(layout, 5)
    try:
        n = p.size(level)
        rng = np.random.RandomState(300 + n)
        cols = normalize_columns(rng, n)
        raw = Raw(p, level, slots=(V,))
        marker = rng.rand(n)
        runs = []
        for round_ in range(2):
            for q, x in enumerate(cols):
                p.upload(level, V, q, x)
            p.upload(level, V, 4, marker)
            before = raw.take()
            p.normalize(level, V, 4)
            after = raw.take()
            raw.assert_only_written(before, after, {(V, q) for q in range(4)}, "normalize")
            runs.append([raw.interior(after, V, q).copy() for q in range(4)])
        for q, x in enumerate(cols):
            check_normalized(runs[0][q], x, n, "normalize n = %d column %d" % (n, q))
            assert np.array_equal(runs[0][q], runs[1][q]), q
    finally:
        p.close()


@functools.lru_cache(maxsize=1)
def _large_reduction_case():
    n = N_REDUCE_SECOND_TRIP
    vs = sample_vectors(np.random.RandomState(22), n, 4)
    exact = {(a, b): exact_dot(vs[a], vs[b]) for a in range(4) for b in range(a, 4)}
    return vs, exact


@pytest.mark.gpu
def test_reductions_where_the_block_count_is_capped(hip_only):
    """n = 2^22: reduce_blocks stops at 1024 and k_dot_partial / k_gram_partial / k_block_gram stride twice (16 elements per
    thread), k_dot_final reads 4 partials per thread.  Four vectors."""
    n = N_REDUCE_SECOND_TRIP
    vs, exact = _large_reduction_case()
    where = WHERE6[:4]
    p = vector_plan(n, 4)
    try:
        for v, (s, q) in zip(vs, where):
            p.upload(0, s, q, v)
        D = chain_length(n)

        def check(got, a, b, what):
            ex, mag = exact[(min(a, b), max(a, b))]
            err = abs(float(xp(got) - ex))
            assert err <= D * U * mag, (what, a, b, err / (U * mag))
            return err / (U * mag)
        worst = max(check(p.dot(0, where[a], where[b]), a, b, "dot") for a, b in ((0, 1), (2, 3), (1, 1), (3, 0)))
        G = p.gram(0, where)
        assert np.array_equal(G, G.T)
        BG = p.block_gram(0, where[:3], where[3:])
        for a in range(4):
            for b in range(a, 4):
                worst = max(worst, check(G[a, b], a, b, "gram"))
        for a in range(3):
            worst = max(worst, check(BG[a, 0], a, 3, "block_gram"))
        assert p.dot(0, where[0], where[1]) == p.dot(0, where[0], where[1])
        assert np.array_equal(p.gram(0, where), G) and np.array_equal(p.block_gram(0, where[:3], where[3:]), BG)
        print("REDACC hip reductions n=%d worst=%.2f units (D=%d)" % (n, worst, D))
        # normalize: two columns in slot F (k_scale_by_norm sums the 1024 partials in index order)
        cols = [vs[0], vs[1] * (1e+150 / np.linalg.norm(vs[1]))]
        for q, x in enumerate(cols):
            p.upload(0, F, q, x)
        p.normalize(0, F, 2)
        for q, x in enumerate(cols):
            check_normalized(p.download(0, F, q), x, n, "normalize n = 2^22 column %d" % q)
    finally:
        p.close()


# =========================================================================================================================
# 2. elementwise kernels
# =========================================================================================================================
COEFFS = [0.75, -2.5, 0.0, -0.0, 1e200, 1e-200, -1e200, 3.0, -1e-200, 1.0, -0.125, 1e3]


class Workspace:
    """eight vectors in each of the four slots of a level, every one with data of its own and a host copy"""
    NVEC = 8

    def __init__(self, layout, seed):
        self.p, self.level = open_layout(layout, self.NVEC)
        self.n = self.p.size(self.level)
        self.rng = np.random.RandomState(seed + self.n)
        self.raw = Raw(self.p, self.level)
        self.host = {}
        for s in (V, F, T, W):
            for q, x in enumerate(sample_vectors(self.rng, self.n, self.NVEC)):
                self.host[(s, q)] = x
                self.p.upload(self.level, s, q, x)

    def run(self, outputs, what, call):
        """call(); -> the outputs' new interiors; everything else checked bit for bit; then the outputs' old contents again"""
        before = self.raw.take()
        call()
        after = self.raw.take()
        self.raw.assert_only_written(before, after, set(outputs), what)
        for s, q in self.host:
            if (s, q) not in outputs:
                assert np.array_equal(self.raw.interior(after, s, q).view(np.uint64), self.host[(s, q)].view(np.uint64)), (what, s, q)
        got = [self.raw.interior(after, s, q).copy() for s, q in outputs]
        for s, q in outputs:         # (the next case starts from the same data: coefficients of 1e200 must not pile up)
            self.p.upload(self.level, s, q, self.host[(s, q)])
        return got

    def close(self):
        self.p.close()


def assert_within(got, ref, tol, what):
    err = np.abs(f64(xp(got) - ref))
    bad = np.flatnonzero(~(err <= tol))
    assert bad.size == 0, "%s: element %d is %r, exact %r, allowed error %.3g" % (what, bad[0], got[bad[0]], float(ref[bad[0]]), tol[bad[0]])


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_lincomb(backend, layout):
    """dst = sum of nt terms c_t v_t, nt = 1..4: k_lincomb rounds the first product and each of the nt - 1 fused
    multiply-adds once (a build that does not fuse: nt products and nt - 1 sums on the longest path, still below) —
    within (nt + 1) 2^-53 sum |c_t v_t| elementwise.  Destinations: a fifth vector, the first input, the last input.
    Coefficients 0, -0.0 and 1e+-200 among them."""
    ws = Workspace(layout, 400)
    try:
        terms_at = [(V, 0), (F, 3), (W, 7), (T, 2)]
        case = 0
        for nt in range(1, 5):
            for dst in ((W, 1), terms_at[0], terms_at[nt - 1]):
                cs = [COEFFS[(case * 5 + 3 * t) % len(COEFFS)] for t in range(nt)]
                case += 1
                ins = [ws.host[w].copy() for w in terms_at[:nt]]
                got, = ws.run([dst], "lincomb", lambda: ws.p.lincomb(ws.level, list(zip(cs, terms_at[:nt])), dst))
                ref = sum(xp(c) * xp(x) for c, x in zip(cs, ins))
                mag = sum(np.abs(c * x) for c, x in zip(cs, ins))
                assert_within(got, ref, (nt + 1) * U * mag, "lincomb nt = %d, coefficients %r, n = %d" % (nt, cs, ws.n))
    finally:
        ws.close()


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_block_combine(backend, layout):
    """out_j = sum of nin inputs c_ij x_i (k_block_combine2: nin fused multiply-adds from zero, one rounding each; unfused
    nin products and nin - 1 sums) — within (nin + 1) 2^-53 sum |c| |x|.  nin in {1, 7, 12}, nout in {1, 3, 4}; outputs
    that are the first and the last input."""
    ws = Workspace(layout, 500)
    try:
        pool = [(W, 0), (F, 1), (V, 2), (T, 3), (W, 4), (F, 5), (V, 6), (T, 7), (W, 7), (F, 0), (V, 1), (T, 2)]
        spare = [(V, 7), (T, 0)]
        case = 0
        for nin in (1, 7, 12):
            for nout in (1, 3, 4):
                ins_at = pool[:nin]
                outs = ([ins_at[0], spare[0], ins_at[-1], spare[1]] if nin > 1 else [ins_at[0], spare[0], spare[1], (F, 7)])[:nout]
                C = np.array([[COEFFS[(case + 5 * i + 7 * j) % len(COEFFS)] for j in range(nout)] for i in range(nin)])
                case += 1
                ins = [ws.host[w].copy() for w in ins_at]
                got = ws.run(outs, "block_combine", lambda: ws.p.block_combine(ws.level, ins_at, outs, C))
                for j in range(nout):
                    ref = sum(xp(C[i, j]) * xp(ins[i]) for i in range(nin))
                    mag = sum(np.abs(C[i, j] * ins[i]) for i in range(nin))
                    assert_within(got[j], ref, (nin + 1) * U * mag, "block_combine nin = %d, nout = %d, output %d, n = %d" % (nin, nout, j, ws.n))
    finally:
        ws.close()


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_axpy_scale_fill_copy(backend, layout):
    """y += alpha x: one product and one sum, within 2 2^-53 (|y| + |alpha x|).  x *= alpha: one correctly rounded product —
    the bits of the fp64 product.  fill and copy: the bits asked for.  Nothing else changes, halo and padding included."""
    ws = Workspace(layout, 600)
    try:
        for i, alpha in enumerate((0.75, 0.0, -0.0, 1e200, 1e-200, -3.0)):
            xw, yw = (F, i), (T, 7 - i)
            x, y = ws.host[xw].copy(), ws.host[yw].copy()
            got, = ws.run([yw], "axpy", lambda: ws.p.axpy(ws.level, alpha, xw, yw))
            assert_within(got, xp(y) + xp(alpha) * xp(x), 2 * U * (np.abs(y) + np.abs(alpha * x)), "axpy alpha = %r, n = %d" % (alpha, ws.n))
        for i, alpha in enumerate((0.75, 0.0, -0.0, 1e200, 1e-200, -3.0)):
            w = (W, i)
            x = ws.host[w].copy()
            got, = ws.run([w], "scale", lambda: ws.p.scale(ws.level, alpha, w))
            assert np.array_equal(got.view(np.uint64), (x * alpha).view(np.uint64)), alpha
        for value, w in ((-0.0, (V, 3)), (1e-310, (F, 6)), (2.5, (V, 0))):
            got, = ws.run([w], "fill", lambda: ws.p.fill(ws.level, w[0], w[1], value))
            assert np.array_equal(got.view(np.uint64), np.full(ws.n, value).view(np.uint64)), value
        for src, dst in (((T, 1), (T, 2)), ((W, 7), (V, 5))):
            x = ws.host[src].copy()
            got, = ws.run([dst], "copy", lambda: ws.p.copy(ws.level, src[0], src[1], dst[0], dst[1]))
            assert np.array_equal(got.view(np.uint64), x.view(np.uint64))
    finally:
        ws.close()


# =========================================================================================================================
# 3. Gram-Schmidt
# =========================================================================================================================
def kappa_s(R):
    """||R~||_F ||R~^-1||_F of the upper-triangular R with its columns scaled to unit length — the quantity the gate of
    k_mgs_factor bounds (there from the Cholesky factor of the unit-diagonal Gram matrix) — in extended precision directly
    from R: R~^-1 by back substitution.  k for orthogonal columns, and never less (Cauchy-Schwarz on trace(R~ R~^-1) = k)."""
    k = R.shape[0]
    Rt = xp(R).copy()
    for j in range(k):
        Rt[:, j] = Rt[:, j] / xsqrt(xdot(Rt[:, j], Rt[:, j]))
    inv = xp(np.zeros((k, k)))
    for j in range(k):
        inv[j, j] = 1 / Rt[j, j]
        for i in range(j - 1, -1, -1):
            inv[i, j] = -xdot(Rt[i, i + 1:j + 1], inv[i + 1:j + 1, j]) / Rt[i, i]
    return float(xsqrt((Rt * Rt).sum() * (inv * inv).sum()))


def mix_matrix(k, t):
    return np.eye(k) + t * np.triu(np.ones((k, k)), 1)


def t_for(k, target, measure=None):
    """t with measure(I + t N) = target, by bisection (both measures grow with t)"""
    measure = measure or kappa_s
    if k == 1 or measure(mix_matrix(k, 0.0)) >= target:
        return 0.0
    lo, hi = 0.0, 1.0
    while measure(mix_matrix(k, hi)) < target:
        lo, hi = hi, 2 * hi
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if measure(mix_matrix(k, mid)) < target:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def cond2_scaled(R):
    Rt = R / np.linalg.norm(R, axis=0)
    return float(np.linalg.cond(Rt))


def exact_q(A):
    """The thin-QR factor of the fp64 matrix A with a positive diagonal of R, in extended precision: modified Gram-Schmidt
    applied twice (the second pass removes what the first left, of the order cond(A) eps).  Checked here, so that a wrong
    reference cannot pass: orthonormal to 1e-17 k, and Q R reproduces A to 1e-17 ||A|| with R = triu(Q^T A), diag(R) > 0.
    -> Q^T, a column of Q per row (contiguous: half the time of strided columns at 2^19 x 12)."""
    n, k = A.shape
    LA = np.ascontiguousarray(xp(A).T)
    Q = LA.copy()
    for _ in range(2):
        for i in range(k):
            Q[i] = Q[i] / xsqrt(xdot(Q[i], Q[i]))
            for j in range(i + 1, k):
                Q[j] = Q[j] - xdot(Q[j], Q[i]) * Q[i]
    for i in range(k):
        for j in range(i, k):
            assert abs(float(xdot(Q[i], Q[j]) - (1 if i == j else 0))) <= 1e-17 * k, (i, j)
    norm_a = float(xsqrt((LA * LA).sum()))
    for j in range(k):
        r = [xdot(Q[i], LA[j]) for i in range(j + 1)]          # column j of R = triu(Q^T A)
        assert r[j] > 0
        d = sum(Q[i] * r[i] for i in range(j + 1)) - LA[j]
        assert float(xsqrt(xdot(d, d))) <= 1e-17 * norm_a, j
    return Q


def distance(X, Qt):
    """e(X) = max over the columns of ||X_j - Q_j||_2 (Qt: exact_q's result)"""
    D = np.ascontiguousarray(xp(X).T) - Qt
    return max(float(xsqrt(xdot(d, d))) for d in D)


def orthogonality(X):
    L = np.ascontiguousarray(xp(X).T)
    k = L.shape[0]
    return max(abs(float(xdot(L[i], L[j]) - (1 if i == j else 0))) for i in range(k) for j in range(i, k))


@functools.lru_cache(maxsize=4)
def gs_case(n, k, target, measure="kappa_s", modified=1):
    """A = Q0 R D with orthonormal Q0, R = I + t N (N strictly upper triangular ones) and column scales D = 10^randint(-3, 4);
    t from the target condition.  -> (A, the kappa_s of R, the exact Q, the fp64 oracle's result and its distance e_ref)"""
    rng = np.random.RandomState(1000 + 7 * k + (n % 1009) + int(math.log10(target) * 16))
    Q0 = np.linalg.qr(rng.randn(n, k))[0]
    R = mix_matrix(k, t_for(k, target, kappa_s if measure == "kappa_s" else cond2_scaled))
    A = np.ascontiguousarray((Q0 @ R) * (10.0 ** rng.randint(-3, 4, size=k))[None, :])
    A.setflags(write=False)
    Q = exact_q(A)
    ref = RefProcessor().gramschmidt(A, modified=modified)
    return A, kappa_s(R), Q, ref, distance(ref, Q)


def device_gs(A, modified=1, option=1):
    """mgcmt_gramschmidt on the columns of A in a workspace of their length; option: MGCMT_OPT_MGS_BLOCK (None: as the plan
    was created — setting the option also sets the blocked form's least length)"""
    n, k = A.shape
    p = vector_plan(n, k)
    try:
        if option is not None:
            p.set_option(_lib.OPT_MGS_BLOCK, option)
        for q in range(k):
            p.upload(0, V, q, A[:, q])
        p.gramschmidt(0, V, k, modified=modified)
        return np.stack([p.download(0, V, q) for q in range(k)], axis=1)
    finally:
        p.close()


def report(backend, path, n, k, ks, e_ref, e_col=None, e_blk=None):
    def fmt(v):
        return "-" if v is None else "%.2e" % v
    print("GSACC %s %s n=%d k=%d kappa_s=%.4g e_ref=%s e_col=%s e_blk=%s" % (backend, path, n, k, ks, fmt(e_ref), fmt(e_col), fmt(e_blk)))


# The column forms compute what the oracle computes — only the summation order and the spelling with the un-normalised u
# differ — so their distance from the exact Q is held to 10 x the oracle's own (never below 10 k 2^-53); a wrong coefficient
# shows at the size of the coefficient, >= 1e-3 here.  Well-conditioned columns: the 2-norm condition of the scaled R is 3
# (the Frobenius product kappa_s is at least k, so it cannot itself stay below 4 for 32 columns; it is printed).
COLUMN_SMALL = [(2, 1), (2, 2), (4, 3), (64, 32), (4096, 1), (4096, 32)]
COLUMN_LONG = [(8192, 1), (8192, 13), (8192, 32), (16384, 12)]


def check_column_form(backend, n, k, modified, path):
    A, ks, Q, ref, e_ref = gs_case(n, k, 3.0, "cond2", modified)
    got = device_gs(A, modified=modified, option=0)
    e = distance(got, Q)
    report(backend, path, n, k, ks, e_ref, e_col=e)
    assert e <= 10 * max(e_ref, k * U), (n, k, e, e_ref)
    return got


@pytest.mark.parametrize("n,k", COLUMN_SMALL)
def test_gram_schmidt_one_workgroup(backend, n, k):
    """k_mgs_small (n <= 4096)"""
    assert n <= MGS_SMALL_MAX_N
    check_column_form(backend, n, k, 1, "small")


@pytest.mark.parametrize("n,k", COLUMN_LONG)
def test_gram_schmidt_column_steps(backend, n, k):
    """k_mgs_step behind one batched dot launch (MGCMT_OPT_MGS_BLOCK = 0)"""
    assert n > MGS_SMALL_MAX_N
    check_column_form(backend, n, k, 1, "step")


@pytest.mark.parametrize("n,k", COLUMN_SMALL + COLUMN_LONG)
def test_gram_schmidt_classical(backend, n, k):
    """modified = 0: launch_dots, k_axpy_dev, k_scale_dev"""
    check_column_form(backend, n, k, 0, "classical")


@pytest.mark.gpu
@pytest.mark.parametrize("modified", [1, 0])
def test_gram_schmidt_columns_where_the_block_count_is_capped(hip_only, modified):
    """(2^22, 4): k_dot_partial and k_mgs_step on 1024 blocks, two trips each"""
    check_column_form("hip", N_REDUCE_SECOND_TRIP, 4, modified, "step" if modified else "classical")


# The blocked form is a Cholesky-QR: it errs as kappa^2 eps where Gram-Schmidt errs as kappa eps — hence the factor kappa_s
# over the column bound below the gate.  Above it the columns must come out of the column-by-column kernels.
BELOW = [None, 30.0, 60.0, 90.0]     # None: t = 0, orthogonal columns, kappa_s = k
ABOVE = [110.0, 300.0, 1e4, 1e8]


def check_blocked_below(backend, n, k, target):
    A, ks, Q, ref, e_ref = gs_case(n, k, float(k) if target is None else target)
    assert ks < 95.0 and (target is None or abs(ks - target) < 1e-6 * target)
    blocked = device_gs(A, option=1)
    column = device_gs(A, option=0)
    e_blk, e_col = distance(blocked, Q), distance(column, Q)
    report(backend, "blocked", n, k, ks, e_ref, e_col=e_col, e_blk=e_blk)
    bound = 10 * ks * max(e_ref, k * U)
    assert e_blk <= bound, (n, k, ks, e_blk, bound)
    assert orthogonality(blocked) <= bound, (n, k, ks)
    assert rel_err(blocked, ref) < NORTH_STAR
    if ks >= 30.0:
        assert not np.array_equal(blocked, column), "the blocked form did not run"


@pytest.mark.parametrize("target", BELOW, ids=["orthogonal", "30", "60", "90"])
@pytest.mark.parametrize("k", [2, 6, 12])
@pytest.mark.parametrize("n", [8192, 16384])
def test_gram_schmidt_blocked_below_the_gate(backend, n, k, target):
    check_blocked_below(backend, n, k, target)


@pytest.mark.gpu
@pytest.mark.parametrize("target", BELOW, ids=["orthogonal", "30", "60", "90"])
def test_gram_schmidt_blocked_second_trip(hip_only, target):
    """(2^19, 12): k_mgs_gram wants 1024 blocks and gets kMgsGramBlocks = 768 — its grid-stride loop makes a second trip"""
    assert N_GRAM_SECOND_TRIP // 2 // RED_THREADS > MGS_GRAM_BLOCKS
    check_blocked_below("hip", N_GRAM_SECOND_TRIP, 12, target)


@pytest.mark.parametrize("target", ABOVE, ids=["110", "300", "1e4", "1e8"])
@pytest.mark.parametrize("n,k", [(8192, 2), (8192, 6), (8192, 12), (16384, 6)])
def test_gram_schmidt_blocked_above_the_gate(backend, n, k, target):
    A, ks, Q, ref, e_ref = gs_case(n, k, target)
    assert ks > 105.0
    gated = device_gs(A, option=1)
    column = device_gs(A, option=0)
    e = distance(gated, Q)
    report(backend, "gated", n, k, ks, e_ref, e_col=distance(column, Q), e_blk=e)
    assert np.array_equal(gated, column), "beyond kMgsBlockCond the columns go through the column-by-column kernels"
    assert e <= 10 * max(e_ref, k * U * ks), (n, k, ks, e, e_ref)


def test_kappa_targets_keep_clear_of_the_gate():
    """no input of this file within [95, 105] of the gate's 100, where rounding in the factor kernel could decide"""
    for k in (2, 6, 12):
        for target in BELOW[1:] + ABOVE:
            ks = kappa_s(mix_matrix(k, t_for(k, target)))
            assert abs(ks - target) <= 1e-6 * target and not 95.0 <= ks <= 105.0
        assert kappa_s(mix_matrix(k, 0.0)) == pytest.approx(k, abs=1e-15)


TRIGGERS = ["zero column", "identical columns", "overflowing diagonal", "one NaN"]


@pytest.mark.parametrize("trigger", TRIGGERS)
@pytest.mark.parametrize("k", [3, 12])
def test_gate_other_triggers(backend, trigger, k):
    """What else sends the columns to the column-by-column kernels: a pivot that is not positive, a zero or overflowing
    diagonal of the Gram matrix, anything not finite.  Each bit-equal to the option switched off (NaNs equal)."""
    n = 8192
    rng = np.random.RandomState(len(trigger) + k)
    A = rng.uniform(-1.0, 1.0, (n, k))
    if trigger == "zero column":
        A[:, k // 2] = 0.0
    elif trigger == "identical columns":
        A[:, k - 1] = A[:, 0]
    elif trigger == "overflowing diagonal":
        A[:, 1] *= 1e160
    else:
        A[n // 3, k - 2] = np.nan
    with np.errstate(all="ignore"):
        assert np.array_equal(device_gs(A, option=1), device_gs(A, option=0), equal_nan=True)


@pytest.mark.parametrize("target", [60.0, 300.0])
@pytest.mark.parametrize("n", [4096, 4097])
def test_processor_gramschmidt(backend, n, target):
    """MGCMTProcessor.gramschmidt: 4096 rows take the one-workgroup kernel; 4097 are padded to 8192 and take the long
    paths — the blocked form at kappa_s = 60, the column steps behind the gate at 300.  The column forms at kappa_s are held
    to the bound of the gated case, the blocked form to its own."""
    k = 6
    A, ks, Q, ref, e_ref = gs_case(n, k, target)
    got = MGCMTProcessor().gramschmidt(A)
    e = distance(got, Q)
    blocked = n > MGS_SMALL_MAX_N and ks < MGS_BLOCK_COND
    report(backend, "processor-" + ("blocked" if blocked else "small" if n <= MGS_SMALL_MAX_N else "gated"), n, k, ks, e_ref,
           e_col=None if blocked else e, e_blk=e if blocked else None)
    assert got.shape == (n, k)
    if blocked:
        assert e <= 10 * ks * max(e_ref, k * U)
        assert orthogonality(got) <= 10 * ks * max(e_ref, k * U)
    else:
        assert e <= 10 * max(e_ref, k * U * ks)
    assert rel_err(got, ref) < NORTH_STAR


def test_mgs_block_min_turns_the_blocked_form_off(backend, monkeypatch):
    """MGCMT_MGS_BLOCK_MIN (read when a plan is created) above the columns' length: bit-equal to MGCMT_OPT_MGS_BLOCK = 0, in
    a plan of its own and through MGCMTProcessor (whose padded length, 8192, is what counts)."""
    n, k = 8192, 6
    A, ks, Q, ref, e_ref = gs_case(n, k, 60.0)
    column = device_gs(A, option=0)
    blocked = device_gs(A, option=1)
    assert not np.array_equal(blocked, column)
    release_plans()
    monkeypatch.setenv("MGCMT_MGS_BLOCK_MIN", str(2 * n))
    try:
        assert np.array_equal(device_gs(A, option=None), column)
        assert np.array_equal(MGCMTProcessor().gramschmidt(A[:n - 5]), device_gs(np.vstack([A[:n - 5], np.zeros((5, k))]), option=0)[:n - 5])
        monkeypatch.setenv("MGCMT_MGS_BLOCK_MIN", str(n))
        assert np.array_equal(device_gs(A, option=None), blocked)
    finally:
        release_plans()              # (the processor's cached plan carries the setting)
