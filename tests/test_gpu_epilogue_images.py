"""The fused SpMV epilogues on every matrix image against an exact host
reference (tests/epilogue_cases.py; the magnitude condition of every case is
asserted on the host by tests/test_epilogue_cases.py).

launch_spmv (csrc/device.hpp) picks one of about twenty kernels per operator
and each is compiled for every epilogue. Here each image configuration is
driven through the CG, GMRES and MINRES cores' start / run / get / scalars
calls on integer data, where every product, row sum and dot is exact in any
summation order, and compared with == on bits:

* start (EpiResidual: operator(), row<C>, rows2 by kernel): the start values
  are the integer <r0, r0>_w = 4^m (CG) or its root 2^m (GMRES, MINRES),
  CG's residual is r0, the GMRES / MINRES start vector is r0 / 2^m;
* one CG step, launch per pass (EpiApDot): alpha is S(rho0) / S(<r0, A r0>_w)
  in the scalar type S of the solve (float64; float32 for unweighted float32
  vectors, where the reference's quotient is a float32 one too), and the
  residual is r0 - V(alpha) * A r0 evaluated by NumPy in the vector type;
* the same step in the persistent CG loop (its own SELL / DIA walk) where it
  accepts the case;
* one GMRES step (EpiStoreDot with q = V0): H[0, 0] = <V0, A V0>_w, dyadic;
* one MINRES step (EpiLanczos without p_old): h1 = <v, A v>_w;
* matrix preconditioners on another image than A's (EpiStoreNorm,
  EpiStoreDot at start, EpiAddStore in kry_gmres_solution).

The second step (the SrcScaled gather with EpiStoreDotV in GMRES, the p_old
branch of EpiLanczos in MINRES) runs on the rounded vectors of step 1, so its
dots are compared with a longdouble reference computed from the device's own
vectors after step 1, within the bound the issue derives: a row sum of
`width` products carries at most width * eps_V * (|A| |x|)_i, the float64
partial sums and the cast to the scalar type at most 2 eps_V of the terms'
absolute sum, so

    |got - ref| <= (width + 2) * eps_V * sum_i |q_i| w_i (|A| |x|)_i

for both dots (for EpiLanczos with p_old the reference is <v, A v - h0 p_old>_w
and the bound keeps the row sums' term alone).

A single missing or misplaced term is about 1 / n of that sum: in float64
ten orders above the bound at every size here, in float32 about 100 times it
at n <= 3,779, but within it at n = 200,003 and 1,200,003 (width 70 and 150),
where the exact first step and the bitwise vectors carry the case. The
largest fraction of the bound any configuration used on an MI355X (printed
per case with -s): GMRES H[0,1] 0.019 (DIA, 5 slot columns), MINRES h1 of step
2 0.013 (DIA, 21 slot columns, two rounds).

V1 as the step-2 SpMV stores it (SrcScaled forms w' / h10 in the gather,
EpiStoreDotV writes the row's own value) is compared bit for bit with the V1
the plain division pass forms when the basis is read after step 1; w' itself
(after the Gram-Schmidt pass) is returned by no call.

The vectors the step-1 epilogues store (w = A V0 by EpiStoreDot, w = A v0 by
EpiLanczos) are checked through the next basis vector, which NumPy replays
from the exact w with the device's own h; MINRES's vector after step 2
likewise from SciPy's csr_matvec of the device's v1 (the p_old branch's
store).

Not covered here: EpiScaleAddStore (tests/test_gpu_isai.py holds it to its
host loops)."""
import ctypes

import numpy as np
import pytest

from tests import epilogue_cases as EC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    EC.clear_caches()


def _bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    u = np.uint64 if got.dtype.itemsize == 8 else np.uint32
    bad = np.flatnonzero(got.view(u).reshape(-1) != want.view(u).reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} elements differ, first at flat index {int(bad[0])}: "
                           f"got {got.reshape(-1)[bad[0]]!r}, want {want.reshape(-1)[bad[0]]!r}")


def _raw_operator(A):
    """A CsrOperator over kry_csr_create with the index arrays as they are
    (int64 stays int64: CsrOperator itself narrows indices that fit int32)."""
    import krylov_amd
    from krylov_amd import _lib
    from krylov_amd.device import get_context

    op = krylov_amd.CsrOperator.__new__(krylov_amd.CsrOperator)
    op.ctx = get_context(None)
    op.shape, op.dtype, op.n, op.nnz = A.shape, np.dtype(A.dtype), A.shape[0], int(A.nnz)
    op.index_dtype = np.dtype(np.int64)
    # SciPy narrows index arrays that fit int32 when it builds a matrix
    ip, ix = np.ascontiguousarray(A.indptr, dtype=np.int64), np.ascontiguousarray(A.indices, dtype=np.int64)
    dv = np.ascontiguousarray(A.data)
    h = ctypes.c_void_p()
    _lib.check(_lib.lib.kry_csr_create(op.ctx.handle, op.n, op.nnz, _lib.ptr(ip), _lib.ptr(ix), _lib.ptr(dv),
                                       _lib.dtype_code(dv.dtype), _lib.KRY_I64, ctypes.byref(h)))
    op.handle = h
    op._fin = _lib.own(op, _lib.lib.kry_csr_destroy, h)
    op.renumbered = op.layout()["renumbered"]
    return op


def _operator(cfg, A):
    import krylov_amd

    op = _raw_operator(A) if cfg.index64 else krylov_amd.CsrOperator(A)
    lay = op.layout()
    for key, want in cfg.expect.items():
        if key == "classes":
            assert lay["dia_classes"] > 0 and lay["dia_class_cols"] > 0, lay
        elif key == "irregular_slices":
            assert lay["irregular"] > 0, lay
        elif key == "two_slice_waves":
            assert EC.dia_waves_walk_two(A)
        else:
            assert lay[key] == want, (key, lay)
    if cfg.form is not None:  # the k = 1 diagonal-offset kernel form, from the image's own counts
        from krylov_amd import _lib

        cols, uni = lay["dia_slots"] // 128, lay["dia_uniform_cols"]
        width = _lib.dia_plan(A.indptr, A.indices)["max_width"]
        got = (2 if uni == cols else (0 if uni == 0 else 1), 8 if uni == cols or width <= 8 else 16)
        assert got == cfg.form == EC.dia_form(A), (got, cfg.form)
        if "dia_classes" not in cfg.expect and "classes" not in cfg.expect:
            plan = _lib.dia_class_plan(A.indptr, A.indices, A.data)
            assert (lay["dia_classes"], lay["dia_class_cols"]) == (plan["classes"], plan["class_cols"])
    return op


def _problem(cfg, op, b, x0, w, **prec):
    from krylov_amd._helpers import Problem, WeightedInner

    V = cfg.vdtype
    inner = WeightedInner(w.astype(np.float64)) if cfg.weighted else None
    prob = Problem(op, b.astype(V), x0.astype(V), inner, **prec)
    assert prob.dtype == V and prob.kpad == cfg.k and prob.n == op.n
    return prob


def _never(prob):
    return np.full(prob.kpad, -1.0)  # a criterion no residual norm meets


def _scalar_type(cfg):
    """The type of the solve's inner products and scalar recurrences."""
    return np.float32 if (cfg.vdtype == np.float32 and not cfg.weighted) else np.float64


def _ldot_rows(A, x):
    """(A x, |A| |x|) per row in longdouble over the stored entries."""
    a = A.data.astype(np.longdouble)
    prod = a * x.astype(np.longdouble)[A.indices]
    lens = np.diff(A.indptr)
    starts = A.indptr[:-1][lens > 0].astype(np.int64)
    s = np.zeros(A.shape[0], dtype=np.longdouble)
    sa = np.zeros(A.shape[0], dtype=np.longdouble)
    s[lens > 0] = np.add.reduceat(prod, starts)
    sa[lens > 0] = np.add.reduceat(np.abs(prod), starts)
    return s, sa, int(lens.max())


def _scaled(ints, m, V):
    """ints / 2^m per column in V (exact: small integers, a power of two)."""
    return ints.astype(V) / np.array([2.0**e for e in m], dtype=V)[None, :]


def _check_cg(cfg, prob, ref, persist):
    from krylov_amd.cg import _CGState

    V, S, k = cfg.vdtype.type, _scalar_type(cfg), cfg.k
    r0 = ref.r0.astype(V)
    st = _CGState(prob)
    _bits(st.start(), np.array([float(4**m) for m in ref.m]), "cg start rho0")
    _bits(st.get(1), r0, "cg r0")
    st.set_criterion(_never(prob))
    hist = st.run(1)
    assert hist.shape == (1, k) and st.path()[0] == persist
    alpha = np.array([float(S(rho) / S(p)) for rho, p in zip(ref.rho0, ref.pAp)])  # pAp != 0: asserted on the host
    sc = st.scalars()
    _bits(sc[2], alpha, "cg alpha")
    t2 = alpha.astype(V)[None, :] * ref.Ar.astype(V)
    assert t2.dtype == r0.dtype
    _bits(st.get(1), r0 - t2, "cg r1 = r0 - alpha A r0")


def _check_gmres(cfg, prob, ref, A):
    from krylov_amd.gmres import _GmresState

    V, k, n = cfg.vdtype, cfg.k, prob.n
    v0 = ref.v0(V).reshape(n, k)
    g = _GmresState(prob, 2, 1)
    _bits(g.start(), np.array([2.0**m for m in ref.m]), "gmres start norm")
    _bits(g.get(1, out=np.empty((1, n, k), dtype=V))[0], v0, "gmres V0")
    g.set_criterion(_never(prob))
    hist, inv = g.run(1)
    assert hist.shape == (1, k) and not inv
    H = g.get(3, out=np.empty((3, 2, k)))
    _bits(H[0, 0], np.array([float(h) for h in ref.h00]), "gmres H[0,0]")
    # V1 = w' / h10 as the plain division pass forms it when the basis is read
    # before the next step (kry_gmres_get); the step still has it pending
    v1 = g.get(1, out=np.empty((2, n, k), dtype=V))[1].copy()
    # ... and as NumPy replays the Gram-Schmidt pass on the exact w = A V0 the
    # epilogue stored: w' = w - V(h00) V0, V1 = w' / V(h10), h10 the device's
    assert np.all(H[1, 0] != 0.0)
    av0 = _scaled(ref.Ar, ref.m, V)
    t = H[0, 0].astype(V)[None, :] * v0
    _bits(v1, (av0 - t) / H[1, 0].astype(V)[None, :], "gmres V1 = (A V0 - h00 V0) / h10")
    # step 2: A (w' / h10) gathered through SrcScaled, V1 stored by EpiStoreDotV
    hist, inv = g.run(1)
    assert hist.shape == (1, k) and not inv
    basis = g.get(1, out=np.empty((3, n, k), dtype=V))
    _bits(basis[0], v0, "gmres V0 after two steps")
    _bits(basis[1], v1, "gmres V1 as the step-2 SpMV stored it")
    H = g.get(3, out=np.empty((3, 2, k)))
    _dot_bound(cfg, A, x=basis[1], q=v0, w=ref.w, got=H[0, 1], what="gmres H[0,1]")


def _dot_bound(cfg, A, x, q, w, got, what, pold=None, h0=None):
    """|got - ref| <= (width + 2) eps_V sum_i |q_i| w_i (|A| |x|)_i, the
    reference in longdouble (with p_old: of <q, A x - h0 p_old>_w; the bound's
    sum stays that of the row sums alone)."""
    eps = float(np.finfo(cfg.vdtype).eps)
    worst = 0.0
    for c in range(cfg.k):
        s, sa, width = _ldot_rows(A, x[:, c])
        if pold is not None:
            s = s - np.longdouble(h0[c]) * pold[:, c].astype(np.longdouble)
        qw = q[:, c].astype(np.longdouble) * w.astype(np.longdouble)
        want = float((qw * s).sum())
        bound = (width + 2) * eps * float((np.abs(qw) * sa).sum())
        err = abs(float(got[c]) - want)
        assert np.isfinite(got[c]) and err <= bound, (what, c, float(got[c]), want, err, bound)
        worst = max(worst, err / bound if bound > 0 else 0.0)
    print(f"\n{cfg.id}: {what} uses {worst:.3g} of its bound")


def _check_minres(cfg, prob, ref, A):
    from krylov_amd.minres import _MinresState

    V, k, n = cfg.vdtype, cfg.k, prob.n
    v0 = ref.v0(V).reshape(n, k)
    m = _MinresState(prob)
    _bits(m.start(), np.array([2.0**e for e in ref.m]), "minres start norm")
    _bits(m.get(1), v0, "minres v0")
    m.set_criterion(_never(prob))
    hist, inv = m.run(1)
    assert hist.shape == (1, k) and not inv
    h = m.get(3, out=np.empty((3, k)))
    _bits(h[1], np.array([float(x) for x in ref.h00]), "minres h1")
    # the next Lanczos vector, replayed on the exact w = A v0 the epilogue
    # stored: (S(w) - alpha S(v0)) -> V, over V(h2) (OpLanczosOrtho and the
    # update pass, csrc/minres.hip); alpha = h1 and h2 are the device's
    S = _scalar_type(cfg)
    assert S == V  # the configurations keep one type for scalars and vectors
    v1, h0 = m.get(1), h[0].copy()
    assert np.all(h0 != 0.0) and np.array_equal(h0, h[2])
    av0 = _scaled(ref.Ar, ref.m, V)
    wv = av0 - h[1].astype(V)[None, :] * v0
    _bits(v1, wv / h[2].astype(V)[None, :], "minres v1 = (A v0 - h1 v0) / h2")
    # step 2: w = A v1 - h0 p_old with p_old = v0, on the device's own v1 and h0
    hist, inv = m.run(1)
    assert hist.shape == (1, k) and not inv
    h2 = m.get(3, out=np.empty((3, k)))
    # stored vectors stay bitwise: A v1 summed in stored order in V (SciPy's
    # csr_matvec(s), to which kry_spmv is held bitwise), minus V(h0) * p_old
    # as EpiLanczos forms it, then the same orthogonalisation and division
    o = (A @ v1).astype(V, copy=False) - h0.astype(V)[None, :] * v0
    assert o.dtype == V and np.all(h2[2] != 0.0)
    wv = o - h2[1].astype(V)[None, :] * v1
    _bits(m.get(1), wv / h2[2].astype(V)[None, :], "minres v2 = (A v1 - h0 v0 - h1 v1) / h2")
    _dot_bound(cfg, A, x=v1, q=v1, w=ref.w, got=h2[1], what="minres h1 (step 2)", pold=v0, h0=h0)


@pytest.mark.parametrize("cfg", EC.CONFIGS, ids=repr)
def test_epilogues_exact(cfg, monkeypatch):
    for name, value in cfg.env.items():
        monkeypatch.setenv(name, value)
    monkeypatch.setenv("KRY_CG_PERSIST", "0")
    A, b, x0, w, ref = cfg.problem()
    assert ref.exact_in(cfg.vdtype)
    op = _operator(cfg, A)
    prob = _problem(cfg, op, b, x0, w)
    _check_cg(cfg, prob, ref, persist=False)
    if cfg.persist:
        monkeypatch.setenv("KRY_CG_PERSIST", "2")  # an ineligible solve raises
        _check_cg(cfg, prob, ref, persist=True)
        monkeypatch.setenv("KRY_CG_PERSIST", "0")
    _check_gmres(cfg, prob, ref, A)
    _check_minres(cfg, prob, ref, A)


# ------------------------------------------------- matrix preconditioners
class _F64Weighted:
    """What the helpers above read of a configuration."""

    vdtype, weighted, k = np.dtype(np.float64), True, 1

    def __init__(self, id):
        self.id = id


@pytest.mark.parametrize("a,m", EC.PRECOND_PAIRS)
def test_preconditioner_epilogues_exact(a, m, monkeypatch):
    """Integer preconditioners on another image than A's: Ml r0 with its norm
    (EpiStoreNorm), z = M Ml r0 with <Ml r0, z>_w (EpiStoreDot) at start, and
    xk = x0 + Mr u in kry_gmres_solution (EpiAddStore)."""
    import krylov_amd
    from krylov_amd.cg import _CGState
    from krylov_amd.gmres import _GmresState

    monkeypatch.setenv("KRY_CG_PERSIST", "0")
    cfg = _F64Weighted(f"precond-{a}-{m}")
    Ai, Pi = EC.matrix(a), EC.matrix(m)
    A, P = EC.as_float(Ai, np.float64), EC.as_float(Pi, np.float64)
    b, x0, w = EC.rhs(Ai, 1, True, seed=5)
    ref = EC.Reference(Ai, b, x0, w)
    opA, opP = krylov_amd.CsrOperator(A), krylov_amd.CsrOperator(P)
    la, lp = opA.layout(), opP.layout()
    assert la["dia"] != lp["dia"] and (la["pair"] or lp["pair"]) and not la["renumbered"] and not lp["renumbered"]
    n = A.shape[0]
    mlr = EC.int_spmv(Pi, ref.r0)
    z = EC.int_spmv(Pi, mlr)
    # CG, Ml alone: Ml r0 and <Ml r0, Ml r0>_w
    st = _CGState(_problem(cfg, opA, b, x0, w, Ml=opP))
    _bits(st.start(), np.array([float(v) for v in EC.wdot(mlr, mlr, w)]), "cg start with Ml")
    _bits(st.get(1), mlr.astype(np.float64), "cg Ml r0")
    # CG, M and Ml: z = M Ml r0 and <Ml r0, z>_w
    st = _CGState(_problem(cfg, opA, b, x0, w, M=opP, Ml=opP))
    _bits(st.start(), np.array([float(v) for v in EC.wdot(mlr, z, w)]), "cg start with M and Ml")
    _bits(st.get(1), mlr.astype(np.float64), "cg Ml r0 under M")
    _bits(st.get(2), z.astype(np.float64), "cg M Ml r0")
    # GMRES, Ml alone: the norm's root is correctly rounded on both sides
    g = _GmresState(_problem(cfg, opA, b, x0, w, Ml=opP), 2, 1)
    nrm = np.sqrt(np.array([float(v) for v in EC.wdot(mlr, mlr, w)]))
    _bits(g.start(), nrm, "gmres start with Ml")
    _bits(g.get(1, out=np.empty((1, n, 1)))[0], mlr.astype(np.float64) / nrm, "gmres V0 with Ml")
    # GMRES, Mr: xk = x0 + Mr (yy V0) after one step. yy = y0 / R00 comes out
    # of the device's Givens rotation; the host forms it from the device's H
    # and accepts the neighbour within 2 ulps for which every bit of xk
    # agrees (a different yy changes the rounding of nearly every element).
    g = _GmresState(_problem(cfg, opA, b, x0, w, Mr=opP), 2, 1)
    beta = g.start()
    v0 = g.get(1, out=np.empty((1, n, 1)))[0]
    _bits(v0, ref.v0(np.float64).reshape(n, 1), "gmres V0 under Mr")
    g.set_criterion(np.full(1, -1.0))
    hist, inv = g.run(1)
    assert len(hist) == 1 and not inv
    H = g.get(3, out=np.empty((3, 2, 1)))
    h00, h10 = H[0, 0, 0], H[1, 0, 0]
    mrv = EC.int_spmv(Pi, ref.r0)
    amr = EC.int_spmv(Ai, mrv)
    _bits(H[0, 0], np.array([float(np.float64(EC.wdot(ref.r0, amr, w)[0]) / 4.0**ref.m[0])]), "gmres H[0,0] under Mr")
    g.solution()
    xk = g.get(0)
    yy = h00 * beta[0] / (h00 * h00 + h10 * h10)
    cands = [yy]
    lo = hi = yy
    for _ in range(2):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cands += [lo, hi]
    x0f = x0.astype(np.float64)
    hit = None
    for i, c in enumerate(cands):
        u = np.float64(c) * v0[:, 0]
        if np.array_equal((x0f + P @ u).view(np.uint64), xk[:, 0].view(np.uint64)):
            hit = i
            break
    print(f"\n{cfg.id}: xk = x0 + Mr (yy V0) bitwise with yy {0 if not hit else (hit + 1) // 2} ulps from the host's")
    assert hit is not None, "no yy within 2 ulps of h00 beta / (h00^2 + h10^2) reproduces xk bit for bit"
