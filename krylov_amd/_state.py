"""The Python side of a solver core (csrc/solver_core.hpp): what ``_CGState``,
``_GmresState`` and ``_MinresState`` share. The C-ABI names of the three
cores differ only by their prefix, so the shared calls are looked up by it.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, lib


class CoreState:
    """One solver core on one problem: create, finaliser and preconditioners,
    and the calls every core has. A state is also the engine ``shard.drive``
    runs, after ``attach_comm``."""

    PREFIX = None  # "kry_cg" / "kry_gmres" / "kry_minres"
    PRECOND = ()  # the core's preconditioner slots, in slot order
    INVARIANT = True  # kry_*_run reports an invariant subspace

    def __init__(self, prob, *create_args):
        self.prob = prob
        self._ncols = prob.kpad
        h = ctypes.c_void_p()
        check(self._fn("create")(prob.ctx.handle, prob.A.handle, prob.kpad, _lib.dtype_code(prob.dtype),
                                 *create_args, ctypes.byref(h)))
        self.h = h
        self._fin = _lib.own(self, self._fn("destroy"), h)
        if prob.ops["Mr"] is not None and "Mr" not in self.PRECOND:
            raise TypeError(f"{self.PREFIX[4:]} has no right preconditioner Mr")
        prob.install_preconditioners(self._fn("set_preconditioners"), self._fn("set_precond"), h, *self.PRECOND)

    def _fn(self, name):
        return getattr(lib, f"{self.PREFIX}_{name}")

    def _pair(self, name):
        info = (ctypes.c_int32 * 2)()
        check(self._fn(name)(self.h, info))
        return int(info[0]), int(info[1])

    def start(self, x0_dev=None):
        """r0 = b - A x0 on the device; x0 = the problem's own x0 or, for a
        restart chain, ``x0_dev`` (a DeviceVector of the solve's shape).
        Returns the core's kpad start values (CG: squared norms)."""
        p = self.prob
        out = np.zeros(p.kpad)
        x0 = x0_dev if x0_dev is not None else p.x0_dev
        check(self._fn("start")(self.h, p.b_dev.handle, x0.handle if x0 is not None else None,
                                p.w_dev.handle if p.w_dev else None, _lib.dptr(out)))
        return out

    def start_norms(self):
        """start() as the kpad initial residual norms (float64)."""
        return self.start()

    def set_criterion(self, crit):
        crit = np.ascontiguousarray(crit, dtype=np.float64)
        check(self._fn("set_criterion")(self.h, _lib.dptr(crit)))

    def attach_comm(self, comm, layout):
        """Run as rank ``layout.rank`` of a sharded solve: one allreduce per
        step, the global stop rule, history rows of ``layout.total`` columns."""
        check(self._fn("attach_comm")(self.h, comm.handle, layout.off, layout.total))
        self._ncols = layout.total

    def run(self, steps, ncols=None):
        """Up to ``steps`` steps: (history rows of the steps done, invariant)."""
        out = np.zeros((max(steps, 1), self._ncols if ncols is None else ncols))
        done, inv = ctypes.c_int32(), ctypes.c_int32()
        tail = (ctypes.byref(inv),) if self.INVARIANT else ()
        check(self._fn("run")(self.h, int(steps), ctypes.byref(done), _lib.dptr(out), *tail))
        return out[: done.value], bool(inv.value)

    def residual_norm2(self):
        out = np.zeros(self.prob.kpad)
        check(self._fn("residual")(self.h, _lib.dptr(out)))
        return out

    def get(self, which, out=None):
        """Device array ``which`` of the core into ``out`` (default: a new
        n x kpad block of the solve's dtype; the caller sizes any other)."""
        p = self.prob
        if out is None:
            out = np.empty((p.n, p.kpad), dtype=p.dtype)
        assert out.flags.c_contiguous
        check(self._fn("get")(self.h, which, _lib.ptr(out)))
        return out

    def xk(self, out=None):
        p = self.prob
        assert out is None or (out.shape == (p.n, p.kpad) and out.dtype == p.dtype)
        return p.unpad_vec(self.get(0, out), p.r0_dtype)
