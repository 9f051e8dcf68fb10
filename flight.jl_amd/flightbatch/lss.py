"""Model(lss) — a batch of LinearizedSS models stepped on the device (FP/linearization.jl:157-192; include/flightbatch.h: FB_MODEL_LSS;
kernels: csrc/lss_kernels.hpp; docs/design/linearize.md, "Model(lss) on the device").

    reference                                                            here
    Model(lss)                          FP/linearization.jl:157-162       LinearWorld(lss)                 (host LinearizedSS -> device)
    Model(subsystem(linearize(ac, trim); x, u, y))  :113-132, demos       linear_world(world, x=, u=, y=)  (device to device, after linearize(world, ...))
    f_ode!(mdl)                         :164-192                          f_ode(world)
    Simulation(mdl; dt) / step!         FC/sim.jl:183-255, 386            Simulation(world, dt=...) / step, or world.step(n)

X = copy(x0) and U = copy(u0): a new world sits at its linearisation point. The labels of the LinearizedSS travel with the world
(x_labels, u_labels, y_labels); the verbs and Simulation / TimeSeries of flightbatch.modeling work on it unchanged."""
from __future__ import annotations

import ctypes as C
import numpy as np

from ._lib import K, FlightBatchError, check, lib
from .linearization import LABELS, LinearizedSS, _index
from .modeling import BatchedWorld, _pd, _pi


def pack_matrix(m: np.ndarray) -> np.ndarray:
    """[N, rows, cols] -> the C ABI's flat block: element (i, r, c) at [(r + rows c) N + i] (include/flightbatch.h, linearize)"""
    m = np.asarray(m, dtype=np.float64)
    return np.ascontiguousarray(m.transpose(2, 1, 0)).reshape(-1)


def unpack_matrix(a: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """the inverse of pack_matrix: flat [(r + rows c) N + i] -> [N, rows, cols]"""
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(cols, rows, -1).transpose(2, 1, 0).copy()


def pack_model(lss: LinearizedSS) -> dict:
    """the eight blocks of a LinearizedSS as fb_linearize writes them (and fb_lss_set_model reads them): vectors [rows, N], matrices flat"""
    vec = lambda v: np.ascontiguousarray(np.asarray(v, dtype=np.float64).T)
    return dict(xdot0=vec(lss.xdot0), x0=vec(lss.x0), u0=vec(lss.u0), y0=vec(lss.y0),
                A=pack_matrix(lss.A), B=pack_matrix(lss.B), C=pack_matrix(lss.C), D=pack_matrix(lss.D))


class LinearWorld(BatchedWorld):
    """N independent Model(lss) on one GPU: x [nx, n], u [nu, n], y [ny, n] (the output record of the last f_ode)."""
    MODEL = "FB_MODEL_LSS"
    _CKPT_ARRAYS = ("x", "u")

    def __init__(self, lss: LinearizedSS | None = None, device: int = 0, _handle=None, _labels=None, Ts: float | None = None):
        """Ts: the LinearizedSS is a sampled model with that sample time, A holding Phi, B Gamma and xdot0 delta (fb_lss_set_sampled)"""
        self._h = C.c_void_p()
        if _handle is not None:      # linear_world(): the library has built the handle on the source's device
            self._h = _handle
            self.x_labels, self.u_labels, self.y_labels = _labels
        else:
            if lss is None:
                raise TypeError("LinearWorld: a LinearizedSS is required (or build it on the device with linear_world)")
            n, nx = np.asarray(lss.x0).shape
            nu, ny = np.asarray(lss.u0).shape[1], np.asarray(lss.y0).shape[1]
            check(lib.fb_lss_create(int(nx), int(nu), int(ny), int(n), int(device), C.byref(self._h)))
            b = pack_model(lss)
            check(lib.fb_lss_set_model(self._h, *[_pd(b[k]) for k in ("xdot0", "x0", "u0", "y0", "A", "B", "C", "D")]))
            if Ts is not None:
                check(lib.fb_lss_set_sampled(self._h, float(Ts)))
            self.x_labels, self.u_labels, self.y_labels = tuple(lss.x_labels), tuple(lss.u_labels), tuple(lss.y_labels)
        self.n = int(lib.fb_size(self._h))
        nx, nu, ny = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib.fb_dims(self._h, C.byref(nx), None, C.byref(nu), C.byref(ny)))
        self.nx, self.ns, self.nu, self.ny = nx.value, 0, nu.value, ny.value
        self.kinematics, self.dtype = None, "f64"
        self.t = 0.0
        self._Δt_root = 1.0
        self._n = 0
        self.squarings = None    # [N] on a world made by c2d: the squarings of each system's discretisation

    @property
    def Ts(self) -> float:
        """the sample time of a sampled world (flightbatch.c2d); 0.0 on a continuous one"""
        ts = C.c_double(-1.0)
        check(lib.fb_lss_sample_time(self._h, C.byref(ts)))
        return ts.value

    # -- mdl.x / mdl.u / mdl.y --
    def set_state(self, x, s=None):   # an INITIAL condition: restarts the clock and the step count (fb_set_state)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.nx, self.n)
        check(lib.fb_set_state(self._h, _pd(x), None))
        self.t = 0.0

    @property
    def s(self):
        return np.zeros((0, self.n), dtype=np.int32)

    @property
    def u(self):
        u = np.empty((self.nu, self.n))
        check(lib.fb_get_inputs(self._h, _pd(u), None))
        return u

    @u.setter
    def u(self, v):
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(self.nu, self.n)
        check(lib.fb_set_inputs(self._h, _pd(v), None))

    @property
    def y(self):
        y = np.empty((self.ny, self.n))
        check(lib.fb_get_outputs(self._h, _pd(y)))
        return y

    def model(self):
        """(A [n, nx, nx], B [n, nx, nu]): the handle's own copy of the model, the matrices the device steps and designs on (read-only);
        (Phi, Gamma) on a sampled world"""
        A, B = np.empty(self.nx * self.nx * self.n), np.empty(self.nx * self.nu * self.n)
        check(lib.fb_lss_get_model(self._h, _pd(A), _pd(B)))
        return unpack_matrix(A, self.nx, self.nx), unpack_matrix(B, self.nx, self.nu)

    def model_cd(self):
        """(C [n, ny, nx], D [n, ny, nu]): the output half of the handle's own copy of the model (read-only)"""
        Cm, D = np.empty(self.ny * self.nx * self.n), np.empty(self.ny * self.nu * self.n)
        check(lib.fb_lss_get_cd(self._h, _pd(Cm), _pd(D)))
        return unpack_matrix(Cm, self.ny, self.nx), unpack_matrix(D, self.ny, self.nu)

    @property
    def exchange(self) -> str:
        """"panel" or "shfl": how the stepper's lanes exchange stage values (FLIGHTBATCH_LSS_EXCHANGE when the handle was created)"""
        xch = C.c_int32(-1)
        check(lib.fb_lss_exchange(self._h, C.byref(xch)))
        return ("panel", "shfl")[xch.value]

    def f_ode(self, xdot: np.ndarray | None = None) -> np.ndarray | None:
        """f_ode!(mdl): refreshes y on the device; with `xdot` ([nx, n]) also returns the derivative"""
        check(lib.fb_f_ode(self._h, _pd(xdot) if xdot is not None else None))
        return xdot

    def step(self, nsteps: int = 1, dt: float | None = None, steps_per_launch: int | None = None) -> None:
        """nsteps of RK4 with u held (asynchronous), or of the map on a sampled world (whose dt is its Ts); dt and the steps fused per
        launch stay as last set"""
        if dt is not None:
            self.set_params(dt=float(dt))
        if steps_per_launch is not None:
            check(lib.fb_set_steps_per_launch(self._h, int(steps_per_launch)))
        check(lib.fb_step(self._h, int(nsteps)))
        self.t = float(lib.fb_time(self._h))

    # -- the on-device log (fb_log_*): output rows by label or index, state rows by label or index --
    def log_configure(self, every: int, capacity: int, y=(), x=()) -> None:
        rows = [self.y_labels.index(r) if isinstance(r, str) else int(r) for r in y]
        rows += [K["FB_LOG_X0"] + (self.x_labels.index(r) if isinstance(r, str) else int(r)) for r in x]
        self._log_rows = np.array(rows, dtype=np.int32)
        check(lib.fb_log_configure(self._h, int(every), int(capacity), _pi(self._log_rows), len(rows)))

    def log_read(self):
        """(t [m], data [m, rows, n]) of the samples recorded so far"""
        cnt = C.c_int64()
        check(lib.fb_log_count(self._h, C.byref(cnt)))
        t = np.zeros(cnt.value)
        data = np.zeros((cnt.value, len(self._log_rows), self.n))
        if cnt.value:
            check(lib.fb_log_read(self._h, 0, cnt.value, _pd(t), _pd(data)))
        return t, data

    def checkpoint(self):
        raise FlightBatchError("checkpoint: not defined for a LinearizedSS world (FB_MODEL_LSS): keep the LinearizedSS, x, u and t")

    def restore(self, ck):
        raise FlightBatchError("restore: not defined for a LinearizedSS world (FB_MODEL_LSS): keep the LinearizedSS, x, u and t")


def linear_world(world: BatchedWorld, x=None, u=None, y=None) -> LinearWorld:
    """Model(subsystem(lss; x, u, y)) with lss = the result of the last linearize(world, ...) / linearize_state(world), taken from the
    device where fb_linearize left it: nothing crosses PCIe. x, u, y: label tuples as subsystem() takes them (None: every variable)."""
    xl0, ul0, yl0 = LABELS[world.MODEL]
    xl, ul, yl = tuple(xl0 if x is None else x), tuple(ul0 if u is None else u), tuple(yl0 if y is None else y)
    arr = lambda labels, all_labels, what: np.array(_index(all_labels, labels, what), dtype=np.int32)
    ix, iu, iy = arr(xl, xl0, "state"), arr(ul, ul0, "input"), arr(yl, yl0, "output")
    h = C.c_void_p()
    check(lib.fb_lss_from_linearization(world._h, _pi(ix), len(ix), _pi(iu), len(iu), _pi(iy), len(iy), C.byref(h)))
    return LinearWorld(_handle=h, _labels=(xl, ul, yl))
