"""fb_attach_state and fb_set_stream: a handle whose state lives in the CALLER's device memory and whose work runs on the CALLER's stream,
held bit for bit to the same sequence on a handle that keeps its own buffers and its own stream (the path tests/test_gpu_dispatch_matrix.py
holds to the oracle, instance by instance). This is the arrangement bench.py measures and the one a torch or Julia host uses.

The caller's memory and streams come from ctypes on the HIP runtime (support.Hip), never from torch in this process. Every caller buffer is one
allocation with a guard row in front of and behind the rows the header promises, filled with the byte 0xA5 (support.GuardedRows); every test ends
by asserting that the guards are unchanged, so an overrun is a red test.

The batch: N = 357 = 256 + 64 + 37 aircraft (a full workgroup, a lone wave, a partial wave) trimmed over a runway (support.runway_batch), three
groups mixed within every wave: airborne throughout, descending through the 10 m band of the air / ground hand-over, sinking onto the wheels.
The run: 200 steps of dt = 0.01 (Cessna172Xv2: Δt = 2 dt), cut as 50 + 7 x 7 + 1 + 100 at 50, 7, 1 and 50 steps per launch. The coverage
(lanes that never enter the band, lanes that do, lanes within 4 m of the terrain) is counted on the owned run's logged height and asserted.

    1. the attached run is the owned run: state, outputs, status, termination record, control-law record, clock and the device log after
       every cut; the raw buffer against the layout of include/flightbatch.h (written here from the header's words); attach and detach copy
       nothing and leave the clock, the status words and the inputs alone
    2. the kinematic rows a mechanisation does not use: fb_attach_state zeroes them (the kernels carry them through every launch and test them
       for finiteness: a NaN left there by torch.empty would freeze the aircraft with FB_ST_NAN)
    3. the derivative Cessna172Xv2 carries from launch to launch: switching buffers, and a device-side write announced by attaching again
    4. stream order with no host synchronisation between the caller's work and fb_step; fb_set_stream(NULL) waits; timing on a caller's stream
    5. LinearizedSS and Robot2D handles on a caller's stream; what fb_attach_state refuses
    6. a buffer that is a view: x 8-byte aligned, s 4-byte aligned (every access to the state rows is one element wide); less is refused
    7. the benchmark's own arrangement with torch tensors, once, in a child process
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import textwrap

import numpy as np
import pytest

from support import (HIP_NOT_READY, ROOT, RUNWAY_BAND, RUNWAY_H_TRN, GuardedRows, Hip, clock, geoid, h_e_row_abi, make_lss, random_env, runway_batch,
                     same, stepper)

pytestmark = pytest.mark.gpu

N = 357
DT = 0.01
CUTS = [(50, 50)] + [(7, 7)] * 7 + [(1, 1), (50, 100)]      # (steps per launch, steps of the fb_step call): 200 steps in all
SCRATCH_BYTES = 256 << 20                                    # the block whose device-to-device copies delay a stream
MAX_DELAY_COPIES = 8                                         # 2 GB moved


class Case:
    def __init__(self, model, kin, duo, dtype="f64", env=False):
        self.model, self.kin, self.duo, self.dtype, self.env = model, kin, duo, dtype, env
        self.ratio = 2 if model == "x2" else 1
        self.key = (model, kin, duo, dtype, env)
        self.id = f"{model}-{kin}-{'duo' if duo else 'air'}" + ("-f32" if dtype == "f32" else "") + ("-env" if env else "")


@pytest.fixture(scope="module")
def hip():
    return Hip()


def check(fb, rc):
    assert rc == 0, fb.lib.fb_last_error().decode()


# ---- the device layout, from the words of include/flightbatch.h (fb_attach_state) and its FB_X2_* constants ------------------------------------
def device_rows(K, model, kin):
    """(device row of every row of the C ABI's state, rows the mechanisation leaves unused, device row count)"""
    n_kin = {"WA": 9, "ECEF": 8, "NED": 6}[kin]
    # Cessna172Sv0: rows 0-11 as they are, the mechanisation's kinematic states from row 12 on, w_eb_b and v_eb_b in rows 21-26
    sv0 = list(range(12)) + [12 + j for j in range(n_kin)] + list(range(21, 27))
    unused = list(range(12 + n_kin, 21))
    if model == "s0":
        return np.array(sv0), unused, K["FB_NX"]
    # Cessna172Xv2: the Sv0 rows first, the seven actuator positions in rows 27-33; the C ABI has the actuators at FB_X2_ACT, ahead of the
    # kinematic states at FB_X2_KIN
    assert K["FB_X2_KIN"] - K["FB_X2_ACT"] == K["FB_NACT"] == 7 and K["FB_X2_ACT"] == 12 and K["FB_X2_NX"] == K["FB_NX"] + K["FB_NACT"]
    return np.array(sv0[:K["FB_X2_ACT"]] + [K["FB_NX"] + j for j in range(K["FB_NACT"])] + sv0[K["FB_X2_ACT"]:]), unused, K["FB_X2_NX"]


def to_device(K, model, kin, x):
    rows, _, nxd = device_rows(K, model, kin)
    raw = np.zeros((nxd, x.shape[1]))
    raw[rows] = x
    return raw


# ---- worlds, start states, the cut run ----------------------------------------------------------------------------------------------------------
def make_world(fb, case, n=N):
    with stepper(case.duo):
        w = fb.Cessna172Xv2World(n, kinematics=case.kin) if case.model == "x2" else fb.BatchedWorld(n, kinematics=case.kin, dtype=case.dtype)
    w.set_params(dt=DT, periodic_n=case.ratio, h_terrain=RUNWAY_H_TRN)
    if case.env:
        w.env = random_env(fb, n, seed=5, h_trn=RUNWAY_H_TRN)
    return w


_START = {}


def start_state(fb, oracle, model, kin):
    """trimmed once per (model, mechanisation); every handle gets it through fb_set_state"""
    if (model, kin) not in _START:
        N0 = geoid(oracle, np.zeros(1), np.zeros(1))[0]
        tp, groups, set_cu = runway_batch(fb, N0, N)
        for g in groups.values():   # the three groups are mixed within every wave
            assert all(g[k:k + 64].any() for k in range(0, N, 64))
        w = make_world(fb, Case(model, kin, True))
        fb.f_init(w, tp)
        assert w.trim_success.all(), f"{int((~w.trim_success).sum())} aircraft did not trim"
        st = dict(x=w.x, s=w.s, u=w.u, ui=w.ui)
        if model == "x2":
            w.cu = set_cu(w.cu)
            st.update(cs=w.cs, cu=w.cu)
        w.close()
        _START[model, kin] = st
    return _START[model, kin]


def other_state(fb, case, st):
    """a perturbed other state of the batch (WA): 0.2 % faster, a quarter of a metre higher"""
    x = st["x"].copy()
    x[-3:] *= 1.002
    x[h_e_row_abi(fb.K, case.model, case.kin)] += 0.25
    return x, st["s"].copy()


def load_start(fb, w, st):
    w.set_state(st["x"], st["s"])
    w.u = st["u"]; w.ui = st["ui"]
    if "cs" in st:
        w.cs = st["cs"]; w.cu = st["cu"]


def step(fb, w, spl, steps):
    check(fb, fb.lib.fb_set_steps_per_launch(w._h, spl))
    check(fb, fb.lib.fb_step(w._h, steps))


def configure_log(fb, w):
    """the orthometric height (an output row: the log refreshes y) and every state row, recorded by hand behind every cut"""
    K = fb.K
    rows = np.array([K["FB_Y_KIN"] + 21] + [K["FB_LOG_X0"] + k for k in range(w.nx)], dtype=np.int32)
    check(fb, fb.lib.fb_log_configure(w._h, 1 << 62, len(CUTS) + 1, rows.ctypes.data_as(C.POINTER(C.c_int32)), rows.size))
    return rows.size


def snapshot(fb, w):
    check(fb, fb.lib.fb_log_record(w._h))
    tstep, twhere = w.termination
    d = dict(x=w.x, s=w.s, y=w.y, status=w.status, tstep=tstep, twhere=twhere, clock=np.array(clock(fb, w)))
    if hasattr(w, "cs"):
        d["cs"] = w.cs
    return d


def read_log(fb, w, nrows):
    cnt = C.c_int64()
    check(fb, fb.lib.fb_log_count(w._h, C.byref(cnt)))
    t, data = np.zeros(cnt.value), np.zeros((cnt.value, nrows, w.n))
    check(fb, fb.lib.fb_log_read(w._h, 0, cnt.value, t.ctypes.data_as(C.POINTER(C.c_double)), data.ctypes.data_as(C.POINTER(C.c_double))))
    return dict(t=t, data=data)


def run_cuts(fb, w):
    """the 200 steps from the state the handle holds; a snapshot at the start and behind every cut, and the log"""
    nrows = configure_log(fb, w)
    snaps = [snapshot(fb, w)]
    for spl, steps in CUTS:
        step(fb, w, spl, steps)
        snaps.append(snapshot(fb, w))
    assert snaps[-1]["clock"][1] == 200 and abs(snaps[-1]["clock"][0] - 200 * DT) < 1e-12
    return snaps, read_log(fb, w, nrows)


def assert_same_snapshots(a, b, label):
    (sa, la), (sb, lb) = a, b
    assert len(sa) == len(sb) == len(CUTS) + 1
    for k, (p, q) in enumerate(zip(sa, sb)):
        for key in p:
            assert same(p[key], q[key]), (label, f"cut {k}", key, np.flatnonzero((np.atleast_2d(p[key]) != np.atleast_2d(q[key])).any(0))[:8])
    assert same(la["t"], lb["t"]) and same(la["data"], lb["data"]), (label, "the device log differs")


_OWNED = {}


def owned_run(fb, oracle, case):
    """the reference: the same sequence on a handle that keeps its own buffers and its own stream; its coverage is asserted here"""
    if case.key not in _OWNED:
        st = start_state(fb, oracle, case.model, case.kin)
        w = make_world(fb, case)
        load_start(fb, w, st)
        snaps, log = run_cuts(fb, w)
        w.close()
        clr = log["data"][:, 0, :] - RUNWAY_H_TRN      # height over the terrain at the start and behind every cut
        lo = clr.min(0)
        stay, enter, near = int((lo > RUNWAY_BAND).sum()), int((lo < RUNWAY_BAND).sum()), int((lo < 4.0).sum())
        print(f"{case.id}: {stay} aircraft never below the {RUNWAY_BAND:g} m band, {enter} below it, {near} within 4 m of the terrain; "
              f"{int((snaps[-1]['status'] != 0).sum())} with a status word")
        assert stay >= 16 and enter >= 16 and near >= 8, (case.id, stay, enter, near)
        assert not same(snaps[0]["x"], snaps[-1]["x"])
        _OWNED[case.key] = (snaps, log)
    return _OWNED[case.key]


class Caller:
    """the caller's side of fb_attach_state: guarded x and s buffers in the device layout, optionally views at a byte offset"""
    def __init__(self, fb, hip, case, offset=(0, 0), fill=0.0):
        self.fb, self.case = fb, case
        self.rows, self.unused, self.nxd = device_rows(fb.K, case.model, case.kin)
        self.xb = GuardedRows(hip, self.nxd, N, np.float64, offset[0], fill)
        self.sb = GuardedRows(hip, fb.K["FB_NS"], N, np.int32, offset[1], 0)

    def attach(self, w):
        check(self.fb, self.fb.lib.fb_attach_state(w._h, C.c_void_p(self.xb.ptr), C.c_void_p(self.sb.ptr)))

    def put(self, x, s):
        """a state written by the caller, straight into the buffers"""
        self.xb.write(to_device(self.fb.K, self.case.model, self.case.kin, x))
        self.sb.write(s)

    def assert_raw_is(self, x, s, label):
        raw = self.xb.read()
        assert same(raw[self.rows], x), (label, "the raw buffer is not the state in the header's layout")
        assert (raw[self.unused] == 0.0).all() and not np.signbit(raw[self.unused]).any(), (label, "the unused kinematic rows are not zero")
        assert same(self.sb.read(), s), (label, "the raw s buffer")

    def close(self, label):
        ok = self.xb.guards_intact(), self.sb.guards_intact()
        self.xb.free(); self.sb.free()
        assert ok == (True, True), (label, "a guard row was written", ok)


def attached_run(fb, hip, case, st, label, offset=(0, 0), fill=0.0, stream=None, switches=False):
    """the cut run on the caller's buffers (and stream); with `switches`, what attach and detach do to the handle is checked on the way"""
    K = fb.K
    w = make_world(fb, case)
    cal = Caller(fb, hip, case, offset, fill)
    try:
        load_start(fb, w, st)
        if switches:
            # the handle's own buffers hold a state of their own; the clock, a status word and a termination record are set
            own_x = st["x"].copy(); own_x[h_e_row_abi(K, case.model, case.kin)] += 300.0
            w.x = own_x
            check(fb, fb.lib.fb_set_step_count(w._h, 3, 3 * DT))
            word = np.zeros(N, np.int32); word[5] = K["FB_ST_NAN"]; word[7] = K["FB_ST_GROUND_CRASH"]
            check(fb, fb.lib.fb_set_status(w._h, word.ctypes.data_as(C.POINTER(C.c_int32))))
            own_s = w.s
            host = lambda: (clock(fb, w), w.status, w.termination, w.u, w.ui)
            before = host()
            assert before[0] == (3 * DT, 3) and before[1][5] != 0 and before[2][0][7] == 3
            pat_x = 0.5 + np.arange(cal.nxd * N, dtype=np.float64).reshape(cal.nxd, N)
            pat_s = np.arange(K["FB_NS"] * N, dtype=np.int32).reshape(K["FB_NS"], N)
            cal.xb.write(pat_x); cal.sb.write(pat_s)
        cal.attach(w)
        if switches:
            # attach copies nothing: the handle holds what the caller's buffer held, the host-side record is as it was
            assert same(w.x, pat_x[cal.rows]) and same(w.s, pat_s), (label, "fb_get_state after attach is not the caller's buffer")
            assert all(same(np.asarray(a), np.asarray(b)) for a, b in zip(_flat(before), _flat(host()))), (label, "attach changed the clock, status or inputs")
            raw = cal.xb.read()
            assert same(raw[cal.rows], pat_x[cal.rows]) and (raw[cal.unused] == 0.0).all(), (label, "attach wrote the rows in use, or left the unused ones")
        else:
            assert (cal.xb.read()[cal.unused] == 0.0).all(), (label, "fb_attach_state left the unused kinematic rows as the caller had them")
        if stream is not None:
            check(fb, fb.lib.fb_set_stream(w._h, C.c_void_p(stream)))
        load_start(fb, w, st)
        cal.assert_raw_is(st["x"], st["s"], label + ", after fb_set_state")
        got = run_cuts(fb, w)
        cal.assert_raw_is(got[0][-1]["x"], got[0][-1]["s"], label + ", at the end")
        if stream is not None:
            check(fb, fb.lib.fb_set_stream(w._h, None))
        if switches:
            before = host()
            check(fb, fb.lib.fb_attach_state(w._h, None, None))
            # detach copies nothing either: the handle's own buffers are as they were before the attach — no kernel wrote them meanwhile
            assert same(w.x, own_x) and same(w.s, own_s), (label, "the handle's own buffers changed while the caller's were attached")
            assert all(same(np.asarray(a), np.asarray(b)) for a, b in zip(_flat(before), _flat(host()))), (label, "detach changed the clock, status or inputs")
            cal.assert_raw_is(got[0][-1]["x"], got[0][-1]["s"], label + ", after detach")
    finally:
        w.close()
        cal.close(label)
    return got


def _flat(rec):
    (t, cnt), status, (tstep, twhere), u, ui = rec
    return [np.array([t, cnt]), status, tstep, twhere, u, ui]


# ---- 1. the attached run is the owned run -------------------------------------------------------------------------------------------------------
CASES_1 = ([Case(m, k, d) for m in ("s0", "x2") for k in ("WA", "ECEF", "NED") for d in (True, False)] +
           [Case("s0", "WA", True, dtype="f32"), Case("s0", "WA", True, env=True)])
assert len(CASES_1) == 14


@pytest.mark.parametrize("case", CASES_1, ids=[c.id for c in CASES_1])
def test_attached_run_is_the_owned_run(fb, oracle, hip, case):
    ref = owned_run(fb, oracle, case)
    got = attached_run(fb, hip, case, start_state(fb, oracle, case.model, case.kin), case.id, switches=True)
    assert_same_snapshots(got, ref, case.id)


# ---- 2. the rows a mechanisation does not use ---------------------------------------------------------------------------------------------------
CASES_2 = [Case(m, k, d) for m in ("s0", "x2") for k in ("ECEF", "NED") for d in (True, False)]


@pytest.mark.parametrize("fill", [1e300, np.nan], ids=["1e300", "nan"])
@pytest.mark.parametrize("case", CASES_2, ids=[c.id for c in CASES_2])
def test_unused_rows_of_a_callers_buffer_are_zeroed_by_attach(fb, oracle, hip, case, fill):
    """k_step_air, k_f_ode and the write-back of every stepping kernel load and store all FB_NX rows of every mechanisation: the rows ECEF and NED
    leave unused get a zero derivative, travel through every launch and take part in the finiteness test behind it. So fb_attach_state zeroes
    them in a caller's buffer (the handle's own are zeroed at creation): attached_run asserts the zeros after the attach and at the end."""
    ref = owned_run(fb, oracle, case)
    label = f"{case.id}, buffer filled with {fill}"
    got = attached_run(fb, hip, case, start_state(fb, oracle, case.model, case.kin), label, fill=fill)
    assert_same_snapshots(got, ref, label)


# ---- 3. the carried derivative ------------------------------------------------------------------------------------------------------------------
def _twin_with_assignment(fb, case, st, x2, s2):
    """step 50, the new state through fb_assign_state, step 50 — on a handle that keeps its own buffers"""
    w = make_world(fb, case)
    load_start(fb, w, st)
    step(fb, w, 50, 50)
    check(fb, fb.lib.fb_assign_state(w._h, x2.ctypes.data_as(C.POINTER(C.c_double)), s2.ctypes.data_as(C.POINTER(C.c_int32))))
    step(fb, w, 50, 50)
    out = end_state(fb, w)
    w.close()
    return out


def end_state(fb, w):
    w.sync()
    d = dict(x=w.x, s=w.s, status=w.status, clock=np.array(clock(fb, w)))
    if hasattr(w, "cs"):
        d["cs"] = w.cs
    return d


def assert_same_end(a, b, label):
    for key in a:
        assert same(a[key], b[key]), (label, key, np.flatnonzero((np.atleast_2d(a[key]) != np.atleast_2d(b[key])).any(0))[:8])


@pytest.mark.parametrize("how", ["another-buffer", "device-write"])
@pytest.mark.parametrize("duo", [True, False], ids=["duo", "air"])
def test_x2_carried_derivative_across_a_change_of_state(fb, oracle, hip, duo, how):
    """Cessna172Xv2 carries k1 / k1_valid from one launch to the next (the ground-capable pass under either stepper). A state that arrives
    without the library's doing — in another buffer, or written into the attached one on the device — must not be stepped from the old
    derivative: fb_attach_state invalidates it, and attaching the same pointers again is how a caller announces its own writes."""
    case = Case("x2", "WA", duo)
    st = start_state(fb, oracle, "x2", "WA")
    x2, s2 = other_state(fb, case, st)
    label = f"{case.id}, {how}"
    ref = _twin_with_assignment(fb, case, st, x2, s2)
    assert not same(ref["x"], x2)
    w = make_world(fb, case)
    A, B = Caller(fb, hip, case), Caller(fb, hip, case)
    try:
        A.attach(w)
        load_start(fb, w, st)
        step(fb, w, 50, 50)
        w.sync()
        B.put(x2, s2)
        if how == "another-buffer":
            B.attach(w)
            final = B
        else:
            hip.copy(A.xb.ptr, B.xb.ptr, A.xb.nbytes)     # device to device, behind the steps (the handle was synchronised)
            hip.copy(A.sb.ptr, B.sb.ptr, A.sb.nbytes)
            A.attach(w)                                   # the same pointers again: "x and s were written"
            final = A
        step(fb, w, 50, 50)
        got = end_state(fb, w)
        final.assert_raw_is(got["x"], got["s"], label)
        assert_same_end(got, ref, label)
    finally:
        w.close()
        A.close(label); B.close(label)


# ---- 4. stream order ----------------------------------------------------------------------------------------------------------------------------
class Delay:
    """device-to-device copies of a 256 MB block, queued on a stream to keep it busy while the host goes on"""
    def __init__(self, hip):
        self.hip = hip
        self.src, self.dst = hip.malloc(SCRATCH_BYTES), hip.malloc(SCRATCH_BYTES)
        hip.memset(self.src, 1, SCRATCH_BYTES)
        hip.device_sync()

    def queue(self, stream, copies):
        for _ in range(copies):
            self.hip.copy_async(self.dst, self.src, SCRATCH_BYTES, stream)
        return self.hip.event(stream)

    def free(self):
        self.hip.free(self.src); self.hip.free(self.dst)


def behind_unfinished_work(hip, delay, stream, queue_work, reset):
    """queue_work() behind a delay on `stream`, with no synchronisation; the number of copies is doubled until the event behind the delay is
    still pending when queue_work has returned. Returns what queue_work returned for that attempt (the stream is left unsynchronised)."""
    copies = 1
    while True:
        reset()
        ev = delay.queue(stream, copies)
        out = queue_work()
        pending = hip.query(ev) == HIP_NOT_READY
        if pending:
            return out, ev
        hip.stream_sync(stream)
        hip.event_destroy(ev)
        assert copies < MAX_DELAY_COPIES, "precondition: 2 GB of copies queued ahead were done before the work behind them was queued"
        copies *= 2


@pytest.mark.parametrize("duo", [True, False], ids=["duo", "air"])
def test_step_is_ordered_on_the_callers_stream(fb, oracle, hip, duo):
    """On the caller's stream S, with no host synchronisation anywhere between: a delay, a device-to-device copy of a new state into the
    attached buffers, fb_step, a copy of the state out, an event. The step was queued behind unfinished work (asserted), must see the state
    copied in front of it, and the copy behind it must see its result. One launch or copy on another stream breaks either."""
    case = Case("s0", "WA", duo)
    st = start_state(fb, oracle, "s0", "WA")
    x2, s2 = other_state(fb, case, st)
    w = make_world(fb, case)
    load_start(fb, w, st)
    w.x = x2; w.s = s2
    step(fb, w, 50, 50)
    ref = end_state(fb, w)
    w.close()
    assert not same(ref["x"], x2)

    S = hip.stream()
    delay = Delay(hip)
    w = make_world(fb, case)
    cal, new, res = Caller(fb, hip, case), Caller(fb, hip, case), Caller(fb, hip, case)
    try:
        cal.attach(w)
        check(fb, fb.lib.fb_set_stream(w._h, C.c_void_p(S)))
        new.put(x2, s2)
        check(fb, fb.lib.fb_set_steps_per_launch(w._h, 50))

        def work():
            hip.copy_async(cal.xb.ptr, new.xb.ptr, cal.xb.nbytes, S)
            hip.copy_async(cal.sb.ptr, new.sb.ptr, cal.sb.nbytes, S)
            check(fb, fb.lib.fb_step(w._h, 50))

        _, ev = behind_unfinished_work(hip, delay, S, work, reset=lambda: load_start(fb, w, st))
        hip.copy_async(res.xb.ptr, cal.xb.ptr, cal.xb.nbytes, S)
        hip.copy_async(res.sb.ptr, cal.sb.ptr, cal.sb.nbytes, S)
        done = hip.event(S)
        hip.stream_sync(S)
        assert hip.query(ev) == 0 and hip.query(done) == 0
        res.assert_raw_is(ref["x"], ref["s"], case.id + ", the copy queued behind the step")
        assert_same_end(end_state(fb, w), ref, case.id)
        hip.event_destroy(ev); hip.event_destroy(done)
        check(fb, fb.lib.fb_set_stream(w._h, None))
    finally:
        w.close()
        for b in (cal, new, res):
            b.close(case.id)
        delay.free()
        hip.stream_destroy(S)


CASES_4 = [Case(m, "WA", d) for m in ("s0", "x2") for d in (True, False)]


@pytest.mark.parametrize("case", CASES_4, ids=[c.id for c in CASES_4])
def test_whole_run_on_the_callers_stream(fb, oracle, hip, case):
    ref = owned_run(fb, oracle, case)
    S = hip.stream()
    try:
        got = attached_run(fb, hip, case, start_state(fb, oracle, case.model, case.kin), case.id + " on a caller's stream", stream=S)
    finally:
        hip.stream_destroy(S)
    assert_same_snapshots(got, ref, case.id + " on a caller's stream")


@pytest.mark.parametrize("duo", [True, False], ids=["duo", "air"])
def test_leaving_the_callers_stream_waits_for_it_and_timing_works_on_it(fb, oracle, hip, duo):
    """fb_set_stream(h, NULL) returns once what was queued on the caller's stream is done, and the handle goes on stepping on its own stream
    with the owned bits; fb_timing_begin / fb_timing_end on the caller's stream count ceil(steps / steps per launch) launches"""
    case = Case("s0", "WA", duo)
    st = start_state(fb, oracle, "s0", "WA")
    w = make_world(fb, case)
    load_start(fb, w, st)
    step(fb, w, 50, 100)
    mid = end_state(fb, w)
    step(fb, w, 50, 50)
    step(fb, w, 7, 50)
    ref = end_state(fb, w)
    w.close()

    S = hip.stream()
    delay = Delay(hip)
    w = make_world(fb, case)
    cal = Caller(fb, hip, case)
    try:
        cal.attach(w)
        check(fb, fb.lib.fb_set_stream(w._h, C.c_void_p(S)))
        load_start(fb, w, st)
        check(fb, fb.lib.fb_set_steps_per_launch(w._h, 50))
        check(fb, fb.lib.fb_timing_begin(w._h))
        check(fb, fb.lib.fb_step(w._h, 100))
        ms, nl = C.c_float(), C.c_int64()
        check(fb, fb.lib.fb_timing_end(w._h, C.byref(ms), C.byref(nl)))
        assert nl.value == 2 and ms.value > 0.0, (nl.value, ms.value)
        assert_same_end(end_state(fb, w), mid, case.id + ", timed on the caller's stream")

        _, ev = behind_unfinished_work(hip, delay, S, lambda: check(fb, fb.lib.fb_step(w._h, 50)), reset=lambda: (load_start(fb, w, st), step(fb, w, 50, 100), w.sync()))
        behind = hip.event(S)
        check(fb, fb.lib.fb_set_stream(w._h, None))
        assert hip.query(ev) == 0 and hip.query(behind) == 0, "fb_set_stream(NULL) returned while work was pending on the caller's stream"
        hip.event_destroy(ev); hip.event_destroy(behind)
        step(fb, w, 7, 50)                      # on the handle's own stream now, the state still in the caller's buffers
        got = end_state(fb, w)
        cal.assert_raw_is(got["x"], got["s"], case.id)
        assert_same_end(got, ref, case.id + ", back on its own stream")
    finally:
        w.close()
        cal.close(case.id)
        delay.free()
        hip.stream_destroy(S)


# ---- 5. the other models ------------------------------------------------------------------------------------------------------------------------
def _runs_behind(fb, hip, delay, S, w, queue_step, reset):
    """the handle's work is ordered on S: queued behind a delay there, fb_sync on the handle returns only once the delay is through"""
    _, ev = behind_unfinished_work(hip, delay, S, queue_step, reset)
    check(fb, fb.lib.fb_sync(w._h))
    assert hip.query(ev) == 0, "fb_sync returned before the caller's stream had drained: the handle does not run on it"
    hip.event_destroy(ev)


def _linear_chain(fb, hip, S, delay):
    """fb_linearize -> fb_lss_from_linearization -> fb_lss_c2d -> 100 steps of the map, n = 63"""
    n = 63
    ac = fb.BatchedWorld(n, kinematics="NED")
    if S is not None:
        check(fb, fb.lib.fb_set_stream(ac._h, C.c_void_p(S)))
    lss = fb.linearize(ac, fb.TrimParameters(EAS=np.linspace(38.0, 55.0, n), h_e=np.linspace(300.0, 2500.0, n)))
    assert lss.success.all() and (lss.status == 0).all()
    lw = fb.linear_world(ac)
    res = fb.c2d(lw, 0.01)
    assert res.ok.all()
    d = res.world
    x0, u0 = d.x, d.u
    rng = np.random.default_rng(63)
    xs, us = x0 + 0.01 * rng.standard_normal(x0.shape), u0 + 0.01 * rng.standard_normal(u0.shape)

    def reset():
        d.set_state(xs); d.u = us

    if S is not None:   # a handle made from a source on a caller's stream runs on it, and so does the one made from that
        _runs_behind(fb, hip, delay, S, d, lambda: d.step(100, steps_per_launch=50), reset)
    else:
        reset(); d.step(100, steps_per_launch=50)
    d.f_ode(); d.sync()
    out = dict(x=d.x, y=d.y, clock=np.array(clock(fb, d)), A=lss.A, B=lss.B, phi=d.model()[0], squarings=res.squarings)
    for w in (d, lw, ac):
        w.close()
    return out


def _robot2d_run(fb, hip, S, delay):
    n = 63
    w = fb.Robot2DWorld(n)
    if S is not None:
        check(fb, fb.lib.fb_set_stream(w._h, C.c_void_p(S)))
    w.set_params(dt=0.01, periodic_n=2)
    u = w.u; u[2] = np.linspace(-0.5, 0.5, n)

    def reset():
        fb.f_init(w, fb.InitParameters(u_m=np.linspace(-0.05, 0.05, n)))
        w.u = u

    def go():
        step(fb, w, 50, 100)

    if S is not None:
        _runs_behind(fb, hip, delay, S, w, go, reset)
    else:
        reset(); go()
    w.sync()
    out = dict(x=w.x, status=w.status, clock=np.array(clock(fb, w)))
    w.close()
    return out


@pytest.mark.parametrize("run", [_linear_chain, _robot2d_run], ids=["linear-chain", "robot2d"])
def test_other_models_on_a_callers_stream(fb, hip, run):
    ref = run(fb, hip, None, None)
    S = hip.stream()
    delay = Delay(hip)
    try:
        got = run(fb, hip, S, delay)
    finally:
        delay.free()
        hip.stream_destroy(S)
    assert not same(ref["x"], np.zeros_like(ref["x"])) and np.isfinite(ref["x"]).all()
    assert_same_end(got, ref, run.__name__)


def test_what_attach_refuses(fb, oracle, hip):
    """LinearizedSS and Robot2D handles, x without s and s without x, a pointer less aligned than an element: each names the verb, and the handle
    steps on as before"""
    K = fb.K
    case = Case("x2", "WA", True)
    cal = Caller(fb, hip, case)
    px, ps = C.c_void_p(cal.xb.ptr), C.c_void_p(cal.sb.ptr)

    def refused(h, x, s, *words):
        assert fb.lib.fb_attach_state(h, x, s) != 0
        msg = fb.lib.fb_last_error().decode()
        assert "fb_attach_state" in msg and all(wd in msg for wd in words), msg

    try:
        # Cessna172Xv2 (the carried derivative would show a refusal that had touched it): every refusal between two halves of a run
        st = start_state(fb, oracle, "x2", "WA")
        w = make_world(fb, case)
        load_start(fb, w, st)
        step(fb, w, 50, 100)
        ref = end_state(fb, w)
        w.close()
        w = make_world(fb, case)
        load_start(fb, w, st)
        step(fb, w, 50, 50)
        refused(w._h, px, None, "both")
        refused(w._h, None, ps, "both")
        refused(w._h, C.c_void_p(cal.xb.ptr + 4), ps, "8-byte")
        refused(w._h, px, C.c_void_p(cal.sb.ptr + 2), "4-byte")
        step(fb, w, 50, 50)
        assert_same_end(end_state(fb, w), ref, "Cessna172Xv2 behind the refusals")
        w.close()
        # Robot2D
        r = fb.Robot2DWorld(8)
        r.set_params(dt=0.01, periodic_n=2)
        fb.f_init(r, fb.InitParameters(u_m=0.03))
        step(fb, r, 10, 20); r.sync(); x_ref = r.x
        fb.f_init(r, fb.InitParameters(u_m=0.03))
        step(fb, r, 10, 10)
        refused(r._h, px, ps, "Robot2D")
        step(fb, r, 10, 10); r.sync()
        assert same(r.x, x_ref)
        r.close()
        # LinearizedSS
        m = make_lss(fb, 5, 2, 3, 8, seed=11, stable=True)
        lw = fb.LinearWorld(m)
        lw.step(20, dt=0.01, steps_per_launch=10); lw.sync(); x_ref = lw.x
        lw.set_state(m.x0.T)
        lw.step(10)
        refused(lw._h, px, ps, "LinearizedSS")
        lw.step(10); lw.sync()
        assert same(lw.x, x_ref)
        lw.close()
        assert same(cal.xb.read(), np.zeros((cal.nxd, N))) and same(cal.sb.read(), np.zeros((K["FB_NS"], N), np.int32))
    finally:
        cal.close("refusals")


# ---- 6. a buffer that is a view -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES_4, ids=[c.id for c in CASES_4])
def test_attached_views_at_element_alignment(fb, oracle, hip, case):
    """A torch slice hands over x 8-byte aligned (not 16) and s 4-byte aligned (not 8). The stepping kernels, k_f_ode, k_log_gather and the
    scenario kernels address the state rows one element per lane (row stride n: nothing to vectorise), so element alignment is all they need."""
    ref = owned_run(fb, oracle, case)
    got = attached_run(fb, hip, case, start_state(fb, oracle, case.model, case.kin), case.id + ", views at +8 / +4 bytes", offset=(8, 4))
    assert_same_snapshots(got, ref, case.id + ", views at +8 / +4 bytes")


# ---- 7. the benchmark's own arrangement ---------------------------------------------------------------------------------------------------------
def test_torch_tensors_on_torchs_stream(fb, oracle):
    """bench.py's arrangement in a child process (torch brings its own HIP runtime: not in this process): torch tensors attached, the handle on
    torch's current stream — a side stream: the default stream's handle is 0, which fb_set_stream reads as "the handle's own" —, x_dev.copy_()
    of a new state, fb_step, x_dev.clone(), one torch.cuda.synchronize() at the end."""
    case = Case("s0", "WA", True)
    st = start_state(fb, oracle, "s0", "WA")
    x2, s2 = other_state(fb, case, st)
    w = make_world(fb, case)
    load_start(fb, w, st)
    w.x = x2; w.s = s2
    step(fb, w, 50, 50)
    ref = end_state(fb, w)
    w.close()
    code = textwrap.dedent("""
        import ctypes as C, os, sys, numpy as np
        import torch
        if not torch.cuda.is_available() or torch.cuda.device_count() < 1:
            print("NO_TORCH_DEVICE"); sys.exit(0)
        sys.path.insert(0, os.path.join(os.getcwd(), "flight.jl_amd"))
        import flightbatch as fb
        d = np.load(sys.argv[1])
        n = d["x0"].shape[1]
        w = fb.BatchedWorld(n)
        w.set_params(dt=float(d["dt"]), periodic_n=1, h_terrain=float(d["h_terrain"]))
        x_dev = torch.zeros((fb.K["FB_NX"], n), dtype=torch.float64, device="cuda")
        s_dev = torch.zeros((fb.K["FB_NS"], n), dtype=torch.int32, device="cuda")
        x_new, s_new = torch.from_numpy(d["x2"]).cuda(), torch.from_numpy(d["s2"]).cuda()
        torch.cuda.synchronize()
        fb._lib.check(fb.lib.fb_attach_state(w._h, C.c_void_p(x_dev.data_ptr()), C.c_void_p(s_dev.data_ptr())))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            S = torch.cuda.current_stream().cuda_stream
            assert S != 0
            fb._lib.check(fb.lib.fb_set_stream(w._h, C.c_void_p(S)))
            w.set_state(d["x0"], d["s0"]); w.u = d["u"]; w.ui = d["ui"]
            fb._lib.check(fb.lib.fb_set_steps_per_launch(w._h, 50))
            x_dev.copy_(x_new); s_dev.copy_(s_new)
            fb._lib.check(fb.lib.fb_step(w._h, 50))
            x_out, s_out = x_dev.clone(), s_dev.clone()
        torch.cuda.synchronize()
        ok = np.array_equal(x_out.cpu().numpy(), d["x_ref"], equal_nan=True) and np.array_equal(s_out.cpu().numpy(), d["s_ref"])
        fb._lib.check(fb.lib.fb_set_stream(w._h, None))
        w.close()
        print("TORCH_ATTACH_OK" if ok else "TORCH_ATTACH_DIFFERS")
    """)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "twin.npz")
        np.savez(path, x0=st["x"], s0=st["s"], u=st["u"], ui=st["ui"], x2=x2, s2=s2, x_ref=ref["x"], s_ref=ref["s"], dt=DT, h_terrain=RUNWAY_H_TRN)
        r = subprocess.run([sys.executable, "-c", code, path], cwd=ROOT, capture_output=True, text=True, timeout=150)
    if "NO_TORCH_DEVICE" in r.stdout:
        pytest.skip("torch in the child process sees no device")
    assert "TORCH_ATTACH_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
