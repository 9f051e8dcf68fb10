"""fb_lss_dtracker_metrics and fb_lss_dsteady (flightbatch.dtracker): the sampled LQR tracker law the stepper flies, on a batch of sampled
models and gain candidates on the device, the steady-state map of a sampled model, and the sampled design chain on top of them, pinned by

  1. the exact side (a literal tick-by-tick transcription of the law) on unbounded pairs at every group edge, D_z = 0 and != 0;
  2. bounded pairs: the clamp and halt counts as integers, the metrics, +-Inf bounds against no bounds;
  3. position independence and reproducibility, bit for bit, the handle left as it was, and the stride rule;
  4. a diverging pair, a non-finite gain and a non-finite model entry flagged in place among healthy ones;
  5. the design chain on the device: c2d -> dlqr_tracker -> dtracker_metrics against the host's design-form loop from dlqr's raw K_aug, against
     timeresp.step on dtracker_world, settled on zref, dpoles inside the unit circle;
  6. dsteady_state against the host solve, a singular L_d and the DIRECT bit;
  7. the refusals of the C ABI on a live device;
  8. fb_lss_steady still refuses a sampled world, fb_lss_dsteady a continuous one;
  9. the reference's stored vh2te and phibeta2ar gains at the 28 design nodes under the law at 50 Hz.

The bound of 1, 2, 5 and 9 is the family's rule (tests/test_gpu_dpid.py): the device differs from the numpy restatement of its algorithm
(tests/dtracker_prototype.py; held to the exact side on the CPU by tests/test_dtracker_host.py) in FMA contraction and <= 1-ulp division only,
so its deviation from the exact side may be ten times the prototype's over the same pairs, with the project's fp64 parity bound of 1e-11 as
the floor. A deviation is, for the samples, the worst |got - exact| over the largest |exact| of that response; for a metric,
|got - exact| / |exact|, the worst over the pairs. Ts = 0.02, t_sim = 2 (100 ticks) unless stated."""
import ctypes as C
import functools

import numpy as np
import pytest

import dtracker_prototype as proto
import reference_fixtures as rf
from support import pd

pytestmark = pytest.mark.gpu
FLOOR, MARGIN = 1e-11, 10.0
TS, T_SIM, N_TICKS = proto.TS, proto.T_SIM, proto.N_TICKS
pi32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
ALL = proto.KEYS + ("counts", "status")


def _dict(res):
    return dict(zs=res.z, us=res.u, zmet=np.stack([res.ie, res.ef, res.zp], axis=-1), umet=np.stack([res.iu, res.up], axis=-1),
                counts=np.stack([res.clamped, res.halted], axis=-1), status=res.status)


def _run(fb, w, iz, K, zref, bounds=None, stride=1, t_sim=T_SIM):
    return _dict(fb.dtracker_metrics(w, iz, *K, zref, t_sim, bounds=bounds, stride=stride))


def _same(p, q, sel=slice(None)):
    return all(np.array_equal(p[k][sel], q[k], equal_nan=True) for k in ALL)


def _hold(tag, got, want, pro, capsys):
    """the rule of the module docstring per key; prints the device's and the prototype's deviation"""
    dd, dp = proto.deviations(got, want), proto.deviations(pro, want)
    with capsys.disabled():
        print(f"\n[{tag}] " + "  ".join(f"{k} {dd[k]:.2e} ({dp[k]:.2e})" for k in proto.KEYS), end="")
    for k in proto.KEYS:
        assert dd[k] <= max(MARGIN * dp[k], FLOOR), (tag, k, dd[k], dp[k])


# ---- 1. the exact side at every group edge ---------------------------------------------------------------------------------------------------------
CASES = [(r, proto.N_REF, proto.M_REF, n, m) for r in proto.EDGES for n, m in ((1, 1), (3, 5), (9, 5))]
CASES += [(9, 130, 5, 130, 5), (9, 130, 5, 130, 1), (8, 3, 64, 3, 64)]


@pytest.mark.parametrize("rows,n_ref,m_ref,n,m", CASES)
def test_unbounded_pairs_against_the_exact_side(fb, rows, n_ref, m_ref, n, m, capsys):
    Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint, zref, pro, ex = proto.edge_reference(rows, n_ref, m_ref)
    w, iz = proto.world(fb, Phi[:n], Gam[:n], Cz[:n], Dz[:n])
    got = _run(fb, w, iz, (Kfbk[:n, :m], Kfwd[:n, :m], Kint[:n, :m]), zref)
    w.close()
    nx, nu, nz = proto.EDGES[rows]
    assert got["zs"].shape == (n, m, nz, N_TICKS + 1) and got["us"].shape == (n, m, nu, N_TICKS + 1)
    assert got["zmet"].shape == (n, m, nz, 3) and got["umet"].shape == got["counts"].shape == (n, m, nu, 2) and got["status"].shape == (n, m)
    assert (got["status"] == 0).all() and (got["counts"] == 0).all()
    assert n == 1 or ((Dz[:n] == 0).all(axis=(1, 2)).any() and (Dz[:n] != 0).any())
    _hold(f"fb_lss_dtracker_metrics vs exact, rows {rows:2d}, {n} x {m}", got, proto.take(ex, n, m, n_ref, m_ref), proto.take(pro, n, m, n_ref, m_ref), capsys)


# ---- 2. bounded pairs ------------------------------------------------------------------------------------------------------------------------------
def test_bounded_pairs_counts_metrics_and_infinite_bounds(fb, capsys):
    Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint, lo, hi = proto.bounded_cases()
    pro, ex, near = proto.bounded_reference()
    n, m = lo.shape[:2]
    assert (near >= 1e-6).all()                                    # decided on the exact side (tests/test_dtracker_host.py): the counts are integers to match
    w, iz = proto.world(fb, Phi, Gam, Cz, Dz)
    K = (Kfbk, Kfwd, Kint)
    got = _run(fb, w, iz, K, proto.B_ZREF, bounds=(lo, hi))
    assert (got["status"] == 0).all()
    want_counts = ex["counts"].reshape(n, m, 2, 2)
    assert np.array_equal(got["counts"], want_counts), got["counts"] - want_counts
    _hold("fb_lss_dtracker_metrics vs exact, bounded, nx 3, nu 2, nz 2", got, proto.take(ex, n, m, n, m), proto.take(pro, n, m, n, m), capsys)
    assert (got["counts"][..., 1] > 0).any()                                                        # halted ticks
    assert ((got["counts"][:, :, 0, 0] > 0) & (got["counts"][:, :, 1, 0] == 0)).any()               # a pair that clamps on one input only
    # bounds of +-Inf are no bounds, bit for bit
    none = _run(fb, w, iz, K, proto.B_ZREF)
    inf = _run(fb, w, iz, K, proto.B_ZREF, bounds=(-np.inf, np.inf))
    w.close()
    assert _same(none, inf) and (none["counts"] == 0).all() and (none["status"] == 0).all()
    # candidate 5 of the bounded run has infinite bounds, candidate 4 finite ones that are never reached: both are the unbounded pair
    for j in (4, 5):
        assert all(np.array_equal(got[k][:, j], none[k][:, j]) for k in ALL), j


# ---- 3. bits ---------------------------------------------------------------------------------------------------------------------------------------
def test_bitwise_independent_of_position_and_slot_repeatable_and_strided(fb):
    n, m = 9, 5
    Phi, Gam, Cz, _, Kfbk, Kfwd, Kint, zref, _, _ = proto.edge_reference(15)
    nx, nu, nz = proto.EDGES[15]
    Dz = np.zeros((n, nz, nu))                            # (so that half of the candidates can be bounded without a word about D_z)
    lo, hi = np.full((n, m, nu), -np.inf), np.full((n, m, nu), np.inf)
    lo[:, 1], hi[:, 1], hi[:, 3, 0] = -0.2, 0.2, 0.1
    w, iz = proto.world(fb, Phi, Gam, Cz, Dz)
    rng = np.random.default_rng(7)
    w.set_state(rng.standard_normal((nx, n)))
    w.u = rng.standard_normal((nu, n))
    w.step(7)
    w.sync()
    state = lambda: (w.x, w.u, float(fb.lib.fb_time(w._h)), w.status, *w.model(), *w.model_cd(), w.Ts)
    before = state()
    first = _run(fb, w, iz, (Kfbk, Kfwd, Kint), zref, (lo, hi))
    again = _run(fb, w, iz, (Kfbk, Kfwd, Kint), zref, (lo, hi))
    for p, q in zip(before, state()):
        assert np.array_equal(p, q)
    assert before[2] == pytest.approx(7 * TS) and (first["status"] == 0).all() and first["counts"][..., 0].max() >= 1
    assert _same(first, again)
    pick_m = lambda sel: ((Kfbk[:, sel], Kfwd[:, sel], Kint[:, sel]), (lo[:, sel], hi[:, sel]))
    perm = np.array([3, 0, 4, 2, 1])
    for sel in (perm, slice(1, 2), slice(2, 3)):
        K, b = pick_m(sel)
        assert _same(first, _run(fb, w, iz, K, zref, b), (slice(None), sel))
    # stride s keeps exactly every s-th sample of stride 1, and the last one; the metrics do not move
    for s in (7, 10, 100):
        strided = _run(fb, w, iz, (Kfbk, Kfwd, Kint), zref, (lo, hi), stride=s)
        keep = proto.sample_rows(N_TICKS, s)
        assert strided["zs"].shape[-1] == len(keep) == fb.timeresp.samples(N_TICKS, s)
        assert np.array_equal(strided["zs"], first["zs"][..., keep]) and np.array_equal(strided["us"], first["us"][..., keep])
        assert all(np.array_equal(strided[k], first[k]) for k in ("zmet", "umet", "counts", "status"))
    w.close()
    for pick in (np.arange(n)[::-1], np.array([8, 0, 5, 3])):
        ws, _ = proto.world(fb, Phi[pick], Gam[pick], Cz[pick], Dz[pick], seed=6)   # (other rows and offsets than the full batch's: they play no part)
        assert np.array_equal(ws.model()[0], before[4][pick])
        assert _same(first, _run(fb, ws, iz, (Kfbk[pick], Kfwd[pick], Kint[pick]), zref, (lo[pick], hi[pick])), pick)
        ws.close()


# ---- 4. failure pairs --------------------------------------------------------------------------------------------------------------------------------
def test_failure_pairs_are_flagged_in_place(fb):
    """Six two-state plants, three candidates each (dtracker_prototype.failure_pairs). System 2's candidate 1 feeds the state back with the wrong
    sign: the loop has a pole at 1.5, and 1.5^100 > 1e12. System 4's candidate 0 has a NaN in K_int, candidate 2 an Inf in K_fwd. Then a NaN in
    system 5's C_z. The inputs are fixed and nothing is retried: the overflow is arithmetic, by design of the input."""
    Phi, Gam, Cz, Dz, Kfbk, Kfwd, Kint, expect = proto.failure_pairs()
    zref = proto.plants(2, 1, 1, 6)[4]
    w, iz = proto.world(fb, Phi, Gam, Cz, Dz)
    res = _run(fb, w, iz, (Kfbk, Kfwd, Kint), zref)
    hf, hw, hi_ = Kfbk.copy(), Kfwd.copy(), Kint.copy()
    hf[2, 1], hi_[4, 0], hw[4, 2] = Kfbk[2, 0], Kint[4, 1], Kfwd[4, 1]
    ref = _run(fb, w, iz, (hf, hw, hi_), zref)
    w.close()
    assert np.array_equal(res["status"], expect), res["status"]
    assert (ref["status"] == 0).all() and all(np.isfinite(ref[k]).all() for k in proto.KEYS)
    assert np.isinf(res["zmet"][2, 1]).all() and np.isinf(res["umet"][2, 1]).all() and (res["zmet"][2, 1] > 0).all() and (res["counts"][2, 1] == 0).all()
    for j in (0, 2):
        assert np.isnan(res["zmet"][4, j]).all() and np.isnan(res["umet"][4, j]).all() and (res["counts"][4, j] == 0).all()
    ok = expect == 0
    for k in ALL:
        assert np.array_equal(res[k][ok], ref[k][ok]), k
    # NaN in one row of C_z: that system's pairs are void, every other pair keeps its bits; a NaN in a row of C that is not in z does nothing
    for row, void in ((iz[0], True), (0, False)):
        wn, _ = proto.world(fb, Phi, Gam, Cz, Dz)
        Cm, D = wn.model_cd()
        A, B = wn.model()
        wn.close()
        Cm[5, row, 1] = np.nan
        n, nx = Phi.shape[:2]
        lss = fb.LinearizedSS(xdot0=np.zeros((n, nx)), x0=np.zeros((n, nx)), u0=np.zeros((n, 1)), y0=np.zeros((n, 3)), A=A, B=B, C=Cm, D=D,
                              x_labels=("a", "b"), u_labels=("u",), y_labels=("y0", "y1", "y2"))
        wb = fb.LinearWorld(lss, Ts=TS)
        resn = _run(fb, wb, iz, (hf, hw, hi_), zref)
        wb.close()
        if void:
            assert (resn["status"][5] == proto.NOT_FINITE).all() and np.isnan(resn["zmet"][5]).all() and (resn["counts"][5] == 0).all()
            assert all(np.array_equal(resn[k][:5], ref[k][:5]) for k in ALL)
        else:
            assert _same(resn, ref)


# ---- 5. the design chain on the device ---------------------------------------------------------------------------------------------------------------
def _double_integrators(fb, n=4):
    """x = (p, v), p' = v, v' = b u with b = 1, 1.2, ..: C = I, z = p"""
    A = np.broadcast_to(np.array([[0.0, 1.0], [0.0, 0.0]]), (n, 2, 2)).copy()
    B = np.zeros((n, 2, 1)); B[:, 1, 0] = 1.0 + 0.2 * np.arange(n)
    z = np.zeros
    lss = fb.LinearizedSS(xdot0=z((n, 2)), x0=z((n, 2)), u0=z((n, 1)), y0=z((n, 2)), A=A, B=B, C=np.broadcast_to(np.eye(2), (n, 2, 2)).copy(),
                          D=z((n, 2, 1)), x_labels=("p", "v"), u_labels=("u",), y_labels=("p", "v"))
    return fb.LinearWorld(lss), "p", np.array([1.0, 0.1]), np.array([[0.1]]), np.array([5.0]), np.array([1.5])


def _robot2d(fb, n=3):
    """the Robot2D linearisation without η (the notebook's velocity loop: LQR with integral action on v and its weights), z = v"""
    r = fb.Robot2DWorld(n)
    fb.linearize(r, None, scheme="forward")
    full = fb.linear_world(r)
    r.close()
    plant = fb.subsystem_world(full, x=["ω", "v", "θ"], y=["ω", "v", "θ", "u_m", "τ_m"])
    full.close()
    return plant, "v", np.array([0.001, 0.01, 0.0]), np.array([[0.1]]), np.array([0.05]), np.array([0.5])


@pytest.mark.parametrize("which", ["double integrator", "Robot2D"])
def test_the_design_chain_on_the_device(fb, which, capsys):
    cont, z, Q, R, Q_int, zref = (_double_integrators if which == "double integrator" else _robot2d)(fb)
    sampled = fb.c2d(cont, TS)
    cont.close()
    w = sampled.world
    assert (sampled.status == 0).all() and w.Ts == TS
    n, nx, nu, nz = w.n, w.nx, w.nu, 1
    K_fbk, K_fwd, K_int, status = fb.dlqr_tracker(w, [z], Q, R, Q_int)
    assert (status == 0).all(), status
    # dlqr's raw gain on the augmentation [x_k; xi_k-1]
    aug = fb.dintegral_augmentation(w, [z])
    raw = fb.dlqr(aug, np.concatenate([Q, Q_int]), R)
    Pa, Ga = aug.model()
    aug.close()
    assert (raw.status == 0).all()
    Phi, Gam = w.model()
    Cm, D = w.model_cd()
    iz = w.y_labels.index(z)
    Cz = Cm[:, [iz]]
    assert (D[:, [iz]] == 0).all()
    assert np.array_equal(Pa[:, :nx, :nx], Phi) and np.array_equal(Pa[:, nx:, :nx], TS * Cz) and np.array_equal(Pa[:, nx:, nx:], np.ones((n, 1, 1)))
    assert np.array_equal(Ga[:, :nx], Gam) and (Ga[:, nx:] == 0).all()
    assert np.array_equal(K_int, raw.K[:, :, nx:])
    # t_sim from the exact side: the loop has settled when its ef is at or below the floor relative to |zref|
    flown = lambda N: [proto.law_exact(Phi[i], Gam[i], Cz[i], np.zeros((nz, nu)), K_fbk[i], K_fwd[i], K_int[i], zref, TS, N) for i in range(n)]
    t_sim = 10.0
    while max(abs(zref[0] - r[0][0, -1]) for r in flown(int(round(t_sim / TS)))) > 0.1 * FLOOR * abs(zref[0]):
        t_sim *= 2.0
        assert t_sim <= 320.0
    N = int(round(t_sim / TS))
    runs = flown(N)
    ex = dict(zs=np.array([r[0] for r in runs])[:, None], us=np.array([r[1] for r in runs])[:, None])
    ex["zmet"], ex["umet"] = proto.metrics_of(ex["zs"], ex["us"], zref, N)
    pro = proto.tracker(Phi, Gam, Cz, np.zeros((n, nz, nu)), K_fbk, K_fwd, K_int, zref, TS, N)
    pro = {k: pro[k][:, None] for k in proto.KEYS}
    got = _run(fb, w, [z], (K_fbk, K_fwd, K_int), zref, t_sim=t_sim)
    assert (got["status"] == 0).all() and (got["counts"] == 0).all()
    # settled: ef at or below the floor relative to |zref|; a relative deviation of such an ef means nothing, so the rule holds ie and zp
    with capsys.disabled():
        print(f"\n[{which}] t_sim {t_sim:g}: ef / |zref| <= {(got['zmet'][..., 1] / abs(zref[0])).max():.2e}", end="")
    assert (got["zmet"][..., 1] <= FLOOR * abs(zref[0])).all()
    for d in (ex, pro, got):
        d["zmet"] = d["zmet"][..., [0, 2]]
    _hold(f"dlqr_tracker -> dtracker_metrics vs the flown law's exact side, {which}, {N} ticks", got, ex, pro, capsys)
    # the host's design-form loop from dlqr's raw K_aug: the same samples
    des = [proto.design_form(Phi[i], Gam[i], Cz[i], raw.K[i], K_fwd[i], zref, TS, N) for i in range(n)]
    dex = dict(ex, zs=np.array([r[0] for r in des])[:, None], us=np.array([r[1] for r in des])[:, None])
    dex["zmet"], dex["umet"] = proto.metrics_of(dex["zs"], dex["us"], zref, N)
    dex["zmet"] = dex["zmet"][..., [0, 2]]
    _hold(f"dtracker_metrics vs the design-form loop from dlqr's K_aug, {which}", got, dex, pro, capsys)
    # the loop as a world: timeresp.step of zref -> z and zref -> u (a unit step: scaled by zref), and its poles
    loop = fb.dtracker_world(w, [z], K_fbk, K_fwd, K_int)
    assert loop.nx == nx + nu and loop.u_labels == (f"{z}_ref",) and loop.Ts == TS
    lam = fb.dpoles(loop)
    assert (lam.status == 0).all() and (np.abs(lam.poles) < 1.0).all()
    # (the plant's input is not among its outputs: the law's output is read back from the samples of z alone, and of x where C = I)
    sr = fb.timeresp.step(loop, [(f"{z}_ref", z)], t_sim)
    loop.close()
    w.close()
    assert (sr.status == 0).all() and sr.y.shape == (n, 1, N + 1)
    other = dict(zs=(zref[0] * sr.y)[:, :, None, :])
    dd = float((np.abs(other["zs"] - ex["zs"]) / np.abs(ex["zs"]).max(axis=-1, keepdims=True)).max())
    dp = proto.deviations(pro, ex)["zs"]
    dv = float((np.abs(other["zs"] - got["zs"]) / np.abs(ex["zs"]).max(axis=-1, keepdims=True)).max())
    with capsys.disabled():
        print(f"\n[timeresp.step on dtracker_world vs exact, {which}] zs {dd:.2e} ({dp:.2e}); against fb_lss_dtracker_metrics {dv:.2e}; "
              f"largest |pole| {np.abs(lam.poles).max():.6f}", end="")
    assert dd <= max(MARGIN * dp, FLOOR) and dv <= 2 * max(MARGIN * dp, FLOOR)


# ---- 6. the steady-state map -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nu", [(1, 1), (7, 2), (14, 3), (24, 8)])       # nx + nu = 2, 9, 17, 32
def test_dsteady_against_the_host_solve(fb, nx, nu, capsys):
    n = 9
    Phi, Gam, Cz, Dz, _ = proto.plants(nx, nu, nu, n)
    rng = np.random.default_rng(21)
    K, K_xi = rng.standard_normal((n, nu, nx)), rng.standard_normal((n, nu, nu))
    w, iz = proto.world(fb, Phi, Gam, Cz, Dz)
    plain = fb.dsteady_state(w, iz, K)
    conv = fb.dsteady_state(w, iz, K, K_xi)
    batch = fb.dsteady_state(w, iz, K[2], K_xi[2])
    bare = fb.dsteady_state(w, iz)
    w.close()
    want = [proto.dsteady(Phi[i], Gam[i], Cz[i], Dz[i], K[i], K_xi[i]) for i in range(n)]
    plain_want = [proto.dsteady(Phi[i], Gam[i], Cz[i], Dz[i], K[i]) for i in range(n)]
    dev = lambda g, h: float(np.abs(g - h).max() / np.abs(h).max())
    assert (plain.status == 0).all() and (bare.status == 0).all() and bare.K_fwd is None and bare.K_fbk is None
    assert np.array_equal(bare.X, plain.X) and np.array_equal(bare.U, plain.U) and np.array_equal(conv.X, plain.X) and np.array_equal(conv.U, plain.U)
    assert np.array_equal(plain.K_fbk, K)
    direct = (Dz != 0).any(axis=(1, 2))
    assert np.array_equal(conv.status, np.where(direct, proto.DIRECT, 0)) and direct.any() and not direct.all()
    assert np.isnan(conv.K_fbk[direct]).all() and np.isnan(conv.K_fwd[direct]).all() and np.isfinite(conv.X).all() and np.isfinite(conv.U).all()
    d = {}
    for i in range(n):
        X, U, K_fbk, K_fwd = want[i]
        cond = np.linalg.cond(np.block([[Phi[i] - np.eye(nx), Gam[i]], [Cz[i], Dz[i]]]))
        tol = max(FLOOR, 1e-14 * cond)                                      # (a solve against LAPACK's: a few ulp times the condition number)
        for key, g, h in (("X", plain.X[i], X), ("U", plain.U[i], U), ("K_fwd", plain.K_fwd[i], plain_want[i][3])):
            d[key] = max(d.get(key, 0.0), dev(g, h))
            assert dev(g, h) <= tol, (key, i, dev(g, h), cond)
        if not direct[i]:
            for key, g, h in (("K_fbk", conv.K_fbk[i], K_fbk), ("K_fwd (K_xi)", conv.K_fwd[i], K_fwd)):
                d[key] = max(d.get(key, 0.0), dev(g, h))
                assert dev(g, h) <= tol, (key, i, dev(g, h), cond)
    assert not direct[2] and np.array_equal(batch.K_fbk[2], conv.K_fbk[2]) and np.array_equal(batch.K_fwd[2], conv.K_fwd[2])      # one K for the batch: the same bits
    with capsys.disabled():
        print(f"\n[fb_lss_dsteady vs numpy.linalg.solve, nx + nu = {nx + nu}] " + "  ".join(f"{k} {v:.2e}" for k, v in d.items()), end="")


def test_dsteady_flags_a_singular_map_in_place(fb):
    """system 1 has an eigenvalue of Phi at exactly 1 that C_z does not see and Gamma does not reach: L_d has a zero row"""
    n, nx, nu = 4, 3, 1
    Phi, Gam, Cz, Dz, _ = (a.copy() for a in proto.plants(nx, nu, nu, n))
    Dz[:] = 0.0
    Phi[1] = np.diag([0.5, 1.0, 0.25]); Gam[1] = np.array([[1.0], [0.0], [0.5]]); Cz[1] = np.array([[1.0, 0.0, 1.0]])
    K = np.ones((nu, nx))
    w, iz = proto.world(fb, Phi, Gam, Cz, Dz)
    res = fb.dsteady_state(w, iz, K, np.ones((nu, nu)))
    w.close()
    healthy, _ = proto.world(fb, Phi[[0, 2, 3]], Gam[[0, 2, 3]], Cz[[0, 2, 3]], Dz[[0, 2, 3]])
    ref = fb.dsteady_state(healthy, iz, K, np.ones((nu, nu)))
    healthy.close()
    assert res.status.tolist() == [0, fb.K["FB_SURGERY_SINGULAR"], 0, 0] and res.rpiv[1] == 0.0 and (res.rpiv[[0, 2, 3]] > 0).all()
    for name in ("X", "U", "K_fbk", "K_fwd"):
        assert np.isnan(getattr(res, name)[1]).all() and np.array_equal(getattr(res, name)[[0, 2, 3]], getattr(ref, name)), name


# ---- 7., 8. refusals on a live device --------------------------------------------------------------------------------------------------------------------
def _launches(fb, h):
    ms, nl = C.c_float(), C.c_int64()
    assert fb.lib.fb_timing_end(h, C.byref(ms), C.byref(nl)) == 0
    assert fb.lib.fb_timing_launches(h, None, 0, C.byref(nl)) == 0
    return nl.value


def test_refusals_name_the_verb_and_the_cause_and_launch_nothing(fb):
    n, m, nx, nu, nz = 4, 2, 3, 2, 2
    Phi, Gam, Cz, Dz, zref0 = proto.plants(nx, nu, nz, n)
    w, iz0 = proto.world(fb, Phi, Gam, Cz, Dz)
    iz0 = np.array(iz0, dtype=np.int32)
    g = lambda cols: np.full(nu * cols * m * n, 0.01)
    bnd = np.concatenate([np.full(nu * m * n, -2.0), np.full(nu * m * n, 2.0)])
    opt = lambda a: pd(a) if a is not None else None

    def track(h, iz=iz0, nz=nz, fbk=g(nx), fwd=g(nz), kin=g(nz), bounds=None, m=m, zref=zref0, t_sim=1.0, stride=1, status=True):
        mm, ns = max(m, 1), 64
        zm, um, cn = np.empty(3 * 8 * mm * n), np.empty(2 * 8 * mm * n), np.empty(2 * 8 * mm * n, dtype=np.int32)
        st = np.empty(mm * n, dtype=np.int32)
        return fb.lib.fb_lss_dtracker_metrics(h, None if iz is None else pi32(iz), nz, opt(fbk), opt(fwd), opt(kin), opt(bounds), m, opt(zref), t_sim,
                                              stride, pd(zm), pd(um), pi32(cn), None, None, pi32(st) if status else None)

    def steady(h, iz=iz0, nz=nz, K=None, K_xi=None, K_fbk=False, K_fwd=False):
        X, U, F, W = np.empty(nx * nz * n), np.empty(nu * nz * n), np.empty(nu * nx * n), np.empty(nu * nz * n)
        st, rp = np.empty(n, dtype=np.int32), np.empty(n)
        return fb.lib.fb_lss_dsteady(h, None if iz is None else pi32(iz), nz, opt(K), opt(K_xi), 0, pd(X), pd(U), pd(F) if K_fbk else None,
                                     pd(W) if K_fwd else None, pd(rp), pi32(st))

    def refused(call, verb, h, msg, **kw):
        assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
        rc = call(h, **kw)
        err = fb.lib.fb_last_error()
        assert rc != 0 and msg in err and verb in err, err
        assert _launches(fb, h) == 0

    h = w._h
    T, S = b"fb_lss_dtracker_metrics", b"fb_lss_dsteady"
    eq_b = bnd.copy(); eq_b[nu * m * n + 5] = -2.0                       # hi = lo at system 1, candidate 1, input 0
    rev_b = bnd.copy(); rev_b[m * n + 2] = 3.0                           # lo = 3 at system 2, candidate 0, input 1
    nan_b = bnd.copy(); nan_b[nu * m * n + 3] = np.nan
    for kw, msg in ((dict(iz=np.array([0, 4], dtype=np.int32)), b"iz[1] = 4"), (dict(iz=np.array([-1, 0], dtype=np.int32)), b"iz[0] = -1"),
                    (dict(iz=None), b"iz is required"), (dict(nz=0), b"nz = 0"), (dict(nz=9), b"nz = 9"),
                    (dict(m=0), b"m = 0"), (dict(m=65), b"m = 65"), (dict(t_sim=5e-3), b"1 <= N <= 200000"), (dict(t_sim=np.inf), b"t_sim = inf"),
                    (dict(t_sim=np.nan), b"t_sim = nan"), (dict(t_sim=4000.02), b"1 <= N <= 200000"), (dict(stride=0), b"stride = 0"),
                    (dict(bounds=eq_b), b"lo = -2, hi = -2 at system 1, candidate 1, input 0"),
                    (dict(bounds=rev_b), b"lo = 3, hi = 2 at system 2, candidate 0, input 1"), (dict(bounds=nan_b), b"hi = nan at system 3, candidate 0, input 0"),
                    (dict(zref=np.array([1.0, np.nan])), b"zref[1] = nan"), (dict(zref=np.array([np.inf, 1.0])), b"zref[0] = inf"),
                    (dict(zref=None), b"are required"), (dict(fbk=None), b"are required"), (dict(fwd=None), b"are required"),
                    (dict(kin=None), b"are required"), (dict(status=False), b"are required")):
        refused(track, T, h, msg, **kw)
    for kw, msg in ((dict(nz=1), b"nz = 1"), (dict(iz=None), b"iz is required"), (dict(iz=np.array([0, 4], dtype=np.int32)), b"iz[1] = 4"),
                    (dict(K_fwd=True), b"needs K"), (dict(K_xi=np.ones(nu * nz)), b"needs K"), (dict(K_fbk=True), b"needs K")):
        refused(steady, S, h, msg, **kw)
    # and the handle still evaluates: one stamped launch each; null outputs
    assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
    assert track(h) == 0, fb.lib.fb_last_error()
    assert steady(h, K=np.ones(nu * nx), K_xi=np.ones(nu * nz), K_fbk=True, K_fwd=True) == 0, fb.lib.fb_last_error()
    assert _launches(fb, h) == 2
    assert track(h, bounds=bnd, t_sim=4000.0, stride=200000) == 0, fb.lib.fb_last_error()         # 200000 ticks, bounds
    # 8. fb_lss_steady keeps refusing the sampled handle, with the message it had
    X, U, st = np.empty(nx * nz * n), np.empty(nu * nz * n), np.empty(n, dtype=np.int32)
    assert fb.lib.fb_timing_begin_per_launch(h, 8) == 0
    assert fb.lib.fb_lss_steady(h, pi32(iz0), nz, None, 0, pd(X), pd(U), None, None, pi32(st)) != 0
    assert b"fb_lss_steady: a continuous-time verb on a sampled model" in fb.lib.fb_last_error()
    assert _launches(fb, h) == 0
    w.close()
    # the handles: continuous, not LSS, no model, too large
    z = np.zeros
    lss = fb.LinearizedSS(xdot0=z((n, nx)), x0=z((n, nx)), u0=z((n, nu)), y0=z((n, nz)), A=Phi, B=Gam, C=Cz, D=Dz, x_labels=("a", "b", "c"),
                          u_labels=("u0", "u1"), y_labels=("y0", "y1"))
    cont = fb.LinearWorld(lss)
    iz2 = np.array([0, 1], dtype=np.int32)
    refused(track, T, cont._h, b"a discrete-time verb on a continuous model", iz=iz2)
    refused(steady, S, cont._h, b"a discrete-time verb on a continuous model", iz=iz2)
    assert fb.lib.fb_lss_steady(cont._h, pi32(iz2), nz, None, 0, pd(X), pd(U), None, None, pi32(st)) == 0, fb.lib.fb_last_error()
    cont.close()
    ac = fb.Cessna172Xv2World(n, kinematics="NED")
    refused(track, T, ac._h, b"not a LinearizedSS handle")
    refused(steady, S, ac._h, b"not a LinearizedSS handle")
    ac.close()
    hh = C.c_void_p()
    assert fb.lib.fb_lss_create(3, 2, 2, n, 0, C.byref(hh)) == 0
    refused(track, T, hh, b"no model yet", iz=iz2)
    refused(steady, S, hh, b"no model yet", iz=iz2)
    fb.lib.fb_destroy(hh)
    for (bx, bu, bz), msg in (((29, 2, 2), b"nx + nu + nz = 33"), ((31, 1, 1), b"nx = 31")):      # (a handle has at most 8 inputs)
        P2, G2, C2, D2, zr = proto.plants(bx, bu, bz, 2)
        big, izb = proto.world(fb, P2, G2, C2, D2)
        gg = lambda cols: np.full(bu * cols * 2, 0.01)
        assert fb.lib.fb_timing_begin_per_launch(big._h, 8) == 0
        zm, st2 = np.empty(3 * 8 * 2), np.empty(2, dtype=np.int32)
        rc = fb.lib.fb_lss_dtracker_metrics(big._h, pi32(np.array(izb, dtype=np.int32)), bz, pd(gg(bx)), pd(gg(bz)), pd(gg(bz)), None, 1, pd(zr), 1.0, 1,
                                            pd(zm), None, None, None, None, pi32(st2))
        err = fb.lib.fb_last_error()
        assert rc != 0 and msg in err and T in err, err
        assert _launches(fb, big._h) == 0
        big.close()
    P2, G2, C2, D2, _ = proto.plants(30, 3, 3, 2)
    big, izb = proto.world(fb, P2, G2, C2, D2)
    refused(steady, S, big._h, b"nx + nu = 33", iz=np.array(izb, dtype=np.int32), nz=3)
    big.close()


# ---- 9. the reference's stored gains under the law at 50 Hz ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sampled_design_worlds(fb):
    """trim -> linearize -> linear_world -> c172x_design_model -> c2d at Ts = 0.02, at the 28 design nodes: the sampled lon (XLonFull) and
    lat-without-ψ (XLatRed) design models"""
    EAS, h, flaps = rf.design_nodes()
    w = fb.Cessna172Xv2World(28, kinematics="NED")
    lss = fb.linearize(w, fb.TrimParameters(h_e=h, EAS=EAS, flaps=flaps), scheme="onesided2")
    src = fb.linear_world(w)
    w.close()
    assert lss.success.all() and (lss.status == 0).all()
    lon, lat = fb.c172x_design_model(src, "lon"), fb.c172x_design_model(src, "lat")
    src.close()
    lat_red = fb.delete_vars_world(lat.world, "ψ")
    out = {}
    for name, cont in (("vh2te", lon.world), ("phibeta2ar", lat_red)):
        res = fb.c2d(cont, TS)
        assert (res.status == 0).all()
        out[name] = res.world
    for x in (lon.world, lat.world, lat_red):
        x.close()
    return out


@pytest.mark.parametrize("name,zref,t_sim", [("vh2te", (1.0, 5.0), 10.0), ("phibeta2ar", (0.1, 0.02), 6.0)])
def test_the_stored_gains_under_the_flown_law(fb, name, zref, t_sim, capsys):
    import reference_lqr as rl
    xl, ul, zl, _, _, _, _ = rl.DESIGNS[name]
    w = _sampled_design_worlds(fb)[name]
    assert w.x_labels == tuple(xl) and w.u_labels == tuple(ul) and w.Ts == TS
    st = rf.stored(name)
    K = tuple(np.ascontiguousarray(np.moveaxis(st[k], -1, 0)) for k in ("K_fbk", "K_fwd", "K_int"))
    zref = np.array(zref)
    N = int(round(t_sim / TS))
    got = _run(fb, w, zl, K, zref, t_sim=t_sim)
    assert (got["status"] == 0).all() and all(np.isfinite(got[k]).all() for k in proto.KEYS) and (got["counts"] == 0).all()
    Phi, Gam = w.model()
    Cm, D = w.model_cd()
    iz = [w.y_labels.index(s) for s in zl]
    args = (Phi, Gam, Cm[:, iz], D[:, iz], *K)
    pro = proto.tracker(*args, zref, TS, N)
    ex, _ = proto.exact(*args, zref, TS, N)
    assert (pro["status"] == 0).all()
    lift = lambda d: {k: d[k][:, None] for k in proto.KEYS}
    with capsys.disabled():
        print(f"\n[{name}, stored gains, flown law at Ts = 0.02, zref {zref.tolist()}, {t_sim:g} s] node | ef | zp | up")
        for k in range(28):
            print(f"  {k:2d} | " + " ".join(f"{v:.3e}" for v in got["zmet"][k, 0, :, 1]) + " | " + " ".join(f"{v:.4f}" for v in got["zmet"][k, 0, :, 2])
                  + " | " + " ".join(f"{v:.4f}" for v in got["umet"][k, 0, :, 1]))
    _hold(f"fb_lss_dtracker_metrics vs exact, {name}, 28 nodes", got, lift(ex), lift(pro), capsys)
