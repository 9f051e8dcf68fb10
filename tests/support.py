"""What the suites share: error scales, the state-row maps between the C ABI and the oracle, attitude / position helpers, batch and handle
helpers, the scenario-table run helpers, and the Robot2D / Model(lss) pieces more than one file uses. No fixtures and no device work at
import; a cache lives here only where more than one test file shares the run behind it (traj_case). Test files import from here and from
reference_fixtures.py / conditioning.py / oracle_binding.py, never from each other (tests/test_support.py scans for that)."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_D = C.POINTER(C.c_double)
_I = C.POINTER(C.c_int32)


def pd(a):
    return a.ctypes.data_as(_D)


# ---- 1. scales and row maps --------------------------------------------------------------------------------------------------------------
# The oracle keeps the nine kinematic rows 12..20 of Cessna172Sv0(WA) in every mechanisation and leaves the ones a mechanisation does not
# use at zero; the C ABI drops them (ecef_dev_row / ned_dev_row / x2_dev_row of csrc/fb_capi.hip). Cessna172Xv2 adds seven actuator rows:
# behind the 27 in the oracle's layout, ahead of the kinematics (FB_X2_ACT .. FB_X2_KIN) in the C ABI's.
N_KIN = {"WA": 9, "ECEF": 8, "NED": 6}
UNUSED_ROWS = {"WA": (), "ECEF": (20,), "NED": (18, 19, 20)}
H_E_ROW = {"WA": 20, "ECEF": 19, "NED": 17}        # the ellipsoidal altitude in the oracle's layout (the last kinematic row in use)


def abi_to_oracle_rows(K, model, kin="WA"):
    """row k of the C ABI state of `model` ("s0": Cessna172Sv0, "x2": Cessna172Xv2) in mechanisation `kin` -> row of the oracle's layout"""
    rows = range(27) if model == "s0" else [k if k < K["FB_X2_ACT"] else (27 + k - K["FB_X2_ACT"] if k < K["FB_X2_KIN"] else k - K["FB_NACT"])
                                            for k in range(34)]
    return np.array([r for r in rows if r not in UNUSED_ROWS[kin]])


def h_e_row_abi(K, model, kin):
    """the ellipsoidal altitude in the C ABI's state (for Cessna172Sv0 the same number as H_E_ROW: the rows dropped lie behind it)"""
    return (12 if model == "s0" else K["FB_X2_KIN"]) + N_KIN[kin] - 1


def state_scale(x, kin="WA"):
    """per-row floors of a state in the oracle's layout, 27 or 34 rows: quaternion components 1, rates 1e-3 rad/s, the
    altitude row of the mechanisation max(|h_e|, 1), actuator rows 1"""
    sc = np.maximum(np.abs(x), 1e-3)
    sc[12:20] = 1.0               # q_wb, q_ew
    sc[0:2] = np.maximum(np.abs(x[0:2]), 1e-2)   # alpha/beta filt
    sc[2:8] = 1.0                 # contact regulators (zero airborne)
    sc[10:12] = 1.0               # engine PI states
    sc[20] = np.maximum(np.abs(x[20]), 1.0)
    sc[24:27] = np.maximum(np.abs(x[24:27]), 1.0)
    sc[27:] = 1.0
    sc[H_E_ROW[kin]] = np.maximum(np.abs(x[H_E_ROW[kin]]), 1.0)
    return sc


# ---- 2. attitude and position ------------------------------------------------------------------------------------------------------------
def qmul(a, b):
    return np.stack([a[0]*b[0]-a[1]*b[1]-a[2]*b[2]-a[3]*b[3], a[0]*b[1]+a[1]*b[0]+a[2]*b[3]-a[3]*b[2],
                     a[0]*b[2]-a[1]*b[3]+a[2]*b[0]+a[3]*b[1], a[0]*b[3]+a[1]*b[2]-a[2]*b[1]+a[3]*b[0]])


def q_from_euler(ps, th, ph):
    z = np.zeros_like(ps)
    return qmul(qmul(np.stack([np.cos(ps/2), z, z, np.sin(ps/2)]), np.stack([np.cos(th/2), z, np.sin(th/2), z])),
                np.stack([np.cos(ph/2), np.sin(ph/2), z, z]))


def q_ew_from_latlon(lat, lon):
    """q_ew = Rz(lon) ∘ Ry(-(lat + π/2)) (wander angle 0)"""
    a = -(lat + np.pi / 2)
    z = np.zeros_like(lat)
    return qmul(np.stack([np.cos(lon/2), z, z, np.sin(lon/2)]), np.stack([np.cos(a/2), z, np.sin(a/2), z]))


def geoid(oracle, lat, lon):
    out = np.zeros_like(lat)
    for k in range(lat.size):
        n_e = np.array([np.cos(lat[k]) * np.cos(lon[k]), np.cos(lat[k]) * np.sin(lon[k]), np.sin(lat[k])])
        out[k] = oracle.lib.fo_geoid_height(n_e.ctypes.data_as(_D))
    return out


def seg_end(oracle, p1, s, chi, dh):
    p1 = np.asarray(p1, dtype=np.float64); p2 = np.zeros(3)
    oracle.lib.fo_segment_end(p1.ctypes.data_as(_D), C.c_double(s), C.c_double(chi), C.c_double(dh), p2.ctypes.data_as(_D))
    return p2


# ---- 3. batches and handles --------------------------------------------------------------------------------------------------------------
class _env_var:
    """os.environ[name] = value for the length of a with block"""
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ[self.name]
        else:
            os.environ[self.name] = self.old


def stepper(duo):
    """worlds created inside are stepped by k_step_duo (duo) or by the one-wave k_step_air (FLIGHTBATCH_DUO=0, read when a handle is created)"""
    return _env_var("FLIGHTBATCH_DUO", "1" if duo else "0")


def lattice_trim_params(fb, n, seed=172):
    rng = np.random.default_rng(seed)
    lat = rng.uniform(-1.2, 1.2, n); lon = rng.uniform(-np.pi, np.pi, n)
    n_e = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)])
    return fb.TrimParameters(n_e=n_e, h_e=rng.uniform(200.0, 3000.0, n), EAS=rng.uniform(35.0, 55.0, n),
                             ψ_nb=rng.uniform(-np.pi, np.pi, n), γ_wb_n=rng.uniform(-0.02, 0.02, n),
                             ψ_wb_dot=rng.uniform(-0.03, 0.03, n), flaps=rng.choice([0.0, 0.0, 0.33], n),
                             fuel_load=rng.uniform(0.1, 1.0, n))


def random_env(fb, n, seed, h_trn=None):
    K = fb.K
    rng = np.random.default_rng(seed)
    e = np.zeros((K["FB_NENV"], n))
    e[K["FB_ENV_WIND_N"]] = rng.uniform(-12, 12, n); e[K["FB_ENV_WIND_E"]] = rng.uniform(-12, 12, n); e[K["FB_ENV_WIND_D"]] = rng.uniform(-2, 2, n)
    e[K["FB_ENV_T_SL"]] = rng.uniform(258.0, 313.0, n); e[K["FB_ENV_P_SL"]] = rng.uniform(97000.0, 104500.0, n)
    e[K["FB_ENV_H_TERRAIN"]] = rng.uniform(-50.0, 150.0, n) if h_trn is None else h_trn
    return e


def default_trim_params(n=1, **kw):
    """C172.TrimParameters() packed (c172.jl:806-818; PayloadY() defaults), rows FB_TP_* given by keyword replaced"""
    from oracle_binding import header_enums
    K = header_enums()
    tp = np.zeros((K["FB_NTP"], n))
    tp[K["FB_TP_N_E"]] = 1.0; tp[K["FB_TP_H_E"]] = 1050.0; tp[K["FB_TP_EAS"]] = 50.0
    tp[K["FB_TP_FUEL_LOAD"]] = 0.5; tp[K["FB_TP_MIXTURE"]] = 0.5
    tp[K["FB_TP_PAYLOAD"]:K["FB_TP_PAYLOAD"] + 5] = np.array([75.0, 75.0, 0.0, 0.0, 50.0])[:, None]
    for k, v in kw.items():
        tp[K[k]] = v
    return tp


def default_trim_state(n=1):
    return np.tile(np.array([[0.08], [0.0], [0.75], [0.4], [0.0], [0.0], [0.0]]), (1, n))


def flying_batch(fb, oracle, n, seed, lat, lon, h_e, climb, env_kw):
    """trimmed aircraft (device trim at a benign altitude) moved to altitude h_e with a vertical speed `climb` (m/s, + up)"""
    rng = np.random.default_rng(seed)
    tp = fb.TrimParameters(EAS=rng.uniform(40.0, 55.0, n), h_e=1000.0, ψ_nb=rng.uniform(-np.pi, np.pi, n))
    w = fb.BatchedWorld(n)
    fb.f_init(w, tp)
    assert w.trim_success.all()
    x, s, u, ui = w.x, w.s, w.u, w.ui
    w.close()
    x[16:20] = q_ew_from_latlon(lat, lon)
    x[20] = h_e
    # pitch the velocity vector: v_eb_b keeps its trimmed body components, the attitude is pitched by asin(climb / V) about body y
    V = np.sqrt(x[24] ** 2 + x[25] ** 2 + x[26] ** 2)
    dth = np.arcsin(np.clip(climb / V, -0.9, 0.9))
    z = np.zeros(n)
    x[12:16] = qmul(x[12:16], np.stack([np.cos(dth / 2), z, np.sin(dth / 2), z]))
    return x, s, u, ui


def clock(fb, w):
    cnt = C.c_int64(-1)
    assert fb.lib.fb_get_step_count(w._h, C.byref(cnt)) == 0
    return float(fb.lib.fb_time(w._h)), cnt.value


def digest(*arrays):
    """sha256 over the arrays' bytes, in the order given"""
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digest_dict(d):
    """sha256 over the keys of `d` in sorted order, each followed by its array's bytes"""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(d):
        h.update(k.encode()); h.update(np.ascontiguousarray(d[k]).tobytes())
    return h.hexdigest()


def library_kernels(tmp_path_factory):
    """name -> lds / scratch / vgpr of every kernel in the built library's gfx950 code object (no GPU needed)"""
    import re
    import shutil
    import subprocess
    import pytest
    lib, llvm = os.path.join(ROOT, "flight.jl_amd", "libflightbatch.so"), "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(lib):
        pytest.fail("libflightbatch.so is not built: python -c 'import __graft_entry__ as g; g.build()'")
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        if not os.path.exists(os.path.join(llvm, tool)):
            pytest.skip(f"{tool} not found under {llvm}")
    d = tmp_path_factory.mktemp("co")
    fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(d, "discard.so")], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"], check=True)
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    recs = re.findall(r"\.group_segment_fixed_size:\s*(\d+).*?\.name:\s*(\S+).*?\.private_segment_fixed_size:\s*(\d+).*?\.vgpr_count:\s*(\d+)", notes, re.S)
    filt = shutil.which("c++filt")
    out = {}
    for lds, name, scratch, vgpr in recs:
        dem = subprocess.run([filt, name], capture_output=True, text=True).stdout.strip() if filt else name
        out[re.sub(r"\(.*", "", dem).replace("void ", "")] = dict(lds=int(lds), scratch=int(scratch), vgpr=int(vgpr))
    return out


# ---- 3b. aircraft trimmed over a runway: the batches of the air / ground hand-over tests -------------------------------------------------------
def band_scenario(fb, N0, n, h_trn, band, s_reverse, s_mirror, seed=7):
    """tests/test_gpu_launch_edges.py's batch: trim parameters, groups and control-law inputs of n Cessna172Xv2 around the `band` metres over
    a runway at h_trn (N0: the geoid height there), drawn once, the same for every case"""
    K = fb.K
    N = n
    rng = np.random.default_rng(seed)
    grp = rng.integers(0, 3, N)
    ga, gb, gc = grp == 0, grp == 1, grp == 2
    lev = ga & (rng.random(N) < 0.5)
    rev = ga & ~lev
    clr0 = np.where(lev, rng.uniform(12, 30, N), np.where(rev, rng.uniform(10.5, 13, N), np.where(gb, rng.uniform(9.0, 11.0, N), rng.uniform(4, 9, N))))
    gam = np.where(lev, -rng.uniform(0.03, 0.06, N), np.where(rev, -rng.uniform(0.04, 0.06, N), np.where(gb, 0.0, rng.uniform(0.02, 0.05, N))))
    tp = fb.TrimParameters(EAS=rng.uniform(42.0, 55.0, N), h_e=h_trn + N0 + clr0, ψ_nb=rng.uniform(-np.pi, np.pi, N), γ_wb_n=gam)
    clm = np.where(lev, -rng.uniform(1.5, 3.5, N), np.where(rev, -rng.uniform(2.0, 3.0, N), rng.uniform(1.5, 3.0, N)))
    clm_up = rng.uniform(3.0, 5.0, N)
    dh = np.where(lev, rng.uniform(5, 8, N), band + rng.uniform(-1, 1, N))

    def set_cu(cu):
        cu[K["FB_CU_LON_MODE_REQ"]] = np.where(lev | gb, float(fb.ModeControlLon.EAS_alt), float(fb.ModeControlLon.EAS_clm))
        cu[K["FB_CU_LAT_MODE_REQ"]] = float(fb.ModeControlLat.φ_β)
        cu[K["FB_CU_CLM_REF"]] = clm
        cu[K["FB_CU_H_REF"]] = h_trn + N0 + dh
        cu[K["FB_CU_EAS_REF"]] = tp.EAS
        return cu

    def write(cu, step):
        """the host's write between two fb.step calls, on the device and on the oracle alike"""
        if step == s_reverse:
            cu[K["FB_CU_CLM_REF"], rev] = clm_up[rev]
        if step in s_mirror:
            cu[K["FB_CU_H_REF"], gb] = 2 * (h_trn + N0 + band) - cu[K["FB_CU_H_REF"], gb]
        return cu
    return tp, dict(a=ga, b=gb, c=gc), set_cu, write


RUNWAY_H_TRN, RUNWAY_BAND = 120.0, 10.0


def runway_batch(fb, N0, n, seed=357):
    """n aircraft trimmed over the runway of band_scenario, three groups mixed within every wave: (air) level at 40-100 m, airborne throughout;
    (band) descending from 10.5-13 m through the band's edge; (gnd) sinking at 1-2 m/s from 2.3-3.8 m, onto the wheels within the first
    second or two. Returns the trim parameters, the groups and set_cu (Cessna172Xv2: the autopilot holds each group to its path)."""
    K = fb.K
    rng = np.random.default_rng(seed)
    grp = rng.integers(0, 3, n)
    air, bnd, gnd = grp == 0, grp == 1, grp == 2
    clr0 = np.where(air, rng.uniform(40, 100, n), np.where(bnd, rng.uniform(10.5, 13, n), rng.uniform(2.3, 3.8, n)))
    gam = np.where(air, 0.0, np.where(bnd, -rng.uniform(0.04, 0.06, n), -rng.uniform(0.02, 0.04, n)))
    tp = fb.TrimParameters(EAS=rng.uniform(42.0, 55.0, n), h_e=RUNWAY_H_TRN + N0 + clr0, ψ_nb=rng.uniform(-np.pi, np.pi, n), γ_wb_n=gam)
    clm = np.where(bnd, -rng.uniform(2.0, 3.0, n), -rng.uniform(1.0, 2.0, n))

    def set_cu(cu):
        cu[K["FB_CU_LON_MODE_REQ"]] = np.where(air, float(fb.ModeControlLon.EAS_alt), float(fb.ModeControlLon.EAS_clm))
        cu[K["FB_CU_LAT_MODE_REQ"]] = float(fb.ModeControlLat.φ_β)
        cu[K["FB_CU_CLM_REF"]] = clm
        cu[K["FB_CU_H_REF"]] = RUNWAY_H_TRN + N0 + clr0
        cu[K["FB_CU_EAS_REF"]] = tp.EAS
        return cu
    return tp, dict(air=air, band=bnd, gnd=gnd), set_cu


# ---- 4. scenario tables: the two ways to run one -------------------------------------------------------------------------------------------
def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def load_scenario_blob(fb, w, blob):
    """a packed table through the C ABI's fb_set_table; returns its status (refusals are what the callers test)"""
    blob = np.ascontiguousarray(blob, dtype=np.float64)
    return fb.lib.fb_set_table(w._h, fb.K["FB_TABLE_SCENARIO"], blob.ctypes.data_as(C.c_void_p), (C.c_int64 * 1)(blob.size), 1)


def table_state(n, scn, par, rec_init=np.nan):
    """what flightbatch.scenario.evaluate_on_host keeps between evaluations"""
    return dict(phase=np.zeros(n, np.int64), since=np.zeros(n, np.int64), step=0, rec=np.full((scn.n_rec, n), rec_init), par=np.array(par, dtype=np.float64))


def scenario_result(w, st=None):
    """everything a run leaves behind: the model's arrays and the table's state (the device's, or the host interpreter's `st`)"""
    st = w.scenario_state() if st is None else st
    out = dict(x=w.x, s=w.s, u=w.u, ui=w.ui, status=w.status, phase=np.asarray(st["phase"]).astype(np.int32), since=np.asarray(st["since"]), rec=st["rec"])
    if w.has_env:
        out["env"] = w.env
    if hasattr(w, "cu"):
        out.update(cu=w.cu, cs=w.cs)
    return out


def run_table_on_device(fb, w, scn, par, steps, dt, spl=50, every=1, ratio=1):
    sim = fb.Simulation(w, dt=dt, Δt=ratio * dt, save_on=False, steps_per_launch=spl)
    w.set_scenario(scn, params=par, every=every, rec_init=np.nan)
    fb.step(sim, steps * dt); w.sync()
    return scenario_result(w)


def run_table_as_callback(fb, w, scn, par, steps, dt, every=1, ratio=1, model=None):
    """the same table from a Simulation(user_callback=...): flightbatch.scenario.host_callback, which fetches what the table names"""
    from flightbatch import scenario as sc
    st = table_state(w.n, scn, par)
    blob = scn.pack() if model is None else scn.pack(model=model)
    sim = fb.Simulation(w, dt=dt, Δt=ratio * dt, save_on=False, user_callback=sc.host_callback(blob, st, dt, every=every))
    fb.step(sim, steps * dt); w.sync()
    return scenario_result(w, st)


def assert_same_run(a, b, label):
    for k in ("x", "s", "u", "ui", "env", "status", "phase", "since", "rec", "cu", "cs"):
        if k in a:
            assert same(a[k], b[k]), (label, k, np.flatnonzero((np.atleast_2d(a[k]) != np.atleast_2d(b[k])).any(0))[:8])


# ---- 5. Robot2D against the oracle ---------------------------------------------------------------------------------------------------------
DEFAULT_VP = np.array([0.15, 0.05, 1.0, 0.1, -1.0, -1.0, 0.32, 0.0189, 0.0014])   # Vehicle(), robot2d.jl:20-30


def gains_from_h5():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "flight.jl_amd", "flightbatch"))
    import hdf5_min
    d = hdf5_min.read_all(os.path.join(ROOT, "flight.jl_amd", "data", "robot2d.h5"))
    return np.concatenate([d["K_fbk"].ravel(), d["K_fwd"].ravel(), d["K_int"].ravel(), d["x_trim"].ravel(), d["u_trim"].ravel(),
                           d["z_trim"].ravel(), [0.6, 0.0, 0.0, 0.01]]).astype(np.float64)


def robot2d_oracle_init(L, vp, ip):
    r = np.zeros((10, ip.shape[1]))
    L.fo_robot2d_init(C.c_int64(ip.shape[1]), vp.ctypes.data_as(_D), np.ascontiguousarray(ip).ctypes.data_as(_D), r.ctypes.data_as(_D))
    return r


def robot2d_oracle_run(L, vp, gp, r, u, dt, ratio, ctl, step0, nsteps):
    st = np.zeros(r.shape[1], np.int32)
    L.fo_robot2d_step(C.c_int64(r.shape[1]), pd(vp), pd(gp), C.c_double(dt), ratio, ctl, pd(u), pd(r), C.c_int64(step0), C.c_int64(nsteps),
                      st.ctypes.data_as(_I))
    return st


# ---- 6. Model(lss): random batches, the host RK4 and the device run --------------------------------------------------------------------------
LSS_DT, LSS_NSTEPS, LSS_N_TRAJ, LSS_STEP_AT = 0.01, 1000, 130, 100
LSS_EXCHANGE_VAR = "FLIGHTBATCH_LSS_EXCHANGE"
LSS_EXCHANGES = ("panel", "shfl")


def make_lss(fb, nx, nu, ny, n, seed, stable=False):
    """every system of the batch has its own random matrices (a group that reads its neighbour's row shows up)"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, nx, nx))
    if stable:   # spectral abscissa <= -0.5 and ||A||_2 <= 5, so that ||A|| dt <= 0.05 at dt = 0.01
        for i in range(n):
            A[i] -= (np.linalg.eigvals(A[i]).real.max() + 0.5) * np.eye(nx)
            A[i] *= min(1.0, 5.0 / np.linalg.norm(A[i], 2))
            assert np.linalg.eigvals(A[i]).real.max() <= 0.0 and np.linalg.norm(A[i], 2) * 0.01 <= 0.5
    mk = lambda *s: rng.standard_normal(s)
    return fb.LinearizedSS(xdot0=0.1 * mk(n, nx), x0=mk(n, nx), u0=mk(n, nu), y0=mk(n, ny), A=A, B=mk(n, nx, nu), C=mk(n, ny, nx), D=mk(n, ny, nu),
                           x_labels=tuple(f"x{k}" for k in range(nx)), u_labels=tuple(f"u{k}" for k in range(nu)),
                           y_labels=tuple(f"y{k}" for k in range(ny)))


def affine(c0, M, dv, N, dw, dtype=np.float64):
    """c0 + M dv + N dw by an explicit column loop, M first; also sum of the magnitudes of every term (for the bound). [n, rows]"""
    acc = c0.astype(dtype).copy()
    mag = np.abs(acc)
    for c in range(M.shape[2]):
        t = M[:, :, c].astype(dtype) * dv[:, c:c + 1].astype(dtype)
        acc += t; mag += np.abs(t)
    for c in range(N.shape[2]):
        t = N[:, :, c].astype(dtype) * dw[:, c:c + 1].astype(dtype)
        acc += t; mag += np.abs(t)
    return acc, mag


def rk4_host(m, x, ua, ub, dtype):
    """the steppers' stage form, u = ua for the first LSS_STEP_AT steps and ub after them; returns x after LSS_NSTEPS. [n, nx]"""
    A, x0 = m.A.astype(dtype), m.x0.astype(dtype)
    x = x.astype(dtype)
    dt, hdt, dt6 = dtype(LSS_DT), dtype(LSS_DT) / 2, dtype(LSS_DT) / 6
    none = np.zeros((x.shape[0], 0, 0))
    for u in (ua, ub):
        c0, _ = affine(m.xdot0, m.B, u - m.u0, none, none, dtype)     # (held over the launch)
        def f(z):
            acc = c0.copy()
            dz = z - x0
            for c in range(A.shape[2]):
                acc += A[:, :, c] * dz[:, c:c + 1]
            return acc
        for _ in range(LSS_STEP_AT if u is ua else LSS_NSTEPS - LSS_STEP_AT):
            k1 = f(x); k2 = f(x + hdt * k1); k3 = f(x + hdt * k2); k4 = f(x + dt * k3)
            x = x + dt6 * (2 * (k2 + k3) + (k1 + k4))
    return x


_TRAJ = {}


def traj_case(fb, shape):
    """model, start, inputs and the two host trajectories of a shape, computed once and shared by the files that use it (never modified)"""
    if shape not in _TRAJ:
        nx, nu, ny = shape
        m = make_lss(fb, nx, nu, ny, LSS_N_TRAJ, seed=31 * nx, stable=True)
        rng = np.random.default_rng(nx)
        xs = m.x0 + rng.standard_normal((LSS_N_TRAJ, nx))
        ua, ub = m.u0 + 0.0, m.u0 + rng.standard_normal((LSS_N_TRAJ, nu))
        _TRAJ[shape] = (m, xs, ua, ub, rk4_host(m, xs, ua, ub, np.longdouble), rk4_host(m, xs, ua, ub, np.float64))
    return _TRAJ[shape]


def lss_run_device(fb, case, spl, cuts=None):
    m, xs, ua, ub = case[:4]
    w = fb.LinearWorld(m)
    w.set_state(xs.T)
    w.set_params(dt=LSS_DT)
    assert fb.lib.fb_set_steps_per_launch(w._h, spl) == 0
    w.u = ua.T
    for k in (cuts[0] if cuts else [LSS_STEP_AT]):
        w.step(k)
    w.u = ub.T
    for k in (cuts[1] if cuts else [LSS_NSTEPS - LSS_STEP_AT]):
        w.step(k)
    w.sync()
    x = w.x.T.copy()
    cnt = C.c_int64()
    assert fb.lib.fb_get_step_count(w._h, C.byref(cnt)) == 0 and cnt.value == LSS_NSTEPS and abs(w.t - LSS_NSTEPS * LSS_DT) < 1e-9
    assert (w.status == 0).all()
    w.close()
    return x


def _exchange(name):
    import flightbatch as fb
    from flightbatch import lss as L
    assert name in LSS_EXCHANGES and fb.LinearWorld is L.LinearWorld
    init = L.LinearWorld.__init__

    def checked(self, *a, **k):
        init(self, *a, **k)
        assert self.exchange == name, (self.exchange, name)

    with _env_var(LSS_EXCHANGE_VAR, name):
        L.LinearWorld.__init__ = checked
        try:
            yield
        finally:
            L.LinearWorld.__init__ = init


def exchange(name):
    """worlds created inside step with the LDS panel ("panel") or with cross-lane reads ("shfl"): FLIGHTBATCH_LSS_EXCHANGE is read when a
    handle is created (fb_lss_create, fb_lss_from_linearization). Every LinearWorld created inside, by whatever helper, is asked which
    exchange it got."""
    import contextlib
    return contextlib.contextmanager(_exchange)(name)


# ---- 7. a caller's device memory and streams: ctypes on the HIP runtime the library is linked against (no torch in the pytest process) ---------
HIP_H2D, HIP_D2H, HIP_D2D = 1, 2, 3          # hipMemcpyKind
HIP_NOT_READY = 600                          # hipErrorNotReady
GUARD_BYTE = 0xA5


class Hip:
    """the few runtime calls a host that owns its state buffers and its stream makes; every call is checked (query() returns the code)"""
    def __init__(self):
        L = self.lib = C.CDLL("libamdhip64.so")
        VP, SZ = C.c_void_p, C.c_size_t
        for name, args in (("hipMalloc", [C.POINTER(VP), SZ]), ("hipFree", [VP]), ("hipMemcpy", [VP, VP, SZ, C.c_int]),
                           ("hipMemcpyAsync", [VP, VP, SZ, C.c_int, VP]), ("hipMemset", [VP, C.c_int, SZ]),
                           ("hipStreamCreateWithFlags", [C.POINTER(VP), C.c_uint]), ("hipStreamDestroy", [VP]), ("hipStreamSynchronize", [VP]),
                           ("hipEventCreate", [C.POINTER(VP)]), ("hipEventRecord", [VP, VP]), ("hipEventQuery", [VP]), ("hipEventDestroy", [VP]),
                           ("hipDeviceSynchronize", [])):
            f = getattr(L, name)
            f.argtypes, f.restype = args, C.c_int

    def _ok(self, rc, what):
        assert rc == 0, f"{what} failed with HIP error {rc}"

    def malloc(self, nbytes):
        p = C.c_void_p()
        self._ok(self.lib.hipMalloc(C.byref(p), nbytes), "hipMalloc")
        return p.value

    def free(self, p):
        self._ok(self.lib.hipFree(p), "hipFree")

    def memset(self, p, byte, nbytes):
        self._ok(self.lib.hipMemset(p, byte, nbytes), "hipMemset")

    def upload(self, dst, a):
        a = np.ascontiguousarray(a)
        self._ok(self.lib.hipMemcpy(dst, a.ctypes.data_as(C.c_void_p), a.nbytes, HIP_H2D), "hipMemcpy (to the device)")

    def download(self, src, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self._ok(self.lib.hipMemcpy(out.ctypes.data_as(C.c_void_p), src, out.nbytes, HIP_D2H), "hipMemcpy (from the device)")
        return out

    def copy(self, dst, src, nbytes):
        """device to device on the null stream, complete on return"""
        self._ok(self.lib.hipMemcpy(dst, src, nbytes, HIP_D2D), "hipMemcpy (device to device)")
        self.device_sync()

    def copy_async(self, dst, src, nbytes, stream):
        self._ok(self.lib.hipMemcpyAsync(dst, src, nbytes, HIP_D2D, stream), "hipMemcpyAsync")

    def stream(self):
        s = C.c_void_p()
        self._ok(self.lib.hipStreamCreateWithFlags(C.byref(s), 1), "hipStreamCreateWithFlags(hipStreamNonBlocking)")
        return s.value

    def stream_destroy(self, s):
        self._ok(self.lib.hipStreamDestroy(s), "hipStreamDestroy")

    def stream_sync(self, s):
        self._ok(self.lib.hipStreamSynchronize(s), "hipStreamSynchronize")

    def device_sync(self):
        self._ok(self.lib.hipDeviceSynchronize(), "hipDeviceSynchronize")

    def event(self, stream):
        """a new event recorded on `stream` behind what is queued there"""
        e = C.c_void_p()
        self._ok(self.lib.hipEventCreate(C.byref(e)), "hipEventCreate")
        self._ok(self.lib.hipEventRecord(e.value, stream), "hipEventRecord")
        return e.value

    def query(self, e):
        """0: everything in front of the event is done; HIP_NOT_READY: not yet"""
        rc = self.lib.hipEventQuery(e)
        assert rc in (0, HIP_NOT_READY), f"hipEventQuery failed with HIP error {rc}"
        return rc

    def event_destroy(self, e):
        self._ok(self.lib.hipEventDestroy(e), "hipEventDestroy")


class GuardedRows:
    """[rows x n] elements of `dtype` in device memory that the CALLER owns: one allocation with a guard row of n elements in front of the rows
    and one behind them, every byte outside the rows GUARD_BYTE. `offset` bytes shift the rows inside the allocation (a view into a larger
    tensor: 8-byte aligned doubles, 4-byte aligned int32). The rows start out as `fill`."""
    def __init__(self, hip, rows, n, dtype, offset=0, fill=0):
        self.hip, self.rows, self.n, self.dtype = hip, rows, n, np.dtype(dtype)
        self.nbytes = rows * n * self.dtype.itemsize
        self.lead = n * self.dtype.itemsize + offset
        self.total = self.nbytes + 2 * n * self.dtype.itemsize + 16
        assert 0 <= offset <= 16
        self.base = hip.malloc(self.total)
        hip.memset(self.base, GUARD_BYTE, self.total)
        self.ptr = self.base + self.lead
        self.write(np.full((rows, n), fill, dtype=self.dtype))

    def write(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.shape == (self.rows, self.n)
        self.hip.upload(self.ptr, a)

    def read(self):
        return self.hip.download(self.ptr, (self.rows, self.n), self.dtype)

    def guards_intact(self):
        raw = self.hip.download(self.base, (self.total,), np.uint8)
        return bool((raw[:self.lead] == GUARD_BYTE).all() and (raw[self.lead + self.nbytes:] == GUARD_BYTE).all())

    def free(self):
        if self.base:
            self.hip.free(self.base)
            self.base = 0
