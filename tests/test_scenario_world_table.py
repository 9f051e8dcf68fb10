"""Scenario tables that reach the world, without a GPU: the three kinds appended to the ABI (FB_SCN_SRC_ENV, FB_SCN_DST_ENV, FB_SCN_SRC_Y), the builder
and pack() refusals, and the host interpreter's semantics of the new kinds on hand-made arrays."""
import numpy as np
import pytest


def test_old_enumerators_keep_their_values_and_the_three_new_ones_exist(fb):
    K = fb.K
    src = ["CONST", "T", "T_IN_PHASE", "X", "CS", "CU", "U", "S", "ON_GND", "H_E", "PSI", "THETA", "PHI", "CHI", "EAS", "CLM", "PAR", "REC"]
    assert [K["FB_SCN_SRC_" + s] for s in src] == list(range(18))
    assert [K["FB_SCN_DST_" + s] for s in ("CU", "U", "UI", "REC")] == [0, 1, 2, 3]
    assert [K["FB_SCN_" + s] for s in ("LT", "GT", "GE", "LE", "EQ", "NE", "ALWAYS")] == list(range(7))
    assert (K["FB_SCN_HDR"], K["FB_SCN_PHASE_REC"], K["FB_SCN_RULE_REC"], K["FB_SCN_ACT_REC"], K["FB_SCN_NTERM"]) == (8, 4, 8, 14, 3)
    # appended behind the existing ones (fails on the parent commit: the names do not exist)
    assert (K["FB_SCN_SRC_ENV"], K["FB_SCN_SRC_Y"], K["FB_SCN_NSRC"]) == (18, 19, 20)
    assert (K["FB_SCN_DST_ENV"], K["FB_SCN_NDST"]) == (4, 5)
    from flightbatch import scenario as sc
    assert sc.MAGIC == 5000001.0 and sc.SRC["ENV"] == 18 and sc.SRC["Y"] == 19 and sc.DST["ENV"] == 4


def _table(sc, action=None, cond=None, n_par=1, n_rec=1):
    scn = sc.Scenario(n_par=n_par, n_rec=n_rec)
    a, b = scn.phase("a"), scn.phase("b")
    scn.when(a, cond if cond is not None else sc.src.T >= 1.0, [action] if action is not None else [], then=b)
    return scn


def test_builder_and_pack(fb):
    from flightbatch import scenario as sc
    K = fb.K
    scn = _table(sc, sc.env("WIND_E", sc.env_("WIND_E") + sc.par(0)), cond=sc.y_(K["FB_Y_AIR"] + 19) - sc.par(0) > 30.0)
    blob = scn.pack()
    assert np.array_equal(blob, scn.pack(model="Cessna172Sv0")) and np.array_equal(blob, scn.pack(model="Cessna172Xv2"))
    ru = blob[K["FB_SCN_HDR"] + 2 * K["FB_SCN_PHASE_REC"]:][:K["FB_SCN_RULE_REC"]]
    assert list(ru[:5]) == [K["FB_SCN_SRC_Y"], K["FB_Y_AIR"] + 19, K["FB_SCN_GT"], 30.0, 0]
    ac = blob[K["FB_SCN_HDR"] + 2 * K["FB_SCN_PHASE_REC"] + K["FB_SCN_RULE_REC"]:]
    assert list(ac[:2]) == [K["FB_SCN_DST_ENV"], K["FB_ENV_WIND_E"]] and ac[4] == 2
    assert list(ac[5:11]) == [K["FB_SCN_SRC_ENV"], K["FB_ENV_WIND_E"], 1.0, K["FB_SCN_SRC_PAR"], 0, 1.0]
    assert sc.table_kinds(blob) == ({K["FB_SCN_SRC_Y"], K["FB_SCN_SRC_ENV"], K["FB_SCN_SRC_PAR"]}, {K["FB_SCN_DST_ENV"]})
    # every environment row may be read; by name or by index
    for k, name in enumerate(("WIND_N", "WIND_E", "WIND_D", "T_SL", "P_SL", "H_TERRAIN")):
        assert sc.env_(name).terms == ((K["FB_SCN_SRC_ENV"], k, 1.0),) and sc.env_(k).terms == sc.env_(name).terms
        _table(sc, sc.rec(0, sc.env_(name))).pack()
    for name in ("WIND_N", "WIND_E", "WIND_D"):
        _table(sc, sc.env(name, 1.0)).pack()


def test_pack_refusals(fb):
    from flightbatch import scenario as sc
    K = fb.K
    for name, why in (("T_SL", "derived rows"), ("P_SL", "derived rows"), ("H_TERRAIN", "constructor argument")):
        for model in (None, "Cessna172Sv0", "Cessna172Xv2"):
            with pytest.raises(ValueError, match=why):
                _table(sc, sc.env(name, 1.0)).pack(model=model)
    with pytest.raises(ValueError, match="WIND_N"):
        _table(sc, sc.env(6, 1.0)).pack()
    with pytest.raises(ValueError, match="environment row out of range"):
        _table(sc, sc.rec(0, sc.env_(K["FB_NENV"]))).pack()
    with pytest.raises(ValueError, match="environment row out of range"):
        _table(sc, cond=sc.env_(-1) > 0.0).pack()
    _table(sc, sc.rec(0, sc.y_(K["FB_NY"] - 1))).pack()
    with pytest.raises(ValueError, match="174 rows"):
        _table(sc, sc.rec(0, sc.y_(K["FB_NY"]))).pack()
    with pytest.raises(ValueError, match="174 rows"):
        _table(sc, cond=sc.y_(K["FB_NY"]) > 0.0).pack()
    with pytest.raises(KeyError):
        sc.env_("WIND")


def test_interpreter_semantics_of_the_world_kinds(fb):
    """Four aircraft, the last one terminated. Phase a: `always` WIND_N = par0 (aircraft 0 has that value already: no write); rule: y[5] > 0.5 ->
    WIND_E = WIND_N + 1 (reads what the `always` action before it wrote), REC0 = WIND_E (reads what the action before it wrote), WIND_D = 0 (there
    already: no write), REC1 = y[5] + T_SL."""
    from flightbatch import scenario as sc
    K = fb.K
    scn = sc.Scenario(n_par=1, n_rec=2)
    A, B = scn.phase("a"), scn.phase("b")
    scn.always(A, [sc.env("WIND_N", sc.par(0))])
    scn.when(A, sc.y_(5) > 0.5, [sc.env("WIND_E", sc.env_("WIND_N") + 1.0), sc.rec(0, sc.env_("WIND_E")), sc.env("WIND_D", 0.0),
                                 sc.rec(1, sc.y_(5) + sc.env_("T_SL"))], then=B)
    blob = scn.pack()
    n = 4
    env = np.zeros((K["FB_NENV"], n)); env[K["FB_ENV_WIND_N"]] = [2.0, 0.0, 0.0, 0.0]; env[K["FB_ENV_T_SL"]] = 288.0
    env0 = env.copy()
    y = np.zeros((K["FB_NY"], n)); y[5] = [1.0, 1.0, 0.0, 1.0]
    st = dict(phase=np.zeros(n, np.int64), since=np.zeros(n, np.int64), step=1, par=np.array([[2.0, 3.0, 4.0, 5.0]]), rec=np.zeros((2, n)),
              u=np.zeros((K["FB_NU"], n)), ui=np.zeros(n, np.int32), s=np.zeros((2, n), np.int32), active=np.array([True, True, True, False]),
              env=env, y=y)
    sc.evaluate_on_host(blob, st, 0.02, 0.02)
    assert st["phase"].tolist() == [1, 1, 0, 0]
    assert np.array_equal(env[K["FB_ENV_WIND_N"]], [2.0, 3.0, 4.0, 0.0])          # the terminated aircraft keeps its wind
    assert np.array_equal(env[K["FB_ENV_WIND_E"]], [3.0, 4.0, 0.0, 0.0])          # WIND_N as the `always` action left it, + 1
    assert np.array_equal(st["rec"][0], [3.0, 4.0, 0.0, 0.0]) and np.array_equal(st["rec"][1], [289.0, 289.0, 0.0, 0.0])
    assert np.array_equal(env[3:], env0[3:])
    assert st["env_changed"].tolist() == [True, True, True, False]
    # write only on change: the same evaluation again changes nothing for the aircraft still in phase a, and nothing at all in phase b
    st["env_changed"][:] = False
    y[5] = 0.0
    sc.evaluate_on_host(blob, st, 0.04, 0.02)
    assert not st["env_changed"].any() and st["phase"].tolist() == [1, 1, 0, 0]
    # ... and only the aircraft whose value differs is marked
    st["par"][0, 2] = 4.5
    sc.evaluate_on_host(blob, st, 0.06, 0.02)
    assert st["env_changed"].tolist() == [False, False, True, False] and env[K["FB_ENV_WIND_N"], 2] == 4.5


def test_y_is_read_as_it_stood_before_the_evaluations_own_actions(fb):
    """The record is the state behind the step: an action that changes an input or the wind does not change what a later action of the same
    evaluation reads from y (on the device nothing re-evaluates f_ode! in between), and the caller's array is not written."""
    from flightbatch import scenario as sc
    K = fb.K
    scn = sc.Scenario(n_par=0, n_rec=2)
    A = scn.phase("a")
    scn.always(A, [sc.rec(0, sc.y_(7)), sc.env("WIND_E", sc.y_(7) * 2.0), sc.u("ELEVATOR", 0.3), sc.rec(1, sc.y_(7) + sc.env_("WIND_E"))])
    n = 2
    y = np.zeros((K["FB_NY"], n)); y[7] = [1.5, -2.0]
    y_before = y.copy()
    st = dict(phase=np.zeros(n, np.int64), since=np.zeros(n, np.int64), step=1, par=np.zeros((0, n)), rec=np.zeros((2, n)), u=np.zeros((K["FB_NU"], n)),
              ui=np.zeros(n, np.int32), s=np.zeros((2, n), np.int32), active=np.ones(n, bool), env=np.zeros((K["FB_NENV"], n)), y=y)
    sc.evaluate_on_host(scn.pack(), st, 0.02, 0.02)
    assert np.array_equal(st["rec"][0], [1.5, -2.0]) and np.array_equal(st["env"][K["FB_ENV_WIND_E"]], [3.0, -4.0])
    assert np.array_equal(st["rec"][1], [4.5, -6.0]) and np.array_equal(y, y_before)


def test_host_callback_refuses_what_the_host_arrays_cannot_serve(fb):
    from flightbatch import scenario as sc
    with pytest.raises(ValueError, match="row order"):
        sc.host_callback(_table(sc, sc.rec(0, sc.x_(3))).pack(), {}, 0.02)


def test_taps_are_renewed_behind_an_always_wind_write(fb):
    """The device's order: `always` actions that read no tap, then the evaluation the taps come from, then the rules. A rule on EAS sees what `retap`
    supplies under the wind just written; y_ stays the record from before; without a wind change `retap` is not called."""
    from flightbatch import scenario as sc
    K = fb.K
    scn = sc.Scenario(n_par=1, n_rec=2)
    A, B = scn.phase("a"), scn.phase("b")
    scn.always(A, [sc.env("WIND_E", sc.par(0))])
    scn.when(A, sc.src.EAS < 40.0, [sc.rec(0, sc.src.EAS), sc.rec(1, sc.y_(K["FB_Y_AIR"] + 20))], then=B)
    n = 2
    y = np.zeros((K["FB_NY"], n)); y[K["FB_Y_AIR"] + 20] = 45.0
    calls = []

    def retap(st):
        calls.append(st["env"][K["FB_ENV_WIND_E"]].copy())
        st["EAS"] = 45.0 - st["env"][K["FB_ENV_WIND_E"]]
    st = dict(phase=np.zeros(n, np.int64), since=np.zeros(n, np.int64), step=1, par=np.array([[10.0, 0.0]]), rec=np.zeros((2, n)), u=np.zeros((K["FB_NU"], n)),
              ui=np.zeros(n, np.int32), s=np.zeros((2, n), np.int32), active=np.ones(n, bool), env=np.zeros((K["FB_NENV"], n)), y=y, EAS=np.full(n, 45.0),
              retap=retap)
    blob = scn.pack()
    sc.evaluate_on_host(blob, st, 0.02, 0.02)
    assert len(calls) == 1 and calls[0].tolist() == [10.0, 0.0]
    assert st["phase"].tolist() == [1, 0] and st["rec"][0].tolist() == [35.0, 0.0] and st["rec"][1].tolist() == [45.0, 0.0]
    sc.evaluate_on_host(blob, st, 0.04, 0.02)          # nothing changes any more: no second call
    assert len(calls) == 1
