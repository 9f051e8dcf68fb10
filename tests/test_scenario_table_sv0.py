"""Scenario tables for a Cessna172Sv0 batch, without a GPU: the host interpreter on a model without control-law rows, Scenario.pack(model=...)
and the blobs of the shipped examples (which must not change)."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_evaluate_on_host_without_control_law_rows(fb):
    """A U / UI / REC table on a state dict that has neither `cu` nor `cs` (a Cessna172Sv0 has none), three aircraft, against the phase sequence
    worked out by hand: `always` first, then the first rule that holds, one transition per evaluation, values read when their action runs,
    terminated aircraft left alone."""
    from flightbatch import scenario as sc
    K = fb.K
    EL, TH = K["FB_U_ELEVATOR"], K["FB_U_THROTTLE"]
    scn = sc.Scenario(n_par=2, n_rec=2)
    A, B, C_ = scn.phase("a"), scn.phase("b"), scn.phase("c")
    scn.always(A, [sc.u("THROTTLE", 0.5)])
    scn.when(A, sc.src.T - sc.par(0) >= 0.0, [sc.u("ELEVATOR", sc.u_("ELEVATOR") + sc.par(1)), sc.rec(0, sc.u_("ELEVATOR")), sc.ui("ENG_STOP", 1.0)], then=B)
    scn.when(A, sc.src.T >= 100.0, [sc.rec(1, 99.0)], then=C_)            # (never holds)
    scn.when(B, sc.src.THETA > 0.1, [sc.rec(1, sc.src.T_IN_PHASE), sc.ui("ENG_STOP", 0.0)], then=C_)
    scn.when(B, sc.src.T_IN_PHASE >= 0.25, [sc.rec(1, -1.0)], then=A)
    blob = scn.pack(model="Cessna172Sv0")
    assert np.array_equal(blob, scn.pack())
    n, dt = 3, 0.125
    u = np.zeros((K["FB_NU"], n)); u[EL] = [0.01, 0.02, 0.03]
    st = dict(phase=np.zeros(n, np.int64), since=np.zeros(n, np.int64), step=0, par=np.array([[0.25, 0.125, 0.0], [0.1, 0.2, 0.3]]), rec=np.zeros((2, n)),
              u=u, ui=np.full(n, K["FB_UI_DEFAULT"], np.int32), s=np.zeros((2, n), np.int32), active=np.array([True, True, False]))
    theta = {1: [0, 0, 0], 2: [0.0, 0.05, 0], 3: [0.2, 0.05, 0], 4: [0.2, 0.05, 0], 5: [0, 0, 0]}
    seen = []
    for k in range(1, 6):
        st.update(step=k, theta=np.array(theta[k], dtype=np.float64))
        sc.evaluate_on_host(blob, st, k * dt, dt)
        seen.append(st["phase"].tolist())
    # aircraft 0: steps at t = 0.25 (step 2), θ > 0.1 at step 3 -> c. aircraft 1: steps at t = 0.125 (step 1), θ never above 0.1, back to a after
    # 0.25 s in b (step 3), where T - 0.125 >= 0 holds at once (step 4: the increment is applied a second time), and again two steps later.
    # aircraft 2 is terminated: never evaluated (its first rule would hold from the first step on)
    assert seen == [[0, 1, 0], [1, 1, 0], [2, 0, 0], [2, 1, 0], [2, 1, 0]]
    assert st["since"].tolist() == [3, 4, 0]
    assert np.array_equal(st["u"][EL], [0.01 + 0.1, 0.02 + 0.2 + 0.2, 0.03]) and np.array_equal(st["u"][TH], [0.5, 0.5, 0.0])
    assert np.array_equal(st["rec"][0], [0.01 + 0.1, 0.02 + 0.2 + 0.2, 0.0])       # (read AFTER the action before it wrote the row)
    assert np.array_equal(st["rec"][1], [0.125, -1.0, 0.0])                        # aircraft 0: one step in b when θ crossed
    stop = K["FB_UI_ENG_STOP"]
    assert ((st["ui"] & stop) != 0).tolist() == [False, True, False] and ((st["ui"] & ~stop) == K["FB_UI_DEFAULT"]).all()
    assert "cu" not in st and "cs" not in st


def test_pack_for_cessna172sv0_refuses_control_law_rows(fb):
    from flightbatch import scenario as sc

    def table(action=None, cond=None):
        scn = sc.Scenario(n_par=1, n_rec=1)
        a, b = scn.phase("a"), scn.phase("b")
        scn.when(a, cond if cond is not None else sc.src.T >= 1.0, [action] if action is not None else [], then=b)
        return scn

    for bad in (table(sc.rec(0, sc.cu_("EAS_REF"))), table(sc.rec(0, sc.cs_("SEG_S_2B"))), table(cond=sc.cs_("SEG_S_2B") > -200.0),
                table(cond=sc.cu_("EAS_REF") > 1.0), table(sc.cu("EAS_REF", sc.par(0)))):
        with pytest.raises(ValueError, match="Cessna172Xv2"):
            bad.pack(model="Cessna172Sv0")
        assert np.array_equal(bad.pack(), bad.pack(model="Cessna172Xv2"))           # (fine on the model that has the rows)
    always = sc.Scenario(n_par=0, n_rec=0)
    always.always(always.phase("a"), [sc.cu("THROTTLE_AXIS", 0.0)])
    with pytest.raises(ValueError, match="Cessna172Xv2"):
        always.pack(model="Cessna172Sv0")
    with pytest.raises(ValueError, match="27 state rows"):
        table(sc.rec(0, sc.x_(27))).pack(model="Cessna172Sv0")
    table(sc.rec(0, sc.x_(26))).pack(model="Cessna172Sv0")
    good = table(sc.u("ELEVATOR", sc.u_("ELEVATOR") + sc.par(0)))
    assert np.array_equal(good.pack(model="Cessna172Sv0"), good.pack())
    with pytest.raises(ValueError, match="unknown model"):
        good.pack(model="Robot2D")


# sha256 of the float64 bytes of the three example tables as the parent commit packs them
EXAMPLE_BLOBS = {
    "crosswind_landing": "f0664a30330a86ce72687281bed77bf9926f3d6d4682ffaefa01a0dd8d2ccc2e",
    "traffic_pattern": "04655fa773899406226bb2284db87513116c93aae3945df5b6d0bf1def473a5f",
    "elevator_doublet": "20f009a94c135cb6ed7980ab7cddac23b2b11983e4de1d077c10814374057712",
}


def test_pack_without_the_argument_is_byte_identical_for_the_example_tables(fb):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import crosswind_landing, traffic_pattern, elevator_doublet
    tables = {"crosswind_landing": crosswind_landing.scenario_table(False), "traffic_pattern": traffic_pattern.scenario_table(),
              "elevator_doublet": elevator_doublet.scenario_table()}
    for name, scn in tables.items():
        blob = scn.pack()
        assert blob.dtype == np.float64
        assert hashlib.sha256(np.ascontiguousarray(blob).tobytes()).hexdigest() == EXAMPLE_BLOBS[name], name
        assert np.array_equal(blob, scn.pack(model="Cessna172Xv2"))
        with pytest.raises(ValueError):      # all three drive the control laws
            scn.pack(model="Cessna172Sv0")
