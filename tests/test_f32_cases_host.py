"""The fp32 stepper's batch (tests/f32_cases.py) is FAIR, shown from the oracle alone on the CPU: it holds what the device tests mean to reach,
and no lane of it has an event that fp32 arithmetic could legitimately move by a step. So test_gpu_f32_events.py may hold EVERY lane's
discrete history to the oracle's, with no exclusions.

Conditioning: the oracle is run 13 times per size and length from start states an fp32 kernel cannot tell apart (the sixteen rows it holds in
fp32 rounded to float32, then moved by a relative uniform ±2^-19, about 32 fp32 ulps). The cap is zero: the per-step history of s and of the
status word of every lane is the same in all 13. A generator that violates it is changed (steeper crossing, other seed), the cap is not."""
import numpy as np
import pytest

import f32_cases as fc
from oracle_binding import header_enums

K = header_enums()
CASES = [(n, L) for n in fc.SIZES for L in fc.LENGTHS]


@pytest.mark.parametrize("n,nsteps", CASES)
def test_batch_holds_every_kind_of_lane(oracle, n, nsteps):
    inp, h = fc.make_inputs(K, oracle, n), fc.history(K, oracle, n, nsteps)
    kind, st0, s, x = inp["kind"], inp["st0"], h["s"], h["x"]
    STALL, ENG = K["FB_S_STALL"], K["FB_S_ENG_STATE"]
    assert n % 256 % 64 == 12 and fc.NKIND == 12                      # full waves and a ragged one of twelve lanes: one of each kind
    wave = np.arange(n) // 64
    dead, airborne, banded = fc.lane_sets(K, inp, h)
    live = ~dead
    # the k1 of the fp32 kernel is evaluated again for the lanes its f_step! modified: q_ew renormalised, stall flag or engine state changed
    qn = lambda v, r: np.sqrt((v[K[r]:K[r] + 4] ** 2).sum(0))
    mod1 = airborne & ((s[1] != s[0]).any(0) | (np.abs(qn(x[0], "FB_X_Q_EW") - 1) > 1e-8))
    assert (mod1 & (kind == 1)).any() and (mod1 & (kind == 2)).any() and (mod1 & (kind == 8)).any() and (mod1 & (kind == 9)).any()
    assert (np.abs(qn(x[1], "FB_X_Q_WB") - 1)[kind == 2] < 1e-12).all() and (np.abs(qn(x[0], "FB_X_Q_WB") - 1)[kind == 2] > 1e-8).all()
    clr = fc.clearance(K, inp, h)
    for wv in range(wave.max() + 1):
        here = wave == wv
        assert set(kind[here].tolist()) == set(range(fc.NKIND)), ("every kind", wv)
        assert 0 < (here & mod1).sum() < (here & live).sum(), ("modified by the first f_step!: a proper subset of the live lanes", wv)
        assert (here & airborne & ~mod1).any() and (here & dead).any() and (here & inp["to_ground"] & (kind == 8)).any() and (here & inp["to_ground"] & banded).any(), wv
    # events strictly inside the run, not on its first or last step
    inside = lambda k: (k > 1) & (k < nsteps)
    stalls = fc.first_step(s[:, STALL] == 1)
    k3 = (kind == 3) & (stalls >= 0)
    assert k3.sum() >= 2 and inside(stalls[k3]).all() and (s[0, STALL, kind == 3] == 0).all()
    runs = fc.first_step(s[:, ENG] == 2)
    for k in (4, 9):
        got = (kind == k) & (runs >= 0)
        assert (s[0, ENG, kind == k] == (1 if k == 4 else 0)).all() and got.sum() >= 2 and inside(runs[got]).all(), k
    assert (s[1, ENG, kind == 9] == 1).all()                          # off -> starting at the first f_step!
    if nsteps == 100:
        assert (runs[kind == 9] >= 5).any() and (runs[kind == 9] <= 40).all() and (runs[kind == 9] >= 0).all()
    off = fc.first_step(s[:, ENG] == 0)
    assert inside(off[kind == 10]).all() and (x[-1, K["FB_X_FUEL"], kind == 10] <= 0).all()        # run dry, all of them
    assert (off[kind == 8] == 1).all() and (s[:, ENG, kind == 5] == 0).all()
    assert (s[1, STALL, kind == 1] == 0).all() and (s[0, STALL, kind == 1] == 1).all()
    # kind 7: first within the band in step m (1-based), in the middle of the launches of 2 and of 7 (and of 14, 50)
    k7 = kind == 7
    m = (clr <= fc.BAND).argmax(0)[k7]
    assert (clr[0, k7] > fc.BAND).all() and (m >= 2).all() and ((m - 1) % 7 != 0).all() and ((m - 1) % 2 != 0).all() and len(set(m.tolist())) == 2
    # kind 11: inside the band, wheels clear of the terrain, all along; the regulator states are reset by the first f_step!
    assert (clr[:, banded] > 4.0).all() and (clr[:, banded] < fc.BAND - 2.0).all() and (h["status"][:, banded] == 0).all()
    frc = x[:, K["FB_X_LDG_FRC"]:K["FB_X_LDG_FRC"] + 6]
    assert ((frc[0] != 0).sum(0)[inp["to_ground"]] == 1).all() and not (frc[0] != 0)[:, ~inp["to_ground"]].any() and not frc[1:][:, :, ~k7].any()
    for spl in fc.PARTITIONS[nsteps]:
        nc = fc.never_committed(K, inp, h, spl)
        assert np.array_equal(nc, dead | banded | (inp["to_ground"] if spl >= nsteps else np.zeros(n, bool)))
    # who ends: nobody within 14 steps; within 100 the sinking lanes crash, well inside the run, and nobody else
    ended = h["status"][-1] != 0
    if nsteps == 14:
        assert np.array_equal(ended, dead)
    else:
        assert np.array_equal(ended, dead | k7) and (h["status"][-1, k7] == K["FB_ST_GROUND_CRASH"]).all()
        assert ((h["term_step"][k7] > 50) & (h["term_step"][k7] < nsteps - 2)).all()
    assert (h["term_step"][dead] == -1).all() and np.array_equal(x[-1][:, dead], x[0][:, dead])
    # the single-call oracle gives the same bits as the step-by-step history
    xo, so, sto, ts, tw = oracle.step_term(inp["x0"], inp["u"], inp["ui"], inp["s0"], oracle.default_env(), fc.DT, nsteps, status=inp["st0"])
    assert np.array_equal(xo, x[-1]) and np.array_equal(so, s[-1]) and np.array_equal(sto, h["status"][-1]) and np.array_equal(ts, h["term_step"])


@pytest.mark.parametrize("n,nsteps", CASES)
def test_no_event_that_fp32_could_move(oracle, n, nsteps):
    h, runs = fc.history(K, oracle, n, nsteps), fc.conditioning_runs(K, oracle, n, nsteps)
    assert len(runs) == fc.K_DRAWS + 1 == 13
    changed = np.zeros(n, bool)
    for r in runs:
        changed |= (r["s"] != h["s"]).any((0, 1)) | (r["status"] != h["status"]).any(0)
    # the smallest margins of the unperturbed run, for the record
    inp = fc.make_inputs(K, oracle, n)
    kind = inp["kind"]
    w = h["x"][:, K["FB_X_ENG_OMEGA"]]
    eng = h["s"][:, K["FB_S_ENG_STATE"]]
    starting = (eng[:-1] == 1) | (eng[1:] == 1)
    if starting.any():
        w_idle = 600 * np.pi / 30
        print("n = %d, %d steps: smallest |engine speed - w_idle| over the steps of a starting engine: %.3f rad/s" % (n, nsteps, np.abs(w[1:] - w_idle)[starting].min()))
    print("n = %d, %d steps: lanes whose discrete history changes in one of the 13 runs: %s (kinds %s)" % (n, nsteps, np.flatnonzero(changed).tolist(), kind[changed].tolist()))
    assert not changed.any()


@pytest.mark.parametrize("n,nsteps", CASES)
def test_the_envelope_moves_every_lane_the_fp32_kernel_steps(oracle, n, nsteps):
    """no floor is needed under the envelope: one fp32 ulp of jitter per step moves every lane that the kernel commits"""
    inp, h = fc.make_inputs(K, oracle, n), fc.history(K, oracle, n, nsteps)
    E = fc.envelope(K, oracle, n, nsteps)
    dead, airborne, banded = fc.lane_sets(K, inp, h)
    assert E.shape == (fc.K_ENVELOPE, n) and np.isfinite(E).all()
    print("n = %d, %d steps: envelope of the airborne lanes, quantiles 0/50/100 %%: %s" % (n, nsteps, np.quantile(E.max(0)[airborne], [0, 0.5, 1.0])))
    assert (E[:, airborne] > 2.0 ** -24).all() and (E[:, dead] == 0).all()
    assert airborne.sum() > 0.6 * n
