"""fbf::k_step_f32 at the edges of a batch and of a launch, device against device, no tolerance — and the throws of an FB_F32 handle.

Position independence. The kernel has no data flow between lanes besides two ballots (is anybody alive; did f_step! modify anybody), so a
lane's words — x, s, status, termination record — must be the same bits wherever it sits and whoever sits beside it: alone, in a prefix that
ends ahead of, on or behind a wave or workgroup boundary, in the reversed batch, among every second lane (another mix of modified,
handed-over and terminated lanes in its wave). A difference is a defect of the `mod` / `redoing` path or of the tail handling.

Lanes the fp32 kernel never commits — terminated before the run, inside the hand-over band or with a friction-regulator state set at every
launch start (tests/f32_cases.py: never_committed, decided from the oracle) — are stepped by k_step_air<WA, false, true, false> from the same
launch-start states as on an FB_F64 handle, whichever airborne stepper that handle has: the same bits, and no trace of the fp32 pass.

Throws. The fp32 pass ends nobody's simulation: an altitude or ISA range bit raises the hand-over, and the fp64 pass decides. With one launch
for the whole run a terminated lane is therefore the FB_F64 handle's, bit for bit, and the oracle's in status, step and place; with shorter
launches the steps ahead of the last launch were fp32 ones and the throw may come a step apart."""
import numpy as np
import pytest

import f32_cases as fc
from support import flying_batch, geoid, stepper

pytestmark = pytest.mark.gpu

N, NSTEPS, SPL = 268, 14, 7
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def reference_run(fb, oracle):
    return cached("ref", lambda: fc.run_device(fb, fc.make_inputs(fb.K, oracle, N), NSTEPS, SPL, dtype="f32"))


def pick(r, sel):
    return dict(x=r["x"][:, sel], s=r["s"][:, sel], status=r["status"][sel], term_step=r["term_step"][sel], term_where=r["term_where"][sel])


SUBSETS = [("first %d" % m, np.arange(m)) for m in (12, 63, 64, 65, 76, 255, 256, 257)] + [("reversed", np.arange(N)[::-1]), ("even lanes", np.arange(0, N, 2)),
                                                                                             ("odd lanes", np.arange(1, N, 2))]


@pytest.mark.parametrize("name,sel", SUBSETS, ids=[s[0].replace(" ", "-") for s in SUBSETS])
def test_a_lanes_words_do_not_depend_on_its_place(fb, oracle, name, sel):
    ref = reference_run(fb, oracle)
    sub = fc.run_device(fb, fc.make_inputs(fb.K, oracle, N), NSTEPS, SPL, dtype="f32", lanes=sel)
    want = pick(ref, sel)
    diff = (sub["x"].view(np.uint64) != want["x"].view(np.uint64)).any(0) | (sub["s"] != want["s"]).any(0) | (sub["status"] != want["status"])
    print("%s: %d of %d lanes differ from the 268-lane run: %s (kinds %s)" % (name, int(diff.sum()), sel.size, sel[diff][:12].tolist(), (sel[diff] % fc.NKIND)[:12].tolist()))
    assert fc.same_words(sub, want)


def test_a_lane_alone(fb, oracle):
    """n = 1, for the first two lanes of every kind (the second of kinds 8 and 11 with a regulator state set)"""
    ref = reference_run(fb, oracle)
    inp = fc.make_inputs(fb.K, oracle, N)
    for lane in range(2 * fc.NKIND):
        sub = fc.run_device(fb, inp, NSTEPS, SPL, dtype="f32", lanes=[lane])
        assert fc.same_words(sub, pick(ref, [lane])), ("lane", lane, "kind", lane % fc.NKIND)


def test_twice_the_same_run(fb, oracle):
    again = fc.run_device(fb, fc.make_inputs(fb.K, oracle, N), NSTEPS, SPL, dtype="f32")
    assert fc.same_words(again, reference_run(fb, oracle))


@pytest.mark.parametrize("spl", fc.PARTITIONS[14])
@pytest.mark.parametrize("n", fc.SIZES)
def test_lanes_the_fp32_kernel_never_commits(fb, oracle, n, spl):
    K = fb.K
    inp, h = fc.make_inputs(K, oracle, n), fc.history(K, oracle, n, NSTEPS)
    nc = fc.never_committed(K, inp, h, spl)
    dead, airborne, banded = fc.lane_sets(K, inp, h)
    assert (nc & dead).any() and (nc & banded & inp["to_ground"]).any() and (nc & banded & ~inp["to_ground"]).any()
    assert (nc & inp["to_ground"] & ~banded).any() == (spl >= NSTEPS)          # f_step! resets the regulators: fp32 steps from the second launch on
    f32 = fc.run_device(fb, inp, NSTEPS, spl, dtype="f32")
    for duo in (False, True):
        f64 = fc.run_device(fb, inp, NSTEPS, spl, dtype="f64", duo=duo)
        diff = (f32["x"].view(np.uint64) != f64["x"].view(np.uint64)).any(0)
        print("n = %d, launches of %d, FB_F64 handle with FLIGHTBATCH_DUO=%d: %d never-committed lanes, %d of them differ; %d of the %d others differ"
              % (n, spl, duo, int(nc.sum()), int((diff & nc).sum()), int((diff & ~nc).sum()), int((~nc).sum())))
        assert fc.same_words(f32, f64, nc)
        assert np.array_equal(f32["s"], f64["s"]) and np.array_equal(f32["status"], f64["status"])      # (every lane: the discrete states are the oracle's)
    # no trace of the fp32 pass: the fp32-held rows of a live never-committed lane are not float values, those of a committed lane are
    live_nc = nc & ~dead
    rows = f32["x"][fc.F32_ROWS]
    is_float = rows == rows.astype(np.float32).astype(np.float64)
    assert (~is_float[:, live_nc]).any(0).all() and is_float[:, airborne].all()
    assert np.array_equal(f32["x"][:, dead].view(np.uint64), inp["x0"][:, dead].view(np.uint64))


# ---- throws on an FB_F32 handle: the three set-ups of tests/test_gpu_termination.py at n = 268 -------------------------------------------------
def floor_orthometric(fb, oracle):
    rng = np.random.default_rng(41)
    lat = np.zeros(N); lon = np.zeros(N)
    h_e = -1000.0 + geoid(oracle, lat[:1], lon[:1])[0] + rng.uniform(0.05, 6.0, N)
    return flying_batch(fb, oracle, N, 41, lat, lon, h_e, -rng.uniform(3.0, 9.0, N), {}), dict(h_trn=-5000.0), 120, fb.K["FB_ST_ALT_RANGE"]


def floor_ellipsoidal_and_wheels(fb, oracle):
    rng = np.random.default_rng(43)
    lat = np.full(N, 0.05); lon = np.full(N, 1.38)
    h_e = -1000.0 + rng.uniform(1.0, 9.0, N)
    return flying_batch(fb, oracle, N, 43, lat, lon, h_e, -rng.uniform(3.0, 9.0, N), {}), dict(h_trn=-5000.0), 150, fb.K["FB_ST_ALT_RANGE"]


def isa_ceiling(fb, oracle):
    rng = np.random.default_rng(47)
    lat = rng.uniform(-1.0, 1.0, N); lon = rng.uniform(-3.0, 3.0, N)
    a = 6378137.0
    h_e = 84852.0 * a / (a - 84852.0) + geoid(oracle, lat, lon) - rng.uniform(0.1, 12.0, N)
    return flying_batch(fb, oracle, N, 47, lat, lon, h_e, rng.uniform(8.0, 30.0, N), {}), {}, 100, fb.K["FB_ST_ISA_RANGE"]


SETUPS = dict(floor_orthometric=floor_orthometric, floor_ellipsoidal_and_wheels=floor_ellipsoidal_and_wheels, isa_ceiling=isa_ceiling)


def throw_case(fb, oracle, name):
    """the set-up's inputs and the oracle's run of them (computed once per set-up, shared, left unchanged)"""
    def make():
        (x, s, u, ui), env_kw, nsteps, bit = SETUPS[name](fb, oracle)
        xo, so, sto, tso, two = oracle.step_term(x, u, ui, s, oracle.default_env(**env_kw), 0.01, nsteps)
        return dict(x=x, s=s, u=u, ui=ui, env_kw=env_kw, nsteps=nsteps, bit=bit, oracle=dict(x=xo, s=so, status=sto, term_step=tso, term_where=two))
    return cached(name, make)


def throw_run(fb, c, spl, dtype, duo=True, further=0):
    with stepper(duo):
        w = fb.BatchedWorld(N, dtype=dtype)
    try:
        if "h_trn" in c["env_kw"]:
            w.set_params(h_terrain=c["env_kw"]["h_trn"])
        w.set_state(c["x"], c["s"]); w.u = c["u"]; w.ui = c["ui"]
        sim = fb.Simulation(w, dt=0.01, save_on=False, steps_per_launch=spl)
        fb.step(sim, c["nsteps"] * 0.01); w.sync()
        ts, tw = w.termination
        out = dict(x=w.x, s=w.s, status=w.status, term_step=ts, term_where=tw)
        if further:
            fb.step(sim, further * 0.01); w.sync()
            out["later"] = dict(x=w.x, s=w.s, status=w.status)
        return out
    finally:
        w.close()


@pytest.mark.parametrize("name", list(SETUPS))
def test_throws_in_one_launch_are_the_fp64_handles(fb, oracle, name):
    c = throw_case(fb, oracle, name)
    o, nsteps = c["oracle"], c["nsteps"]
    early = (o["status"] != 0) & (o["term_step"] <= nsteps - 2)
    assert early.sum() > N // 2 and (o["status"][early] == c["bit"]).all()
    f32 = throw_run(fb, c, nsteps, "f32")
    f64 = throw_run(fb, c, nsteps, "f64", duo=False)
    print("%s, one launch of %d steps: %d lanes terminated by step %d; places %s" % (name, nsteps, int(early.sum()), nsteps - 2, np.unique(o["term_where"][early]).tolist()))
    for k in ("status", "term_step", "term_where"):                                                                # status, step and place: the oracle's
        assert np.array_equal(f32[k][early], o[k][early]), k
    assert fc.same_words(f32, f64, early)                                                                          # every word: the fp64 handle's
    assert ((f32["status"] & fb.K["FB_ST_NAN"]) == 0).all()


@pytest.mark.parametrize("spl", [1, 7])
@pytest.mark.parametrize("name", list(SETUPS))
def test_throws_in_short_launches(fb, oracle, name, spl):
    K = fb.K
    c = throw_case(fb, oracle, name)
    o, nsteps = c["oracle"], c["nsteps"]
    early = (o["status"] != 0) & (o["term_step"] <= nsteps - 2)
    r = throw_run(fb, c, spl, "f32", further=5)
    off = r["term_step"][early] - o["term_step"][early]
    print("%s, launches of %d: %d lanes terminated by step %d, termination step off by one on %d, place differs on %d"
          % (name, spl, int(early.sum()), nsteps - 2, int((off != 0).sum()), int((r["term_where"][early] != o["term_where"][early]).sum())))
    assert np.array_equal(r["status"][early], o["status"][early]) and (np.abs(off) <= 1).all()
    term = r["status"] != 0
    assert np.array_equal(r["x"][:, term].view(np.uint64), r["later"]["x"][:, term].view(np.uint64)) and np.array_equal(r["s"][:, term], r["later"]["s"][:, term])
    assert np.array_equal(r["status"][term], r["later"]["status"][term])
    assert ((r["status"] & K["FB_ST_NAN"]) == 0).all() and ((r["later"]["status"] & K["FB_ST_NAN"]) == 0).all()
    assert np.isfinite(r["x"]).all()
