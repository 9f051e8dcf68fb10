"""The four frequency-domain verbs of the linear-model family — fb_lss_freqresp, fb_lss_margins, fb_lss_dfreqresp, fb_lss_dmargins — pinned
bit for bit at both ends of every group size: the kernels behind them hold the same complex elimination three times and the same margins
body twice, and writing either once must not move a bit in either time domain (profiles/freq_family_refactor.txt: the compiler's
contraction of the pivot row's products did, per instance). tests/golden/freq_pin.json holds DEVICE-GENERATED digests
(tests/support.digest), recorded with the build before the change that added this test; tests/golden/make_freq_pin.py holds
the cases and made it: nx = 1, 8, 9, 16, 17, 32; 67 systems (whole waves of groups and a ragged one at P = 8, 16 and 32); 66 frequencies
for the margins (a full 64-interval chunk and one interval of a second), 3 for the grid response; the margins call of every shape carries
a per-system gain vector, all = 1, a system with a NaN entry and one the elimination refuses among healthy ones with 0 to 3 crossings.

So that the test still means something after a regeneration, the same run must also agree with the numpy restatements
(tests/margins_prototype.py, tests/dmargins_prototype.py) under the rule of tests/test_gpu_margins.py and tests/test_gpu_dmargins.py: the
device may deviate from the exact side ten times as far as the prototype does over the same loops, with a floor of 1e-11, counts and
status equal — on loops that are checked here to be fair in those tests' sense. The 67 systems deal 5 distinct systems with period 5 and
3 gains with period 3: the first 15 are every distinct loop, and every later healthy system must repeat its loop's bits."""
import functools
import json

import numpy as np
import pytest

import dmargins_prototype as dproto
import margins_prototype as proto
from golden import make_freq_pin as pin
from support import digest

pytestmark = pytest.mark.gpu
DISTINCT = 15


@functools.lru_cache(maxsize=None)
def _pinned():
    with open(pin.OUT, encoding="utf-8") as f:
        return json.load(f)["cases"]


@functools.lru_cache(maxsize=None)
def _refs(nx, sampled):
    """(prototype's deviation, exact result) of each distinct loop, and that the loops are fair"""
    S, g = pin.systems(nx, sampled)
    out, fair = [], [np.inf, np.inf, np.inf]
    for i in range(DISTINCT):
        if sampled:
            got, (ex, L) = dproto.margins(*S[i], pin.DW, pin.TS, g[i]), dproto.exact(*S[i], pin.DW, pin.TS, g[i])
        else:
            got, (ex, L) = proto.margins(*S[i], pin.W, g[i]), proto.exact(*S[i], pin.W, g[i])
        out.append((proto.deviation(got, ex), ex))
        fair = [min(a, b) for a, b in zip(fair, proto.fairness(L, ex))]
    assert fair[0] >= proto.FAIR_GRID and fair[1] >= proto.FAIR_GRID and fair[2] >= proto.FAIR_GM, fair
    assert max(d for d, _ in out) <= proto.PROTO_MAX
    return out


def test_the_pin_covers_every_shape():
    want = {f"fb_lss_{d}{verb} nx={nx}" for d in ("", "d") for verb in ("freqresp", "margins") for nx in pin.NX}
    want.discard("fb_lss_freqresp nx=32")          # (a PID verb: nx <= FB_PID_NX_MAX = 28; k_lss_freqresp<32> is stage 1 of fb_lss_margins there)
    assert set(_pinned()) == want and (pin.N, pin.NW, len(pin.I3)) == (67, 66, 3)
    for P in (8, 16, 32):          # whole waves of 64 / P groups, then a ragged one; the two flagged systems lie in whole waves
        assert pin.N % (64 // P) != 0 and max(pin.I_NAN, pin.I_SING) < pin.N - pin.N % (64 // P)


@pytest.mark.parametrize("sampled", [False, True], ids=["continuous", "sampled"])
@pytest.mark.parametrize("nx", pin.NX)
def test_bit_identical_to_the_recorded_build_and_close_to_the_prototype(fb, nx, sampled, capsys):
    (re, im), out = pin.run(fb, nx, sampled)
    sel, counts, allv, status = out
    d = "d" if sampled else ""
    healthy = [i for i in range(pin.N) if i not in (pin.I_NAN, pin.I_SING)]

    # ---- the restatement: the flagged systems, the distinct loops under the family's rule, and every repeat of a loop
    want = np.zeros(pin.N, dtype=np.int32)
    want[pin.I_NAN], want[pin.I_SING] = proto.NOT_FINITE, proto.SINGULAR
    assert status.tolist() == want.tolist()
    for i in (pin.I_NAN, pin.I_SING):
        assert np.isnan(sel[:, i]).all() and np.isnan(allv[:, :, i]).all() and (counts[:, i] == 0).all()
    refs = _refs(nx, sampled)
    dev_d = max(proto.deviation(proto.from_device(*out, i), refs[i][1]) for i in range(DISTINCT))
    dev_p = max(dp for dp, _ in refs)
    with capsys.disabled():
        print(f"\n[freq pin] fb_lss_{d}margins nx = {nx:2d}: device {dev_d:.2e}, prototype {dev_p:.2e}; crossings kept {int(counts[:, healthy].sum())}", end="")
    assert dev_d <= max(proto.FACTOR * dev_p, proto.FLOOR), (dev_d, dev_p)
    for i in healthy:
        k = i % DISTINCT
        assert all(np.array_equal(a[..., i], a[..., k], equal_nan=True) for a in out), (i, k)
    if re is not None:
        assert np.isnan(re[:, pin.I_NAN]).all() and np.isnan(im[:, pin.I_NAN]).all()
        assert np.isfinite(re[:, healthy]).all() and np.isfinite(im[:, healthy]).all()
        assert np.isnan(re[:, pin.I_SING]).any()          # (the continuous singular system: at w = 1, the middle frequency, alone)
        for i in healthy:
            assert np.array_equal(re[:, i], re[:, i % 5]) and np.array_equal(im[:, i], im[:, i % 5]), i

    # ---- the pin
    cases = _pinned()
    if re is not None:
        assert digest(re, im) == cases[f"fb_lss_{d}freqresp nx={nx}"]
    assert digest(*out) == cases[f"fb_lss_{d}margins nx={nx}"]
