#!/usr/bin/env python3
"""Generates tests/golden/freq_pin.json ON THE GPU, from the library that is built in the tree: DEVICE-GENERATED digests of everything the
four frequency-domain verbs of the linear-model family return — fb_lss_freqresp, fb_lss_margins (continuous), fb_lss_dfreqresp,
fb_lss_dmargins (sampled) — for tests/test_gpu_freq_pin.py, which imports the cases and `run` from here.

The shapes: nx = 1, 8, 9, 16, 17, 32, both ends of each group size (P = 8, 16, 32 lanes to a system); 67 systems, whole waves of groups
plus a ragged one at every P; 66 frequencies for the margins (one full 64-interval chunk of brackets and one interval of a second), 3 for
the grid response alone. Per nx and domain ONE margins call carries a per-system gain vector, all = 1, a system with a NaN entry and a
system the elimination refuses, among healthy ones with zero to three crossings:
  continuous   1 / (s^2 + 1) beside decoupled stable states: jw I - A is exactly singular at w = 1, which the grid holds. At nx = 1 no
               jw - a vanishes for w > 0: there, and in the sampled domain (no grid point is exactly a pole: w > 0, and sin pi is not 0 in
               double), L overflows instead (b and c of 1e308), which the elimination reports the same way
Record it with the build a change starts from; regenerate it whenever a later change MEANS to alter rounding (and say so in that change).

    python tests/golden/make_freq_pin.py
"""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import dmargins_prototype as dproto  # noqa: E402
import margins_prototype as proto  # noqa: E402
from support import digest  # noqa: E402

OUT = os.path.join(HERE, "freq_pin.json")
NX = (1, 8, 9, 16, 17, 32)
N, NW = 67, 66
I_NAN, I_SING = 21, 45          # in whole waves at every P, away from the ragged end
GAINS = (1.0, 0.6, 1.7)         # dealt with period 3 over systems dealt with period 5: 15 distinct loops
TS = 0.01
IU, IY = 1, 1
W = np.logspace(-2.0, 3.0, NW)
W[26] = 1.0                     # (the grid point of the continuous singular system, exactly)
DW = dproto.w_zoh(TS, NW)       # ends at nine tenths of the Nyquist frequency
I3 = [3, 26, 64]                # the three frequencies of the grid-response calls

pd = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
pi = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _kinds(nx):
    """the distinct healthy continuous systems at this nx: 0 to 3 crossings"""
    if nx == 1:
        return [proto.tf([K], [1.0, 1.0]) for K in (3.0, 0.5, 2.0, 7.0, 1.5)]
    rng = np.random.default_rng(3000 + nx)
    return [proto.embed(s, nx, rng) for s in (proto.cube(2.0), proto.cube(4.0), proto.conditionally_stable(), proto.tf([3.0], [1.0, 1.0, 0.0]), proto.cube(7.0))]


def _dkinds(nx):
    """the distinct healthy sampled systems at this nx"""
    if nx == 1:
        return [(np.array([[a]]), np.array([1.0]), np.array([K]), 0.0) for a, K in ((0.5, 1.0), (0.9, 0.3), (-0.5, 1.0), (0.5, 0.2), (0.0, 2.0))]
    rng = np.random.default_rng(4000 + nx)
    return [dproto.dembed(s, nx, rng) for s in (dproto.delay_integrator(0.3), dproto.zoh(proto.cube(4.0), TS), dproto.zoh(proto.conditionally_stable(), TS),
                                                dproto.delay_integrator(0.8), dproto.zoh(proto.cube(7.0), TS))]


def _overflow(s):
    return s[0], np.full(s[1].shape, 1e308), np.full(s[2].shape, 1e308), 0.0


@functools.lru_cache(maxsize=None)
def systems(nx, sampled):
    """(the N systems as (A, b, c, d), the N gains); the distinct healthy loops are the first 15"""
    kinds = _dkinds(nx) if sampled else _kinds(nx)
    out = [kinds[i % len(kinds)] for i in range(N)]
    A = out[I_NAN][0].copy(); A[nx - 1, 0] = np.nan
    out[I_NAN] = (A,) + out[I_NAN][1:]
    if sampled or nx == 1:
        out[I_SING] = _overflow(out[I_SING])
    else:
        A = -np.diag(np.arange(1.0, nx + 1.0)); A[:2, :2] = [[0.0, 1.0], [-1.0, 0.0]]
        b = np.zeros(nx); b[1] = 1.0
        out[I_SING] = (A, b, np.ones(nx), 0.0)
    return out, np.array([GAINS[i % len(GAINS)] for i in range(N)])


def _world(fb, nx, sampled):
    M = proto.lss_arrays(systems(nx, sampled)[0], iu=IU, iy=IY)
    lss = fb.LinearizedSS(**M, x_labels=tuple(f"x{k}" for k in range(nx)), u_labels=("u0", "u1"), y_labels=("y0", "y1"))
    return fb.LinearWorld(lss, Ts=TS) if sampled else fb.LinearWorld(lss)


def run(fb, nx, sampled):
    """the two calls of one shape through the C ABI: (re, im) [3, N] of the grid response; (sel, counts, all, status) of the margins.
    fb_lss_freqresp is a PID verb and takes nx <= FB_PID_NX_MAX = 28: at nx = 32 its (re, im) stay None (k_lss_freqresp<32> runs there as
    the margins' stage 1, and under the verb at nx = 17)"""
    world = _world(fb, nx, sampled)
    grid = DW if sampled else W
    w3 = np.ascontiguousarray(grid[I3])
    re, im = np.empty((3, N)), np.empty((3, N))
    fr = fb.lib.fb_lss_dfreqresp if sampled else fb.lib.fb_lss_freqresp
    if sampled or nx <= fb.K["FB_PID_NX_MAX"]:
        assert fr(world._h, IU, IY, pd(w3), 3, pd(re), pd(im)) == 0, fb.lib.fb_last_error()
    else:
        re = im = None
    sel, counts, status, allv = np.empty((10, N)), np.empty((2, N), dtype=np.int32), np.empty(N, dtype=np.int32), np.empty((6, proto.KMAX, N))
    mg = fb.lib.fb_lss_dmargins if sampled else fb.lib.fb_lss_margins
    assert mg(world._h, IU, IY, pd(grid), NW, pd(systems(nx, sampled)[1]), pd(sel), pi(counts), pd(allv), pi(status)) == 0, fb.lib.fb_last_error()
    world.close()
    return (re, im), (sel, counts, allv, status)          # (two calls on one world: the margins' own stage 1 is a second grid response)


def digests(fb):
    out = {}
    for sampled in (False, True):
        for nx in NX:
            fr, mg = run(fb, nx, sampled)
            d = "d" if sampled else ""
            if fr[0] is not None:
                out[f"fb_lss_{d}freqresp nx={nx}"] = digest(*fr)
            out[f"fb_lss_{d}margins nx={nx}"] = digest(*mg)
    return out


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import flightbatch as fb
    first, second = digests(fb), digests(fb)
    assert first == second, "the verbs are not deterministic run to run"
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump({"generated_by": "device, tests/golden/make_freq_pin.py", "digest": "tests/support.digest (sha256 of the arrays' bytes)",
                   "cases": first}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written:", OUT, len(first), "digests")


if __name__ == "__main__":
    main()
