import ctypes as C, sys, time
import pytest
sys.path.insert(0, "flight.jl_amd"); sys.path.insert(0, "."); sys.path.insert(0, "tests")
import flightbatch as fb
# usage: tools/dbg_sync.py [n spl kin]   one case of tests/test_gpu_duo.py::test_duo_and_air_steppers_agree, run in this process so that the
# counters the kernels leave behind can be read afterwards
case = "-".join(sys.argv[1:4]) if len(sys.argv) > 3 else "1000-50-WA"
t0 = time.time()
rc = pytest.main(["-q", "-x", f"tests/test_gpu_duo.py::test_duo_and_air_steppers_agree[{case}]"])
print("test passed" if rc == 0 else f"pytest exit status {int(rc)}")
print("took", time.time() - t0)
out = (C.c_uint * 40)()
fb.lib.fb_debug_duo_sync(out)
o = list(out)
print("failures", o[0])
for k in range(0, min(o[1], 28), 4):
    print("block %d thread %d (role %s pair %d) count %d partner %d" % (o[2 + k], o[3 + k], "P" if o[3 + k] < 256 else "D", (o[3 + k] & 255) >> 6, o[4 + k], o[5 + k]))
