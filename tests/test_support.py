"""tests/support.py itself: the state-row maps against the layouts they stand for, the error scale against values written out by hand, and
that no test module is used as a library (on the CPU, in milliseconds)."""
import os
import re

import numpy as np
import pytest

from oracle_binding import header_enums
from support import H_E_ROW, ROOT, UNUSED_ROWS, abi_to_oracle_rows, h_e_row_abi, state_scale

K = header_enums()
PAIRS = [(model, kin) for model in ("s0", "x2") for kin in ("WA", "ECEF", "NED")]
ABI_ROWS = {("s0", "WA"): 27, ("s0", "ECEF"): 26, ("s0", "NED"): 24, ("x2", "WA"): 34, ("x2", "ECEF"): 33, ("x2", "NED"): 31}


@pytest.mark.parametrize("model,kin", PAIRS)
def test_row_map_has_the_abi_length_and_is_injective(model, kin):
    rows = abi_to_oracle_rows(K, model, kin)
    n_oracle = 27 if model == "s0" else 34
    assert rows.size == ABI_ROWS[model, kin] and np.unique(rows).size == rows.size
    assert rows.min() >= 0 and rows.max() < n_oracle


@pytest.mark.parametrize("model,kin", PAIRS)
def test_row_map_leaves_out_the_rows_the_mechanisation_keeps_at_zero(model, kin):
    left_out = np.setdiff1d(np.arange(27 if model == "s0" else 34), abi_to_oracle_rows(K, model, kin))
    assert left_out.tolist() == {"WA": [], "ECEF": [20], "NED": [18, 19, 20]}[kin] == list(UNUSED_ROWS[kin])


@pytest.mark.parametrize("model,kin", PAIRS)
def test_altitude_row_of_the_abi_layout_maps_to_the_oracles(model, kin):
    want = {"WA": 20, "ECEF": 19, "NED": 17}[kin]
    assert abi_to_oracle_rows(K, model, kin)[h_e_row_abi(K, model, kin)] == want == H_E_ROW[kin]


def test_state_scale_on_a_vector_written_out_by_hand():
    x = np.array([0.5, -0.001,                        # filtered α, β: floor 1e-2
                  3.0, -4.0, 0.0, 9.0, 2.0, 1.0,      # contact regulators: 1
                  0.25, -250.0,                       # fuel, engine speed: max(|x|, 1e-3)
                  7.0, -8.0,                          # engine PI states: 1
                  0.5, 0.5, -0.5, 0.5,                # q_wb: 1
                  0.1, 0.2, 0.3, 0.9,                 # q_ew: 1
                  -1234.5,                            # h_e: max(|x|, 1)
                  1e-5, -0.02, 0.3,                   # body rates: floor 1e-3
                  -50.0, 0.5, 2.0,                    # velocity: floor 1
                  0.7, -3.0, 0.0, 1e-9, 5.0, -0.2, 0.4])   # actuators: 1
    want = np.array([0.5, 0.01, 1, 1, 1, 1, 1, 1, 0.25, 250.0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1234.5, 1e-3, 0.02, 0.3, 50.0, 1.0, 2.0,
                     1, 1, 1, 1, 1, 1, 1])
    assert x.size == 34 and np.array_equal(state_scale(x), want) and np.array_equal(state_scale(x[:27]), want[:27])
    assert np.array_equal(state_scale(np.stack([x, x], axis=1)), np.stack([want, want], axis=1))
    # another mechanisation: its own altitude row as well (row 20 is unused there, and zero)
    y = x.copy(); y[20] = 0.0; y[19] = -640.0; y[17] = 0.5
    assert state_scale(y, "ECEF")[19] == 640.0 and state_scale(y, "ECEF")[20] == 1.0 and state_scale(y, "NED")[17] == 1.0
    assert np.array_equal(np.delete(state_scale(y, "ECEF"), [19, 20]), np.delete(want, [19, 20]))


def test_no_test_module_is_used_as_a_library():
    pattern = re.compile(r"^\s*(import|from)\s+test_", re.M)
    offenders = []
    for d in ("tests", "tools"):
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in files:
                if f.endswith(".py") and pattern.search(open(os.path.join(base, f), encoding="utf-8").read()):
                    offenders.append(os.path.relpath(os.path.join(base, f), ROOT))
    assert not offenders, f"helpers belong in tests/support.py (or reference_fixtures.py / conditioning.py): {offenders}"
