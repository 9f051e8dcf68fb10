"""flightbatch — Python host mirror of the Flight.jl operator surface over libflightbatch (HIP, gfx950).

Julia is the reference's host language and is not available in this environment; this package plays the
role the `FlightBatch.jl` ccall shim (flight.jl_amd/julia/FlightBatch.jl) plays for a
Julia host. Importing it requires the built shared library; there is no CPU fallback.
"""
from ._lib import K, EXPORTED, LIB_PATH, FlightBatchError, lib  # noqa: F401
from .modeling import (BatchedWorld, Simulation, SimulationTermination, TimeSeries, TrimParameters, TrimState,  # noqa: F401
                       f_init, f_ode, f_periodic, f_step, init, run, step, checkpoint, restore)
from . import tables  # noqa: F401
from . import sharding  # noqa: F401
from .robot2d import Robot2DWorld, InitParameters  # noqa: F401
from .c172x import Cessna172Xv2World, ModeControlLon, ModeControlLat, ModeGuidance  # noqa: F401
from . import ctl_gains  # noqa: F401
from . import scenario  # noqa: F401
from .fleet import MixedFleet  # noqa: F401
from .linearization import LinearizedSS, linearize, linearize_state, subsystem, delete_vars  # noqa: F401
from .lss import LinearWorld, linear_world  # noqa: F401
from .lqr import LqrResult, lqr, closed_loop, design_model, DlqrResult, dlqr  # noqa: F401
from .poles import PolesResult, poles, dampreport  # noqa: F401
from . import timeresp  # noqa: F401
from .timeresp import StepInfo, StepResult, stepinfo  # noqa: F401  (the response itself is timeresp.step: `step` is the Simulation verb)
from .connect import ConnectResult, connect, integrator_world, pid_world, state_feedback, unity_feedback  # noqa: F401
from . import surgery  # noqa: F401
from .surgery import (TransformResult, SteadyResult, transform, subsystem_world, delete_vars_world, steady_state, integrators_world,  # noqa: F401
                      integral_augmentation, lqr_tracker, c172x_design_model)
from .c2d import C2dResult, c2d  # noqa: F401  (`c2d` is the verb; the status words are K["FB_C2D_NOT_FINITE"], K["FB_C2D_RANGE"])
from .timeresp import lsim  # noqa: F401
from .margins import MarginsResult, margins  # noqa: F401  (`margins` is the verb; the status words are K["FB_MARGINS_*"])
from .dfreq import DPolesResult, dfreqresp, dmargins, dpoles, ddampreport, default_dgrid  # noqa: F401  (the verbs of a sampled LinearWorld)
from . import pidopt  # noqa: F401
from .pidopt import (PIDData, Metrics, Settings, PIDMetricsResult, PIDOptResult, build_pid, freqresp, pid_metrics, optimize_pid,  # noqa: F401
                     check_results)
from . import dpid  # noqa: F401
from .dpid import DPIDMetricsResult, build_dpid, dpid_metrics, optimize_dpid  # noqa: F401  (the sampled law on a sampled LinearWorld)
from .dconnect import dconnect, dintegrator_world, dpid_world, dstate_feedback, dseries, dunity_feedback  # noqa: F401  (`dconnect` is the verb)
from . import dtracker  # noqa: F401
from .dtracker import (DSteadyResult, DTrackerResult, dsteady_state, dtracker_metrics, dintegrators_world, dintegral_augmentation,  # noqa: F401
                       dlqr_tracker, dtracker_world)
