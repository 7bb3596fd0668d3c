"""
neo_planner_amd -- MI355X-native replan inner loop of neo-planner (MINCO minimum-jerk
trajectory optimisation: coefficient solve, cost/gradient with ESDF lookups, L-BFGS-B),
behind the reference's Python interface.  See DESIGN.md / INTEGRATION.md.

Importing the package does not touch the GPU; the HIP library is loaded on first use and
there is no CPU fallback.
"""
from ._lib import Context, NeoError, default_context  # noqa: F401
from .esdf import ESDF, ESDF3D  # noqa: F401
from .planner import BatchPlanner, MinJerkPlanner, PlannerConfig  # noqa: F401
from .geo import GeoPlanner  # noqa: F401
from .geo_resident import BatchGeoPlanner  # noqa: F401
from .fleet import FleetReplanLoop  # noqa: F401
from .goal_routes import GoalRoutes  # noqa: F401
from .goal_sequences import GoalSequences  # noqa: F401
from .flight_model import FlightModel  # noqa: F401
from .depth import DepthCamera  # noqa: F401
from .onboard import OnboardMapper  # noqa: F401
from .record import DemoRecorder  # noqa: F401
from .training import train_initializer  # noqa: F401  (torch and the network are imported when it is called)
# the initializer network (torch) is imported on demand: `from neo_planner_amd import initializer`

__all__ = ["Context", "NeoError", "default_context", "ESDF", "ESDF3D", "BatchPlanner", "MinJerkPlanner",
           "PlannerConfig", "GeoPlanner", "BatchGeoPlanner", "FleetReplanLoop", "GoalRoutes", "GoalSequences", "FlightModel", "DepthCamera", "OnboardMapper", "DemoRecorder",
           "train_initializer"]
