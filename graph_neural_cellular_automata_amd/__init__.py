"""MI355X-native NCA rollout step (Psylocibe23/Graph_Neural_Cellular_Automata hot path).

The HIP kernels live in csrc/ and are built into libgnca.so (C ABI: include/gnca.h).  The
``modules`` subpackage mirrors the reference's nn.Module API on top of it.
"""
from .damage import DamagePolicy, regrow_trace
from .forward_grad import ParamDirections, forward_gradient_, loss_tangent
from .gauss_newton import cg_solve
from .loss import loss_curvature
from .lyapunov import TangentQR, orthonormalize_tangents
from .modules import FixedSobelPerception, GraphAugmentation, NeuralCA, NeuralCAGraph
from .modules._stepper import GaussNewtonProduct, ObjectiveTangent, TangentBlockResult, TangentResult
from .render import CMAPS, colorize, render_rgb
from .vitals import StateVitals, state_vitals

__all__ = ["FixedSobelPerception", "NeuralCA", "GraphAugmentation", "NeuralCAGraph",
           "render_rgb", "colorize", "CMAPS", "DamagePolicy", "regrow_trace",
           "state_vitals", "StateVitals", "TangentResult", "TangentBlockResult", "TangentQR",
           "orthonormalize_tangents", "ObjectiveTangent", "ParamDirections", "forward_gradient_", "loss_tangent",
           "GaussNewtonProduct", "cg_solve", "loss_curvature"]
